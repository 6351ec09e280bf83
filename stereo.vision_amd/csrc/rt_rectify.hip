// svx runtime: the stereo rectification — the maker of OpenCV's fixed-point map pair on the host
// (svx_rectify_host.h), the remap of host pictures through one (kernels/remap.hip), and the batch stage that remaps
// every frame's stored BGR pair, both eyes in one launch, between upload / decode / synth and sv_batch_preprocess.
#include <utility>
#include <vector>

#include "svx_rectify.h"
#include "svx_rectify_host.h"
#include "svx_runtime.h"

namespace {

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

extern "C" {

int sv_rectify_map(const double* K9, const double* D8, const double* R9, const double* P9, int dh, int dw, int16_t* xy,
                   uint16_t* frac) {
    if (const char* why = rectify_fill_map(K9, D8, R9, P9, dh, dw, xy, frac))
        return fail(SV_E_ARG, "sv_rectify_map: %s (dh=%d dw=%d)", why, dh, dw);
    return SV_OK;
}

int sv_remap_u8(const uint8_t* src, int n, int sh, int sw, int channels, const int16_t* xy, const uint16_t* frac,
                int dh, int dw, uint8_t* dst) {
    if (const char* why = remap_check_args(src, n, sh, sw, channels, xy, frac, dh, dw, dst))
        return fail(SV_E_ARG, "sv_remap_u8: bad arguments (%s)", why);
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    const size_t px = (size_t)dh * dw, sf = (size_t)sh * sw * channels, df = px * channels;
    // the device block: xy | frac | the pictures | the remapped pictures
    const size_t off_frac = up256(4 * px), off_src = off_frac + up256(2 * px), off_dst = off_src + up256(sf * n);
    HIP_TRY(d->rmp.ensure(off_dst + up256(df * n)));
    uint8_t* base = d->rmp.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(base, xy, 4 * px, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + off_frac, frac, 2 * px, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + off_src, src, sf * n, hipMemcpyHostToDevice, s));
    RemapArgs a{};
    a.src[0] = base + off_src, a.dst[0] = base + off_dst;
    a.xy[0] = reinterpret_cast<const int16_t*>(base), a.frac[0] = reinterpret_cast<const uint16_t*>(base + off_frac);
    a.eyes = 1, a.n = n, a.sh = sh, a.sw = sw, a.channels = channels, a.dh = dh, a.dw = dw;
    HIP_TRY(launch_remap(a, s));
    HIP_TRY(hipMemcpyAsync(dst, base + off_dst, df * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

// ---------------------------------------------------------------------------
// the batch: the stored BGR pairs through the two eyes' maps
// ---------------------------------------------------------------------------
int sv_batch_rectify_maps(sv_batch* b, const int16_t* xyL, const uint16_t* fracL, const int16_t* xyR,
                          const uint16_t* fracR) {
    if (!b || !xyL || !fracL || !xyR || !fracR) return fail(SV_E_ARG, "sv_batch_rectify_maps: null batch or map");
    const int H = b->pairH ? b->pairH : b->H, W = b->pairW ? b->pairW : b->Wu;
    if (const char* why = remap_check_dst(H, W)) return fail(SV_E_ARG, "sv_batch_rectify_maps: %s", why);
    for (const uint16_t* fr : {fracL, fracR})
        if (const char* why = remap_check_frac(fr, H, W)) return fail(SV_E_ARG, "sv_batch_rectify_maps: %s", why);
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));   // a rectify in flight still reads the maps these replace
    const size_t px = (size_t)H * W, xyb = up256(4 * px), frb = up256(2 * px);
    b->rect_h = b->rect_w = 0;
    HIP_TRY(b->rectmaps.ensure(2 * xyb + 2 * frb, false, 0, true));
    uint8_t* base = b->rectmaps.as<uint8_t>();
    HIP_TRY(hipMemcpy(base, xyL, 4 * px, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(base + xyb, xyR, 4 * px, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(base + 2 * xyb, fracL, 2 * px, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(base + 2 * xyb + frb, fracR, 2 * px, hipMemcpyHostToDevice));
    b->rect_h = H, b->rect_w = W;
    return SV_OK;
}

int sv_batch_rectify(sv_batch* b, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    const int H = b->pairH ? b->pairH : b->H, W = b->pairW ? b->pairW : b->Wu;
    if (!b->rect_h || b->rect_h != H || b->rect_w != W)
        return fail(SV_E_STATE, "no rectification maps of the pair shape %d x %d (sv_batch_rectify_maps first)", H, W);
    const size_t px3 = (size_t)H * W * 3, need = px3 * b->frames;
    if (!b->bgrL.p || !b->bgrR.p || b->bgrL.bytes < need || b->bgrR.bytes < need)
        return fail(SV_E_STATE, "no BGR pairs (sv_batch_synth_bgr_pair / upload_bgr_pair / decode_bgr_pair)");
    if (b->rect_done)
        return fail(SV_E_STATE, "the stored pairs are rectified already: no pair was uploaded, decoded or generated "
                                "since the last sv_batch_rectify");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    for (hipEvent_t& e : b->rect_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    b->rect_have_ms = false;
    // the gather cannot run in place: the second store, of the pairs' own size, made by the first call and kept
    HIP_TRY(b->rawL.ensure(need, false, 0, true));
    HIP_TRY(b->rawR.ensure(need, false, 0, true));
    const size_t xyb = up256(4 * (size_t)H * W), frb = up256(2 * (size_t)H * W);
    const uint8_t* maps = b->rectmaps.as<uint8_t>();
    RemapArgs a{};
    a.src[0] = b->bgrL.as<uint8_t>(), a.src[1] = b->bgrR.as<uint8_t>();
    a.dst[0] = b->rawL.as<uint8_t>(), a.dst[1] = b->rawR.as<uint8_t>();
    a.xy[0] = reinterpret_cast<const int16_t*>(maps), a.xy[1] = reinterpret_cast<const int16_t*>(maps + xyb);
    a.frac[0] = reinterpret_cast<const uint16_t*>(maps + 2 * xyb);
    a.frac[1] = reinterpret_cast<const uint16_t*>(maps + 2 * xyb + frb);
    a.eyes = 2, a.n = b->frames, a.sh = H, a.sw = W, a.channels = 3, a.dh = H, a.dw = W;
    HIP_TRY(hipEventRecord(b->rect_ev[0], s));
    HIP_TRY(launch_remap(a, s));
    HIP_TRY(hipEventRecord(b->rect_ev[1], s));
    // the stores change places: bgrL / bgrR are what every later stage and read-back takes, rawL / rawR keep the
    // pictures as they came (pair_store_written puts them back before the next one is written)
    std::swap(b->bgrL, b->rawL);
    std::swap(b->bgrR, b->rawR);
    b->rect_done = true;
    b->rect_have_ms = true;
    if (sync) HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_rectify_ms(sv_batch* b, float* ms) {
    if (!b || !ms) return fail(SV_E_ARG, "null batch or ms");
    if (!b->rect_have_ms) return fail(SV_E_STATE, "no sv_batch_rectify has run on this batch");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipEventSynchronize(b->rect_ev[1]));
    HIP_TRY(hipEventElapsedTime(ms, b->rect_ev[0], b->rect_ev[1]));
    return SV_OK;
}

}  // extern "C"
