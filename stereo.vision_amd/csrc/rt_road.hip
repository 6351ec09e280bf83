// svx runtime: the road chain. Road raster + non-zero walk, sanitiseRoadImage's clean-up, the obstacle stage, the
// result image and the image tile, each as a host-frame drop-in and as a batch stage; the batch's stages form one
// chain whose validity is the batch's road_level (svx_runtime.h).
#include "svx_hull_host.h"
#include "svx_morph.h"
#include "svx_result.h"
#include "svx_result_host.h"
#include "svx_runtime.h"
#include "svx_tile.h"
#include "svx_tile_host.h"

extern "C" {

// SV_E_STATE with the stage's message unless the batch's road chain has reached `need`
static int need_level(const sv_batch* b, RoadLevel need, const char* msg) {
    return b->road_level >= need ? SV_OK : fail(SV_E_STATE, "%s", msg);
}

// a stage's n events (b->road_ev + first), made on the stage's first call
static hipError_t stage_events(sv_batch* b, int first, int n, hipEvent_t** ev) {
    *ev = b->road_ev + first;
    for (int i = 0; i < n; ++i)
        if (!(*ev)[i])
            if (hipError_t e = hipEventCreate(*ev + i); e != hipSuccess) return e;
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// road raster + non-zero walk (functions.py:339-344, :359-365)
// ---------------------------------------------------------------------------
int sv_road_raster(const int32_t* pts, int64_t n, int H, int W, uint8_t* out_img) {
    if (n < 0 || H < 0 || W < 0 || !out_img || (n > 0 && !pts)) return fail(SV_E_ARG, "sv_road_raster: bad arguments");
    for (int64_t i = 0; i < n; ++i) {   // numpy raises IndexError past these; negatives wrap
        const int32_t x = pts[2 * i], y = pts[2 * i + 1];
        if (x < -W || x >= W || y < -H || y >= H)
            return fail(SV_E_ARG, "index out of range: point %lld is [%d, %d] for a %d x %d image", (long long)i, x, y, H, W);
    }
    if ((int64_t)H * W == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    HIP_TRY(d->aux.ensure((size_t)H * W));
    HIP_TRY(d->xy.ensure(sizeof(int32_t) * 2 * (size_t)(n > 0 ? n : 1)));
    if (n) HIP_TRY(hipMemcpyAsync(d->xy.p, pts, sizeof(int32_t) * 2 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_raster(d->xy.as<int32_t>(), d->xy.as<int32_t>() + 1, 2, nullptr, 0, 0, n, d->aux.as<uint8_t>(), 1, H,
                          W, W, s));
    HIP_TRY(hipMemcpyAsync(out_img, d->aux.p, (size_t)H * W, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_nonzero_points(const uint8_t* img, int H, int W, int32_t* out, int64_t cap, int64_t* out_n) {
    if (!img || !out_n || H < 0 || W < 0 || W > 4096 || (int64_t)H * W >= (1ll << 28))
        return fail(SV_E_ARG, "sv_nonzero_points: bad arguments (W <= 4096, H*W < 2^28)");
    *out_n = 0;
    const int64_t px = (int64_t)H * W;
    if (px == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    const int64_t padded = (px + 3) / 4 * 4;   // zero tail: no extra non-zero pixels
    HIP_TRY(d->aux.ensure((size_t)padded));
    if (padded != px) HIP_TRY(hipMemsetAsync(d->aux.as<uint8_t>() + px, 0, (size_t)(padded - px), s));
    HIP_TRY(hipMemcpyAsync(d->aux.p, img, (size_t)px, hipMemcpyHostToDevice, s));
    HIP_TRY(d->xy.ensure(sizeof(int32_t) * 2 * (size_t)px + 64));
    int64_t* cnt = reinterpret_cast<int64_t*>(d->xy.as<char>() + sizeof(int32_t) * 2 * (size_t)px);
    HIP_TRY(launch_nonzero(d->aux.as<uint8_t>(), 1, padded, W, d->xy.as<int32_t>(), px, cnt, false, s));
    int64_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, cnt, sizeof n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n > cap) return fail(SV_E_CAP, "capacity %lld < %lld non-zero pixels", (long long)cap, (long long)n);
    if (n) {
        HIP_TRY(hipMemcpyAsync(out, d->xy.p, sizeof(int32_t) * 2 * n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    *out_n = n;
    return SV_OK;
}

int sv_batch_road_raster(sv_batch* b, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (!b->ppxy.p) return fail(SV_E_STATE, "no pipeline points (create the batch with points and run the pipeline)");
    HIP_TRY(hipSetDevice(b->device));
    const size_t px = (size_t)b->H * b->W;
    HIP_TRY(b->road.ensure(px * b->frames));
    HIP_TRY(b->nz.ensure(sizeof(uint32_t) * b->cap * b->frames));   // packed entries x | y << 16 (walk_pk)
    HIP_TRY(b->nzcount.ensure(sizeof(int64_t) * b->frames));
    // the images and their non-zero walks in one pass (memset + raster + walk measured slower)
    b->rmap_fresh = false;
    b->road_level = kRoadImages;
    uint8_t* paint = nullptr;
    if (b->want_rmap) {   // imageRoadMap in the same pass (stereovision.py:131-133)
        HIP_TRY(b->rmap.ensure(px * 3 * b->frames));
        paint = b->rmap.as<uint8_t>();
    }
    if (b->rbits_fresh) {   // from the pipeline's bitmap (68 KB a frame) instead of its points (8 B a point)
        HIP_TRY(b->roff.ensure(sizeof(int32_t) * (size_t)b->H * b->frames));
        HIP_TRY(launch_road_bits(b->rbits.as<uint32_t>(), b->frames, b->H, b->W, b->roff.as<int32_t>(),
                                 (int64_t)b->cap, b->road.as<uint8_t>(), b->nz.as<int32_t>(),
                                 b->nzcount.as<int64_t>(), b->bgr.as<uint8_t>(), paint, b->stream));
    } else {
        HIP_TRY(launch_road(b->ppxy.as<uint32_t>(), b->counts, (int64_t)b->cap, b->road.as<uint8_t>(), b->frames,
                            b->H, b->W, b->Wu, b->nz.as<int32_t>(), b->nzcount.as<int64_t>(), b->bgr.as<uint8_t>(),
                            paint, b->stream));
    }
    b->rmap_fresh = paint != nullptr;
    if (sync) HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_nonzero(sv_batch* b, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (!b->road.p) return fail(SV_E_STATE, "no road images (sv_batch_road_raster first)");
    HIP_TRY(hipSetDevice(b->device));
    // sv_batch_road_raster walked the images as it wrote them: nothing left to launch
    if (sync) HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_road_bits(sv_batch* b, int enable) {
    if (!b) return fail(SV_E_ARG, "null batch");
    b->road_bits = enable != 0;
    return SV_OK;
}

int sv_batch_road_map(sv_batch* b, int enable) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (enable && !b->with_bgr) return fail(SV_E_STATE, "imageRoadMap needs the batch's BGR (with_bgr)");
    b->want_rmap = enable != 0;
    return SV_OK;
}

int sv_batch_read_road_map(sv_batch* b, int frame, uint8_t* out) {
    if (!b || !out || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    if (!b->rmap_fresh) return fail(SV_E_STATE, "no imageRoadMap (sv_batch_road_map(b, 1), then sv_batch_road_raster)");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const size_t px3 = (size_t)b->H * b->W * 3;
    HIP_TRY(hipMemcpy2D(out, (size_t)b->Wu * 3, b->rmap.as<uint8_t>() + px3 * frame, (size_t)b->W * 3,
                        (size_t)b->Wu * 3, b->H, hipMemcpyDeviceToHost));
    return SV_OK;
}

// packed walk entries (x | y << 16, walk_pk) widened to the reference's [x, y] int32 pairs
static void widen_walk(const std::vector<uint32_t>& pk, int32_t* out) {
    for (size_t i = 0; i < pk.size(); ++i) {
        out[2 * i] = (int32_t)(pk[i] & 0xFFFFu);
        out[2 * i + 1] = (int32_t)(pk[i] >> 16);
    }
}

// One frame's non-zero walk back (the stream is idle): its count into *n, then, when they fit the caller's cap,
// its packed entries (frame f's at walk + f per_frame) widened into nzpts
static int read_walk(const DevBuf& walk, size_t per_frame, const DevBuf& counts, int frame, int32_t* nzpts,
                     int64_t cap, int64_t* n) {
    int64_t k = 0;
    HIP_TRY(hipMemcpy(&k, counts.as<int64_t>() + frame, sizeof k, hipMemcpyDeviceToHost));
    *n = k;
    if (k > cap) return fail(SV_E_CAP, "capacity %lld < %lld", (long long)cap, (long long)k);
    if (k && nzpts) {
        std::vector<uint32_t> pk((size_t)k);
        HIP_TRY(hipMemcpy(pk.data(), walk.as<uint32_t>() + per_frame * frame, sizeof(uint32_t) * k,
                          hipMemcpyDeviceToHost));
        widen_walk(pk, nzpts);
    }
    return SV_OK;
}

int sv_batch_read_road(sv_batch* b, int frame, uint8_t* img, int32_t* nzpts, int64_t cap, int64_t* n) {
    if (!b || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const size_t px = (size_t)b->H * b->W;
    if (img) {
        if (!b->road.p) return fail(SV_E_STATE, "no road images");
        HIP_TRY(hipMemcpy2D(img, b->Wu, b->road.as<uint8_t>() + px * frame, b->W, b->Wu, b->H, hipMemcpyDeviceToHost));
    }
    if (n) {
        if (!b->nz.p) return fail(SV_E_STATE, "no non-zero walk (sv_batch_nonzero first)");
        return read_walk(b->nz, b->cap, b->nzcount, frame, nzpts, cap, n);
    }
    return SV_OK;
}

// ---------------------------------------------------------------------------
// sanitiseRoadImage's clean-up (functions.py:346-366): kernels/morph.hip, then the image and the walk
// ---------------------------------------------------------------------------

// 1024-wide frames of up to 1024 rows: the bitmap road pass (launch_road_bits) makes image and walk from the
// cleaned bitmap; other shapes: unpack, then the non-zero walk
static bool clean_by_road_bits(int H, int Wu) { return Wu == 1024 && H <= 1024; }

int sv_sanitise_road(const uint8_t* img, const uint8_t* mask, int H, int W, uint8_t* out_img, int32_t* out_pts,
                     int64_t cap, int64_t* out_n) {
    if (!img || H < 0 || W < 2 || W > 4096 || (int64_t)H * W >= (1ll << 28) || (out_pts && cap < 0))
        return fail(SV_E_ARG, "sv_sanitise_road: bad arguments (2 <= W <= 4096, H*W < 2^28)");
    if (out_n) *out_n = 0;
    if (H == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    const int pitch = (W + 7) / 8 * 8, WW = (W + 31) / 32;
    const size_t px = (size_t)H * pitch, words = (size_t)H * WW;
    // bitmaps: the image | the cleaned image | the mask | (bitmap road pass) the rows' walk offsets
    HIP_TRY(d->mbits.ensure(sizeof(uint32_t) * (3 * words + (size_t)H)));
    uint32_t* bin = d->mbits.as<uint32_t>();
    uint32_t* bout = bin + words;
    uint32_t* bmask = bout + words;
    int32_t* roff = reinterpret_cast<int32_t*>(bmask + words);
    if (int rc = upload_u8(d->aux, img, H, W, pitch, s)) return rc;
    HIP_TRY(launch_morph_pack(d->aux.as<uint8_t>(), (int64_t)px, pitch, W, H, 1, bin, s));
    if (mask) {
        if (int rc = upload_u8(d->aux2, mask, H, W, pitch, s)) return rc;
        HIP_TRY(launch_morph_pack(d->aux2.as<uint8_t>(), (int64_t)px, pitch, W, H, 1, bmask, s));
    }
    HIP_TRY(launch_morph_clean(bin, mask ? bmask : nullptr, bout, 1, H, W, s));
    // the image (into aux: the pack above has read it, in stream order) and the walk
    const bool bits_pass = clean_by_road_bits(H, W);
    HIP_TRY(d->xy.ensure(sizeof(int32_t) * 2 * px + 64));
    int64_t* cnt = reinterpret_cast<int64_t*>(d->xy.as<char>() + sizeof(int32_t) * 2 * px);
    if (bits_pass) {   // packed walk entries (x | y << 16)
        HIP_TRY(launch_road_bits(bout, 1, H, W, roff, (int64_t)px, d->aux.as<uint8_t>(), d->xy.as<int32_t>(), cnt,
                                 nullptr, nullptr, s));
    } else {           // [x, y] int32 pairs
        HIP_TRY(launch_morph_unpack(bout, 1, H, W, pitch, d->aux.as<uint8_t>(), s));
        HIP_TRY(launch_nonzero(d->aux.as<uint8_t>(), 1, (int64_t)px, pitch, d->xy.as<int32_t>(), (int64_t)px, cnt,
                               false, s));
    }
    int64_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, cnt, sizeof n, hipMemcpyDeviceToHost, s));
    if (out_img) HIP_TRY(hipMemcpy2DAsync(out_img, W, d->aux.p, pitch, W, H, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (out_n) *out_n = n;
    if (!out_pts || n == 0) return SV_OK;
    if (n > cap) return fail(SV_E_CAP, "capacity %lld < %lld non-zero pixels", (long long)cap, (long long)n);
    if (bits_pass) {
        std::vector<uint32_t> pk((size_t)n);
        HIP_TRY(hipMemcpyAsync(pk.data(), d->xy.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        widen_walk(pk, out_pts);
    } else {
        HIP_TRY(hipMemcpyAsync(out_pts, d->xy.p, sizeof(int32_t) * 2 * n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return SV_OK;
}

int sv_batch_road_mask(sv_batch* b, const uint8_t* mask) {
    if (!b) return fail(SV_E_ARG, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    b->road_level = std::min(b->road_level, kRoadImages);   // a clean-up made with the mask before is stale
    if (!mask) {
        b->have_rmask = false;
        return SV_OK;
    }
    if (b->Wu > 4096) return fail(SV_E_ARG, "the road clean-up takes frames up to 4096 wide");
    const size_t px = (size_t)b->H * b->W, words = (size_t)b->H * ((b->Wu + 31) / 32);
    HIP_TRY(b->rmask.ensure(px + sizeof(uint32_t) * words));   // the staged bytes, then the bitmap (px % 8 == 0)
    uint8_t* grey = b->rmask.as<uint8_t>();
    HIP_TRY(hipMemsetAsync(grey, 0, px, b->stream));
    HIP_TRY(hipMemcpy2DAsync(grey, b->W, mask, b->Wu, b->Wu, b->H, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(launch_morph_pack(grey, (int64_t)px, b->W, b->Wu, b->H, 1, reinterpret_cast<uint32_t*>(grey + px),
                              b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->have_rmask = true;
    return SV_OK;
}

int sv_batch_road_clean(sv_batch* b, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (int rc = need_level(b, kRoadImages, "no current road pass (sv_batch_road_raster after the pipeline first)"))
        return rc;
    if (b->Wu < 2 || b->Wu > 4096) return fail(SV_E_ARG, "the road clean-up takes frames 2..4096 wide");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    const int H = b->H, Wu = b->Wu, WW = (Wu + 31) / 32;
    const size_t px = (size_t)H * b->W, words = (size_t)H * WW;
    hipEvent_t* cev;
    HIP_TRY(stage_events(b, kEvClean, 4, &cev));
    b->road_level = kRoadImages;
    b->ccap = ((size_t)H * Wu + 63) / 64 * 64;
    HIP_TRY(b->cbits.ensure(sizeof(uint32_t) * words * b->frames));
    HIP_TRY(b->cimg.ensure(px * b->frames));
    HIP_TRY(b->cnz.ensure(sizeof(uint32_t) * b->ccap * b->frames));   // packed entries x | y << 16 (walk_pk)
    HIP_TRY(b->cnzcount.ensure(sizeof(int64_t) * b->frames));
    HIP_TRY(hipEventRecord(cev[0], s));
    const uint32_t* src;
    if (b->rbits_fresh && Wu == 1024) {   // the pipeline's own bitmap of the road pixels (32 words a row)
        src = b->rbits.as<uint32_t>();
    } else {
        HIP_TRY(b->cpack.ensure(sizeof(uint32_t) * words * b->frames));
        HIP_TRY(launch_morph_pack(b->road.as<uint8_t>(), (int64_t)px, b->W, Wu, H, b->frames, b->cpack.as<uint32_t>(), s));
        src = b->cpack.as<uint32_t>();
    }
    const uint32_t* mk = b->have_rmask ? reinterpret_cast<const uint32_t*>(b->rmask.as<uint8_t>() + px) : nullptr;
    HIP_TRY(hipEventRecord(cev[1], s));
    HIP_TRY(launch_morph_clean(src, mk, b->cbits.as<uint32_t>(), b->frames, H, Wu, s));
    HIP_TRY(hipEventRecord(cev[2], s));
    if (clean_by_road_bits(H, Wu)) {
        HIP_TRY(b->croff.ensure(sizeof(int32_t) * (size_t)H * b->frames));
        HIP_TRY(launch_road_bits(b->cbits.as<uint32_t>(), b->frames, H, b->W, b->croff.as<int32_t>(), (int64_t)b->ccap,
                                 b->cimg.as<uint8_t>(), b->cnz.as<int32_t>(), b->cnzcount.as<int64_t>(), nullptr,
                                 nullptr, s));
    } else {
        HIP_TRY(launch_morph_unpack(b->cbits.as<uint32_t>(), b->frames, H, Wu, b->W, b->cimg.as<uint8_t>(), s));
        HIP_TRY(launch_nonzero(b->cimg.as<uint8_t>(), b->frames, (int64_t)px, b->W, b->cnz.as<int32_t>(),
                               (int64_t)b->ccap, b->cnzcount.as<int64_t>(), true, s));
    }
    HIP_TRY(hipEventRecord(cev[3], s));
    b->road_level = kRoadCleaned;
    if (sync) HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_road_clean_ms(sv_batch* b, float* kernel_ms, float* total_ms) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (int rc = need_level(b, kRoadCleaned, "no road clean-up (sv_batch_road_clean first)")) return rc;
    HIP_TRY(hipSetDevice(b->device));
    const hipEvent_t* cev = b->road_ev + kEvClean;
    HIP_TRY(hipEventSynchronize(cev[3]));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, cev[1], cev[2]));
    if (total_ms) HIP_TRY(hipEventElapsedTime(total_ms, cev[0], cev[3]));
    return SV_OK;
}

int sv_batch_read_road_clean(sv_batch* b, int frame, uint8_t* img, int32_t* nzpts, int64_t cap, int64_t* n) {
    if (!b || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    if (int rc = need_level(b, kRoadCleaned, "no road clean-up (sv_batch_road_clean first)")) return rc;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const size_t px = (size_t)b->H * b->W;
    if (img)
        HIP_TRY(hipMemcpy2D(img, b->Wu, b->cimg.as<uint8_t>() + px * frame, b->W, b->Wu, b->H, hipMemcpyDeviceToHost));
    if (n) return read_walk(b->cnz, b->ccap, b->cnzcount, frame, nzpts, cap, n);
    return SV_OK;
}

// ---------------------------------------------------------------------------
// the obstacle stage (stereovision.py:170-189, functions.py:396-421): kernels/hull.hip
// ---------------------------------------------------------------------------
int sv_road_obstacles(const uint8_t* cleaned, const uint8_t* disp, const sv_plane* plane, int H, int W,
                      const sv_camera* cam, int32_t* hull_pts, int64_t cap, uint8_t* hull_mask, uint8_t* obstacles,
                      sv_hull_info* info) {
    if (const char* why = hull_check_args(cleaned, cam, H, W, hull_pts, cap, info))
        return fail(SV_E_ARG, "sv_road_obstacles: bad arguments (%s)", why);
    *info = sv_hull_info{0, 0, 0, 0, 0, 0};
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    const HullLayout l = hull_layout(H, W, 1, true);
    HIP_TRY(d->hull.ensure(l.bytes));
    char* base = d->hull.as<char>();
    uint32_t* bin = reinterpret_cast<uint32_t*>(base + l.off_in);
    uint32_t* bmask = reinterpret_cast<uint32_t*>(base + l.off_mask);
    uint32_t* bobst = reinterpret_cast<uint32_t*>(base + l.off_obst);
    int32_t* dpts = reinterpret_cast<int32_t*>(base + l.off_pts);
    sv_hull_info* dinfo = reinterpret_cast<sv_hull_info*>(base + l.off_info);
    if (int rc = upload_u8(d->aux, cleaned, H, W, l.pitch, s)) return rc;
    HIP_TRY(launch_morph_pack(d->aux.as<uint8_t>(), (int64_t)l.px, l.pitch, W, H, 1, bin, s));
    const uint8_t* ddisp = nullptr;
    HullPlane hp{};
    if (disp && plane) {
        if (int rc = upload_u8(d->disp, disp, H, W, l.pitch, s)) return rc;
        ddisp = d->disp.as<uint8_t>();
        hp = HullPlane{plane->a, plane->b, plane->c, cam->f, cam->f * cam->B, cam->cw, cam->ch, 1u};
    }
    HIP_TRY(launch_road_hull(bin, 1, H, W, ddisp, (int64_t)l.px, l.pitch, nullptr, 0, hp, dpts,
                             hull_mask ? bmask : nullptr, obstacles ? bobst : nullptr, dinfo, s));
    // the images (into aux / aux2: the pack above has read aux, in stream order)
    if (hull_mask) {
        HIP_TRY(launch_morph_unpack(bmask, 1, H, W, l.pitch, d->aux.as<uint8_t>(), s));
        HIP_TRY(hipMemcpy2DAsync(hull_mask, W, d->aux.p, l.pitch, W, H, hipMemcpyDeviceToHost, s));
    }
    if (obstacles) {
        HIP_TRY(d->aux2.ensure(l.px));
        HIP_TRY(launch_morph_unpack(bobst, 1, H, W, l.pitch, d->aux2.as<uint8_t>(), s));
        HIP_TRY(hipMemcpy2DAsync(obstacles, W, d->aux2.p, l.pitch, W, H, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipMemcpyAsync(info, dinfo, sizeof *info, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (info->n > cap && hull_pts)
        return fail(SV_E_CAP, "capacity %lld < %d hull vertices", (long long)cap, info->n);
    if (hull_pts && info->n > 0) {
        HIP_TRY(hipMemcpyAsync(hull_pts, dpts, sizeof(int32_t) * 2 * (size_t)info->n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return SV_OK;
}

int sv_min_circle_centre(const int32_t* pts, int64_t n, int32_t* out_xy) {
    if (!pts || !out_xy || n < 1 || n > kCircleMaxPoints)
        return fail(SV_E_ARG, "sv_min_circle_centre: bad arguments (1 <= n <= %d)", kCircleMaxPoints);
    for (int64_t i = 0; i < 2 * n; ++i)
        if (pts[i] < -kHullMaxCoord || pts[i] > kHullMaxCoord)
            return fail(SV_E_RANGE, "sv_min_circle_centre: coordinate %d outside +-%d", pts[i], kHullMaxCoord);
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    HIP_TRY(d->xy.ensure(sizeof(int32_t) * 2 * (size_t)n));
    HIP_TRY(d->hull.ensure(16));
    HIP_TRY(hipMemcpyAsync(d->xy.p, pts, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_min_circle(d->xy.as<int32_t>(), n, d->hull.as<int32_t>(), s));
    int32_t out[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(out, d->hull.p, sizeof out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (!out[2]) return fail(SV_E_DEVICE, "sv_min_circle_centre: the circle's iteration did not end");
    out_xy[0] = out[0];
    out_xy[1] = out[1];
    return SV_OK;
}

int sv_batch_road_hull(sv_batch* b, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (int rc = need_level(b, kRoadCleaned, "no current road clean-up (sv_batch_road_clean first)")) return rc;
    if (b->H < 1 || b->H > kHullMaxH) return fail(SV_E_ARG, "the obstacle stage takes frames of 1..4096 rows");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    hipEvent_t* hev;
    HIP_TRY(stage_events(b, kEvHull, 2, &hev));
    b->road_level = kRoadCleaned;
    b->olist_fresh = false;   // the obstacle list (rt_objects.hip) is of the bitmaps about to be overwritten
    b->ggrid_fresh = false;   // ... and so is the ground grid (rt_ground.hip)
    const HullLayout l = hull_layout(b->H, b->Wu, b->frames, false);
    HIP_TRY(b->hbuf.ensure(l.bytes));
    char* base = b->hbuf.as<char>();
    HIP_TRY(hipEventRecord(hev[0], s));
    HIP_TRY(launch_road_hull(b->cbits.as<uint32_t>(), b->frames, b->H, b->Wu, b->disp.as<uint8_t>(),
                             (int64_t)b->H * b->W, b->W, b->hull_planes, b->hull_plane_stride, b->hull_shared,
                             reinterpret_cast<int32_t*>(base + l.off_pts),
                             reinterpret_cast<uint32_t*>(base + l.off_mask),
                             reinterpret_cast<uint32_t*>(base + l.off_obst),
                             reinterpret_cast<sv_hull_info*>(base + l.off_info), s));
    HIP_TRY(hipEventRecord(hev[1], s));
    b->road_level = kRoadObstacles;
    if (sync) HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_road_hull_ms(sv_batch* b, float* ms) {
    if (!b || !ms) return fail(SV_E_ARG, "null batch or ms");
    if (int rc = need_level(b, kRoadObstacles, "no obstacle stage (sv_batch_road_hull first)")) return rc;
    HIP_TRY(hipSetDevice(b->device));
    const hipEvent_t* hev = b->road_ev + kEvHull;
    HIP_TRY(hipEventSynchronize(hev[1]));
    HIP_TRY(hipEventElapsedTime(ms, hev[0], hev[1]));
    return SV_OK;
}

int sv_batch_read_road_hull(sv_batch* b, int frame, int32_t* hull_pts, int64_t cap, uint8_t* hull_mask,
                            uint8_t* obstacles, sv_hull_info* info) {
    if (!b || frame < 0 || frame >= b->frames || cap < 0) return fail(SV_E_ARG, "bad args");
    if (int rc = need_level(b, kRoadObstacles, "no obstacle stage (sv_batch_road_hull first)")) return rc;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    const HullLayout l = hull_layout(b->H, b->Wu, b->frames, false);
    const char* base = b->hbuf.as<char>();
    const size_t px = (size_t)b->H * b->W;
    uint8_t* imgs[2] = {hull_mask, obstacles};
    const size_t offs[2] = {l.off_mask, l.off_obst};
    if (hull_mask || obstacles) HIP_TRY(b->rdbuf.ensure(2 * px));
    for (int k = 0; k < 2; ++k)
        if (imgs[k])
            HIP_TRY(launch_morph_unpack(reinterpret_cast<const uint32_t*>(base + offs[k]) + l.words * frame, 1, b->H,
                                        b->Wu, b->W, b->rdbuf.as<uint8_t>() + px * k, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 2; ++k)
        if (imgs[k])
            HIP_TRY(hipMemcpy2D(imgs[k], b->Wu, b->rdbuf.as<uint8_t>() + px * k, b->W, b->Wu, b->H,
                                hipMemcpyDeviceToHost));
    sv_hull_info hi;
    HIP_TRY(hipMemcpy(&hi, reinterpret_cast<const sv_hull_info*>(base + l.off_info) + frame, sizeof hi,
                      hipMemcpyDeviceToHost));
    if (info) *info = hi;
    if (hull_pts) {
        if (hi.n > cap) return fail(SV_E_CAP, "capacity %lld < %d hull vertices", (long long)cap, hi.n);
        if (hi.n > 0)
            HIP_TRY(hipMemcpy(hull_pts, reinterpret_cast<const int32_t*>(base + l.off_pts) + 4 * (size_t)b->H * frame,
                              sizeof(int32_t) * 2 * (size_t)hi.n, hipMemcpyDeviceToHost));
    }
    return SV_OK;
}

// ---------------------------------------------------------------------------
// the result image (stereovision.py:181-209, functions.py:390-394, :424-431): kernels/result.hip
// ---------------------------------------------------------------------------
int sv_result_image(const uint8_t* bgr, const uint8_t* obstacles, const int32_t* hull_pts, int64_t n,
                    const sv_hull_info* info, int H, int W, uint8_t* out) {
    if (const char* why = result_check_args(bgr, obstacles, hull_pts, n, info, H, W, out))
        return fail(SV_E_ARG, "sv_result_image: bad arguments (%s)", why);
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    const ResultLayout l = result_layout(H, W, n);
    HIP_TRY(d->res.ensure(l.bytes));
    HIP_TRY(d->bgr.ensure(l.img));
    char* base = d->res.as<char>();
    uint32_t* bits = reinterpret_cast<uint32_t*>(base + l.off_bits);
    int32_t* dpts = reinterpret_cast<int32_t*>(base + l.off_pts);
    sv_hull_info* dinfo = reinterpret_cast<sv_hull_info*>(base + l.off_info);
    sv_hull_info hi = info ? *info : sv_hull_info{0, 0, 0, 0, 0, 0};
    hi.n = (int32_t)n;
    // the BGR at the batch's stride (pad columns zero), the obstacles as a bitmap
    if (l.pitch != W) HIP_TRY(hipMemsetAsync(d->bgr.p, 0, l.img, s));
    HIP_TRY(hipMemcpy2DAsync(d->bgr.p, l.ld3, bgr, 3 * (size_t)W, 3 * (size_t)W, H, hipMemcpyHostToDevice, s));
    if (int rc = upload_u8(d->aux, obstacles, H, W, l.pitch, s)) return rc;
    HIP_TRY(launch_morph_pack(d->aux.as<uint8_t>(), (int64_t)H * l.pitch, l.pitch, W, H, 1, bits, s));
    if (n > 0) HIP_TRY(hipMemcpyAsync(dpts, hull_pts, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(dinfo, &hi, sizeof hi, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_result(d->bgr.as<uint8_t>(), (int64_t)l.img, l.ld3, bits, dpts, 0, dinfo, 1, H, W,
                          reinterpret_cast<uint8_t*>(base + l.off_out), s));
    HIP_TRY(hipMemcpy2DAsync(out, 3 * (size_t)W, base + l.off_out, l.ld3, 3 * (size_t)W, H, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_result(sv_batch* b, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (!b->with_bgr) return fail(SV_E_STATE, "the result image needs the batch's BGR (with_bgr)");
    if (int rc = need_level(b, kRoadObstacles, "no current obstacle stage (sv_batch_road_hull first)")) return rc;
    if (b->H > kResultMaxH || b->Wu > kResultMaxW)
        return fail(SV_E_ARG, "the result image takes frames of at most 4096 x 4096");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    hipEvent_t* rev;
    HIP_TRY(stage_events(b, kEvResult, 2, &rev));
    b->road_level = kRoadObstacles;
    const size_t px3 = (size_t)b->H * b->W * 3;
    HIP_TRY(b->rimg.ensure(px3 * b->frames, false, 0, true));   // a buffer of its own: the pipeline reads the BGR
    const HullLayout l = hull_layout(b->H, b->Wu, b->frames, false);
    const char* base = b->hbuf.as<char>();
    HIP_TRY(hipEventRecord(rev[0], s));
    // probe (tools/_probe_result.py; the picture is NOT made): the floor of this traffic, a device copy of the BGR
    // into the result buffer between the same events
    const char* copy_only = svx_knob("SVX_RESULT_COPY");
    if (copy_only && *copy_only == '1') {
        HIP_TRY(hipMemcpyAsync(b->rimg.p, b->bgr.p, px3 * b->frames, hipMemcpyDeviceToDevice, s));
    } else {
        HIP_TRY(launch_result(b->bgr.as<uint8_t>(), (int64_t)px3, 3 * b->W,
                              reinterpret_cast<const uint32_t*>(base + l.off_obst),
                              reinterpret_cast<const int32_t*>(base + l.off_pts), 4 * (int64_t)b->H,
                              reinterpret_cast<const sv_hull_info*>(base + l.off_info), b->frames, b->H, b->Wu,
                              b->rimg.as<uint8_t>(), s));
    }
    HIP_TRY(hipEventRecord(rev[1], s));
    b->road_level = kRoadResult;
    if (sync) HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_result_ms(sv_batch* b, float* ms) {
    if (!b || !ms) return fail(SV_E_ARG, "null batch or ms");
    if (int rc = need_level(b, kRoadResult, "no result image (sv_batch_result first)")) return rc;
    HIP_TRY(hipSetDevice(b->device));
    const hipEvent_t* rev = b->road_ev + kEvResult;
    HIP_TRY(hipEventSynchronize(rev[1]));
    HIP_TRY(hipEventElapsedTime(ms, rev[0], rev[1]));
    return SV_OK;
}

int sv_batch_read_result(sv_batch* b, int frame, uint8_t* out) {
    if (!b || !out || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    if (int rc = need_level(b, kRoadResult, "no result image (sv_batch_result first)")) return rc;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const size_t px3 = (size_t)b->H * b->W * 3;
    HIP_TRY(hipMemcpy2D(out, (size_t)b->Wu * 3, b->rimg.as<uint8_t>() + px3 * frame, (size_t)b->W * 3,
                        (size_t)b->Wu * 3, b->H, hipMemcpyDeviceToHost));
    return SV_OK;
}

// ---------------------------------------------------------------------------
// the image tile (stereovision.py:216, functions.py:452-499 batchImages): kernels/tile.hip
// ---------------------------------------------------------------------------
int sv_image_tile(const uint8_t* disparity, const uint8_t* bgr, const uint8_t* road, const uint8_t* cleaned,
                  const uint8_t* result, int H, int W, uint8_t* out) {
    if (const char* why = tile_check_args(disparity, bgr, road, cleaned, result, H, W, out))
        return fail(SV_E_ARG, "sv_image_tile: bad arguments (%s)", why);
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    const TileLayout l = tile_layout(H, W);
    HIP_TRY(d->tile.ensure(l.bytes));
    HIP_TRY(d->bgr.ensure(l.img));
    uint8_t* base = d->tile.as<uint8_t>();
    // the u8 pictures at the staging stride, the BGR and the result at the batch's (pad columns zero)
    if (int rc = upload_u8(d->disp, disparity, H, W, l.pitch, s)) return rc;
    if (int rc = upload_u8(d->aux, road, H, W, l.pitch, s)) return rc;
    if (int rc = upload_u8(d->aux2, cleaned, H, W, l.pitch, s)) return rc;
    if (l.pitch != W) {
        HIP_TRY(hipMemsetAsync(d->bgr.p, 0, l.img, s));
        HIP_TRY(hipMemsetAsync(base + l.off_res, 0, l.img, s));
    }
    HIP_TRY(hipMemcpy2DAsync(d->bgr.p, l.ld3, bgr, 3 * (size_t)W, 3 * (size_t)W, H, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpy2DAsync(base + l.off_res, l.ld3, result, 3 * (size_t)W, 3 * (size_t)W, H, hipMemcpyHostToDevice,
                             s));
    TileArgs a{};
    a.disp = TilePlane{d->disp.p, 0, l.pitch};
    a.bgr = TilePlane{d->bgr.p, 0, l.ld3};
    a.road = TilePlane{d->aux.p, 0, l.pitch};
    a.clean = TilePlane{d->aux2.p, 0, l.pitch};
    a.res = TilePlane{base + l.off_res, 0, l.ld3};
    a.H = H;
    a.W = W;
    HIP_TRY(launch_tile(a, 1, base + l.off_out, s));
    HIP_TRY(hipMemcpyAsync(out, base + l.off_out, tile_frame_bytes(H, W), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_tile(sv_batch* b, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (!b->with_bgr) return fail(SV_E_STATE, "the image tile needs the batch's BGR (with_bgr)");
    if (const char* why = tile_check_shape(b->H, b->Wu))
        return fail(SV_E_ARG, "the image tile takes frames with %s (the batch's are %d x %d)", why, b->H, b->Wu);
    if (int rc = need_level(b, kRoadResult, "no current result image (sv_batch_result first)")) return rc;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    hipEvent_t* tev;
    HIP_TRY(stage_events(b, kEvTile, 2, &tev));
    b->road_level = kRoadResult;
    const int H = b->H, WW = (b->Wu + 31) / 32;
    const int64_t px = (int64_t)H * b->W;
    HIP_TRY(b->timg.ensure(tile_frame_bytes(H, b->Wu) * b->frames, false, 0, true));
    TileArgs a{};
    a.disp = TilePlane{b->disp.p, px, b->W};
    a.bgr = TilePlane{b->bgr.p, 3 * px, 3 * b->W};
    a.res = TilePlane{b->rimg.p, 3 * px, 3 * b->W};
    // the two pictures of 0 and 255 from the packed bitmaps where the batch holds current ones: the clean-up's
    // always, the pipeline's own (32 words a row) when it wrote one for the current points
    if (b->rbits_fresh && b->Wu == 1024) a.rbits = TilePlane{b->rbits.p, 32 * (int64_t)H, 32};
    else a.road = TilePlane{b->road.p, px, b->W};
    a.cbits = TilePlane{b->cbits.p, (int64_t)H * WW, WW};
    a.H = H;
    a.W = b->Wu;
    HIP_TRY(hipEventRecord(tev[0], s));
    HIP_TRY(launch_tile(a, b->frames, b->timg.as<uint8_t>(), s));
    HIP_TRY(hipEventRecord(tev[1], s));
    b->road_level = kRoadTile;
    if (sync) HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_tile_ms(sv_batch* b, float* ms) {
    if (!b || !ms) return fail(SV_E_ARG, "null batch or ms");
    if (int rc = need_level(b, kRoadTile, "no image tile (sv_batch_tile first)")) return rc;
    HIP_TRY(hipSetDevice(b->device));
    const hipEvent_t* tev = b->road_ev + kEvTile;
    HIP_TRY(hipEventSynchronize(tev[1]));
    HIP_TRY(hipEventElapsedTime(ms, tev[0], tev[1]));
    return SV_OK;
}

int sv_batch_read_tile(sv_batch* b, int frame, uint8_t* out) {
    if (!b || !out || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    if (int rc = need_level(b, kRoadTile, "no image tile (sv_batch_tile first)")) return rc;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const size_t bytes = tile_frame_bytes(b->H, b->Wu);
    HIP_TRY(hipMemcpy(out, b->timg.as<uint8_t>() + bytes * frame, bytes, hipMemcpyDeviceToHost));
    return SV_OK;
}

}  // extern "C"
