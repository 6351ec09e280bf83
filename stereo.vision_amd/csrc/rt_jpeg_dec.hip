// svx runtime: the MJPG playback's JPEG decoder (kernels/jpeg_dec.hip) as host-picture entry points
// (one stream, or a packed run of streams in one upload and one read-back) and as a batch's input stage, which
// decodes stereo pairs into the storage sv_batch_upload_bgr_pair fills. The host parser (svx_jpeg_dec_host.h) accepts
// or refuses every stream before anything is launched.
#include "svx_jpeg_dec.h"
#include "svx_runtime.h"

namespace {

size_t up16(size_t v) { return (v + 15) / 16 * 16; }

// The streams of one launch, parsed: what goes to the device in front of their bytes.
struct DecodePlan {
    std::vector<JpegDecFrame> frames;
    std::vector<JpegDecTables> tabs;
    std::vector<JpegDecQuant> quant;
    int maxi = 1;
    int64_t total = 0;   // bytes of the packed streams
    size_t off_tabs = 0, off_quant = 0, off_status = 0, off_packed = 0, bytes = 0;
    std::vector<uint8_t> blob;   // frames | tabs | quant as they lie on the device
};

// offsets: count + 1 ascending positions in packed. SV_E_ARG (with the stream's index and what was met) unless every
// stream is of the accepted kind and h x w.
int plan_streams(const char* who, const uint8_t* packed, const int64_t* offsets, int count, int h, int w,
                 DecodePlan* p) {
    p->frames.resize((size_t)count);
    p->total = offsets[count] - offsets[0];
    for (int f = 0; f < count; ++f) {
        const int64_t at = offsets[f], n = offsets[f + 1] - at;
        if (n < 0) return fail(SV_E_ARG, "%s: offsets must ascend (stream %d)", who, f);
        JpegDecHeader hd;
        JpegDecTables t;
        JpegDecQuant q;
        if (const char* why = jpeg_dec_parse(packed + at, n, &hd, &t, &q))
            return fail(SV_E_ARG, "%s: stream %d is outside the accepted kind: %s", who, f, why);
        if (hd.h != h || hd.w != w)
            return fail(SV_E_ARG, "%s: stream %d is %d x %d, not %d x %d", who, f, hd.h, hd.w, h, w);
        if (p->tabs.empty() || memcmp(&t, &p->tabs.back(), sizeof t) || memcmp(&q, &p->quant.back(), sizeof q)) {
            p->tabs.push_back(t);
            p->quant.push_back(q);
        }
        p->frames[(size_t)f] = JpegDecFrame{at - offsets[0], (int32_t)n, hd.scan_at, hd.intervals, hd.per,
                                            (int32_t)p->tabs.size() - 1, 0};
        p->maxi = std::max(p->maxi, hd.intervals);
    }
    const size_t nf = sizeof(JpegDecFrame) * (size_t)count, nt = sizeof(JpegDecTables) * p->tabs.size();
    const size_t nq = sizeof(JpegDecQuant) * p->quant.size();
    p->off_tabs = up16(nf);
    p->off_quant = p->off_tabs + up16(nt);
    p->off_status = p->off_quant + up16(nq);
    p->off_packed = p->off_status + up16(sizeof(int32_t) * (size_t)count);
    p->bytes = p->off_packed + up16((size_t)p->total);
    p->blob.assign(p->off_status, 0);
    memcpy(p->blob.data(), p->frames.data(), nf);
    memcpy(p->blob.data() + p->off_tabs, p->tabs.data(), nt);
    memcpy(p->blob.data() + p->off_quant, p->quant.data(), nq);
    return SV_OK;
}

// Uploads the plan and its streams into `in`, decodes chunk by chunk through `work` into out_d (frame f at
// out_d + f * frame_stride, rows ld apart) on stream s and waits; status_h[count]. ms4 (nullable): the four kernels'
// ms, added up over the chunks.
int run_plan(const DecodePlan& p, const uint8_t* packed_h, int h, int w, DevBuf& in, DevBuf& work, uint8_t* out_d,
             int64_t frame_stride, int64_t ld, int32_t* status_h, hipStream_t s, float* ms4) {
    const int count = (int)p.frames.size();
    HIP_TRY(in.ensure(p.bytes));
    char* base = in.as<char>();
    HIP_TRY(hipMemcpyAsync(base, p.blob.data(), p.blob.size(), hipMemcpyHostToDevice, s));
    if (p.total) HIP_TRY(hipMemcpyAsync(base + p.off_packed, packed_h, (size_t)p.total, hipMemcpyHostToDevice, s));
    // the scratch is 3.5 B a pixel: the frames go through it in chunks of at most 1 GiB and half the free memory,
    // at least a frame
    size_t fr = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&fr, &tot));
    const size_t per = jpeg_dec_work_frame_bytes(h, w, p.maxi) + 64;
    const size_t budget = std::max(work.bytes, std::min<size_t>((size_t)1 << 30, fr / 2));
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)count, budget / per));
    const JpegDecWorkLayout wl = jpeg_dec_work_layout(h, w, p.maxi, chunk);
    HIP_TRY(work.ensure(wl.bytes, false, 0, true));
    char* wb = work.as<char>();
    const JpegDecWork wk{reinterpret_cast<int16_t*>(wb + wl.off_coef), reinterpret_cast<uint8_t*>(wb + wl.off_chroma),
                         reinterpret_cast<int32_t*>(wb + wl.off_first), reinterpret_cast<int32_t*>(wb + wl.off_end)};
    hipEvent_t ev[5] = {};
    if (ms4) {
        for (int i = 0; i < 4; ++i) ms4[i] = 0;
        for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    }
    int rc = SV_OK;
    const JpegDecFrame* fr_d = reinterpret_cast<const JpegDecFrame*>(base);
    int32_t* status_d = reinterpret_cast<int32_t*>(base + p.off_status);
    for (int f0 = 0; f0 < count && rc == SV_OK; f0 += chunk) {
        const int n = std::min(chunk, count - f0);
        hipError_t e = launch_jpeg_decode(reinterpret_cast<const uint8_t*>(base + p.off_packed), fr_d + f0,
                                          reinterpret_cast<const JpegDecTables*>(base + p.off_tabs),
                                          reinterpret_cast<const JpegDecQuant*>(base + p.off_quant), n, h, w, p.maxi, wk,
                                          out_d + (int64_t)f0 * frame_stride, frame_stride, ld, status_d + f0, s,
                                          ms4 ? ev : nullptr);
        if (e == hipSuccess && ms4) {   // the events are used again by the next chunk
            e = hipStreamSynchronize(s);
            for (int i = 0; i < 4 && e == hipSuccess; ++i) {
                float t = 0;
                e = hipEventElapsedTime(&t, ev[i], ev[i + 1]);
                ms4[i] += t;
            }
        }
        if (e != hipSuccess) rc = fail(SV_E_HIP, "the JPEG decoder's launch failed: %s", hipGetErrorString(e));
    }
    if (ms4)
        for (auto& e : ev) (void)hipEventDestroy(e);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(status_h, status_d, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

}  // namespace

extern "C" {

int sv_jpeg_info(const uint8_t* stream, int64_t n, sv_jpeg_desc* desc) {
    if (!stream || !desc) return fail(SV_E_ARG, "sv_jpeg_info: null pointer");
    JpegDecHeader hd;
    if (const char* why = jpeg_dec_parse(stream, n, &hd, nullptr, nullptr))
        return fail(SV_E_ARG, "sv_jpeg_info: the stream is outside the accepted kind: %s", why);
    desc->h = hd.h;
    desc->w = hd.w;
    desc->restart_interval = hd.ri;
    desc->header_len = hd.scan_at;
    return SV_OK;
}

int sv_jpeg_decode(const uint8_t* stream, int64_t n, uint8_t* bgr_out, int h, int w, int64_t ld, int32_t* status) {
    if (!stream || !bgr_out || !status) return fail(SV_E_ARG, "sv_jpeg_decode: null pointer");
    if (h < 1 || h > kJpegMaxDim || w < 1 || w > kJpegMaxDim || ld < 3 * (int64_t)w)
        return fail(SV_E_ARG, "sv_jpeg_decode: 1 <= h, w <= 4096 and ld >= 3 w bytes");
    if (n < 0) return fail(SV_E_ARG, "sv_jpeg_decode: n < 0");
    *status = 0;
    const int64_t offsets[2] = {0, n};
    DecodePlan p;
    if (int rc = plan_streams("sv_jpeg_decode", stream, offsets, 1, h, w, &p)) return rc;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    const size_t ld16 = up16(3 * (size_t)w);
    HIP_TRY(d->jdout.ensure(ld16 * (size_t)h));
    if (int rc = run_plan(p, stream, h, w, d->jdin, d->jdwork, d->jdout.as<uint8_t>(), (int64_t)(ld16 * (size_t)h),
                          (int64_t)ld16, status, d->stream, nullptr))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(bgr_out, (size_t)ld, d->jdout.p, ld16, 3 * (size_t)w, h, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return SV_OK;
}

int sv_jpeg_decode_many(int device, const uint8_t* packed, const int64_t* offsets, int count, int h, int w,
                        uint8_t* out, int32_t* status) {
    if (!packed || !offsets || !out || !status) return fail(SV_E_ARG, "sv_jpeg_decode_many: null pointer");
    if (count < 1 || h < 1 || h > kJpegMaxDim || w < 1 || w > kJpegMaxDim)
        return fail(SV_E_ARG, "sv_jpeg_decode_many: count >= 1 and 1 <= h, w <= 4096");
    DecodePlan p;
    if (int rc = plan_streams("sv_jpeg_decode_many", packed, offsets, count, h, w, &p)) return rc;
    Locked L;
    if (int rc = lock_device(device, L)) return rc;
    Device* d = L.d;
    const size_t pic = (size_t)h * w * 3;
    HIP_TRY(d->jdout.ensure(up16(pic * (size_t)count), false, 0, true));
    d->jd_have_ms = false;
    if (int rc = run_plan(p, packed + offsets[0], h, w, d->jdin, d->jdwork, d->jdout.as<uint8_t>(), (int64_t)pic,
                          3 * (int64_t)w, status, d->stream, d->jd_ms))
        return rc;
    d->jd_have_ms = true;
    HIP_TRY(hipMemcpyAsync(out, d->jdout.p, pic * (size_t)count, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return SV_OK;
}

int sv_jpeg_decode_stage_ms(int device, float* ms4) {
    if (!ms4) return fail(SV_E_ARG, "sv_jpeg_decode_stage_ms: null pointer");
    Locked L;
    if (int rc = lock_device(device, L)) return rc;
    if (!L.d->jd_have_ms) return fail(SV_E_STATE, "no sv_jpeg_decode_many has run on device %d", device);
    for (int i = 0; i < 4; ++i) ms4[i] = L.d->jd_ms[i];
    return SV_OK;
}

int sv_batch_decode_bgr_pair(sv_batch* b, int first, int count, const uint8_t* packedL, const int64_t* offsL,
                             const uint8_t* packedR, const int64_t* offsR, int32_t* status) {
    if (!b || !packedL || !offsL || !packedR || !offsR || !status)
        return fail(SV_E_ARG, "sv_batch_decode_bgr_pair: null pointer");
    if (first < 0 || count < 1 || first > b->frames - count)
        return fail(SV_E_ARG, "sv_batch_decode_bgr_pair: frames [%d, %d + %d) outside the batch's %d", first, first,
                    count, b->frames);
    const int H = b->pairH ? b->pairH : b->H, W = b->pairW ? b->pairW : b->Wu;
    if (W % 8) return fail(SV_E_ARG, "batched SGBM needs W %% 8 == 0 (W=%d)", W);
    DecodePlan pl, pr;
    if (int rc = plan_streams("sv_batch_decode_bgr_pair (left)", packedL, offsL, count, H, W, &pl)) return rc;
    if (int rc = plan_streams("sv_batch_decode_bgr_pair (right)", packedR, offsR, count, H, W, &pr)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    const size_t px3 = (size_t)H * W * 3;
    pair_store_written(b);
    HIP_TRY(b->bgrL.ensure(px3 * b->frames));
    HIP_TRY(b->bgrR.ensure(px3 * b->frames));
    b->jd_have_ms = false;
    float ms[2][4];
    if (int rc = run_plan(pl, packedL + offsL[0], H, W, b->jdin, b->jdwork, b->bgrL.as<uint8_t>() + px3 * first,
                          (int64_t)px3, 3 * (int64_t)W, status, b->stream, ms[0]))
        return rc;
    if (int rc = run_plan(pr, packedR + offsR[0], H, W, b->jdin, b->jdwork, b->bgrR.as<uint8_t>() + px3 * first,
                          (int64_t)px3, 3 * (int64_t)W, status + count, b->stream, ms[1]))
        return rc;
    b->jd_ms = 0;
    for (int i = 0; i < 4; ++i) b->jd_ms += ms[0][i] + ms[1][i];
    b->jd_have_ms = true;
    return SV_OK;
}

int sv_batch_decode_ms(sv_batch* b, float* ms) {
    if (!b || !ms) return fail(SV_E_ARG, "null batch or ms");
    if (!b->jd_have_ms) return fail(SV_E_STATE, "no sv_batch_decode_bgr_pair has run on this batch");
    *ms = b->jd_ms;
    return SV_OK;
}

int sv_batch_read_bgr_pair(sv_batch* b, int frame, uint8_t* L, uint8_t* R) {
    if (!b || !L || !R || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "sv_batch_read_bgr_pair: bad args");
    const int H = b->pairH ? b->pairH : b->H, W = b->pairW ? b->pairW : b->Wu;
    const size_t px3 = (size_t)H * W * 3;
    if (b->bgrL.bytes < px3 * b->frames || b->bgrR.bytes < px3 * b->frames)
        return fail(SV_E_STATE, "no BGR pairs (sv_batch_synth_bgr_pair / upload_bgr_pair / decode_bgr_pair)");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(L, b->bgrL.as<uint8_t>() + px3 * frame, px3, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(R, b->bgrR.as<uint8_t>() + px3 * frame, px3, hipMemcpyDeviceToHost));
    return SV_OK;
}

}  // extern "C"
