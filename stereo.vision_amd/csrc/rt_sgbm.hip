// svx runtime: the disparity stage. StereoSGBM, the speckle filter and the grey pre-processing as host-frame
// drop-ins, and the batched SGBM over a batch's stereo pairs.
#include <cstring>

#include "svx_runtime.h"

extern "C" {

// ---------------------------------------------------------------------------
// disparity stage (functions.py:61-128)
// ---------------------------------------------------------------------------
namespace {
// StereoSGBM parameters with OpenCV's substitutions for zero / negative values
// (computeDisparitySGBM): P1 -> 2, P2 -> max(5, P1 + 1), preFilterCap ->
// max(cap, 15) | 1, uniquenessRatio < 0 -> 10, disp12MaxDiff <= 0 -> 1.
int make_sgbm(int H, int W, const sv_sgbm_params* prm, int max_disparity, int crop, SgbmK* k) {
    if (!prm) return fail(SV_E_ARG, "null sgbm params");
    if (prm->min_disp != 0) return fail(SV_E_ARG, "minDisparity must be 0 (got %d)", prm->min_disp);
    if (prm->num_disp != kSgD) return fail(SV_E_ARG, "numDisparities must be %d (got %d)", kSgD, prm->num_disp);
    const int SW = prm->block > 0 ? prm->block : 5;
    if (SW % 2 == 0 || SW > 63) return fail(SV_E_ARG, "blockSize must be odd and <= 63 (got %d)", SW);
    if (max_disparity < 1) return fail(SV_E_ARG, "max_disparity must be >= 1");
    std::memset(k, 0, sizeof *k);
    k->H = H;
    k->W = W;
    k->minX1 = kSgD;
    k->width1 = W - kSgD;
    k->SW2 = k->SH2 = SW / 2;
    k->P1 = prm->P1 > 0 ? prm->P1 : 2;
    k->P2 = std::max(prm->P2 > 0 ? prm->P2 : 5, k->P1 + 1);
    k->ftzero = std::max(prm->prefilter_cap, 15) | 1;
    k->uniq = prm->uniqueness >= 0 ? prm->uniqueness : 10;
    k->d12 = prm->disp12_max_diff > 0 ? prm->disp12_max_diff : 1;
    k->frame_px = (int64_t)H * W;
    // functions.py:111 filterSpeckles(disparity, 0, 4000, max_disparity - 5)
    k->new_val = 0;
    k->max_size = 4000;
    k->max_diff = max_disparity - 5;
    k->out_rows = crop ? std::min(390, H) : H;
    k->out_cols = crop ? std::max(W - 135, 0) : W;
    k->out_c0 = crop ? 135 : 0;
    k->out_stride = k->out_cols;
    k->scale = 256. / max_disparity;
    if (H < 1 || W <= kSgD || !sgbm_supported(*k))
        return fail(SV_E_ARG, "SGBM needs 1 <= H, %d + blockSize/2 < W <= 2048 (H=%d W=%d)", kSgD, H, W);
    return SV_OK;
}

int sgbm_check_flags(const uint32_t* flags, int n, hipStream_t s) {
    std::vector<uint32_t> fl(n);
    HIP_TRY(hipMemcpyAsync(fl.data(), flags, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i)
        if (fl[i])
            return fail(SV_E_RANGE, "SGBM frame %d: a path cost left the int16 range (block cost sums above "
                                    "32,763: unsupported)", i);
    return SV_OK;
}

// upload a grey pair (or take the device's copies) and run StereoSGBM.compute into d->sg.d16
int sgbm_frame(Device* d, const uint8_t* L, const uint8_t* R, const SgbmK& k) {
    const size_t px = (size_t)k.frame_px;
    hipStream_t s = d->stream;
    HIP_TRY(d->sg_l.ensure(px));
    HIP_TRY(d->sg_r.ensure(px));
    HIP_TRY(d->sg.ensure(k, 1));
    HIP_TRY(hipMemcpyAsync(d->sg_l.p, L, px, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d->sg_r.p, R, px, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_sgbm_compute(k, d->sg_l.as<uint8_t>(), d->sg_r.as<uint8_t>(), 1, d->sg.scratch(), s));
    return sgbm_check_flags(d->sg.flags.as<uint32_t>(), 1, s);
}
}  // namespace

int sv_lut_u8(const uint8_t* in, int64_t n, const uint8_t* lut, uint8_t* out) {
    if (n < 0 || (n > 0 && (!in || !out)) || !lut) return fail(SV_E_ARG, "sv_lut_u8: bad arguments");
    if (n == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    HIP_TRY(d->sg_l.ensure((size_t)n));
    HIP_TRY(d->sg_hist.ensure(256));
    HIP_TRY(hipMemcpyAsync(d->sg_l.p, in, (size_t)n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d->sg_hist.p, lut, 256, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_lut(d->sg_l.as<uint8_t>(), n, d->sg_hist.as<uint8_t>(), d->sg_l.as<uint8_t>(), s));
    HIP_TRY(hipMemcpyAsync(out, d->sg_l.p, (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_grey_equalize(const uint8_t* bgr, int H, int W, uint8_t* out) {
    if (!bgr || !out || H < 0 || W < 0) return fail(SV_E_ARG, "sv_grey_equalize: bad arguments");
    const int64_t px = (int64_t)H * W;
    if (px == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    HIP_TRY(d->sg_l.ensure((size_t)px * 3));
    HIP_TRY(d->sg_r.ensure((size_t)px));
    HIP_TRY(d->sg_hist.ensure(sizeof(uint32_t) * 256));
    HIP_TRY(hipMemcpyAsync(d->sg_l.p, bgr, (size_t)px * 3, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_grey_equalize(d->sg_l.as<uint8_t>(), px, 1, d->sg_r.as<uint8_t>(), d->sg_hist.as<uint32_t>(), s));
    HIP_TRY(hipMemcpyAsync(out, d->sg_r.p, (size_t)px, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_sgbm_compute(const uint8_t* L, const uint8_t* R, int H, int W, const sv_sgbm_params* prm, int16_t* out) {
    if (!L || !R || !out) return fail(SV_E_ARG, "sv_sgbm_compute: null buffer");
    SgbmK k;
    if (int rc = make_sgbm(H, W, prm, kSgD, 0, &k)) return rc;
    Locked lk;
    if (int rc = lock_current(lk)) return rc;
    Device* d = lk.d;
    if (int rc = sgbm_frame(d, L, R, k)) return rc;
    HIP_TRY(hipMemcpyAsync(out, d->sg.d16.p, sizeof(int16_t) * k.frame_px, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return SV_OK;
}

int sv_filter_speckles(int16_t* img, int H, int W, int new_val, int max_size, int max_diff) {
    if (!img || H < 0 || W < 0) return fail(SV_E_ARG, "sv_filter_speckles: bad arguments");
    const int64_t px = (int64_t)H * W;
    if (px == 0) return SV_OK;
    if (px > INT32_MAX) return fail(SV_E_ARG, "sv_filter_speckles: image too large");
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    SgbmK k;
    std::memset(&k, 0, sizeof k);
    k.H = H;
    k.W = W;
    k.frame_px = px;
    k.new_val = new_val;
    k.max_size = max_size;
    k.max_diff = max_diff;
    k.out_rows = 0;   // no scaled output
    k.scale = 1;
    HIP_TRY(d->sg.d16.ensure(sizeof(int16_t) * px));
    HIP_TRY(d->sg.par.ensure(sizeof(int32_t) * px));
    HIP_TRY(d->sg.size.ensure(sizeof(int32_t) * px));
    HIP_TRY(d->sg_filt.ensure(sizeof(int16_t) * px));
    HIP_TRY(hipMemcpyAsync(d->sg.d16.p, img, sizeof(int16_t) * px, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_speckle_scale(k, 1, d->sg.scratch(), nullptr, d->sg_filt.as<int16_t>(), s));
    HIP_TRY(hipMemcpyAsync(img, d->sg_filt.p, sizeof(int16_t) * px, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_disparity(const uint8_t* L, const uint8_t* R, int H, int W, const sv_sgbm_params* prm, int max_disparity,
                 int crop, uint8_t* out, int16_t* raw16, int16_t* filt16) {
    if (!L || !R || !out) return fail(SV_E_ARG, "sv_disparity: null buffer");
    SgbmK k;
    if (int rc = make_sgbm(H, W, prm, max_disparity, crop, &k)) return rc;
    Locked lk;
    if (int rc = lock_current(lk)) return rc;
    Device* d = lk.d;
    hipStream_t s = d->stream;
    if (int rc = sgbm_frame(d, L, R, k)) return rc;
    if (raw16) HIP_TRY(hipMemcpyAsync(raw16, d->sg.d16.p, sizeof(int16_t) * k.frame_px, hipMemcpyDeviceToHost, s));
    const size_t ob = (size_t)k.out_rows * k.out_cols;
    HIP_TRY(d->sg_out.ensure(ob ? ob : 1));
    if (filt16) HIP_TRY(d->sg_filt.ensure(sizeof(int16_t) * k.frame_px));
    HIP_TRY(launch_speckle_scale(k, 1, d->sg.scratch(), d->sg_out.as<uint8_t>(),
                                 filt16 ? d->sg_filt.as<int16_t>() : nullptr, s));
    if (ob) HIP_TRY(hipMemcpyAsync(out, d->sg_out.p, ob, hipMemcpyDeviceToHost, s));
    if (filt16) HIP_TRY(hipMemcpyAsync(filt16, d->sg_filt.p, sizeof(int16_t) * k.frame_px, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

// the pairs' shape: the batch's own, unless sv_batch_pair_shape chose the uncropped one
static void pair_shape(const sv_batch* b, int* H, int* W) {
    *H = b->pairH ? b->pairH : b->H;
    *W = b->pairW ? b->pairW : b->Wu;
}

int sv_batch_pair_shape(sv_batch* b, int H, int W) {
    if (!b) return fail(SV_E_ARG, "null batch");
    const bool own = H == b->H && W == b->Wu;
    // functions.py:122-124: disparity_scaled[0:390, 135:W] of an H x W pair
    if (!own && !(W > 135 && W - 135 == b->Wu && std::min(390, H) == b->H))
        return fail(SV_E_ARG, "pair shape %d x %d: the batch (%d x %d) must be the pair's shape or its crop "
                              "[0:390, 135:W]", H, W, b->H, b->Wu);
    if (!own && W % 8) return fail(SV_E_ARG, "batched SGBM needs the pair width %% 8 == 0 (W=%d)", W);
    int h0, w0;
    pair_shape(b, &h0, &w0);
    if (h0 != H || w0 != W) {   // a new shape: the grey and the BGR pairs are uploaded again, and the maps
        for (DevBuf* x : {&b->pairL, &b->pairR, &b->bgrL, &b->bgrR, &b->rawL, &b->rawR, &b->rectmaps}) x->release();
        b->rect_h = b->rect_w = 0;
        b->rect_done = false;
    }
    b->pairH = own ? 0 : H;
    b->pairW = own ? 0 : W;
    return SV_OK;
}

int sv_batch_synth_pair(sv_batch* b, int64_t first_frame_id) {
    if (!b) return fail(SV_E_ARG, "null batch");
    int H, W;
    pair_shape(b, &H, &W);
    if (W % 8) return fail(SV_E_ARG, "batched SGBM needs W %% 8 == 0 (W=%d)", W);
    if (W + kSgD > 4096) return fail(SV_E_ARG, "synthetic pairs need W <= %d", 4096 - kSgD);
    HIP_TRY(hipSetDevice(b->device));
    const size_t px = (size_t)H * W * b->frames;
    HIP_TRY(b->pairL.ensure(px));
    HIP_TRY(b->pairR.ensure(px));
    HIP_TRY(launch_synth_pair(b->pairL.as<uint8_t>(), b->pairR.as<uint8_t>(), H, W, b->frames, first_frame_id,
                              b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_upload_pair(sv_batch* b, int frame, const uint8_t* L, const uint8_t* R) {
    if (!b || !L || !R || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "sv_batch_upload_pair: bad args");
    int H, W;
    pair_shape(b, &H, &W);
    if (W % 8) return fail(SV_E_ARG, "batched SGBM needs W %% 8 == 0 (W=%d)", W);
    HIP_TRY(hipSetDevice(b->device));
    const size_t px = (size_t)H * W;
    HIP_TRY(b->pairL.ensure(px * b->frames));
    HIP_TRY(b->pairR.ensure(px * b->frames));
    HIP_TRY(hipMemcpyAsync(b->pairL.as<uint8_t>() + px * frame, L, px, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->pairR.as<uint8_t>() + px * frame, R, px, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_upload_bgr_pair(sv_batch* b, int frame, const uint8_t* L, const uint8_t* R) {
    if (!b || !L || !R || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "sv_batch_upload_bgr_pair: bad args");
    int H, W;
    pair_shape(b, &H, &W);
    if (W % 8) return fail(SV_E_ARG, "batched SGBM needs W %% 8 == 0 (W=%d)", W);
    HIP_TRY(hipSetDevice(b->device));
    const size_t px3 = (size_t)H * W * 3;
    pair_store_written(b);
    HIP_TRY(b->bgrL.ensure(px3 * b->frames));
    HIP_TRY(b->bgrR.ensure(px3 * b->frames));
    HIP_TRY(hipMemcpyAsync(b->bgrL.as<uint8_t>() + px3 * frame, L, px3, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(b->bgrR.as<uint8_t>() + px3 * frame, R, px3, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_synth_bgr_pair(sv_batch* b, int64_t first_frame_id) {
    if (!b) return fail(SV_E_ARG, "null batch");
    int H, W;
    pair_shape(b, &H, &W);
    if (W % 8) return fail(SV_E_ARG, "batched SGBM needs W %% 8 == 0 (W=%d)", W);
    if (W + kSgD > 4096) return fail(SV_E_ARG, "synthetic pairs need W <= %d", 4096 - kSgD);
    HIP_TRY(hipSetDevice(b->device));
    const size_t px3 = (size_t)H * W * 3 * b->frames;
    pair_store_written(b);
    HIP_TRY(b->bgrL.ensure(px3));
    HIP_TRY(b->bgrR.ensure(px3));
    HIP_TRY(launch_synth_bgr_pair(b->bgrL.as<uint8_t>(), b->bgrR.as<uint8_t>(), H, W, b->frames, first_frame_id,
                                  b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_preprocess(sv_batch* b, const uint8_t* lut, int sync) {
    if (!b || !lut) return fail(SV_E_ARG, "sv_batch_preprocess: bad args");
    if (!b->bgrL.p || !b->bgrR.p) return fail(SV_E_STATE, "no BGR pairs (sv_batch_synth_bgr_pair / upload_bgr_pair)");
    int H, W;
    pair_shape(b, &H, &W);
    const int64_t px = (int64_t)H * W;
    // the BGR pairs must hold every frame at the current pair shape (a partial upload after a shape change
    // would otherwise be read past its allocation)
    if (b->bgrL.bytes < (size_t)px * 3 * b->frames || b->bgrR.bytes < (size_t)px * 3 * b->frames)
        return fail(SV_E_STATE, "BGR pairs hold fewer bytes than %d frames of %d x %d x 3", b->frames, H, W);
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(b->glut.ensure(256));
    HIP_TRY(b->ghist.ensure(sizeof(uint32_t) * 256 * b->frames));
    HIP_TRY(b->pairL.ensure((size_t)px * b->frames));
    HIP_TRY(b->pairR.ensure((size_t)px * b->frames));
    HIP_TRY(hipMemcpyAsync(b->glut.p, lut, 256, hipMemcpyHostToDevice, b->stream));
    // preProcessImages' gamma table (functions.py:81-87) is applied as the pairs are read: cv2.LUT returns new
    // images, so the stored pairs stay the raw ones and every call corrects them exactly once (stereovision.py:44)
    const uint8_t* lut_d = b->glut.as<uint8_t>();
    // greyscale: BGR2GRAY + equalizeHist of both, functions.py:89-97 -> the SGBM pairs
    HIP_TRY(launch_grey_equalize(b->bgrL.as<uint8_t>(), px, b->frames, b->pairL.as<uint8_t>(),
                                 b->ghist.as<uint32_t>(), b->stream, lut_d));
    HIP_TRY(launch_grey_equalize(b->bgrR.as<uint8_t>(), px, b->frames, b->pairR.as<uint8_t>(),
                                 b->ghist.as<uint32_t>(), b->stream, lut_d));
    // the pipeline's colours: projectDisparityTo3d(disparity, 128, imgL) reads the gamma-corrected left image at
    // the disparity's own (y, x) (stereovision.py:44, :84), the top-left H x W of it when the disparity is cropped
    if (b->with_bgr)
        HIP_TRY(launch_copy_bgr_region(b->bgrL.as<uint8_t>(), H, W, b->bgr.as<uint8_t>(), b->H, b->W, b->Wu, b->frames,
                                       b->stream, lut_d));
    if (sync) HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

// The cost volumes, placed (as K1's planes, k1_place): where the four streamed volumes land moves the walks by
// up to 7 % from one allocation to the next (30.9-33.1 ms per 128 frames over five processes of the same build,
// profiles/r04/ab_sgbm_volcontig.txt). A chunk of >= 64 frames allocates up to SVX_SGBM_TRIES (default 2)
// contiguous sets (all held until the end, at most 7/8 of the free memory), runs the first chunk's SGBM on each
// (the second of two runs timed) and keeps the fastest; the results are the same on every set.
static int sgbm_place(sv_batch* b, const SgbmK& k, int chunk, const uint8_t* left, const uint8_t* right) {
    int tries = 2;
    if (const char* e = svx_knob("SVX_SGBM_TRIES")) tries = std::max(1, std::atoi(e));
    const size_t vb = sgbm_volume_bytes(k) * (size_t)chunk, set_b = 4 * vb;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    for (DevBuf& v : b->sg.vol) v.release();   // the old volumes go (a new size)
    if (chunk < 64) tries = 1;
    else tries = (int)std::min<size_t>((size_t)tries, std::max<size_t>(1, free_b / 8 * 7 / set_b));
    std::vector<std::array<DevBuf, 4>> sets((size_t)tries);
    int best = -1;
    float best_ms = 0.f;
    for (int t = 0; t < tries; ++t) {
        auto& c = sets[(size_t)t];
        hipError_t e = hipSuccess;
        for (int i = 0; i < 4 && e == hipSuccess; ++i) e = c[i].ensure(vb, true, 0, true);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        if (tries > 1) {
            for (int i = 0; i < 4; ++i) b->sg.vol[i] = c[i];   // (borrowed: the set's owner is `sets`)
            SgbmScratch sc = b->sg.scratch();
            sc.flags = b->sgflags.as<uint32_t>();
            float ms = 0.f;
            for (int rep = 0; rep < 2 && e == hipSuccess; ++rep) {   // the second run is timed
                e = hipEventRecord(b->ev[0], b->stream);
                if (e == hipSuccess) e = launch_sgbm_compute(k, left, right, chunk, sc, b->stream);
                if (e == hipSuccess) e = hipEventRecord(b->ev[1], b->stream);
                if (e == hipSuccess) e = hipEventSynchronize(b->ev[1]);
                if (e == hipSuccess) e = hipEventElapsedTime(&ms, b->ev[0], b->ev[1]);
            }
            if (e != hipSuccess) break;
            if (t < 8) {
                b->place_ms[2][t] = ms;
                b->place_n[2] = t + 1;
            }
            if (best < 0 || ms < best_ms) {
                best = t;
                best_ms = ms;
            }
        } else {
            best = t;
        }
    }
    for (DevBuf& v : b->sg.vol) v = DevBuf{};
    int rc = SV_OK;
    if (best < 0) rc = fail(SV_E_HIP, "SGBM volumes: allocation failed (%zu bytes each)", vb);
    b->place_kept[2] = tries > 1 ? best : -1;
    for (int t = 0; t < (int)sets.size(); ++t)
        for (int i = 0; i < 4; ++i) {
            DevBuf& x = sets[(size_t)t][i];
            if (t == best) b->sg.vol[i] = x;
            else x.release();
        }
    b->sg.placed = rc == SV_OK;
    return rc;
}

int sv_batch_sgbm(sv_batch* b, const sv_sgbm_params* prm, int max_disparity, int chunk) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (!b->pairL.p || !b->pairR.p) return fail(SV_E_STATE, "no stereo pairs (sv_batch_synth_pair / upload_pair)");
    int H, W;
    pair_shape(b, &H, &W);
    const int crop = b->pairW ? 1 : 0;   // the batch is the pair's [0:390, 135:W] (sv_batch_pair_shape)
    SgbmK k;
    if (int rc = make_sgbm(H, W, prm, max_disparity, crop, &k)) return rc;
    k.out_stride = b->W;   // the batch's row stride (a cropped 889-wide row is stored in 896 bytes)
    if (b->pairL.bytes < (size_t)k.frame_px * b->frames || b->pairR.bytes < (size_t)k.frame_px * b->frames)
        return fail(SV_E_STATE, "stereo pairs hold fewer bytes than %d frames of %d x %d", b->frames, H, W);
    HIP_TRY(hipSetDevice(b->device));
    // 128 frames a chunk (64 GB of volumes at 544 x 1024): the walks' last round of workgroups is a smaller share
    // of a larger launch — 388 vs 401-424 us per frame at 32 and 403 at 64 (128 frames, alternating runs). The
    // default is capped by the device's free memory: the largest chunk whose scratch (what the batch does not
    // hold already, with DevBuf's 1/4 slack) fits in 3/4 of it, at least 1 frame.
    if (chunk <= 0) {
        chunk = std::min(128, b->frames);
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        const size_t per = (4 * sgbm_volume_bytes(k) + (size_t)k.frame_px * (2 * sizeof(int16_t) + 2 * sizeof(int32_t))) *
                           5 / 4;
        const size_t held = b->sg.held_bytes();
        const size_t budget = (fr + held) / 4 * 3;
        while (chunk > 1 && (size_t)chunk * per > budget) chunk = chunk * 3 / 4;
    }
    chunk = std::min(chunk, b->frames);
    // the range flags of every frame of the batch, checked once after the last chunk (no host sync between chunks)
    HIP_TRY(b->sgflags.ensure(sizeof(uint32_t) * b->frames));
    const size_t px = (size_t)k.frame_px, opx = (size_t)b->H * b->W;
    if (b->sg.vol[0].bytes < sgbm_volume_bytes(k) * (size_t)chunk) {
        HIP_TRY(b->sg.ensure_rest(k, chunk));
        if (int rc = sgbm_place(b, k, chunk, b->pairL.as<uint8_t>(), b->pairR.as<uint8_t>())) return rc;
    }
    HIP_TRY(b->sg.ensure(k, chunk));
    b->rdisp_fresh = false;
    int t0, t1;
    HIP_TRY(hipEventRecord(b->ev[4], b->stream));
    HIP_TRY(b->timed_event(&t0));
    for (int f0 = 0; f0 < b->frames; f0 += chunk) {
        const int n = std::min(chunk, b->frames - f0);
        SgbmScratch sc = b->sg.scratch();
        sc.flags = b->sgflags.as<uint32_t>() + f0;
        HIP_TRY(launch_sgbm_compute(k, b->pairL.as<uint8_t>() + px * f0, b->pairR.as<uint8_t>() + px * f0, n, sc,
                                    b->stream));
        HIP_TRY(launch_speckle_scale(k, n, sc, input_disp(b) + opx * f0, nullptr, b->stream));
    }
    HIP_TRY(b->timed_event(&t1));
    HIP_TRY(hipEventRecord(b->ev[5], b->stream));
    if (int rc = sgbm_check_flags(b->sgflags.as<uint32_t>(), b->frames, b->stream)) return rc;
    if (t0 >= 0) b->pending[2].push_back({t0, t1});
    b->have_ms[2] = true;
    return SV_OK;
}

}  // extern "C"
