// svx runtime: the host-frame drop-ins of the projection, the back-projection and the stages a2-a6, each one
// synchronous call on the current device's scratch and stream.
#include "svx_runtime.h"

extern "C" {

// ---------------------------------------------------------------------------
// drop-in: projectDisparityTo3d (functions.py:178-198)
// ---------------------------------------------------------------------------
// The drop-in projection on the device: the frame (and its colours) up, the compact fp64 kernel, the point count
// back (one sync). On success *n is the count and d's xyz / rgb buffers hold the points; the device mutex is held
// by the caller.
static int project_on_device(Device* d, const uint8_t* disp, int H, int W, int64_t ld_disp, const uint8_t* bgr,
                             int64_t ld_bgr, bool want_rgb, const KParams& p, int64_t* n) {
    hipStream_t s = d->stream;
    const int tiles = project_compact_tiles(p);
    const int64_t ng = (int64_t)p.Hg * p.Wg;
    HIP_TRY(d->disp.ensure((size_t)H * W));
    HIP_TRY(d->xyz.ensure(sizeof(double) * 3 * ng));
    HIP_TRY(d->ctrl.ensure(sizeof(uint64_t) * (tiles + 2)));
    HIP_TRY(hipMemcpy2DAsync(d->disp.p, W, disp, ld_disp, W, H, hipMemcpyHostToDevice, s));
    if (want_rgb) {
        HIP_TRY(d->bgr.ensure((size_t)H * W * 3));
        HIP_TRY(d->rgb.ensure(3 * ng));
        HIP_TRY(hipMemcpy2DAsync(d->bgr.p, 3 * (size_t)W, bgr, ld_bgr, 3 * (size_t)W, H,
                                 hipMemcpyHostToDevice, s));
    }
    uint64_t* status = d->ctrl.as<uint64_t>();
    uint32_t* small = reinterpret_cast<uint32_t*>(status + tiles);  // ticket, count, err
    HIP_TRY(hipMemsetAsync(d->ctrl.p, 0, sizeof(uint64_t) * (tiles + 2), s));
    HIP_TRY(launch_project_compact_f64(p, d->disp.as<uint8_t>(), W, want_rgb ? d->bgr.as<uint8_t>() : nullptr,
                                       3ll * W, d->xyz.as<double>(), want_rgb ? d->rgb.as<uint8_t>() : nullptr,
                                       status, small, small + 1, small + 2, s));
    uint32_t hs[3];
    HIP_TRY(hipMemcpyAsync(hs, small, sizeof hs, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hs[2]) return fail(SV_E_DEVICE, "projection look-back timed out");
    *n = hs[1];
    return SV_OK;
}

int sv_project_frame(const uint8_t* disp, int H, int W, int64_t ld_disp, const uint8_t* bgr,
                     int64_t ld_bgr, int step, const sv_camera* cam, double* out_xyz, uint8_t* out_rgb,
                     int64_t cap, int64_t* out_n) {
    if (!disp || !cam || !out_n || H < 0 || W < 0 || step < 1 || ld_disp < W)
        return fail(SV_E_ARG, "sv_project_frame: bad arguments (H=%d W=%d step=%d)", H, W, step);
    if (bgr && ld_bgr < 3ll * W) return fail(SV_E_ARG, "sv_project_frame: ld_bgr < 3*W");
    *out_n = 0;
    const KParams p = make_params(H, W, step, *cam);
    if ((int64_t)p.Hg * p.Wg == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    const bool want_rgb = bgr && out_rgb;
    int64_t n = 0;
    if (int rc = project_on_device(d, disp, H, W, ld_disp, bgr, ld_bgr, want_rgb, p, &n)) return rc;
    if (n > cap) return fail(SV_E_CAP, "output capacity %lld < %lld points", (long long)cap, (long long)n);
    if (n) {
        HIP_TRY(hipMemcpyAsync(out_xyz, d->xyz.p, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
        if (want_rgb) HIP_TRY(hipMemcpyAsync(out_rgb, d->rgb.p, 3 * n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    *out_n = n;
    return SV_OK;
}

int sv_project_rows(const uint8_t* disp, int H, int W, int64_t ld_disp, const uint8_t* bgr, int64_t ld_bgr,
                    int step, const sv_camera* cam, double* out_rows, int cols, int64_t cap, int64_t* out_n) {
    if (!disp || !cam || !out_n || H < 0 || W < 0 || step < 1 || ld_disp < W || (cols != 3 && cols != 6) ||
        (cols == 6 && !bgr))
        return fail(SV_E_ARG, "sv_project_rows: bad arguments (H=%d W=%d step=%d cols=%d)", H, W, step, cols);
    if (bgr && ld_bgr < 3ll * W) return fail(SV_E_ARG, "sv_project_rows: ld_bgr < 3*W");
    *out_n = 0;
    const KParams p = make_params(H, W, step, *cam);
    if ((int64_t)p.Hg * p.Wg == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    int64_t n = 0;
    if (int rc = project_on_device(d, disp, H, W, ld_disp, bgr, ld_bgr, cols == 6, p, &n)) return rc;
    if (n > cap) return fail(SV_E_CAP, "output capacity %lld < %lld points", (long long)cap, (long long)n);
    if (!n) return SV_OK;
    if (!out_rows) return fail(SV_E_ARG, "sv_project_rows: null out_rows");
    const double* src = d->xyz.as<double>();
    if (cols == 6) {
        HIP_TRY(d->aux2.ensure(sizeof(double) * 6 * (size_t)n));
        HIP_TRY(launch_rows6(d->xyz.as<double>(), d->rgb.as<uint8_t>(), n, d->aux2.as<double>(), s));
        src = d->aux2.as<double>();
    }
    HIP_TRY(hipMemcpyAsync(out_rows, src, sizeof(double) * cols * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out_n = n;
    return SV_OK;
}

// ---------------------------------------------------------------------------
// drop-in: project3DPointsTo2DImagePoints (functions.py:201-209)
// ---------------------------------------------------------------------------
int sv_backproject(const double* xyz, int64_t n, int64_t ld, const sv_camera* cam, double* out_xy) {
    if (n < 0 || ld < 3 || !cam || (n > 0 && (!xyz || !out_xy)))
        return fail(SV_E_ARG, "sv_backproject: bad arguments");
    if (n == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    HIP_TRY(d->xyz.ensure(sizeof(double) * ld * n));
    HIP_TRY(d->xy.ensure(sizeof(double) * 2 * n));
    HIP_TRY(hipMemcpyAsync(d->xyz.p, xyz, sizeof(double) * ld * n, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_backproject_f64(d->xyz.as<double>(), n, ld, cam->f, cam->cw, cam->ch, d->xy.as<double>(), s));
    HIP_TRY(hipMemcpyAsync(out_xy, d->xy.p, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

// ---------------------------------------------------------------------------
// a2-a6 as separate calls (functions.py:212-230, :300-323) for the stage drop-ins
// ---------------------------------------------------------------------------
int sv_point_errors(const double* xyz, int64_t n, int64_t ld, const double* abcd, double* out) {
    if (n < 0 || ld < 3 || !abcd || (n > 0 && (!xyz || !out))) return fail(SV_E_ARG, "sv_point_errors: bad arguments");
    if (n == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    hipStream_t s = L.d->stream;
    HIP_TRY(L.d->xyz.ensure(sizeof(double) * (size_t)n * ld));
    HIP_TRY(L.d->aux.ensure(sizeof(double) * (size_t)n));
    HIP_TRY(hipMemcpyAsync(L.d->xyz.p, xyz, sizeof(double) * (size_t)n * ld, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_point_errors(L.d->xyz.as<double>(), n, ld, abcd, L.d->aux.as<double>(), s));
    HIP_TRY(hipMemcpyAsync(out, L.d->aux.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_hue_histogram(const uint8_t* rgb, int64_t n, int64_t ld, int16_t* out_bins, uint32_t* out_hist,
                     int64_t* out_first) {
    if (n < 0 || ld < 3 || n >= INT32_MAX || (n > 0 && !rgb) || !out_hist || !out_first)
        return fail(SV_E_ARG, "sv_hue_histogram: bad arguments");
    for (int k = 0; k < 1000; ++k) {
        out_hist[k] = 0;
        out_first[k] = -1;
    }
    if (n == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    hipStream_t s = L.d->stream;
    HIP_TRY(L.d->rgb.ensure((size_t)n * ld));
    HIP_TRY(L.d->aux.ensure(sizeof(int16_t) * (size_t)n + 8192));
    int16_t* bins = L.d->aux.as<int16_t>();
    uint32_t* hist = reinterpret_cast<uint32_t*>(L.d->aux.as<char>() + (sizeof(int16_t) * (size_t)n + 15) / 16 * 16);
    int32_t* first = reinterpret_cast<int32_t*>(hist + 1000);
    HIP_TRY(hipMemcpyAsync(L.d->rgb.p, rgb, (size_t)n * ld, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(hist, 0, sizeof(uint32_t) * 1000, s));
    HIP_TRY(hipMemsetAsync(first, 0x7f, sizeof(int32_t) * 1000, s));   // 0x7f7f7f7f > any index
    HIP_TRY(launch_hue_hist(L.d->rgb.as<uint8_t>(), n, ld, out_bins ? bins : nullptr, hist, first, s));
    std::vector<int32_t> f(1000);
    HIP_TRY(hipMemcpyAsync(out_hist, hist, sizeof(uint32_t) * 1000, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(f.data(), first, sizeof(int32_t) * 1000, hipMemcpyDeviceToHost, s));
    if (out_bins) HIP_TRY(hipMemcpyAsync(out_bins, bins, sizeof(int16_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 1000; ++k) out_first[k] = out_hist[k] ? (int64_t)f[k] : -1;
    return SV_OK;
}

static int select_impl(int mode, const double* vals, double thr, const int16_t* bins, const uint8_t* ok, int64_t n,
                       int64_t* out_idx, int64_t* out_n) {
    if (n < 0 || !out_n || (n > 0 && !out_idx) || (mode == 0 && n > 0 && !vals) ||
        (mode == 1 && (!ok || (n > 0 && !bins))))
        return fail(SV_E_ARG, "sv_select: bad arguments");
    *out_n = 0;
    if (n == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    hipStream_t s = L.d->stream;
    const size_t in_bytes = mode == 0 ? sizeof(double) * (size_t)n : sizeof(int16_t) * (size_t)n;
    HIP_TRY(L.d->aux.ensure((in_bytes + 15) / 16 * 16 + 1024));
    HIP_TRY(L.d->aux2.ensure(sizeof(int64_t) * ((size_t)n + 1)));
    char* in = L.d->aux.as<char>();
    uint8_t* dok = reinterpret_cast<uint8_t*>(in + (in_bytes + 15) / 16 * 16);
    int64_t* idx = L.d->aux2.as<int64_t>();
    int64_t* cnt = idx + n;
    HIP_TRY(hipMemcpyAsync(in, mode == 0 ? (const void*)vals : (const void*)bins, in_bytes, hipMemcpyHostToDevice, s));
    if (mode == 1) HIP_TRY(hipMemcpyAsync(dok, ok, 1000, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_select(mode, reinterpret_cast<const double*>(in), thr, reinterpret_cast<const int16_t*>(in), dok, n,
                          idx, cnt, s));
    int64_t k = 0;
    HIP_TRY(hipMemcpyAsync(&k, cnt, sizeof k, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (k) {
        HIP_TRY(hipMemcpyAsync(out_idx, idx, sizeof(int64_t) * (size_t)k, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    *out_n = k;
    return SV_OK;
}

int sv_select_less(const double* vals, int64_t n, double thr, int64_t* out_idx, int64_t* out_n) {
    return select_impl(0, vals, thr, nullptr, nullptr, n, out_idx, out_n);
}

int sv_select_bins(const int16_t* bins, int64_t n, const uint8_t* ok, int64_t* out_idx, int64_t* out_n) {
    for (int64_t i = 0; bins && i < n; ++i)
        if (bins[i] < 0 || bins[i] >= 1000) return fail(SV_E_ARG, "sv_select_bins: bin %d out of range", (int)bins[i]);
    return select_impl(1, nullptr, 0.0, bins, ok, n, out_idx, out_n);
}

}  // extern "C"
