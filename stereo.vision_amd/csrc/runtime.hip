// svx runtime: device/stream management, buffers, tables and the C ABI
// declared in include/svx.h. Host-side C++ compiled by hipcc; every compute
// step is a hand-written gfx950 kernel (kernels/*.hip). There is no CPU
// compute path: if a kernel cannot run, the call fails with an error.
// This unit: the error slot, the device state and the shared helpers of svx_runtime.h, and the entries that
// belong to no stage. The stages' entries are in rt_batch.hip, rt_dropin.hip, rt_prepass.hip, rt_road.hip,
// rt_ransac.hip, rt_sgbm.hip and rt_loop.hip.
#include <cstdarg>
#include <cstring>

#include "svx_runtime.h"

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_err;

namespace svx {

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

void set_error(const std::string& msg) { g_err = msg; }

const std::string& last_error() { return g_err; }

}  // namespace svx

// ---------------------------------------------------------------------------
// per-device state
// ---------------------------------------------------------------------------
namespace {

constexpr int kMaxDev = 64;
Device g_dev[kMaxDev];
std::mutex g_init_mu;

bool same_cam(const sv_camera& a, const sv_camera& b) {
    return a.f == b.f && a.B == b.B && a.cw == b.cw && a.ch == b.ch;
}

}  // namespace

namespace svx {

KParams make_params(int H, int W, int step, const sv_camera& cam, int Wu) {
    KParams p;
    std::memset(&p, 0, sizeof p);
    p.H = H;
    p.W = W;
    p.step = step;
    p.Hg = grid_len(H, step);
    p.Wg = grid_len(Wu > 0 ? Wu : W, step);
    p.pitch = (p.Wg + 3) / 4 * 4;
    p.Q = p.pitch / 4;
    p.frame_quads = p.Hg * p.Q;
    p.Q_m40 = p.Q > 0 ? (((uint64_t)1 << 40) + (uint64_t)p.Q - 1) / (uint64_t)p.Q : 0;
    p.frame_px = (int64_t)H * W;
    p.f = cam.f;
    p.B = cam.B;
    p.cw = cam.cw;
    p.ch = cam.ch;
    p.fB = cam.f * cam.B;  // functions.py:191 evaluates f*B in fp64
    p.fB32 = (float)p.fB;
    p.B32 = (float)cam.B;
    p.cw_hi = (float)cam.cw;
    p.cw_lo = (float)(cam.cw - (double)p.cw_hi);
    p.ch_hi = (float)cam.ch;
    p.ch_lo = (float)(cam.ch - (double)p.ch_hi);
    p.dx_words = (W + 31) / 32;
    p.dy_words = (H + 31) / 32;
    return p;
}

void set_plane(KParams& p, const sv_plane& pl, double thr, int hist_thr) {
    p.thr = thr;
    p.thr32 = (float)thr;
    FramePlane fp;
    plane_fields(fp, pl.a, pl.b, pl.c, p.f, p.B, p.cw, p.ch, thr, p.W, p.H);
    apply_plane(p, fp);
    p.hist_thr = hist_thr;
    // Diagnostic ablation for profiling only (documented in DESIGN.md): when set,
    // kernels skip parts of their work and the results are NOT valid.
    const char* ab = svx_knob("SVX_ABLATE");
    p.ablate = ab ? std::atoi(ab) : 0;
}

int dev_get(int device, Device** out) {
    if (device < 0 || device >= kMaxDev) return fail(SV_E_ARG, "device %d out of range", device);
    Device& d = g_dev[device];
    std::lock_guard<std::mutex> lk(g_init_mu);
    if (!d.init) {
        int n = 0;
        HIP_TRY(hipGetDeviceCount(&n));
        if (device >= n) return fail(SV_E_ARG, "device %d not present (%d visible)", device, n);
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
        d.init = true;
    }
    HIP_TRY(hipSetDevice(device));
    *out = &d;
    return SV_OK;
}

int current_device(int* dev) {
    HIP_TRY(hipGetDevice(dev));
    return SV_OK;
}

int lock_device(int device, Locked& L) {
    if (int rc = dev_get(device, &L.d)) return rc;
    L.device = device;
    L.lk = std::unique_lock<std::mutex>(L.d->mu);
    return SV_OK;
}

int lock_current(Locked& L) {
    int dev;
    if (int rc = current_device(&dev)) return rc;
    return lock_device(dev, L);
}

int ensure_tables(Device& d, int H, int W, const sv_camera& cam, hipStream_t s) {
    Tables& t = d.tables;
    if (t.valid && t.H == H && t.W == W && same_cam(t.cam, cam)) return SV_OK;
    KParams p = make_params(H, W, 1, cam);
    HIP_TRY(t.dx.ensure(sizeof(uint32_t) * 256 * p.dx_words));
    HIP_TRY(t.dy.ensure(sizeof(uint32_t) * 256 * p.dy_words));
    HIP_TRY(launch_delta_tables(p, t.dx.as<uint32_t>(), t.dy.as<uint32_t>(), nullptr, nullptr, s));
    HIP_TRY(t.dxT.ensure(sizeof(uint32_t) * 8 * 32 * p.dx_words));
    HIP_TRY(t.dyT.ensure(sizeof(uint32_t) * 8 * 32 * p.dy_words));
    HIP_TRY(launch_delta_transpose(p, t.dx.as<uint32_t>(), t.dy.as<uint32_t>(), t.dxT.as<uint32_t>(),
                                   t.dyT.as<uint32_t>(), s));
    HIP_TRY(hipStreamSynchronize(s));
    t.valid = true;
    t.H = H;
    t.W = W;
    t.cam = cam;
    return SV_OK;
}

int upload_u8(DevBuf& buf, const uint8_t* src, int H, int W, int pitch, hipStream_t s) {
    HIP_TRY(buf.ensure((size_t)H * pitch));
    if (pitch != W) HIP_TRY(hipMemsetAsync(buf.p, 0, (size_t)H * pitch, s));
    HIP_TRY(hipMemcpy2DAsync(buf.p, pitch, src, W, W, H, hipMemcpyHostToDevice, s));
    return SV_OK;
}
int download_u8(uint8_t* dst, const DevBuf& buf, int H, int W, int pitch, hipStream_t s) {
    HIP_TRY(hipMemcpy2DAsync(dst, W, buf.p, pitch, W, H, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

}  // namespace svx

extern "C" {

const char* sv_version(void) { return "svx 0.1.0 (gfx950)"; }

const char* sv_last_error(void) { return g_err.c_str(); }

int sv_device_count(int* n) {
    if (!n) return fail(SV_E_ARG, "null out");
    hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) {
        *n = 0;
        return fail(SV_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    return SV_OK;
}

int sv_init(int device) {
    Device* d;
    return dev_get(device, &d);
}

int sv_host_alloc(int64_t bytes, void** out) {
    if (!out || bytes <= 0) return fail(SV_E_ARG, "sv_host_alloc: bad arguments");
    *out = nullptr;
    int dev;
    if (int rc = current_device(&dev)) return rc;   // (no GPU: fails like every compute entry point)
    HIP_TRY(hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault));
    return SV_OK;
}

int sv_host_free(void* p) {
    if (p) HIP_TRY(hipHostFree(p));
    return SV_OK;
}

int sv_source_id(int which, char* buf, int cap) {
#ifndef SVX_SRCID_K1
#define SVX_SRCID_K1 "unknown"
#define SVX_SRCID_PIPE "unknown"
#endif
    if (which < 0 || which > 1 || !buf || cap <= 0) return fail(SV_E_ARG, "sv_source_id: bad arguments");
    std::snprintf(buf, (size_t)cap, "%s", which == 0 ? SVX_SRCID_K1 : SVX_SRCID_PIPE);
    return SV_OK;
}

// ---------------------------------------------------------------------------
// verification helpers
// ---------------------------------------------------------------------------
int sv_hue_lut(int device, int16_t* out_lut) { return sv_hue_lut_variant(device, 0, out_lut); }

int sv_hue_lut_variant(int device, int variant, int16_t* out_lut) {
    if (!out_lut) return fail(SV_E_ARG, "null");
    if (variant != 0 && variant != 1) return fail(SV_E_ARG, "sv_hue_lut_variant: variant %d not 0 or 1", variant);
    Locked L;
    if (int rc = lock_device(device, L)) return rc;
    Device* d = L.d;
    DevBuf buf;
    HIP_TRY(buf.ensure(sizeof(int16_t) << 24));
    hipError_t e = launch_hue_lut(buf.as<int16_t>(), variant, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_lut, buf.p, sizeof(int16_t) << 24, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    buf.release();
    HIP_TRY(e);
    return SV_OK;
}

int sv_delta_tables(int device, int H, int W, const sv_camera* cam, int8_t* dx, int8_t* dy) {
    if (!cam || !dx || !dy || H < 1 || W < 1) return fail(SV_E_ARG, "bad args");
    Locked L;
    if (int rc = lock_device(device, L)) return rc;
    Device* d = L.d;
    KParams p = make_params(H, W, 1, *cam);
    DevBuf bx, by, b8;
    HIP_TRY(bx.ensure(4 * 256 * p.dx_words));
    HIP_TRY(by.ensure(4 * 256 * p.dy_words));
    HIP_TRY(b8.ensure(256 * (size_t)(H + W)));
    int8_t* dx8 = b8.as<int8_t>();
    int8_t* dy8 = dx8 + 256 * (size_t)W;
    hipError_t e = launch_delta_tables(p, bx.as<uint32_t>(), by.as<uint32_t>(), dx8, dy8, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dx, dx8, 256 * (size_t)W, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dy, dy8, 256 * (size_t)H, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    bx.release();
    by.release();
    b8.release();
    HIP_TRY(e);
    return SV_OK;
}

int sv_synth_frame(int device, int64_t frame_id, int H, int W, uint8_t* disp, uint8_t* bgr) {
    if (!disp || H < 1 || W < 4 || (W % 4)) return fail(SV_E_ARG, "bad args (W%%4 == 0 required)");
    Locked L;
    if (int rc = lock_device(device, L)) return rc;
    Device* d = L.d;
    sv_camera cam0{1, 1, 0, 0};
    KParams p = make_params(H, W, 1, cam0);
    DevBuf bd, bc;
    HIP_TRY(bd.ensure((size_t)H * W));
    HIP_TRY(bc.ensure((size_t)H * W * 3));
    hipError_t e = launch_synth(p, bd.as<uint8_t>(), bc.as<uint8_t>(), 1, frame_id, d->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(disp, bd.p, (size_t)H * W, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess && bgr) e = hipMemcpyAsync(bgr, bc.p, (size_t)H * W * 3, hipMemcpyDeviceToHost, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    bd.release();
    bc.release();
    HIP_TRY(e);
    return SV_OK;
}

}  // extern "C"
