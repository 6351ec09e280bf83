// svx runtime: RANSAC. The batched RANSAC in two phases (which the frame loop enqueues as separate stages), its
// read-backs and trace, and the host drop-ins with the exact draw replay.
#include "svx_runtime.h"

// ---------------------------------------------------------------------------
// batched RANSAC (stereovision.py:85-94 per frame, seeded per frame)
// ---------------------------------------------------------------------------

// DIAGNOSTIC ONLY (env SVX_RANSAC_ABLATE, diagnostic build, documented in DESIGN.md): 1 skips the trial
// evaluation (results invalid); 4 evaluates every trial in fp64 (no fp32 screen; results valid, for A/B); draw
// kernel (results invalid): 8 no collinearity test, 16 no random.sample (both also skip the evaluation). Any other
// bit is refused (-1): an undocumented bit once rode along in an A/B run that faulted.
static constexpr int kRansacAblateBits = 1 | 4 | 8 | 16 | 32 | 128;

static int ransac_ablate() {
    const char* e = svx_knob("SVX_RANSAC_ABLATE");
    const int v = e ? std::atoi(e) : 0;
    return (v & ~kRansacAblateBits) ? -1 : v;
}

// Batched RANSAC in two phases, so that a caller with other streams to feed (the frame loop) is not held by the
// one read-back: phase 1 enqueues the step-2 tables, maskpoints and the copy of the per-frame counts into pinned
// host memory (+ an event); phase 2 waits for that event — the largest frame sizes the draw kernel's LDS (bitmap /
// pool list) and the sample index width — and enqueues the draw and evaluation kernels.
// An upper bound of every frame's maskpoints count that sizes the RANSAC launches with no read-back, or -1: the
// mask's step-2 grid points when a mask is set and they keep the draw kernel's sample LDS (a bitmap of n bits, or
// the pool branch's k-entry list) within 8 KiB and the sample indices 16-bit; otherwise the counts are read.
static int64_t ransac_device_bound(const sv_batch* b, int k) {
    if (!b->have_mask) return -1;
    // DIAGNOSTIC A/B (diagnostic build): SVX_RANSAC_BOUND=0 sizes the draw from the counts read back even with a mask
    if (const char* e = svx_knob("SVX_RANSAC_BOUND"); e && e[0] == '0') return -1;
    const int64_t n = std::min(b->mask_n2, b->mcap);
    const int64_t words = std::max<int64_t>((n + 31) / 32, k);
    return (words <= 2048 && n <= 65535) ? n : -1;
}

namespace svx {

#ifdef SVX_DIAG
hipError_t diag_eval_phases(unsigned long long* out, bool reset);
#endif

int batch_ransac_prepare(sv_batch* b, const sv_camera* cam, int trials, int k) {
    if (!b || !cam || trials < 0 || k < 1 || k > 1024)
        return fail(SV_E_ARG, "sv_batch_ransac: bad arguments (1 <= k <= 1024, trials >= 0)");
    if (trials > 4096) return fail(SV_E_ARG, "sv_batch_ransac: trials <= 4096");
    const int Hg = grid_len(b->H, 2), Wg = grid_len(b->W, 2);
    const int64_t mcap = (int64_t)Hg * Wg;
    if (mcap > 163840)
        return fail(SV_E_ARG, "sv_batch_ransac: %lld step-2 grid points per frame > 163,840 (LDS sample bitmap)",
                    (long long)mcap);
    if (b->H > 4096 || b->W > 4096) return fail(SV_E_ARG, "sv_batch_ransac: frames up to 4096 x 4096");
    HIP_TRY(hipSetDevice(b->device));
    const size_t F = (size_t)b->frames;
    HIP_TRY(b->mpk.ensure(sizeof(uint32_t) * (size_t)(mcap > 0 ? mcap : 1) * F));
    HIP_TRY(b->rres.ensure(F * (sizeof(double) * 4 + sizeof(int64_t) + sizeof(int32_t) + sizeof(uint32_t))));
    if (!b->hcnt) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->hcnt), sizeof(int64_t) * F));
    if (!b->cnt_ev) HIP_TRY(hipEventCreateWithFlags(&b->cnt_ev, hipEventDisableTiming));
    b->mcap = mcap;
    const RansacRes r = ransac_res(b);
    const KParams p = make_params(b->H, b->W, 2, *cam, b->Wu);
    // the fp64 X / Y / Z tables of the step-2 grid for this camera (the RANSAC kernels and the read-back gather
    // them instead of dividing)
    HIP_TRY(b->rtab.ensure(ransac_tables_bytes(b->H, b->W)));
    HIP_TRY(launch_ransac_tables(b->H, b->W, p, b->rtab.as<double>(), b->stream));
    const uint8_t* mff = b->have_mask ? b->carmask.as<uint8_t>() : nullptr;
    HIP_TRY(launch_maskpoints(b->disp.as<uint8_t>(), mff, b->frames, b->H, b->W, p, b->mpk.as<uint32_t>(), mcap,
                              r.mcount, b->stream));
    // the launches are sized from an upper bound of every frame's count when one is small enough (the mask's grid
    // points: ransac_device_bound), else from the counts read back (the host waits for them in the launch)
    b->rbound = ransac_device_bound(b, k);
    if (b->rbound < 0) {
        HIP_TRY(hipMemcpyAsync(b->hcnt, r.mcount, sizeof(int64_t) * F, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipEventRecord(b->cnt_ev, b->stream));
    }
    return SV_OK;
}

// phases: 1 = the draw kernel (waits for phase 1's counts on the host), 2 = the evaluation kernel (after a phase-1
// launch with the same arguments), 3 = both. The frame loop enqueues the two as separate stages.
// started / epoch: the frame loop's dispatch signal (the draw kernel's last workgroup stores epoch there)
int batch_ransac_launch(sv_batch* b, const sv_camera* cam, uint64_t seed_base, int64_t first_frame, int trials, int k,
                        hipStream_t stream, int phases, uint64_t* started, uint64_t epoch) {
    if (first_frame < 0) return fail(SV_E_ARG, "sv_batch_ransac: first_frame >= 0");
    HIP_TRY(hipSetDevice(b->device));
    const size_t F = (size_t)b->frames;
    const int64_t mcap = b->mcap;
    const RansacRes r = ransac_res(b);
    const KParams p = make_params(b->H, b->W, 2, *cam, b->Wu);
    int32_t* trace = nullptr;
    if (b->trace_trials > 0 && (phases & 1)) {
        HIP_TRY(b->rtrace.ensure(sizeof(int32_t) * F * b->trace_trials * (size_t)(k + 3)));
        HIP_TRY(hipMemsetAsync(b->rtrace.p, 0xff, sizeof(int32_t) * F * b->trace_trials * (size_t)(k + 3), stream));
        trace = b->rtrace.as<int32_t>();
    }
    if (phases & 1) {
        b->trace_k = k;
        b->traced_trials = trace ? b->trace_trials : 0;   // what rtrace holds now (sv_batch_read_ransac_trace)
    }
    // the largest frame sizes the kernel's LDS (bitmap / pool list): the device bound of batch_ransac_prepare, or
    // the counts phase 1 copied back
    if ((phases & 1) && b->rbound >= 0) {
        b->rmax_n = b->rbound;
        b->rmax_pool_n = b->rbound >= k ? std::min<int64_t>(b->rbound, ransac_setsize(k)) : 0;
    } else if (phases & 1) {
        HIP_TRY(hipEventSynchronize(b->cnt_ev));
        int64_t max_n = 0, max_pool_n = 0;
        const int64_t setsize = ransac_setsize(k);
        for (size_t f = 0; f < F; ++f) {
            const int64_t c = b->hcnt[f];
            max_n = std::max(max_n, c);
            if (c >= k && c <= setsize) max_pool_n = std::max(max_pool_n, c);
        }
        b->rmax_n = max_n;
        b->rmax_pool_n = max_pool_n;
    }
    const int64_t max_n = b->rmax_n, max_pool_n = b->rmax_pool_n;
    const int ablate = ransac_ablate();
    if (ablate < 0)
        return fail(SV_E_ARG, "SVX_RANSAC_ABLATE: only the documented bits 1, 4, 8, 16, 32 and 128 (diagnostic build)");
    HIP_TRY(b->rsidx.ensure(std::max<size_t>(ransac_sidx_bytes(max_n, b->frames, trials, k), 4)));
    HIP_TRY(b->rtri.ensure(sizeof(double) * 5 * F * (size_t)std::max(trials, 1) + sizeof(int32_t) * 2 * F));
    const RansacScratch rs{b->rsidx.p, b->rtri.as<double>(),
                           reinterpret_cast<int32_t*>(b->rtri.as<double>() + 5 * F * (size_t)std::max(trials, 1))};
    HIP_TRY(launch_ransac_batch(b->mpk.as<uint32_t>(), b->rtab.as<double>(), b->H, b->W, mcap, p, r.mcount, max_n,
                                max_pool_n,
                                seed_base, first_frame, b->frames, trials, k, rs, r.abc, r.err, r.trial, r.flags, trace,
                                b->trace_trials, ablate, phases, started, epoch, stream));
    return SV_OK;
}

}  // namespace svx

extern "C" {

#ifdef SVX_DIAG
// DIAGNOSTIC (diagnostic build only, not in include/svx.h): the evaluation's phase clocks (SVX_RANSAC_ABLATE bit 32)
int sv_diag_eval_phases(unsigned long long* out8, int reset) {
    if (!out8) return fail(SV_E_ARG, "sv_diag_eval_phases: null argument");
    HIP_TRY(diag_eval_phases(out8, reset != 0));
    return SV_OK;
}
#endif

int sv_batch_ransac(sv_batch* b, const sv_camera* cam, uint64_t seed_base, int64_t first_frame, int trials, int k,
                    int sync) {
    if (first_frame < 0) return fail(SV_E_ARG, "sv_batch_ransac: bad arguments (first_frame >= 0)");
    if (int rc = batch_ransac_prepare(b, cam, trials, k)) return rc;
    if (int rc = batch_ransac_launch(b, cam, seed_base, first_frame, trials, k, b->stream)) return rc;
    if (sync) HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_read_ransac(sv_batch* b, int frame, double* abc, double* err, int32_t* trial, uint32_t* flags) {
    if (!b || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    if (!b->rres.p) return fail(SV_E_STATE, "no RANSAC results (sv_batch_ransac first)");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const RansacRes r = ransac_res(b);
    if (abc) HIP_TRY(hipMemcpy(abc, r.abc + 3 * frame, 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (err) HIP_TRY(hipMemcpy(err, r.err + frame, sizeof(double), hipMemcpyDeviceToHost));
    if (trial) HIP_TRY(hipMemcpy(trial, r.trial + frame, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (flags) HIP_TRY(hipMemcpy(flags, r.flags + frame, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SV_OK;
}

int sv_batch_ransac_trace(sv_batch* b, int trials) {
    if (!b || trials < 0) return fail(SV_E_ARG, "bad args");
    b->trace_trials = trials;
    return SV_OK;
}

int sv_batch_read_ransac_trace(sv_batch* b, int frame, int32_t* out, int64_t cap, int* out_trials, int* out_k) {
    if (!b || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    if (!b->traced_trials || !b->rtrace.p) return fail(SV_E_STATE, "no trace (sv_batch_ransac_trace, then sv_batch_ransac)");
    const size_t per = (size_t)b->traced_trials * (b->trace_k + 3);
    if (out_trials) *out_trials = b->traced_trials;
    if (out_k) *out_k = b->trace_k;
    if (!out) return SV_OK;   // sizes only
    if (cap < (int64_t)per) return fail(SV_E_CAP, "trace needs %zu int32, buffer holds %lld", per, (long long)cap);
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(out, b->rtrace.as<int32_t>() + per * frame, sizeof(int32_t) * per, hipMemcpyDeviceToHost));
    return SV_OK;
}

int sv_batch_read_maskpoints(sv_batch* b, int frame, double* xyz, int64_t cap, int64_t* n) {
    if (!b || frame < 0 || frame >= b->frames || !n) return fail(SV_E_ARG, "bad args");
    if (!b->rres.p) return fail(SV_E_STATE, "no maskpoints (sv_batch_ransac first)");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const RansacRes r = ransac_res(b);
    int64_t k = 0;
    HIP_TRY(hipMemcpy(&k, r.mcount + frame, sizeof k, hipMemcpyDeviceToHost));
    *n = k;
    if (k > cap) return fail(SV_E_CAP, "capacity %lld < %lld", (long long)cap, (long long)k);
    if (k && xyz) {   // the frame's fp64 X, Y, Z from its packed points (the reference's arithmetic)
        HIP_TRY(b->mpts.ensure(sizeof(double) * 3 * (size_t)k));
        HIP_TRY(launch_maskpoints_xyz(b->mpk.as<uint32_t>() + (size_t)b->mcap * frame, k, b->rtab.as<double>(), b->H,
                                      b->W, b->mpts.as<double>(), b->stream));
        HIP_TRY(hipMemcpyAsync(xyz, b->mpts.p, sizeof(double) * 3 * k, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(hipStreamSynchronize(b->stream));
    }
    return SV_OK;
}

// ---------------------------------------------------------------------------
// RANSAC (functions.py:240-298): exact draw replay on the host, trials on the GPU
// ---------------------------------------------------------------------------
int sv_ransac_draw(uint32_t* mt_state, const double* pts, int64_t n, int64_t ld, int trials, int k, int32_t* sidx,
                   int32_t* tri, int* out_trials) {
    if (!mt_state || !out_trials || trials < 0 || k < 0 || ld < 3 || n < 0 || (n > 0 && !pts) ||
        (trials > 0 && (!sidx || !tri)))
        return fail(SV_E_ARG, "sv_ransac_draw: bad arguments");
    if (mt_state[624] > 624) return fail(SV_E_ARG, "sv_ransac_draw: MT index %u > 624", mt_state[624]);
    *out_trials = ransac_draw(mt_state, pts, n, ld, trials, k, sidx, tri);
    return SV_OK;
}

// The draws are replayed on the host in chunks of trials; each chunk's samples go up (asynchronously when the
// caller's sidx / tri are page-locked, as svx/ransac.py allocates them) and are evaluated on the device while the
// next chunk is drawn, so only the last chunk's evaluation is exposed after the replay.
int sv_ransac(uint32_t* mt_state, const double* pts, int64_t n, int64_t ld, int trials, int k, int32_t* sidx,
              int32_t* tri, double* out_abc, double* out_err, uint8_t* out_flag, int* out_trials) {
    if (!mt_state || !out_trials || trials < 0 || k < 0 || ld < 3 || n < 0 || (n > 0 && !pts) ||
        (trials > 0 && (!sidx || !tri)))
        return fail(SV_E_ARG, "sv_ransac: bad arguments");
    if (mt_state[624] > 624) return fail(SV_E_ARG, "sv_ransac: MT index %u > 624", mt_state[624]);
    *out_trials = 0;
    if (trials == 0 || n < k || n < 1 || n >= (1ll << 31)) return SV_OK;   // random.sample raises: no draw
    if (!out_abc || !out_err || !out_flag) return fail(SV_E_ARG, "sv_ransac: null outputs");
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    const size_t pbytes = sizeof(double) * (size_t)n * ld;
    const size_t ibytes = sizeof(int32_t) * ((size_t)trials * k + 3 * (size_t)trials);
    const size_t obytes = sizeof(double) * 4 * (size_t)trials + (size_t)trials;
    HIP_TRY(d->xyz.ensure(pbytes));
    HIP_TRY(d->aux.ensure(ibytes));
    HIP_TRY(d->aux2.ensure(obytes));
    int32_t* dsidx = d->aux.as<int32_t>();
    int32_t* dtri = dsidx + (size_t)trials * k;
    double* dabc = d->aux2.as<double>();
    double* derr = dabc + 3 * (size_t)trials;
    uint8_t* dflag = reinterpret_cast<uint8_t*>(derr + trials);
    HIP_TRY(hipMemcpyAsync(d->xyz.p, pts, pbytes, hipMemcpyHostToDevice, s));
    constexpr int kChunks = 4;
    const int per = (trials + kChunks - 1) / kChunks;
    for (int t0 = 0; t0 < trials; t0 += per) {
        const int c = std::min(per, trials - t0);
        if (ransac_draw(mt_state, pts, n, ld, c, k, sidx + (size_t)t0 * k, tri + 3 * (size_t)t0) != c)
            return fail(SV_E_ARG, "sv_ransac: draw replay stopped");
        HIP_TRY(hipMemcpyAsync(dsidx + (size_t)t0 * k, sidx + (size_t)t0 * k, sizeof(int32_t) * (size_t)c * k,
                               hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dtri + 3 * (size_t)t0, tri + 3 * (size_t)t0, sizeof(int32_t) * 3 * (size_t)c,
                               hipMemcpyHostToDevice, s));
        HIP_TRY(launch_ransac_eval(d->xyz.as<double>(), ld, dsidx + (size_t)t0 * k, dtri + 3 * (size_t)t0, c, k,
                                   dabc + 3 * (size_t)t0, derr + t0, dflag + t0, s));
    }
    HIP_TRY(hipMemcpyAsync(out_abc, dabc, sizeof(double) * 3 * trials, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_err, derr, sizeof(double) * trials, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_flag, dflag, (size_t)trials, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out_trials = trials;
    return SV_OK;
}

}  // extern "C"
