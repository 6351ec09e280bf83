// svx runtime: the batch object. Its life, inputs and tuning, K1 (the dense projection) and the pipeline with
// their placement probes, timing, the read-backs of points / dense / hist / counts, the digest, and the one-frame
// chain over a cached batch.
#include "svx_runtime.h"

// auto mode: one workgroup per frame needs enough frames to fill 256 CUs
static constexpr int kResidentMinFrames = 512;

// The pipeline's fp32 outputs: three planes of frames x cap in separate allocations (frame f's X at
// X + f cap), or, with SVX_PIPE_PLANES=0 (A/B), SoA per frame (X[cap] Y[cap] Z[cap] of frame f at 3 cap f).
// The planes were faster and steadier: 5.94-6.06 vs 5.98-6.23 ms for the pipeline, 6.66-6.87 vs 6.63-7.70
// with per-frame planes (five alternating processes each).
static hipError_t ensure_points(sv_batch* b) {
    const size_t plane = sizeof(float) * b->cap * (size_t)b->frames;
    hipError_t e;
    if (b->out_planes) {
        e = b->oxb.ensure(plane, false, 4);
        if (e == hipSuccess) e = b->oyb.ensure(plane, false, 4);
        if (e == hipSuccess) e = b->ozb.ensure(plane, false, 4);
    } else {
        e = b->xyz.ensure(3 * plane, false, 4);
    }
    if (e == hipSuccess) e = b->ppxy.ensure(plane, false, 4);
    return e;
}

static void point_planes(const sv_batch* b, PipeBuffers& bf) {
    if (b->out_planes) {
        bf.ox = b->oxb.as<float>();
        bf.oy = b->oyb.as<float>();
        bf.oz = b->ozb.as<float>();
        bf.ofs = (int64_t)b->cap;
    } else {
        bf.ox = b->xyz.as<float>();
        bf.oy = bf.ox + b->cap;
        bf.oz = bf.oy + b->cap;
        bf.ofs = 3 * (int64_t)b->cap;
    }
    bf.pxy = b->ppxy.as<uint32_t>();
    bf.cap = (int64_t)b->cap;
}

// The pipeline's four output planes (X, Y, Z, planePoints), placed like K1's (k1_place): where they land moves the resident pipeline
// by up to 8 % (5.85-5.96 ms, one placement in four 6.36-6.46 ms). On a large batch's first resident call,
// up to two more sets are allocated beside the current one (at most half the free memory), one call is timed
// on each (all held), and the fastest set is kept. SVX_PIPE_TRIES=1 turns it off.
static hipError_t pipe_place(sv_batch* b, const KParams& p, PipeBuffers bf, hipStream_t s) {
    int tries = 3;
    if (const char* e = svx_knob("SVX_PIPE_TRIES")) tries = std::max(1, std::atoi(e));
    const size_t plane = sizeof(float) * b->cap * (size_t)b->frames;
    const size_t set_b = 4 * (plane + plane / 4);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    tries = (int)std::min<size_t>((size_t)tries, 1 + free_b / 2 / set_b);
    if (tries <= 1) return hipSuccess;
    std::vector<std::array<DevBuf, 4>> sets((size_t)tries);
    sets[0] = {b->oxb, b->oyb, b->ozb, b->ppxy};
    std::vector<float> set_ms((size_t)tries, 0.f);
    int placed = tries;   // sets allocated
    hipError_t e = hipSuccess;
    // Two passes over the sets, each set's time the faster of its two timed calls: the kernel speeds up over
    // its first calls on a cold GPU (clocks; 6.8-7.0 -> 5.8 ms), which a single pass in set order would charge
    // to the first sets.
    for (int pass = 0; pass < 2 && e == hipSuccess; ++pass) {
        for (int t = 0; t < placed && e == hipSuccess; ++t) {
            auto& c = sets[(size_t)t];
            for (int k = 0; k < 4 && e == hipSuccess && t > 0 && pass == 0; ++k) e = c[k].ensure(plane, false, 4);
            if (e != hipSuccess) {   // out of memory: place among the sets held so far
                (void)hipGetLastError();
                for (int k = 0; k < 4; ++k) c[k].release();
                e = hipSuccess;
                placed = t;
                break;
            }
            bf.ox = c[0].as<float>();
            bf.oy = c[1].as<float>();
            bf.oz = c[2].as<float>();
            bf.ofs = (int64_t)b->cap;
            bf.pxy = c[3].as<uint32_t>();
            float ms = 0.f;
            for (int rep = pass == 0 ? 0 : 1; rep < 2 && e == hipSuccess; ++rep) {   // the last call is timed
                e = hipEventRecord(b->ev[0], s);
                if (e == hipSuccess) e = launch_pipeline_resident(p, bf, b->frames, true, s, true);
                if (e == hipSuccess) e = hipEventRecord(b->ev[1], s);
                if (e == hipSuccess) e = hipEventSynchronize(b->ev[1]);
                if (e == hipSuccess) e = hipEventElapsedTime(&ms, b->ev[0], b->ev[1]);
            }
            if (e != hipSuccess) break;
            if (svx_knob("SVX_CONTIG_LOG")) std::fprintf(stderr, "svx: pipeline placement %d: %.3f ms\n", t, ms);
            set_ms[(size_t)t] = pass == 0 ? ms : std::min(set_ms[(size_t)t], ms);
        }
    }
    int best = 0;
    for (int t = 1; t < placed; ++t)
        if (set_ms[(size_t)t] < set_ms[(size_t)best]) best = t;
    b->place_n[1] = std::min(placed, 8);
    for (int t = 0; t < b->place_n[1]; ++t) b->place_ms[1][t] = set_ms[(size_t)t];
    b->place_kept[1] = best;
    for (int t = 0; t < (int)sets.size(); ++t)
        for (int k = 0; k < 4; ++k) {
            DevBuf& x = sets[(size_t)t][k];
            if (t == best) {
                DevBuf* dst[4] = {&b->oxb, &b->oyb, &b->ozb, &b->ppxy};
                *dst[k] = x;
            } else if (t != 0 || best != 0) {
                x.release();
            }
        }
    return e;
}

namespace svx {

// planes: device planes, frame f uses planes[f * plane_stride] (NULL: the host plane)
int batch_pipeline_impl(sv_batch* b, const sv_camera* cam, const sv_plane* plane, double point_thr, int hist_thr,
                        int chunk, int sync, Device* d, const FramePlane* planes, int plane_stride) {
    if (!b->with_bgr) return fail(SV_E_ARG, "pipeline needs a batch created with bgr");
    KParams p = make_params(b->H, b->W, b->step, *cam, b->Wu);
    if (p.Wg > 4096 || p.Hg > 4096) return fail(SV_E_ARG, "pipeline supports grids up to 4096 x 4096");
    set_plane(p, *plane, point_thr, hist_thr);
    if (chunk <= 0) chunk = 1024;
    if (chunk > b->frames) chunk = b->frames;
    HIP_TRY(ensure_points(b));
    const size_t tiles = (size_t)pipeline_tiles_per_frame(p);
    const size_t kb_bytes = sizeof(uint16_t) * 256 * tiles * b->frames;
    const size_t pres_bytes = sizeof(uint32_t) * (kBins / 32) * tiles * b->frames;
    const size_t tc_bytes = sizeof(uint32_t) * tiles * b->frames;
    HIP_TRY(b->masks.ensure(kb_bytes + pres_bytes + 2 * tc_bytes, false, 16));
    if (int rc = ensure_tables(*d, b->H, b->W, *cam, b->stream)) return rc;
    PipeBuffers bf;
    bf.disp = b->disp.as<uint8_t>();
    bf.bgr = b->bgr.as<uint8_t>();
    bf.hist = b->hist;
    bf.counts = b->counts;
    bf.kbits = b->masks.as<uint16_t>();
    bf.pres = reinterpret_cast<uint32_t*>(b->masks.as<char>() + kb_bytes);
    bf.tcount = reinterpret_cast<uint32_t*>(b->masks.as<char>() + kb_bytes + pres_bytes);
    bf.toff = bf.tcount + tiles * b->frames;
    point_planes(b, bf);
    bf.dxbits = d->tables.dx.as<uint32_t>();
    bf.dybits = d->tables.dy.as<uint32_t>();
    bf.dxT = d->tables.dxT.as<uint32_t>();
    bf.dyT = d->tables.dyT.as<uint32_t>();
    bf.planes = planes;
    bf.plane_stride = plane_stride;
    int mode = b->pipe_mode;
    if (mode == 0) mode = (b->frames >= kResidentMinFrames && resident_supported(p)) ? 2 : 1;
    if (mode >= 2 && !resident_supported(p))
        return fail(SV_E_ARG, "frame-resident pipeline: frame too large (grid %d x %d)", p.Hg, p.Wg);
    if (mode >= 2 && !planes) {   // the host plane, stream-ordered into device memory
        HIP_TRY(b->dplane.ensure(sizeof(FramePlane)));
        FramePlane fp;
        plane_fields(fp, plane->a, plane->b, plane->c, p.f, p.B, p.cw, p.ch, point_thr, p.W, p.H);
        HIP_TRY(launch_store_plane(fp, b->dplane.as<FramePlane>(), b->stream));
        bf.planes = b->dplane.as<FramePlane>();
        bf.plane_stride = 0;
    }
    b->rbits_fresh = false;
    b->road_level = kRoadNone;   // the road images no longer belong to the points
    // the glyph tip of the obstacle stage takes this call's planes (sv_batch_road_hull)
    b->hull_planes = planes;
    b->hull_plane_stride = planes ? plane_stride : 0;
    b->hull_shared = HullPlane{plane->a, plane->b, plane->c, p.f, p.fB, p.cw, p.ch, planes ? 0u : 1u};
    if (mode >= 2 && b->road_bits && resident_road_bits_supported(p)) {   // the road bitmap too (sv_batch_road_bits)
        HIP_TRY(b->rbits.ensure(sizeof(uint32_t) * 32 * (size_t)b->H * b->frames));
        bf.rbits = b->rbits.as<uint32_t>();
        bf.rb_H = b->H;
        bf.rb_Wu = b->Wu;
        b->rbits_fresh = true;
    }
    if (mode == 2 && !b->pipe_placed && b->out_planes && b->frames >= 1024) {   // outside the timed region
        b->pipe_placed = true;
        HIP_TRY(pipe_place(b, p, bf, b->stream));
        point_planes(b, bf);
    }
    int t0, t1;
    HIP_TRY(hipEventRecord(b->ev[2], b->stream));
    HIP_TRY(b->timed_event(&t0));
    if (mode >= 2) {   // every output word (hist, counts, points) is rewritten: no memset, no host sync
        HIP_TRY(launch_pipeline_resident(p, bf, b->frames, mode != 3, b->stream, mode == 2, &b->kname[1]));
    } else {
        b->kname[1] = "svx::stage_kernel + svx::offsets_kernel";
        const int nchunks = (b->frames + chunk - 1) / chunk;
        while ((int)b->sync_ev.size() < 2 * nchunks) {
            hipEvent_t e;
            HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            b->sync_ev.push_back(e);
        }
        if (!b->stream2) HIP_TRY(hipStreamCreateWithFlags(&b->stream2, hipStreamNonBlocking));
        HIP_TRY(hipMemsetAsync(b->ctrl.p, 0, b->ctrl_bytes, b->stream));
        HIP_TRY(launch_pipeline(p, bf, b->frames, chunk, b->stream, b->stream2, b->sync_ev.data()));
    }
    HIP_TRY(b->timed_event(&t1));
    HIP_TRY(hipEventRecord(b->ev[3], b->stream));
    if (t0 >= 0) b->pending[1].push_back({t0, t1});
    b->have_ms[1] = true;
    if (sync) HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

}  // namespace svx

extern "C" {

// ---------------------------------------------------------------------------
// batch API
// ---------------------------------------------------------------------------
int sv_batch_create(int device, int frames, int H, int W, int step, int with_bgr, int with_points,
                    sv_batch** out) {
    if (!out) return fail(SV_E_ARG, "null out");
    *out = nullptr;
    if (frames < 1 || H < 2 || W < 2 || W > 65536 || (step != 1 && step != 2))
        return fail(SV_E_ARG, "sv_batch_create: need frames>=1, H>=2, 2<=W<=65536, step in {1,2} "
                              "(frames=%d H=%d W=%d step=%d)", frames, H, W, step);
    const int Wu = W;
    W = (W + 7) / 8 * 8;
    Device* d;
    if (int rc = dev_get(device, &d)) return rc;
    sv_batch* b = new sv_batch;
    b->device = device;
    b->frames = frames;
    b->H = H;
    b->W = W;
    b->Wu = Wu;
    b->step = step;
    b->with_bgr = with_bgr != 0;
    sv_camera cam0{1, 1, 0, 0};
    b->kp = make_params(H, W, step, cam0, Wu);
    b->Ng = (int64_t)b->kp.Hg * b->kp.Wg;
    b->cap = ((size_t)b->Ng + 63) / 64 * 64;   // (extra points between frames' outputs: no consistent effect, §4.1)
    b->dense_per_frame = (int64_t)b->kp.Hg * b->kp.pitch;
    const size_t px = (size_t)frames * H * W;
    hipError_t e = b->disp.ensure(px, false, 8);
    if (e == hipSuccess && b->with_bgr) e = b->bgr.ensure(px * 3, false, 8);
    b->out_planes = true;   // three planes (A/B: SVX_PIPE_PLANES=0 for SoA per frame)
    if (const char* e2 = svx_knob("SVX_PIPE_PLANES")) b->out_planes = *e2 != '0';
    if (e == hipSuccess && with_points) e = ensure_points(b);
    if (e == hipSuccess) {
        const size_t hist_b = sizeof(uint32_t) * kBins * frames, cnt_b = sizeof(int64_t) * 4 * frames;
        e = b->ctrl.ensure(hist_b + cnt_b + 64);
        if (e == hipSuccess) {
            char* base = b->ctrl.as<char>();
            b->hist = reinterpret_cast<uint32_t*>(base);
            b->counts = reinterpret_cast<int64_t*>(base + hist_b);
            b->err = reinterpret_cast<uint32_t*>(base + hist_b + cnt_b);
            b->ctrl_bytes = hist_b + cnt_b + 64;
            e = hipMemset(b->ctrl.p, 0, b->ctrl_bytes);
        }
    }
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipEventCreate(&b->ev[i]);
    if (e != hipSuccess) {
        sv_batch_destroy(b);
        return fail(SV_E_HIP, "sv_batch_create: %s", hipGetErrorString(e));
    }
    *out = b;
    return SV_OK;
}

int sv_batch_destroy(sv_batch* b) {
    if (!b) return SV_OK;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (DevBuf* x : {&b->disp, &b->bgr, &b->X, &b->Y, &b->Z, &b->oxb, &b->oyb, &b->ozb, &b->xyz, &b->ppxy, &b->ctrl, &b->masks,
                      &b->carmask, &b->road, &b->rmap, &b->nz, &b->nzcount, &b->mpts, &b->mpk, &b->rres, &b->rtab, &b->rtrace, &b->fplanes, &b->dplane, &b->abc,
                      &b->pairL, &b->pairR, &b->rsidx, &b->rtri, &b->bgrL, &b->bgrR,
                      &b->glut, &b->ghist, &b->sgflags, &b->prev0buf, &b->rdbuf, &b->rbits, &b->roff, &b->raw, &b->rmask, &b->cpack,
                      &b->cbits, &b->cimg, &b->cnz, &b->cnzcount, &b->croff, &b->hbuf, &b->rimg, &b->timg, &b->rdisp, &b->rdtab,
                      &b->jconst, &b->jwork, &b->jout, &b->jsizes, &b->jpack, &b->joffs, &b->jdin, &b->jdwork, &b->owork,
                      &b->olist, &b->gbuf, &b->rectmaps, &b->rawL, &b->rawR})
        x->release();
    if (b->hcnt) (void)hipHostFree(b->hcnt);
    if (b->cnt_ev) (void)hipEventDestroy(b->cnt_ev);
    b->sg.release();
    for (auto& ev : b->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : b->road_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : b->rd_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : b->rect_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : b->pool) (void)hipEventDestroy(ev);
    for (auto& ev : b->sync_ev) (void)hipEventDestroy(ev);
    if (b->stream2) {
        (void)hipStreamSynchronize(b->stream2);
        (void)hipStreamDestroy(b->stream2);
    }
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
    return SV_OK;
}

int sv_batch_info(const sv_batch* b, int64_t* o) {
    if (!b || !o) return fail(SV_E_ARG, "null");
    o[0] = b->kp.Hg;
    o[1] = b->kp.Wg;
    o[2] = b->kp.pitch;
    o[3] = b->Ng;
    o[4] = (int64_t)(b->disp.bytes + b->bgr.bytes + b->X.bytes * 3 + b->xyz.bytes + b->oxb.bytes * 3 + b->ppxy.bytes +
                     b->ctrl.bytes);
    o[5] = b->frames;
    o[6] = b->H;
    o[7] = b->Wu;
    return SV_OK;
}

int sv_batch_tune(sv_batch* b, int qpl, int nontemporal) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (qpl == 0) qpl = 1;
    if (qpl != 1 && qpl != 2 && qpl != 4) return fail(SV_E_ARG, "qpl must be 1, 2 or 4");
    if (nontemporal < 0 || nontemporal > 2) return fail(SV_E_ARG, "nontemporal must be 0, 1 or 2");
    b->qpl = qpl;
    b->nontemporal = nontemporal;
    return SV_OK;
}

int sv_batch_synth(sv_batch* b, int64_t first_frame_id) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (b->Wu != b->W) return fail(SV_E_ARG, "synthetic frames need W %% 8 == 0 (W=%d)", b->Wu);
    HIP_TRY(hipSetDevice(b->device));
    b->rdisp_fresh = false;
    HIP_TRY(launch_synth(b->kp, input_disp(b), b->with_bgr ? b->bgr.as<uint8_t>() : nullptr,
                         b->frames, first_frame_id, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_upload(sv_batch* b, int frame, const uint8_t* disp, const uint8_t* bgr) {
    if (!b || !disp || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "sv_batch_upload: bad args");
    if (bgr && !b->with_bgr) return fail(SV_E_ARG, "batch created without bgr");
    HIP_TRY(hipSetDevice(b->device));
    const size_t px = (size_t)b->H * b->W;
    uint8_t* dd = input_disp(b) + px * frame;
    b->rdisp_fresh = false;
    if (b->Wu == b->W) {
        HIP_TRY(hipMemcpyAsync(dd, disp, px, hipMemcpyHostToDevice, b->stream));
    } else {   // rows at the padded stride, pad columns zero (outside every grid)
        HIP_TRY(hipMemcpy2DAsync(dd, b->W, disp, b->Wu, b->Wu, b->H, hipMemcpyHostToDevice, b->stream));
        HIP_TRY(hipMemset2DAsync(dd + b->Wu, b->W, 0, b->W - b->Wu, b->H, b->stream));
    }
    if (bgr)
        HIP_TRY(hipMemcpy2DAsync(b->bgr.as<uint8_t>() + 3 * px * frame, 3 * (size_t)b->W, bgr, 3 * (size_t)b->Wu,
                                 3 * (size_t)b->Wu, b->H, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

// K1's planes, placed. K1 is a pure store stream, and where its three planes land in physical memory moves it
// by 12-15 % (4.22 vs 4.9 ms for 4096 frames, the same code and bytes): hipMalloc's pages vary it
// from allocation to allocation, contiguous planes from box state to box state. So a large batch's first
// projection allocates up to SVX_K1_TRIES (default 3) contiguous sets, times one K1 launch on each (all sets
// held until the end, so each lands elsewhere; at most half the free memory), and keeps the fastest.
static int k1_place(sv_batch* b, const KParams& p, size_t plane) {
    int tries = 3;
    if (const char* e = svx_knob("SVX_K1_TRIES")) tries = std::max(1, std::atoi(e));
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    const size_t set_b = 3 * (plane + plane / 4);   // DevBuf::ensure's slack
    if (b->frames < 1024 || set_b == 0) tries = 1;
    else tries = (int)std::min<size_t>((size_t)tries, std::max<size_t>(1, free_b / 2 / set_b));
    for (DevBuf* x : {&b->X, &b->Y, &b->Z}) x->release();   // a new size: the old planes go
    std::vector<std::array<DevBuf, 3>> sets((size_t)tries);
    int best = -1;
    float best_ms = 0.f;
    for (int t = 0; t < tries; ++t) {
        auto& c = sets[(size_t)t];
        hipError_t e = hipSuccess;
        for (int k = 0; k < 3 && e == hipSuccess; ++k) e = c[k].ensure(plane, true);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            break;
        }
        if (tries > 1) {
            float ms = 0.f;
            for (int rep = 0; rep < 2 && e == hipSuccess; ++rep) {   // the second launch is timed
                e = hipEventRecord(b->ev[0], b->stream);
                if (e == hipSuccess)
                    e = launch_project_dense(p, b->disp.as<uint8_t>(), c[0].as<float>(), c[1].as<float>(),
                                             c[2].as<float>(), b->frames, b->qpl, b->nontemporal, b->stream);
                if (e == hipSuccess) e = hipEventRecord(b->ev[1], b->stream);
                if (e == hipSuccess) e = hipEventSynchronize(b->ev[1]);
                if (e == hipSuccess) e = hipEventElapsedTime(&ms, b->ev[0], b->ev[1]);
            }
            if (e != hipSuccess) break;
            if (svx_knob("SVX_CONTIG_LOG")) std::fprintf(stderr, "svx: K1 placement %d: %.3f ms\n", t, ms);
            if (t < 8) {
                b->place_ms[0][t] = ms;
                b->place_n[0] = t + 1;
            }
            if (best < 0 || ms < best_ms) {
                best = t;
                best_ms = ms;
            }
        } else {
            best = t;
        }
    }
    int rc = SV_OK;
    if (best < 0) rc = fail(SV_E_HIP, "K1 planes: allocation failed (%zu bytes each)", plane);
    b->place_kept[0] = tries > 1 ? best : -1;
    for (int t = 0; t < (int)sets.size(); ++t) {
        for (int k = 0; k < 3; ++k) {
            DevBuf& x = sets[(size_t)t][k];
            if (t == best) {
                DevBuf& dst = k == 0 ? b->X : k == 1 ? b->Y : b->Z;
                dst = x;
            } else {
                x.release();
            }
        }
    }
    return rc;
}

int sv_batch_project(sv_batch* b, const sv_camera* cam, int sync) {
    if (!b || !cam) return fail(SV_E_ARG, "null");
    HIP_TRY(hipSetDevice(b->device));
    const size_t plane = sizeof(float) * (size_t)b->dense_per_frame * b->frames;
    KParams p = make_params(b->H, b->W, b->step, *cam, b->Wu);
    if (b->X.bytes < plane || b->Y.bytes < plane || b->Z.bytes < plane)
        if (int rc = k1_place(b, p, plane)) return rc;
    int t0, t1;
    HIP_TRY(hipEventRecord(b->ev[0], b->stream));
    HIP_TRY(b->timed_event(&t0));
    HIP_TRY(launch_project_dense(p, b->disp.as<uint8_t>(), b->X.as<float>(), b->Y.as<float>(), b->Z.as<float>(),
                                 b->frames, b->qpl, b->nontemporal, b->stream, &b->kname[0]));
    HIP_TRY(b->timed_event(&t1));
    HIP_TRY(hipEventRecord(b->ev[1], b->stream));
    if (t0 >= 0) b->pending[0].push_back({t0, t1});
    b->have_ms[0] = true;
    if (sync) HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_pipeline(sv_batch* b, const sv_camera* cam, const sv_plane* plane, double point_thr, int hist_thr,
                      int chunk, int sync) {
    if (!b || !cam || !plane) return fail(SV_E_ARG, "null");
    Device* d;
    if (int rc = dev_get(b->device, &d)) return rc;
    return batch_pipeline_impl(b, cam, plane, point_thr, hist_thr, chunk, sync, d);
}

int sv_batch_pipeline_planes(sv_batch* b, const sv_camera* cam, double point_thr, int hist_thr, int chunk,
                             int sync) {
    if (!b || !cam) return fail(SV_E_ARG, "null");
    if (!b->rres.p) return fail(SV_E_STATE, "no per-frame planes (sv_batch_ransac first)");
    Device* d;
    if (int rc = dev_get(b->device, &d)) return rc;
    HIP_TRY(b->fplanes.ensure(sizeof(FramePlane) * (size_t)b->frames));
    const RansacRes r = ransac_res(b);
    const KParams kp = make_params(b->H, b->W, b->step, *cam, b->Wu);
    HIP_TRY(launch_frame_planes(r.abc, r.trial, b->frames, kp, point_thr, b->fplanes.as<FramePlane>(), b->stream));
    const sv_plane none{0.0, 0.0, 0.0};   // per-frame planes replace it
    return batch_pipeline_impl(b, cam, &none, point_thr, hist_thr, chunk, sync, d, b->fplanes.as<FramePlane>());
}

int sv_batch_pipeline_dev(sv_batch* b, const sv_camera* cam, const double* dplane, double point_thr, int hist_thr,
                          int chunk, int sync) {
    if (!b || !cam || !dplane) return fail(SV_E_ARG, "null");
    Device* d;
    if (int rc = dev_get(b->device, &d)) return rc;
    HIP_TRY(b->dplane.ensure(sizeof(FramePlane)));
    const KParams kp = make_params(b->H, b->W, b->step, *cam, b->Wu);
    HIP_TRY(launch_frame_planes(dplane, nullptr, 1, kp, point_thr, b->dplane.as<FramePlane>(), b->stream));
    const sv_plane none{0.0, 0.0, 0.0};   // the device plane replaces it
    return batch_pipeline_impl(b, cam, &none, point_thr, hist_thr, chunk, sync, d, b->dplane.as<FramePlane>(), 0);
}

int sv_batch_read_frame_plane(sv_batch* b, int frame, double* out4) {
    if (!b || frame < 0 || frame >= b->frames || !out4) return fail(SV_E_ARG, "bad args");
    if (!b->fplanes.p) return fail(SV_E_STATE, "no per-frame planes (sv_batch_pipeline_planes first)");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    FramePlane fp;
    HIP_TRY(hipMemcpy(&fp, b->fplanes.as<FramePlane>() + frame, sizeof fp, hipMemcpyDeviceToHost));
    out4[0] = fp.a;
    out4[1] = fp.b;
    out4[2] = fp.c;
    out4[3] = fp.valid ? fp.nrm : -1.0;
    return SV_OK;
}

int sv_batch_placement(sv_batch* b, int which, float* ms, int cap, int* n, int* kept) {
    if (!b || which < 0 || which > 2 || !n || !kept || cap < 0 || (cap > 0 && !ms))
        return fail(SV_E_ARG, "sv_batch_placement: bad arguments");
    *n = b->place_n[which];
    *kept = b->place_kept[which];
    for (int t = 0; t < std::min(cap, *n); ++t) ms[t] = b->place_ms[which][t];
    return SV_OK;
}

int sv_batch_kernel_name(sv_batch* b, int which, char* buf, int cap) {
    if (!b || which < 0 || which > 2 || !buf || cap <= 0) return fail(SV_E_ARG, "sv_batch_kernel_name: bad arguments");
    const char* n = which == 2 ? (b->have_ms[2] ? "sgbm stage" : nullptr) : b->kname[which];
    if (!n) return fail(SV_E_STATE, "no kernel of this kind launched yet");
    std::snprintf(buf, (size_t)cap, "%s", n);
    return SV_OK;
}

int sv_batch_pipeline_mode(sv_batch* b, int mode) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (mode < 0 || mode > 4)
        return fail(SV_E_ARG, "pipeline mode must be 0 (auto), 1 (tiled), 2 (resident), 3 (resident, no prefetch) "
                              "or 4 (resident, pass-2 prefetch only)");
    b->pipe_mode = mode;
    return SV_OK;
}

int sv_batch_sync(sv_batch* b) {
    if (!b) return fail(SV_E_ARG, "null");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (b->err) {
        uint32_t err = 0;
        HIP_TRY(hipMemcpy(&err, b->err, 4, hipMemcpyDeviceToHost));
        if (err) return fail(SV_E_DEVICE, "pipeline look-back timed out");
    }
    return SV_OK;
}

int sv_batch_last_ms(sv_batch* b, int which, float* ms) {
    if (!b || !ms || which < 0 || which > 2) return fail(SV_E_ARG, "bad args");
    if (!b->have_ms[which]) return fail(SV_E_STATE, "no timing recorded");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipEventSynchronize(b->ev[2 * which + 1]));
    HIP_TRY(hipEventElapsedTime(ms, b->ev[2 * which], b->ev[2 * which + 1]));
    return SV_OK;
}

int sv_batch_timing(sv_batch* b, int which, double* total_ms, int64_t* count) {
    if (!b || which < 0 || which > 2 || !total_ms || !count) return fail(SV_E_ARG, "bad args");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    double tot = 0;
    for (auto& pr : b->pending[which]) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, b->pool[pr.first], b->pool[pr.second]));
        tot += ms;
    }
    *total_ms = tot;
    *count = (int64_t)b->pending[which].size();
    return SV_OK;
}

int sv_batch_timing_reset(sv_batch* b) {
    if (!b) return fail(SV_E_ARG, "null");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (auto& p : b->pending) p.clear();
    b->pool_next = 0;
    return SV_OK;
}

int sv_batch_read_dense(sv_batch* b, int frame, float* X, float* Y, float* Z) {
    if (!b || frame < 0 || frame >= b->frames || !b->X.p) return fail(SV_E_ARG, "bad args / nothing projected");
    HIP_TRY(hipSetDevice(b->device));
    const size_t n = (size_t)b->dense_per_frame, off = n * frame;
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (X) HIP_TRY(hipMemcpy(X, b->X.as<float>() + off, n * 4, hipMemcpyDeviceToHost));
    if (Y) HIP_TRY(hipMemcpy(Y, b->Y.as<float>() + off, n * 4, hipMemcpyDeviceToHost));
    if (Z) HIP_TRY(hipMemcpy(Z, b->Z.as<float>() + off, n * 4, hipMemcpyDeviceToHost));
    return SV_OK;
}

int sv_batch_read_counts(sv_batch* b, int64_t* counts) {
    if (!b || !counts) return fail(SV_E_ARG, "null");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    int64_t* tmp = new int64_t[4 * (size_t)b->frames];
    hipError_t e = hipMemcpy(tmp, b->counts, sizeof(int64_t) * 4 * b->frames, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        for (int f = 0; f < b->frames; ++f)
            for (int k = 0; k < 3; ++k) counts[3 * f + k] = tmp[4 * f + k];
    delete[] tmp;
    HIP_TRY(e);
    return SV_OK;
}

int sv_batch_read_hist(sv_batch* b, int frame, uint32_t* hist) {
    if (!b || !hist || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(hist, b->hist + (size_t)kBins * frame, 4 * kBins, hipMemcpyDeviceToHost));
    return SV_OK;
}

int sv_batch_read_points(sv_batch* b, int frame, float* xyz, int32_t* pts, int64_t cap, int64_t* n) {
    if (!b || !n || frame < 0 || frame >= b->frames || !b->ppxy.p) return fail(SV_E_ARG, "bad args");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    int64_t c[4];
    HIP_TRY(hipMemcpy(c, b->counts + 4 * (size_t)frame, sizeof c, hipMemcpyDeviceToHost));
    *n = c[2];
    if (c[2] > cap) return fail(SV_E_CAP, "capacity %lld < %lld", (long long)cap, (long long)c[2]);
    const size_t np = (size_t)c[2], cap_f = b->cap;
    if (xyz && np) {   // device layout: X, Y, Z planes of the frame (point_planes)
        std::vector<float> soa(3 * np);
        PipeBuffers bf;
        point_planes(b, bf);
        const float* src[3] = {bf.ox + bf.ofs * frame, bf.oy + bf.ofs * frame, bf.oz + bf.ofs * frame};
        for (int k = 0; k < 3; ++k)
            HIP_TRY(hipMemcpy(soa.data() + k * np, src[k], 4 * np, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < np; ++i)
            for (int k = 0; k < 3; ++k) xyz[3 * i + k] = soa[k * np + i];
    }
    if (pts && np) {   // device layout: one pp_pack word a point; the caller gets the int32 (x, y) pairs
        std::vector<uint32_t> pl(np);
        HIP_TRY(hipMemcpy(pl.data(), b->ppxy.as<uint32_t>() + cap_f * frame, 4 * np, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < np; ++i) {
            pts[2 * i] = pp_x(pl[i]);
            pts[2 * i + 1] = pp_y(pl[i]);
        }
    }
    return SV_OK;
}

int sv_batch_digest(sv_batch* b, const sv_camera* cam, int which, uint64_t* out) {
    if (!b || !cam || !out || which < 0 || which > 1) return fail(SV_E_ARG, "sv_batch_digest: bad args");
    if (which == 0 && !b->Z.p) return fail(SV_E_STATE, "sv_batch_digest: nothing projected");
    if (which == 1 && !b->ppxy.p) return fail(SV_E_STATE, "sv_batch_digest: no pipeline outputs");
    if ((b->kp.frame_px % 4) != 0) return fail(SV_E_ARG, "sv_batch_digest: H * W must be a multiple of 4");
    HIP_TRY(hipSetDevice(b->device));
    KParams p = make_params(b->H, b->W, b->step, *cam, b->Wu);
    DevBuf buf;
    HIP_TRY(buf.ensure(sizeof(uint64_t) * 8 * (size_t)b->frames));
    hipError_t e;
    if (which == 0)
        e = launch_digest_dense(p, b->disp.as<uint8_t>(), b->X.as<float>(), b->Y.as<float>(), b->Z.as<float>(),
                                b->frames, buf.as<uint64_t>(), b->stream);
    else
    {
        PipeBuffers bf;
        point_planes(b, bf);
        e = launch_digest_pipe(p, b->disp.as<uint8_t>(), b->hist, b->counts, bf, b->frames, buf.as<uint64_t>(),
                               b->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, buf.p, sizeof(uint64_t) * 8 * (size_t)b->frames, hipMemcpyDeviceToHost,
                                            b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    buf.release();
    HIP_TRY(e);
    return SV_OK;
}

// ---------------------------------------------------------------------------
// fused one-frame chain (stereovision.py:84,97-113) through a cached batch
// ---------------------------------------------------------------------------
int sv_pipeline_frame(const uint8_t* disp, const uint8_t* bgr, int H, int W, int step, const sv_camera* cam,
                      const sv_plane* plane, double point_thr, int hist_thr, int64_t* out_counts,
                      uint32_t* out_hist, float* out_xyz, int32_t* out_pts, int64_t cap) {
    if (!disp || !bgr || !cam || !plane || !out_counts)
        return fail(SV_E_ARG, "sv_pipeline_frame: null argument");
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    sv_batch* b = d->frame_batch;
    if (!b || b->H != H || b->W != W || b->step != step) {
        if (b) sv_batch_destroy(b);
        d->frame_batch = nullptr;
        if (int rc = sv_batch_create(L.device, 1, H, W, step, 1, 1, &b)) return rc;
        d->frame_batch = b;
    }
    if (int rc = sv_batch_upload(b, 0, disp, bgr)) return rc;
    if (int rc = batch_pipeline_impl(b, cam, plane, point_thr, hist_thr, 1, 1, d)) return rc;
    if (int rc = sv_batch_read_counts(b, out_counts)) return rc;
    if (out_hist)
        if (int rc = sv_batch_read_hist(b, 0, out_hist)) return rc;
    if (out_pts || out_xyz) {
        int64_t n = 0;
        if (int rc = sv_batch_read_points(b, 0, out_xyz, out_pts, cap, &n)) return rc;
    }
    return SV_OK;
}

}  // extern "C"
