// svx runtime: the software-pipelined frame loop (sv_loop) over the batch stages of the other units.
#include "svx_runtime.h"
#include "svx_tile_host.h"

// ---------------------------------------------------------------------------
// software-pipelined frame loop (stereovision.py:53-136 minus the cv2 drawing, over a sequence of batches)
// ---------------------------------------------------------------------------
// Every batch goes through the same stages on its slot's stream: input -> pre-pass -> maskpoints -> RANSAC draw ->
// RANSAC evaluation -> pipeline with the frames' own planes -> road raster + walk. A stage of batch k also waits
// for the same stage of batch k - 1 (an event on the other slot's stream), so each stage handles one batch at a
// time and in order; the evaluation of batch k also waits for batch k - 1's road pass. With two slots the steady
// state alternates two phases: batch k's evaluation beside batch k + 1's pre-pass and maskpoints, then batch k's
// pipeline and road pass beside batch k + 1's draw (one wave's dependent chain per frame). fillDisparity's previous cleaned frame is carried from
// batch to batch in a loop-owned buffer, so a sequence of batches cleans exactly as one long batch would.
namespace {
enum LoopStage { kLsInput = 0, kLsPrepass, kLsMaskpoints, kLsDraw, kLsEval, kLsPipeline, kLsRoad, kLsCount };
}

struct sv_loop {
    int device = 0;
    sv_loop_params prm{};
    sv_camera cam{};
    std::vector<sv_batch*> slot;
    std::vector<int64_t> slot_seq, slot_first;
    std::vector<std::array<hipEvent_t, kLsCount>> t0, t1;   // per slot: start / end of each stage (its last batch)
    hipEvent_t epoch = nullptr;
    // the previous batch's last cleaned frame (fillDisparity's previousDisparity), double-buffered: a submit reads
    // carry[cur] and writes carry[cur ^ 1], and only a submit that enqueued every stage makes its write current
    DevBuf carry[2];
    int carry_cur = 0;
    bool carry_valid = false;
    DevBuf gate;               // uint64: the last draw kernel whose grid is resident (its epoch = seq + 1)
    int64_t next = 0;          // sequence number of the next submitted batch
    int64_t pending = -1;      // the batch whose pipeline + road pass are not enqueued yet (see sv_loop_submit)
    int jpeg_quality = 75;     // road = 7: the streams' quality and slot capacity (sv_loop_jpeg; 0 = the default slot)
    int64_t jpeg_cap = 0;
};

// A stage of batch seq on its slot's stream: begin waits for the same stage of the batch before (on the other
// slot's stream) and records the stage's start, end records its end.
static hipError_t stage_begin(sv_loop* L, int64_t seq, int stage) {
    const int slots = L->prm.slots;
    const size_t s = (size_t)(seq % slots), ps = (size_t)((seq + slots - 1) % slots);
    hipStream_t st = L->slot[s]->stream;
    if (seq > 0 && ps != s) {
        hipError_t e = hipStreamWaitEvent(st, L->t1[ps][stage], 0);
        if (e != hipSuccess) return e;
    }
    return hipEventRecord(L->t0[s][stage], st);
}

static hipError_t stage_end(sv_loop* L, int64_t seq, int stage) {
    const size_t s = (size_t)(seq % L->prm.slots);
    return hipEventRecord(L->t1[s][stage], L->slot[s]->stream);
}

extern "C" {

int sv_loop_destroy(sv_loop* L) {
    if (!L) return SV_OK;
    (void)hipSetDevice(L->device);
    for (sv_batch* b : L->slot)
        if (b && b->stream) (void)hipStreamSynchronize(b->stream);
    for (auto& a : L->t0)
        for (auto& e : a)
            if (e) (void)hipEventDestroy(e);
    for (auto& a : L->t1)
        for (auto& e : a)
            if (e) (void)hipEventDestroy(e);
    if (L->epoch) (void)hipEventDestroy(L->epoch);
    for (DevBuf* x : {&L->carry[0], &L->carry[1], &L->gate}) x->release();
    for (sv_batch* b : L->slot) sv_batch_destroy(b);
    delete L;
    return SV_OK;
}

int sv_loop_create(int device, const sv_loop_params* prm, const sv_camera* cam, const uint8_t* carmask,
                   sv_loop** out) {
    if (!prm || !cam || !out) return fail(SV_E_ARG, "sv_loop_create: null argument");
    *out = nullptr;
    const sv_loop_params& q = *prm;
    if (q.frames < 1 || q.slots < 1 || q.slots > 8 || (q.source != 0 && q.source != 1) || q.prepass < 0 ||
        q.prepass > 2 || q.road < 0 || q.road > 7 || (q.step != 1 && q.step != 2) || q.trials < 0 || q.k < 1)
        return fail(SV_E_ARG, "sv_loop_create: bad parameters (frames >= 1, 1 <= slots <= 8, source 0/1, prepass "
                              "0..2, road 0..7, step 1/2, trials >= 0, k >= 1)");
    if (q.road >= 6)   // the image tile's shape (sv_batch_tile would refuse it only after a batch's other stages)
        if (const char* why = tile_check_shape(q.H, q.W))
            return fail(SV_E_ARG, "sv_loop_create: road >= 6 (the image tile) takes frames with %s", why);
    // what a submit would only find out after enqueueing the input and pre-pass stages (the RANSAC and synthetic
    // input limits of batch_ransac_prepare / sv_batch_synth)
    if (q.trials > 4096 || q.k > 1024) return fail(SV_E_ARG, "sv_loop_create: RANSAC trials <= 4096, k <= 1024");
    if (q.H > 4096 || q.W > 4096) return fail(SV_E_ARG, "sv_loop_create: frames up to 4096 x 4096");
    if ((int64_t)grid_len(q.H, 2) * grid_len(q.W, 2) > 163840)
        return fail(SV_E_ARG, "sv_loop_create: more than 163,840 step-2 grid points per frame (RANSAC)");
    if (q.source == 1 && q.W % 8) return fail(SV_E_ARG, "sv_loop_create: synthetic frames need W %% 8 == 0 (W=%d)", q.W);
    sv_loop* L = new sv_loop;
    L->device = device;
    L->prm = q;
    L->cam = *cam;
    L->slot.assign((size_t)q.slots, nullptr);
    L->slot_seq.assign((size_t)q.slots, -1);
    L->slot_first.assign((size_t)q.slots, 0);
    L->t0.resize((size_t)q.slots);
    L->t1.resize((size_t)q.slots);
    for (auto& a : L->t0) a.fill(nullptr);
    for (auto& a : L->t1) a.fill(nullptr);
    int rc = SV_OK;
    for (int i = 0; i < q.slots && rc == SV_OK; ++i) {
        rc = sv_batch_create(device, q.frames, q.H, q.W, q.step, 1, 1, &L->slot[(size_t)i]);
        if (rc == SV_OK) L->slot[(size_t)i]->timing = false;
        if (rc == SV_OK && q.source == 0) {   // caller-fed: the frames the caller writes stay as written
            sv_batch* sb = L->slot[(size_t)i];
            const hipError_t ee = sb->raw.ensure(sb->disp.bytes);
            if (ee != hipSuccess) rc = fail(SV_E_HIP, "sv_loop_create: %s", hipGetErrorString(ee));
            else sb->keep_input = true;
        }
        if (rc == SV_OK && carmask) rc = sv_batch_set_mask(L->slot[(size_t)i], carmask);
        if (rc == SV_OK && q.road == 2) rc = sv_batch_road_map(L->slot[(size_t)i], 1);
        if (rc == SV_OK && q.road) rc = sv_batch_road_bits(L->slot[(size_t)i], 1);
    }
    hipError_t e = hipSuccess;
    if (rc == SV_OK) {
        e = hipSetDevice(device);
        for (int i = 0; i < q.slots && e == hipSuccess; ++i)
            for (int st = 0; st < kLsCount && e == hipSuccess; ++st) {
                e = hipEventCreate(&L->t0[(size_t)i][st]);
                if (e == hipSuccess) e = hipEventCreate(&L->t1[(size_t)i][st]);
            }
        if (e == hipSuccess) e = hipEventCreate(&L->epoch);
        for (DevBuf& c : L->carry)
            if (e == hipSuccess) e = c.ensure((size_t)L->slot[0]->H * L->slot[0]->W);
        if (e == hipSuccess) e = L->gate.ensure(sizeof(uint64_t));
        if (e == hipSuccess) e = hipMemset(L->gate.p, 0, sizeof(uint64_t));
        if (e != hipSuccess) rc = fail(SV_E_HIP, "sv_loop_create: %s", hipGetErrorString(e));
    }
    if (rc != SV_OK) {
        const std::string msg = last_error();
        sv_loop_destroy(L);
        set_error(msg);
        return rc;
    }
    *out = L;
    return SV_OK;
}

static int loop_flush(sv_loop* L);

int sv_loop_road_mask(sv_loop* L, const uint8_t* mask) {
    if (!L) return fail(SV_E_ARG, "sv_loop_road_mask: null loop");
    for (sv_batch* b : L->slot)
        if (int rc = sv_batch_road_mask(b, mask)) return rc;
    return SV_OK;
}

int sv_loop_jpeg(sv_loop* L, int quality, int64_t cap_per_frame) {
    if (!L) return fail(SV_E_ARG, "sv_loop_jpeg: null loop");
    if (quality < 1 || quality > 100 || cap_per_frame < 0 || cap_per_frame > 0x7FFFFFFF)
        return fail(SV_E_ARG, "sv_loop_jpeg: 1 <= quality <= 100, 0 <= cap_per_frame < 2^31");
    if (L->next > 0) return fail(SV_E_STATE, "sv_loop_jpeg: set before the first sv_loop_submit");
    L->jpeg_quality = quality;
    L->jpeg_cap = cap_per_frame;
    return SV_OK;
}

// The batch the next sv_loop_submit processes (source 0: the caller fills it first); waits on the host until
// the batch that last used its slot has finished every stage.
int sv_loop_acquire(sv_loop* L, sv_batch** out) {
    if (!L || !out) return fail(SV_E_ARG, "sv_loop_acquire: null argument");
    const size_t s = (size_t)(L->next % L->prm.slots);
    HIP_TRY(hipSetDevice(L->device));
    if (L->pending >= 0 && (size_t)(L->pending % L->prm.slots) == s)
        if (int rc = loop_flush(L)) return rc;   // (one slot) the batch held there still has its tail to run
    if (L->slot_seq[s] >= 0) HIP_TRY(hipEventSynchronize(L->t1[s][kLsRoad]));
    *out = L->slot[s];
    return SV_OK;
}

// The pipeline and road pass of batch seq (slot s), behind a dispatch gate on the draw kernel of batch seq + 1
// when that has been enqueued (gate_epoch > 0): the draw's 4096 one-wave workgroups are a dependent chain each
// and must all be resident to finish in one pass, so they are placed first and the pipeline takes what is left
// of the CUs; launched together, the pipeline's workgroups would take the LDS and the draw would run in rounds.
static int loop_enqueue_tail(sv_loop* L, int64_t seq, uint64_t gate_epoch) {
    const sv_loop_params& q = L->prm;
    sv_batch* b = L->slot[(size_t)(seq % q.slots)];
    hipStream_t st = b->stream;
    if (gate_epoch) HIP_TRY(launch_loop_gate(L->gate.as<uint64_t>(), gate_epoch, 50.0, st));
    // the pipeline with every frame's own plane (stereovision.py:97-113)
    HIP_TRY(stage_begin(L, seq, kLsPipeline));
    if (int rc = sv_batch_pipeline_planes(b, &L->cam, q.point_thr, q.hist_thr, 0, 0)) return rc;
    HIP_TRY(stage_end(L, seq, kLsPipeline));
    // road raster + non-zero walk (+ imageRoadMap) (stereovision.py:131-156)
    HIP_TRY(stage_begin(L, seq, kLsRoad));
    if (q.road) {
        if (int rc = sv_batch_road_raster(b, 0)) return rc;
    }
    if (q.road >= 3) {   // sanitiseRoadImage's clean-up of the images just made (functions.py:346-366)
        if (int rc = sv_batch_road_clean(b, 0)) return rc;
    }
    if (q.road >= 4) {   // the obstacle stage on the cleaned images (stereovision.py:170-189)
        if (int rc = sv_batch_road_hull(b, 0)) return rc;
    }
    if (q.road >= 5) {   // the result image from the BGR and the obstacle stage (stereovision.py:181-209)
        if (int rc = sv_batch_result(b, 0)) return rc;
    }
    if (q.road >= 6) {   // batchImages' tile of the five pictures above (stereovision.py:216)
        if (int rc = sv_batch_tile(b, 0)) return rc;
    }
    if (q.road == 7) {   // the recording (loop.py:49-54,82-89): the tiles' JPEG streams, packed for one copy
        if (int rc = sv_batch_jpeg(b, L->jpeg_quality, L->jpeg_cap, 0)) return rc;
        if (int rc = sv_batch_jpeg_pack(b, 0)) return rc;
    }
    HIP_TRY(stage_end(L, seq, kLsRoad));
    if (L->pending == seq) L->pending = -1;
    return SV_OK;
}

static int loop_flush(sv_loop* L) {
    if (L->pending < 0) return SV_OK;
    HIP_TRY(hipSetDevice(L->device));
    return loop_enqueue_tail(L, L->pending, 0);
}

// Enqueue order of sv_loop_submit(k), slot s = k % slots, the previous batch k - 1 on slot ps:
//   slot s:  input(k) -> pre-pass(k) -> maskpoints(k)   [without a carmask the host reads k's counts: they size
//            the draw launch; with one, the mask's step-2 points bound them and nothing is read]
//   slot s:  draw(k)  (after batch k - 1's evaluation: a frame's evaluation needs a whole CU's LDS)
//   slot ps: gate(draw(k) resident) -> pipeline(k - 1) -> road(k - 1)
//   slot s:  evaluation(k)  (after road(k - 1): beside pre-pass(k + 1) and maskpoints(k + 1), which use no LDS)
// so batch k's pipeline and road pass are enqueued by the next submit (or by sv_loop_wait / _timeline).
int sv_loop_submit(sv_loop* L, int64_t first_frame_id, int64_t* out_seq) {
    if (!L) return fail(SV_E_ARG, "sv_loop_submit: null loop");
    if (first_frame_id < 0) return fail(SV_E_ARG, "sv_loop_submit: first_frame_id >= 0");
    const sv_loop_params& q = L->prm;
    const int64_t seq = L->next;
    const size_t s = (size_t)(seq % q.slots), ps = (size_t)((seq + q.slots - 1) % q.slots);
    sv_batch* b = L->slot[s];
    hipStream_t st = b->stream;
    HIP_TRY(hipSetDevice(L->device));
    if (q.slots == 1) {   // one slot: nothing to overlap, the previous batch's tail first
        if (int rc = loop_flush(L)) return rc;
    }
    if (seq == 0) HIP_TRY(hipEventRecord(L->epoch, st));
    // input: for synthetic frames, the batch's global frame ids generated on the device
    HIP_TRY(stage_begin(L, seq, kLsInput));
    if (q.source == 1) {
        if (b->Wu != b->W) return fail(SV_E_ARG, "synthetic frames need W %% 8 == 0 (W=%d)", b->Wu);
        HIP_TRY(launch_synth(b->kp, input_disp(b), b->bgr.as<uint8_t>(), b->frames, first_frame_id, st));
    }
    HIP_TRY(stage_end(L, seq, kLsInput));
    // pre-pass (stereovision.py:53-76): frame 0 cleaned with the previous batch's last cleaned frame
    HIP_TRY(stage_begin(L, seq, kLsPrepass));
    bool carried = false;
    {   // option 0 (no pre-pass) still runs: a caller-fed slot (keep_input) holds its frames in `raw`, and the
        // impl copies them into `disp`, which every later stage reads
        const uint8_t* prev = q.prepass == 1 && L->carry_valid ? L->carry[L->carry_cur].as<uint8_t>() : nullptr;
        if (int rc = batch_prepass_impl(b, q.prepass, prev)) return rc;
        if (q.prepass == 1) {
            const size_t px = (size_t)b->H * b->W;
            HIP_TRY(hipMemcpyAsync(L->carry[L->carry_cur ^ 1].p, b->disp.as<uint8_t>() + px * (b->frames - 1), px,
                                   hipMemcpyDeviceToDevice, st));
            carried = true;
        }
    }
    HIP_TRY(stage_end(L, seq, kLsPrepass));
    // maskpoints (stereovision.py:74-85): the masked step-2 points of every frame, their counts to the host
    HIP_TRY(stage_begin(L, seq, kLsMaskpoints));
    if (int rc = batch_ransac_prepare(b, &L->cam, q.trials, q.k)) return rc;
    HIP_TRY(stage_end(L, seq, kLsMaskpoints));
    // RANSAC draw (stereovision.py:94): frame g draws after random.seed(seed_base + g); sized from the carmask's
    // bound of the counts (no host wait; without a mask the host waits here for this batch's counts, with the
    // previous batch's evaluation already enqueued)
    if (seq > 0 && ps != s) HIP_TRY(hipStreamWaitEvent(st, L->t1[ps][kLsEval], 0));
    HIP_TRY(stage_begin(L, seq, kLsDraw));
    if (int rc = batch_ransac_launch(b, &L->cam, q.seed_base, first_frame_id, q.trials, q.k, st, 1,
                                     L->gate.as<uint64_t>(), (uint64_t)seq + 1))
        return rc;
    HIP_TRY(stage_end(L, seq, kLsDraw));
    // the previous batch's pipeline and road pass, gated on this draw's dispatch
    if (L->pending >= 0) {
        if (int rc = loop_enqueue_tail(L, L->pending, (uint64_t)seq + 1)) return rc;
    }
    // RANSAC evaluation, after the previous batch's road pass (after its pipeline, or after this batch's draw
    // only, measured equal: DESIGN §8.2)
    if (seq > 0 && ps != s) HIP_TRY(hipStreamWaitEvent(st, L->t1[ps][kLsRoad], 0));
    HIP_TRY(stage_begin(L, seq, kLsEval));
    if (int rc = batch_ransac_launch(b, &L->cam, q.seed_base, first_frame_id, q.trials, q.k, st, 2)) return rc;
    HIP_TRY(stage_end(L, seq, kLsEval));
    if (carried) {   // every stage enqueued: this batch's last cleaned frame is the next batch's previous one
        L->carry_cur ^= 1;
        L->carry_valid = true;
    }
    L->pending = seq;
    L->slot_seq[s] = seq;
    L->slot_first[s] = first_frame_id;
    L->next = seq + 1;
    if (out_seq) *out_seq = seq;
    return SV_OK;
}

static int loop_slot_of(sv_loop* L, int64_t seq, size_t* out) {
    if (!L || seq < 0) return fail(SV_E_ARG, "sv_loop: bad arguments");
    const size_t s = (size_t)(seq % L->prm.slots);
    if (L->slot_seq[s] != seq)
        return fail(SV_E_STATE, "sv_loop: batch %lld is not held (submitted: %lld, slots: %d)", (long long)seq,
                    (long long)L->next, L->prm.slots);
    *out = s;
    return SV_OK;
}

int sv_loop_wait(sv_loop* L, int64_t seq) {
    size_t s;
    if (int rc = loop_slot_of(L, seq, &s)) return rc;
    if (int rc = loop_flush(L)) return rc;
    HIP_TRY(hipSetDevice(L->device));
    HIP_TRY(hipEventSynchronize(L->t1[s][kLsRoad]));
    return SV_OK;
}

int sv_loop_batch(sv_loop* L, int64_t seq, sv_batch** out, int64_t* first_frame_id) {
    size_t s;
    if (!out) return fail(SV_E_ARG, "sv_loop_batch: null out");
    if (int rc = loop_slot_of(L, seq, &s)) return rc;
    // the batch's pipeline and road pass may not be enqueued yet (the next submit enqueues them): enqueue them and
    // wait for them, so that sv_batch_read_* of the returned batch never mixes this batch's RANSAC with the points
    // and road images of the batch the slot held before
    if (L->pending == seq)
        if (int rc = loop_flush(L)) return rc;
    HIP_TRY(hipSetDevice(L->device));
    HIP_TRY(hipEventSynchronize(L->t1[s][kLsRoad]));
    *out = L->slot[s];
    if (first_frame_id) *first_frame_id = L->slot_first[s];
    return SV_OK;
}

int sv_loop_timeline(sv_loop* L, int64_t seq, double* out) {
    size_t s;
    if (!out) return fail(SV_E_ARG, "sv_loop_timeline: null out");
    if (int rc = loop_slot_of(L, seq, &s)) return rc;
    if (int rc = loop_flush(L)) return rc;
    HIP_TRY(hipSetDevice(L->device));
    HIP_TRY(hipEventSynchronize(L->t1[s][kLsRoad]));
    for (int st = 0; st < kLsCount; ++st) {
        float a = 0.f, z = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, L->epoch, L->t0[s][st]));
        HIP_TRY(hipEventElapsedTime(&z, L->epoch, L->t1[s][st]));
        out[2 * st] = a;
        out[2 * st + 1] = z;
    }
    return SV_OK;
}

}  // extern "C"
