// The runtime's internal header: the error slot, the device state and the batch object that the runtime's units
// (runtime.hip, rt_*.hip) and comm.hip share. Host-only: never included by kernels/*.hip. Its helpers live in
// namespace svx (like the launchers of svx_launch.h), so none of them reads as a C ABI name.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/svx.h"
#include "svx_ground_host.h"
#include "svx_hull.h"
#include "svx_launch.h"
#include "svx_sgbm.h"

using namespace svx;   // every includer is a unit of the runtime

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
namespace svx {
// the thread-local message behind sv_last_error (runtime.hip holds it)
int fail(int code, const char* fmt, ...);
void set_error(const std::string& msg);
const std::string& last_error();
}  // namespace svx

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(SV_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                              \
    } while (0)

// ---------------------------------------------------------------------------
// per-device state
// ---------------------------------------------------------------------------
namespace svx {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    // contiguous: physically contiguous pages (hipDeviceMallocContiguous, falling back to hipMalloc). With
    // hipMalloc's pages, where K1's planes land decides how its three store streams spread over the HBM
    // channels: K1 took 4.35-5.0 ms from one allocation to the next, 4.23-4.34 ms contiguous.
    // SVX_CONTIG: 0 = never, 2 = every large buffer (A/B).
    // exact: no 1/4 growth slack (the SGBM volumes, 16 GB each at 128 frames, whose size follows the chunk)
    hipError_t ensure(size_t n, bool contiguous = false, int tag = 0, bool exact = false) {
        if (n <= bytes) return hipSuccess;
        release();
        size_t want = n < 4096 ? 4096 : exact ? n : n + n / 4;
        hipError_t e = hipErrorUnknown;
        static const int mode = [] {
            const char* v = svx_knob("SVX_CONTIG");
            return v && *v ? std::atoi(v) : 1;
        }();
        // A/B: SVX_CONTIG bit 4 also the pipeline outputs (tag 4), 8 the inputs (tag 8), 16 the masks (tag 16)
        if (mode != 0 && (contiguous || mode == 2 || (mode & tag)) && want >= (256u << 20)) {
            e = hipExtMallocWithFlags(&p, want, hipDeviceMallocContiguous);
            if (svx_knob("SVX_CONTIG_LOG"))
                std::fprintf(stderr, "svx: contiguous %zu bytes: %s\n", want, hipGetErrorString(e));
            if (e != hipSuccess) {
                (void)hipGetLastError();
                p = nullptr;
            }
        }
        if (e != hipSuccess) e = hipMalloc(&p, want);
        if (e == hipSuccess) bytes = want;
        return e;
    }
    // free and zero (no destructor: g_dev[] is static, and the HIP runtime may be gone by then)
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// SGBM scratch for a chunk of frames (kernels/sgbm.hip): four int16 cost
// volumes, the int16 disparity, union-find parents / sizes, overflow flags.
struct SgbmBufs {
    DevBuf vol[4], raw, d16, par, size, flags;
    int frames = 0;
    bool placed = false;   // the volumes came from sgbm_place (re-placed when they have to grow)
    hipError_t ensure_rest(const SgbmK& k, int n) {   // the per-pixel scratch (the volumes: sgbm_place)
        const size_t px = (size_t)k.frame_px * n;
        hipError_t e = raw.ensure(px * sizeof(int16_t));
        if (e == hipSuccess) e = d16.ensure(px * sizeof(int16_t));
        if (e == hipSuccess) e = par.ensure(px * sizeof(int32_t));
        if (e == hipSuccess) e = size.ensure(px * sizeof(int32_t));
        if (e == hipSuccess) e = flags.ensure(sizeof(uint32_t) * n);
        return e;
    }
    hipError_t ensure(const SgbmK& k, int n) {
        const size_t vb = sgbm_volume_bytes(k) * n;
        hipError_t e = hipSuccess;
        // the cost volumes physically contiguous: 32.37 vs 33.09 ms per 128 frames over five alternating
        // processes with every large buffer contiguous (profiles/r04/ab_sgbm_contig.txt); the walks stream them
        // (sgbm_place allocates them first for a large chunk and keeps the faster of two sets)
        for (int i = 0; i < 4 && e == hipSuccess; ++i) e = vol[i].ensure(vb, true, 0, true);
        if (e == hipSuccess) e = ensure_rest(k, n);
        if (e == hipSuccess) frames = n;
        return e;
    }
    size_t held_bytes() const {
        size_t n = 0;
        for (const DevBuf* x : {&vol[0], &vol[1], &vol[2], &vol[3], &raw, &d16, &par, &size}) n += x->bytes;
        return n;
    }
    SgbmScratch scratch() const {
        return SgbmScratch{vol[0].as<uint32_t>(), vol[1].as<uint32_t>(), vol[2].as<uint32_t>(), vol[3].as<uint32_t>(),
                           raw.as<int16_t>(), d16.as<int16_t>(), par.as<int32_t>(), size.as<int32_t>(),
                           flags.as<uint32_t>()};
    }
    void release() {
        for (DevBuf* x : {&vol[0], &vol[1], &vol[2], &vol[3], &raw, &d16, &par, &size, &flags}) x->release();
    }
};

struct Tables {
    bool valid = false;
    int H = 0, W = 0;
    sv_camera cam{};
    DevBuf dx, dy;
    DevBuf dxT, dyT;   // transposed (launch_delta_transpose): the resident pipeline's lane-contiguous delta stage
};

// The ground grid's mapping (svx_ground_host.h: the folded cell table) of one (camera, grid, W), made on the host in
// fp64.
struct GroundMap {
    bool valid = false;
    int W = 0;
    sv_camera cam{};
    sv_grid grid{};
    DevBuf tab;
};

struct Device {
    bool init = false;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // drop-in scratch
    DevBuf disp, bgr, xyz, rgb, ctrl, xy, aux, aux2;
    DevBuf mbits;                     // sv_sanitise_road: the image, the cleaned image and the mask as bitmaps
    DevBuf hull;                      // sv_road_obstacles: bitmaps, vertices and info (HullLayout)
    DevBuf objs, objwork;             // sv_obstacle_list: the bitmap, the entries and the count; the labelling scratch
    DevBuf ground;                    // sv_ground_grid: the two bitmaps, the planes, the profile and the totals
    GroundMap gmap;                   // the ground grid's mapping, shared with the device's batches (ensure_ground_map)
    DevBuf res;                       // sv_result_image: image, obstacle bitmap, vertices and info (ResultLayout)
    DevBuf tile;                      // sv_image_tile: the staged result image and the tile (TileLayout)
    DevBuf rsz;                       // sv_resize_linear_u8, sv_images_tile: tables, staged pictures, stack, output
    DevBuf rmp;                       // sv_remap_u8: the map pair, the staged pictures and the remapped ones
    DevBuf jpg;                       // sv_jpeg_encode: tables, the staged picture, the scratch and the stream
    DevBuf jdin, jdwork, jdout;       // sv_jpeg_decode(_many): descriptors, tables and streams; scratch; pictures
    float jd_ms[4] = {0, 0, 0, 0};    // the last sv_jpeg_decode_many's four kernels (sv_jpeg_decode_stage_ms)
    bool jd_have_ms = false;
    DevBuf sg_l, sg_r, sg_out, sg_filt, sg_hist;   // host-frame SGBM / grey drop-ins
    SgbmBufs sg;
    Tables tables;
    sv_batch* frame_batch = nullptr;  // cached 1-frame batch for sv_pipeline_frame
};

inline int grid_len(int n, int step) { return n > 1 ? (n - 1 + step - 1) / step : 0; }

// W: the row stride of the frames in memory; Wu: the frame's own width (the
// grid range(0, Wu-1, step) of functions.py:185-186), 0 = W. A batch of any
// width stores its rows at a stride rounded up to 8 bytes (aligned quad loads).
KParams make_params(int H, int W, int step, const sv_camera& cam, int Wu = 0);
void set_plane(KParams& p, const sv_plane& pl, double thr, int hist_thr);
int dev_get(int device, Device** out);
int current_device(int* dev);
// Delta tables for (H, W, camera), built on the device in fp64 (tables.hip).
int ensure_tables(Device& d, int H, int W, const sv_camera& cam, hipStream_t s);
// The ground grid's mapping for (camera, grid, W) in d.gmap (rt_ground.hip), under the device's mutex. A new key
// waits for the whole device first: a batch's launch may still be reading the mapping it replaces.
int ensure_ground_map(Device& d, const sv_camera& cam, const sv_grid& grid, int W);

// A device's scratch + stream, under its mutex: every drop-in's prologue.
struct Locked {
    Device* d = nullptr;
    int device = -1;
    std::unique_lock<std::mutex> lk;
};
int lock_device(int device, Locked& L);
int lock_current(Locked& L);   // the calling thread's current device

// upload an H x W u8 host image into a pitch = round_up(W, 4) device buffer (zero pad)
int upload_u8(DevBuf& buf, const uint8_t* src, int H, int W, int pitch, hipStream_t s);
int download_u8(uint8_t* dst, const DevBuf& buf, int H, int W, int pitch, hipStream_t s);

// How far the road chain of the batch's current pipeline points has come. Each stage needs the level below it,
// drops the chain to that level on entry and raises it once its work is enqueued, so a call that fails midway
// leaves the level of the stage below; a pipeline call starts over.
enum RoadLevel {
    kRoadNone,        // the road images (if any) are not of the current points
    kRoadImages,      // sv_batch_road_raster: road holds the images of the current points
    kRoadCleaned,     // sv_batch_road_clean: cbits / cimg / cnz hold the clean-up of those images
    kRoadObstacles,   // sv_batch_road_hull: hbuf holds the obstacle stage of that clean-up
    kRoadResult,      // sv_batch_result: rimg holds the result image of that obstacle stage
    kRoadTile,        // sv_batch_tile: timg holds the image tile of that result image
    kRoadJpeg         // sv_batch_jpeg: jout / jsizes hold the JPEG streams of that tile
};
// the road chain's events in sv_batch::road_ev, made by a stage's first call: the clean-up's start, its kernel's
// start / end and its end, then start / end of the obstacle stage, of the result image, of the image tile and of its
// JPEG streams, of the obstacle list, of the ground grid
enum {
    kEvClean = 0, kEvHull = 4, kEvResult = 6, kEvTile = 8, kEvJpeg = 10, kEvObjects = 12, kEvGround = 14,
    kEvRoadCount = 16
};

}  // namespace svx

// ---------------------------------------------------------------------------
// batch object
// ---------------------------------------------------------------------------
struct sv_batch {
    int device = 0;
    int frames = 0, H = 0, W = 0, step = 1;
    int Wu = 0;                // the frames' own width; W = row stride = round_up(Wu, 8)
    bool with_bgr = false;
    KParams kp{};
    int64_t Ng = 0;            // grid points per frame
    size_t cap = 0;            // per-frame point capacity of the pipeline outputs (Ng rounded up to 64)
    int64_t dense_per_frame = 0;
    hipStream_t stream = nullptr;    // K1, pass 1 (stream A)
    hipStream_t stream2 = nullptr;   // tiled pipeline's offsets kernels (stream B), beside the stage launches; made
                                     // on the first tiled call: streams share the device's few hardware queues (4),
                                     // and two streams on one queue run in order, so no stream is made unused
    std::vector<hipEvent_t> sync_ev; // pipeline hand-offs between A and B (timing disabled)
    DevBuf disp, bgr, X, Y, Z, xyz, ctrl, masks;
    DevBuf ppxy;                // the pipeline's planePoints: one pp_pack word (x, y as int16 halves) a point
    DevBuf oxb, oyb, ozb;       // pipeline X, Y, Z: three planes of frames x cap (default; SoA in xyz: A/B)
    bool out_planes = false;
    bool pipe_placed = false;   // the resident pipeline's outputs were placed (pipe_place)
    DevBuf carmask;             // maskDisparity's 0x00/0xFF mask (H x W)
    DevBuf road, nz, nzcount;   // road images (frames x H x W), their non-zero walks (frames x cap x 2)
    DevBuf rmap;                // imageRoadMap (stereovision.py:131-133): frames x H x W x 3, on request
    bool road_bits = false;     // the resident pipeline also writes the road bitmap (sv_batch_road_bits)
    bool rbits_fresh = false;   // rbits holds the bitmap of the current pipeline points
    DevBuf rbits, roff;         // the bitmap (frames x H x 32 words); the road pass's per-row walk offsets
    bool want_rmap = false, rmap_fresh = false;
    RoadLevel road_level = kRoadNone;   // which of road / cimg / hbuf / rimg / timg / jout belong to the current points
    hipEvent_t road_ev[kEvRoadCount] = {};
    // sanitiseRoadImage's clean-up (sv_batch_road_clean): the mask as a bitmap (behind its staged bytes), the packed
    // road images (when the pipeline wrote no bitmap), the cleaned bitmaps, images, walks (frames x ccap packed
    // entries: a cleaned image can hold more pixels than the pipeline has points), counts and row offsets
    DevBuf rmask, cpack, cbits, cimg, cnz, cnzcount, croff;
    bool have_rmask = false;
    size_t ccap = 0;            // walk entries per frame of cnz: H x Wu rounded up to 64
    // the obstacle stage (sv_batch_road_hull): hull masks, obstacles, vertices and infos (HullLayout); the planes
    // of the last pipeline call (device planes at a stride, else the shared host plane) for the glyph tip
    DevBuf hbuf;
    const FramePlane* hull_planes = nullptr;
    int hull_plane_stride = 0;
    HullPlane hull_shared{};
    // the obstacle list (sv_batch_obstacle_list; rt_objects.hip), a side branch of the chain at kRoadObstacles: the
    // labelling scratch (ObjLayout), frames x olist_cap entries with the frames' counts behind them; olist_fresh:
    // they are of the current obstacle stage (sv_batch_road_hull clears it). olist_host: the whole of olist, copied
    // by the first read after a call (4096 lists of 16 are 3.7 MB: one copy, not two small ones a frame)
    DevBuf owork, olist;
    std::vector<char> olist_host;
    int olist_cap = 0;
    bool olist_fresh = false, olist_host_fresh = false;
    // the ground grid (sv_batch_ground_grid; rt_ground.hip), a side branch like the list: the results of ggrid
    // (GroundLayout); ggrid_fresh: they are of the current obstacle stage (sv_batch_road_hull clears it)
    DevBuf gbuf;
    sv_grid ggrid{};
    bool ggrid_fresh = false;
    // the result image (sv_batch_result): frames x H rows of 3 W bytes, the BGR's layout; made on first use
    DevBuf rimg;
    // the image tile (sv_batch_tile): frames x H / 2 rows of 3 Wu bytes, packed; made on first use
    DevBuf timg;
    // the tile's JPEG streams (sv_batch_jpeg; rt_jpeg.hip): the tables and header of jquality (jhost: the host block
    // they are copied from), the scratch of a chunk of jchunk frames, frames slots of jcap bytes, the sizes; the
    // packed run and its frames + 1 offsets (sv_batch_jpeg_pack; jpacked: of the current streams)
    DevBuf jconst, jwork, jout, jsizes, jpack, joffs;
    std::vector<uint8_t> jhost;
    int jquality = 0, jchunk = 0;
    int64_t jcap = 0;
    bool jpacked = false;
    // the decoder of sv_batch_decode_bgr_pair (rt_jpeg_dec.hip): descriptors, tables and streams of one side; the
    // scratch of a chunk of frames; the ms of the last call's kernels
    DevBuf jdin, jdwork;
    float jd_ms = 0;
    bool jd_have_ms = false;
    // the cleaned disparity at a display size (sv_batch_resize_disp): frames x rd_h x rd_w bytes, packed, and the
    // coefficient tables of that size (svx_resize_host.h); made on first use. rdisp_fresh: it is the resize of what
    // `disp` holds now: whatever writes the batch's frames or cleans them again clears it.
    DevBuf rdisp, rdtab;
    int rd_h = 0, rd_w = 0, rdtab_h = 0, rdtab_w = 0;
    bool rdisp_fresh = false;
    hipEvent_t rd_ev[2] = {nullptr, nullptr};
    // the rectification (sv_batch_rectify; rt_rectify.hip): the two eyes' maps of rect_h x rect_w, the pair shape
    // they were uploaded for (0: none); the second store of the BGR pairs, made by the first call. A call remaps
    // bgrL / bgrR into rawL / rawR and swaps the stores, so that bgrL / bgrR hold the rectified pairs and rawL / rawR
    // the pictures as they came; rect_done says so, and whatever writes a pair swaps them back first
    // (pair_store_written), so a frame written after a call lands beside the other frames' raw pictures.
    DevBuf rectmaps, rawL, rawR;
    int rect_h = 0, rect_w = 0;
    bool rect_done = false, rect_have_ms = false;
    hipEvent_t rect_ev[2] = {nullptr, nullptr};
    DevBuf mpts, rres;          // one frame's maskpoints as fp64 (read-back scratch); counts + batched RANSAC results
    DevBuf prev0buf, rdbuf;     // the host prev0 of sv_batch_prepass; sv_batch_read_disp's masked frame (batch-owned:
                                // the device-wide drop-in scratch is used on other streams)
    int64_t* hcnt = nullptr;    // pinned host copy of the maskpoints counts (sized frames), read by the RANSAC launch
    hipEvent_t cnt_ev = nullptr;   // the counts' copy has landed in hcnt
    DevBuf rtab;                // fp64 X / Y / Z tables of the step-2 grid (the last sv_batch_ransac's camera)
    DevBuf mpk;                 // maskpoints packed (frames x mcap words x | y << 12 | d << 24): RANSAC's fp32 screen
    DevBuf rtrace;              // optional: frames x trace_trials x (k + 3) drawn indices
    DevBuf rsidx, rtri;         // batched RANSAC scratch: every trial's sample; trial records + frame status
    DevBuf fplanes;             // per-frame keep1 plane fields (FramePlane) for sv_batch_pipeline_planes
    DevBuf dplane;              // the FramePlane of a device plane (sv_batch_pipeline_dev)
    DevBuf abc;                 // this batch's slot for a broadcast plane (sv_comm_broadcast_plane_dev)
    DevBuf pairL, pairR;        // rectified grey stereo pairs (frames x pairH x pairW each), SGBM input
    int pairH = 0, pairW = 0;   // the pairs' shape: the batch's (H, W), or (Hp, Wp) whose crop is the batch
    DevBuf bgrL, bgrR, glut, ghist;   // BGR stereo pairs (frames x pairH x pairW x 3), gamma table, hist scratch
    SgbmBufs sg;                // SGBM scratch for one chunk of frames
    DevBuf sgflags;             // SGBM range flags, one word per frame of the batch
    int64_t mcap = 0;
    int64_t rmax_n = 0, rmax_pool_n = 0;   // the last RANSAC draw launch's largest frame (they size the eval too)
    int64_t rbound = -1;        // the last prepare's device-side bound of the counts (-1: the counts are read back)
    int trace_trials = 0, trace_k = 0, traced_trials = 0;   // requested; k and trials of the recorded trace
    bool have_mask = false;
    // keep_input (a caller-fed frame loop slot): the frames written by synth / upload / sgbm go to `raw`, and the
    // pre-pass reads them there and writes the cleaned frames to `disp`, so resubmitting the slot cleans the same
    // raw frames again (fillDisparity returns a new array, functions.py:140-147)
    bool keep_input = false;
    DevBuf raw;
    int64_t mask_n2 = 0;        // the mask's points on the step-2 grid (an upper bound of every frame's maskpoints)
    // pipeline control block (one memset per call): hist | counts | err
    uint32_t* hist = nullptr;
    int64_t* counts = nullptr;
    uint32_t* err = nullptr;
    size_t ctrl_bytes = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    float last_ms[3] = {0, 0, 0};
    bool have_ms[3] = {false, false, false};
    int qpl = 1;               // K1 quads per lane (1, 2 or 4)
    int nontemporal = 1;       // K1 store flavour (non-temporal: measured faster)
    int pipe_mode = 0;         // 0 auto, 1 tiled (pipeline.hip), 2 frame-resident (resident.hip, both
                               // passes prefetch the next chunk), 3 same without prefetch, 4 pass-2 prefetch only
    // per-launch timing accumulator: event pairs recorded on the batch stream
    std::vector<hipEvent_t> pool;
    std::vector<std::pair<int, int>> pending[3];  // (start idx, end idx) per op kind: project, pipeline, sgbm
    size_t pool_next = 0;
    // the placement probes of the first K1 / resident pipeline call (k1_place / pipe_place): each set's timed
    // call (ms), how many sets were tried and which one was kept (-1: no probe ran)
    float place_ms[3][8] = {};
    int place_n[3] = {0, 0, 0}, place_kept[3] = {-1, -1, -1};
    // the kernel instance the last timed call of each kind launched (rocprofv3's name; sv_batch_kernel_name)
    const char* kname[3] = {nullptr, nullptr, nullptr};
    bool timing = true;        // record per-launch timing events (off for a frame loop's slots: they run unbounded)
    hipError_t timed_event(int* idx) {
        if (!timing) {
            *idx = -1;
            return hipSuccess;
        }
        if (pool_next == pool.size()) {
            hipEvent_t e;
            hipError_t r = hipEventCreate(&e);
            if (r != hipSuccess) return r;
            pool.push_back(e);
        }
        *idx = (int)pool_next++;
        return hipEventRecord(pool[*idx], stream);
    }
};

namespace svx {

// where the batch's frames are written: the raw-input buffer (keep_input) or the disparity the stages read
inline uint8_t* input_disp(sv_batch* b) { return b->keep_input ? b->raw.as<uint8_t>() : b->disp.as<uint8_t>(); }

// Before a BGR pair is written (upload, decode, synth): after a rectify the raw store becomes the pair store again.
// Host pointers only: what is enqueued on the batch's stream keeps the addresses it was given, and what follows is
// enqueued behind it.
inline void pair_store_written(sv_batch* b) {
    if (!b->rect_done) return;
    std::swap(b->bgrL, b->rawL);
    std::swap(b->bgrR, b->rawR);
    b->rect_done = false;
}

struct RansacRes {   // layout of b->rres
    double* abc;
    double* err;
    int32_t* trial;
    uint32_t* flags;
    int64_t* mcount;
};
inline RansacRes ransac_res(sv_batch* b) {
    RansacRes r;
    const size_t F = (size_t)b->frames;
    r.abc = b->rres.as<double>();
    r.err = r.abc + 3 * F;
    r.mcount = reinterpret_cast<int64_t*>(r.err + F);
    r.trial = reinterpret_cast<int32_t*>(r.mcount + F);
    r.flags = reinterpret_cast<uint32_t*>(r.trial + F);
    return r;
}

// What the frame loop (rt_loop.hip) calls of the stages' units.
// rt_prepass.hip: the pre-pass over the batch's frames in order; dprev0: frame 0's previous cleaned frame in
// device memory (the frame loop's carry from the batch before), or null.
int batch_prepass_impl(sv_batch* b, int option, const uint8_t* dprev0);
// rt_ransac.hip: batched RANSAC in two phases (see there)
int batch_ransac_prepare(sv_batch* b, const sv_camera* cam, int trials, int k);
int batch_ransac_launch(sv_batch* b, const sv_camera* cam, uint64_t seed_base, int64_t first_frame, int trials, int k,
                        hipStream_t stream, int phases = 3, uint64_t* started = nullptr, uint64_t epoch = 0);
// rt_batch.hip: the pipeline behind the three batch entries and sv_pipeline_frame
int batch_pipeline_impl(sv_batch* b, const sv_camera* cam, const sv_plane* plane, double point_thr, int hist_thr,
                        int chunk, int sync, Device* d, const FramePlane* planes = nullptr, int plane_stride = 1);

}  // namespace svx
