// Frame-resident pipeline (gfx950), config 4: one workgroup owns one frame.
//
// Same chain as pipeline.hip (stereovision.py:97-113): keep1 = dist(P, plane)
// < point_thr (functions.py:300-323); hist = hue-bin counts over keep1
// (functions.py:215-226); keep2 = keep1 & hist[bin] > hist_thr
// (functions.py:228-230); the keep2 points in raster order as fp32 X, Y, Z +
// the int32 (x, y) back-projection (functions.py:201-209, stereovision.py:112) as int16 halves of one word.
//
// keep1 is evaluated per grid point from the frame's plane (FramePlane: the
// per-call plane, the frame's own RANSAC plane, or a plane broadcast into
// device memory): the division-free fp32 test |u - d| < t*d (keep1_lean) with
// a rigorous guard, the reference's fp64 arithmetic inside the guard. A chunk
// whose rows the plane rules out for every d in 1..255 (the u range at its
// corners, rows_keepable) reads no BGR and evaluates no keep1.
//
// Because one workgroup walks its frame chunk by chunk (chunk = 256 lanes x
// QPL quads x 4 grid points, raster order), nothing crosses workgroups: the
// histogram lives in LDS, the output offset is a running register, and there
// are no tickets, look-back, global atomics or hand-off buffers.
//
//   pass 1  per chunk: disparity + BGR + table in; the colours of keep1 points
//           are packed densely into the wave's LDS region and binned there
//           (fp32 hue, exact integer/fp64 path in the tie band) with LDS
//           atomics whose return value marks "candidate" chunks: a point whose
//           bin had fewer than hist_thr points before it. A bin that ends
//           <= hist_thr has ALL its points candidates, so only candidate
//           ("dirty") chunks can lose keep1 points in pass 2.
//   pass 2  per chunk: disparity + table in; dirty chunks re-read BGR and drop
//           points whose bin ends <= hist_thr (dense, same LDS staging); block
//           scan; 4-byte descriptors (d | gy | gx) scattered into LDS; lane j
//           then produces outputs 4j..4j+3 with 16-byte non-temporal stores to
//           the SoA planes, so every store instruction is contiguous.
#include "../svx_launch.h"

namespace svx {

constexpr int kRMaxChunks = 256;   // chunks per frame at the default 4 quads per lane (= maxchunks_of<4>)
constexpr int kRBins = 1000;    // bins 0..999: t < 1000 - 1000/(6*255) so rint(t) <= 999
// Pass 2 stages the back-projection delta words (tables.hip: dx bits [256][dx_words],
// dy bits [256][dy_words]) of kRDN consecutive disparities — the chunk's keep1
// range, recorded by pass 1 — in LDS: dx rows at stride 33 words (bank spread),
// then the kRDN dy words of the chunk's 32-row word. The scatter looks up each
// kept point's two delta bits there ("narrow" chunk: keep1 range within kRDN
// disparities, one row word, dx_words <= 32) or in the tables in memory, and
// packs them into its descriptor (rdesc).
constexpr int kRDN = 32;
constexpr int kRDxStride = 33;
constexpr int kRDyOff = kRDN * kRDxStride;
// Lane-contiguous quads (LC) stage the same window transposed, from dxT / dyT (tables.hip): one word per
// x whose bit dd is the delta bit of d = dlo + dd, in groups of 16 x at a stride of 20 words (16-byte aligned,
// so a lane's 16 consecutive x are four ds_read_b128 without bank conflicts between its 8-lane groups), then
// one word per row of the chunk's 32-row word. A lane's 16 points then cost four LDS reads for dx and one
// for dy instead of 16 + 16.
constexpr int kRTxGroup = 20;
constexpr int kRTyOff = 64 * kRTxGroup;   // x < 1024 (dx_words <= 32)
constexpr int kRDeltaWords = kRTyOff + 32 > kRDyOff + kRDN ? kRTyOff + 32 : kRDyOff + kRDN;

// both 16-bit halves: max (v_pk_max_u16)
__device__ __forceinline__ uint32_t pk_max16(uint32_t a, uint32_t b) {
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}


template <int STEP, int QP, bool LC>
struct RCfg {
    static constexpr int QPL = QP;                 // quads per lane per chunk
    static constexpr int CW = 3 * STEP;            // BGR dwords per quad
};
template <int STEP>
constexpr int default_qpl() { return STEP == 1 ? 4 : 2; }
// Per-workgroup chunk = 256 lanes x QP quads = 1024 * QP grid points; the LDS
// stage holds one chunk's outputs; a frame has at most 2^20 quads.
template <int QP>
constexpr int stage_of() { return 1024 * QP; }
template <int QP>
constexpr int maxchunks_of() { return 1024 / QP; }

int resident_chunks_per_frame(const KParams& p, int qpl) {
    const int per = 256 * qpl;
    return (p.frame_quads + per - 1) / per;
}

// ---------------------------------------------------------------------------
// Streaming loops
// ---------------------------------------------------------------------------
struct RParams {      // what the streaming kernel needs (kept small: SGPR budget)
    int W, Wg, Q, pitch, frame_quads, nchunks, hist_thr, dx_words, dy_words, ablate;
    int drow, dq;   // a chunk's quads (QPL * 256) as whole rows + quads
    uint64_t Q_m40;
    int64_t frame_px;
    float B32, fB32, cw_hi, cw_lo, ch_hi, ch_lo;
};

// quad slot i of lane tid in chunk c. Default: slot-major ((c * QPL + i) * 256
// + tid: each load instruction covers 256 contiguous quads). LC (lane-contiguous;
// step 1, Q % 4 == 0, W % 16 == 0, so a lane's QPL quads are one 16-byte-aligned
// run of one row): c * QPL * 256 + tid * QPL + i, loaded with one wide load per plane.
template <int QPL, bool LC>
__device__ __forceinline__ int r_qi(int c, int tid, int i) {
    return LC ? c * QPL * 256 + tid * QPL + i : (c * QPL + i) * 256 + tid;
}

template <int STEP, int QP, bool LC>
struct RQuads {   // this lane's quads of one chunk
    int gy[RCfg<STEP, QP, LC>::QPL];   // grid row, -1 past the frame end
    int q[RCfg<STEP, QP, LC>::QPL];    // quad within the row
};

template <int STEP, int QP, bool LC>
__device__ __forceinline__ void r_geometry(int c, int tid, const RParams& p, RQuads<STEP, QP, LC>& g) {
    constexpr int QPL = RCfg<STEP, QP, LC>::QPL;
#pragma unroll
    for (int i = 0; i < QPL; ++i) {
        const int qi = r_qi<QPL, LC>(c, tid, i);
        const bool ok = qi < p.frame_quads;
        const int qc = ok ? qi : p.frame_quads - 1;
        const int gy = fastdiv40(qc, p.Q_m40);
        g.q[i] = qc - gy * p.Q;
        g.gy[i] = ok ? gy : -1;
    }
}

// the geometry of chunk c from that of chunk c - 1 (all its quads inside the
// frame): every quad slot advances by drow rows and dq quads, no division
template <int STEP, int QP, bool LC>
__device__ __forceinline__ void r_geometry_next(int c, int tid, const RParams& p, RQuads<STEP, QP, LC>& g) {
    constexpr int QPL = RCfg<STEP, QP, LC>::QPL;
#pragma unroll
    for (int i = 0; i < QPL; ++i) {
        int q = g.q[i] + p.dq, gy = g.gy[i] + p.drow;
        const bool wrap = q >= p.Q;
        q -= wrap ? p.Q : 0;
        gy += wrap ? 1 : 0;
        const bool ok = r_qi<QPL, LC>(c, tid, i) < p.frame_quads;
        g.q[i] = ok ? q : p.Q - 1;   // past the end: an in-range load address (row 0), gy = -1
        g.gy[i] = ok ? gy : -1;
    }
}

// byte offset of quad (gy, q) in a frame plane with `bpp` bytes per pixel
// (24-bit multiplies: full-rate, operands < 2^24 for frames the resident kernel takes)
template <int STEP, int QP, bool LC>
__device__ __forceinline__ uint32_t r_off(int gy, int q, int bpp, const RParams& p) {
    const uint32_t px = __umul24((uint32_t)(gy < 0 ? 0 : gy) * STEP, (uint32_t)p.W) + 4u * STEP * (uint32_t)q;
    return bpp == 3 ? 3u * px : px;
}

template <int STEP, int QP, bool LC>
__device__ __forceinline__ void r_load_disp(const uint8_t* fdisp, const RQuads<STEP, QP, LC>& g, const RParams& p,
                                            uint32_t (&dw)[RCfg<STEP, QP, LC>::QPL][STEP]) {
    if constexpr (LC) {   // the lane's QPL (= 4) quads: one 16-byte load
        static_assert(STEP == 1 && RCfg<STEP, QP, LC>::QPL == 4, "lane-contiguous quads: step 1, 4 quads a lane");
        const uint4 w = *reinterpret_cast<const uint4*>(fdisp + r_off<STEP, QP, LC>(g.gy[0], g.q[0], 1, p));
        dw[0][0] = w.x;
        dw[1][0] = w.y;
        dw[2][0] = w.z;
        dw[3][0] = w.w;
        return;
    }
#pragma unroll
    for (int i = 0; i < RCfg<STEP, QP, LC>::QPL; ++i) {
        const uint8_t* a = fdisp + r_off<STEP, QP, LC>(g.gy[i], g.q[i], 1, p);
        if constexpr (STEP == 1) {
            dw[i][0] = *reinterpret_cast<const uint32_t*>(a);
        } else {
            const uint2 w = *reinterpret_cast<const uint2*>(a);
            dw[i][0] = w.x;
            dw[i][1] = w.y;
        }
    }
}

template <int STEP, int QP, bool LC>
__device__ __forceinline__ void r_load_bgr(const uint8_t* fbgr, const RQuads<STEP, QP, LC>& g, const RParams& p,
                                           uint32_t (&cw)[RCfg<STEP, QP, LC>::QPL][RCfg<STEP, QP, LC>::CW]) {
    if constexpr (LC) {   // 48 contiguous bytes: three 16-byte loads, quad i = dwords 3i .. 3i + 2
        const uint4* cp = reinterpret_cast<const uint4*>(fbgr + r_off<STEP, QP, LC>(g.gy[0], g.q[0], 3, p));
        const uint4 x = cp[0], y = cp[1], z = cp[2];
        const uint32_t v[12] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w, z.x, z.y, z.z, z.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            cw[i][0] = v[3 * i];
            cw[i][1] = v[3 * i + 1];
            cw[i][2] = v[3 * i + 2];
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < RCfg<STEP, QP, LC>::QPL; ++i) {
        const uint8_t* a = fbgr + r_off<STEP, QP, LC>(g.gy[i], g.q[i], 3, p);
        if constexpr (STEP == 1) {
            const uint32_t* cp = reinterpret_cast<const uint32_t*>(a);
            cw[i][0] = cp[0];
            cw[i][1] = cp[1];
            cw[i][2] = cp[2];
        } else {
            const uint2* cp = reinterpret_cast<const uint2*>(a);
            const uint2 x = cp[0], y = cp[1], z = cp[2];
            cw[i][0] = x.x; cw[i][1] = x.y; cw[i][2] = y.x; cw[i][3] = y.y; cw[i][4] = z.x; cw[i][5] = z.y;
        }
    }
}

// disparity byte of point k of a quad
template <int STEP, int QP, bool LC>
__device__ __forceinline__ uint32_t r_d(const uint32_t (&w)[STEP], int k) {
    if constexpr (STEP == 1) return (w[0] >> (8 * k)) & 0xFF;
    else return (w[k >> 1] >> (16 * (k & 1))) & 0xFF;
}

// colour (B | G<<8 | R<<16, top byte junk) of point k of a quad
template <int STEP, int QP, bool LC>
__device__ __forceinline__ uint32_t r_col(const uint32_t (&c)[RCfg<STEP, QP, LC>::CW], int k) {
    const int o = 3 * STEP * k, w = o >> 2, sh = o & 3;
    const uint32_t hi = (w + 1 < RCfg<STEP, QP, LC>::CW) ? c[w + 1] : 0u;
    return sh == 0 ? c[w] : __builtin_amdgcn_alignbyte(hi, c[w], sh);
}


// The reference's keep1 in fp64 (functions.py:191-193, :300-323), op for op.
// Plane and camera are read from memory here (the rare path), so that they do
// not occupy registers for the whole kernel.
__device__ __forceinline__ bool r_keep1_f64(int x, int y, uint32_t d, const FramePlane* Lp) {
    const double f = Lp->f, cw = Lp->cw, ch = Lp->ch;
    const double Z = Lp->fB / (double)d;
    const double X = (((double)x - cw) * Z) / f;
    const double Y = (((double)y - ch) * Z) / f;
    const double dot = __builtin_fma(Z, Lp->c, __builtin_fma(X, Lp->a, Y * Lp->b));
    return __builtin_fabs((dot - 1.0) / Lp->nrm) < Lp->thr;
}

// The fp32 constants of keep1_lean for one frame (uniform, scalar registers).
struct RLean {
    float al, bb, b0, tn, g;
};

// keep1 bits of this lane's chunk (bit 4i+k = point k of quad i) under the
// frame's plane: keep1_lean in fp32 (the same fp32 operations as keep1_lean,
// svx_device.h), the fp64 reference arithmetic for the points inside its guard
// (rare; one fp64 evaluation site, looped over the lane's uncertain points).
template <int STEP, int QP, bool LC>
__device__ __forceinline__ uint32_t r_keep1(const uint32_t (&dw)[RCfg<STEP, QP, LC>::QPL][STEP], const RQuads<STEP, QP, LC>& g,
                                            const RLean& L, const FramePlane* Lp, int Wg) {
    constexpr int QPL = RCfg<STEP, QP, LC>::QPL;
    uint32_t keep = 0, unc = 0;
#pragma unroll
    for (int i = 0; i < QPL; ++i) {
        const float beta = __builtin_fmaf(L.bb, (float)(max(g.gy[i], 0) * STEP), L.b0);
        uint32_t k4 = 0, u4 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t d = r_d<STEP, QP, LC>(dw[i], k);
            const float df = (float)d;
            const float u = __builtin_fmaf(L.al, (float)((4 * g.q[i] + k) * STEP), beta);
            const float s = u - df;
            const float e = __builtin_fmaf(-L.tn, df, __builtin_fabsf(s));
            k4 |= (uint32_t)(e < 0.0f) << k;
            u4 |= (uint32_t)(!(__builtin_fabsf(e) > L.g) && d != 0) << k;
        }
        // rows past the frame end and the pad columns gx >= Wg (the grid stops at W - 1) keep nothing
        const int nin = Wg - 4 * g.q[i];
        const uint32_t in = g.gy[i] < 0 ? 0u : (nin >= 4 ? 0xFu : (1u << max(nin, 0)) - 1u);
        keep |= (k4 & in) << (4 * i);
        unc |= (u4 & in) << (4 * i);
    }
    if (__builtin_expect(__ballot(unc != 0) != 0, 0)) {
        uint32_t m = unc;
        while (m) {   // per lane
            const uint32_t b = __builtin_ctz(m);
            m &= m - 1;
            int x = 0, y = 0;
            uint32_t d = 0;
#pragma unroll
            for (int i = 0; i < QPL; ++i) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool hit = b == (uint32_t)(4 * i + k);
                    x = hit ? (4 * g.q[i] + k) * STEP : x;
                    y = hit ? g.gy[i] * STEP : y;
                    d = hit ? r_d<STEP, QP, LC>(dw[i], k) : d;
                }
            }
            keep = r_keep1_f64(x, y, d, Lp) ? (keep | (1u << b)) : (keep & ~(1u << b));
        }
    }
    return keep;
}

// grid points with d != 0 in this lane's chunk (pad columns and rows past the end excluded)
template <int STEP, int QP, bool LC>
__device__ __forceinline__ uint32_t r_nvalid(const uint32_t (&dw)[RCfg<STEP, QP, LC>::QPL][STEP], const RQuads<STEP, QP, LC>& g,
                                             const RParams& p) {
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < RCfg<STEP, QP, LC>::QPL; ++i) {
        const int nin = g.gy[i] < 0 ? 0 : min(4, p.Wg - 4 * g.q[i]);
        uint32_t v;   // the quad's 4 disparity bytes, point k at byte k
        if constexpr (STEP == 1) v = dw[i][0];
        else v = __builtin_amdgcn_perm(dw[i][1], dw[i][0], 0x06040200u);
        v &= nin >= 4 ? 0xFFFFFFFFu : ((1u << (8 * nin)) - 1u);
        const uint32_t nz = (((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u;
        n += __builtin_popcount(nz);
    }
    return n;
}

// The hue bin of a kept colour: hue_bin_sel (svx_device.h), fp32 with the exact path in the tie band. (A 392 KB
// (rng, n) -> bin table gather instead: 7.40 vs 6.32 ms per call)
__device__ __forceinline__ uint32_t r_bin_sel(uint32_t col) { return hue_bin_sel(col); }

// Pack the colours of the keep bits into this wave's LDS region, (lane, bit)
// order, without branching on lane masks: a point that is not kept writes its
// colour to this lane's private dump slot instead. Returns the wave's total
// and this lane's first slot.
template <int STEP, int QP, bool LC>
__device__ __forceinline__ uint32_t r_stage_colours_sel(uint32_t keep,
                                                        const uint32_t (&cw)[RCfg<STEP, QP, LC>::QPL][RCfg<STEP, QP, LC>::CW],
                                                        uint32_t* wstage, uint32_t* dump, uint32_t& pos0) {
    const uint32_t cnt = __builtin_popcount(keep);
    const uint32_t inc = wave_incl_scan(cnt);
    pos0 = inc - cnt;
    uint32_t pos = pos0;
#pragma unroll
    for (int i = 0; i < RCfg<STEP, QP, LC>::QPL; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t bit = (keep >> (4 * i + k)) & 1u;
            *(bit ? wstage + pos : dump) = r_col<STEP, QP, LC>(cw[i], k);
            pos += bit;
        }
    }
    return __shfl(inc, 63, kWave);
}

typedef float v4f __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));

template <int STEP, int QP, bool LC>
struct P1Regs {
    RQuads<STEP, QP, LC> g;
    uint32_t dw[RCfg<STEP, QP, LC>::QPL][STEP];
    uint32_t cw[RCfg<STEP, QP, LC>::QPL][RCfg<STEP, QP, LC>::CW];
};

template <int STEP, int QP, bool LC>
struct P2Regs {
    RQuads<STEP, QP, LC> g;
    uint32_t dw[RCfg<STEP, QP, LC>::QPL][STEP];
    uint32_t kb;                 // step 1: the keep1 bits of pass 1 (step 2 evaluates keep1 again)
    uint32_t fx[kRDN / 8], fy;   // the chunk's staged delta words (this lane's share)
    uint32_t fx2[4], fy2;        // LC: the transposed window's next words (funnel-shifted with fx, fy)
    int dlo, ywb;                // first staged disparity; the chunk's 32-row word
    bool narrow;                 // the chunk's keep1 range and rows fit the stage
    bool staged, reuse;          // a window is staged in LDS; this chunk reuses it (no loads, no stage writes)
};

template <int STEP, int QP, bool LC>
__device__ __forceinline__ void p1_load(P1Regs<STEP, QP, LC>& r, int c, int tid, const uint8_t* fdisp, const uint8_t* fbgr,
                                        const RParams& p, bool next, bool any) {
    if (next) r_geometry_next<STEP, QP, LC>(c, tid, p, r.g);   // r.g holds chunk c - 1
    else r_geometry<STEP, QP, LC>(c, tid, p, r.g);
    r_load_disp<STEP, QP, LC>(fdisp, r.g, p, r.dw);
    if (any) r_load_bgr<STEP, QP, LC>(fbgr, r.g, p, r.cw);   // uniform: a chunk the plane rules out needs only its valid count
}

template <int STEP, int QP, bool LC>
__device__ __forceinline__ void p2_load(P2Regs<STEP, QP, LC>& r, int c, int tid, const uint8_t* fdisp,
                                        const uint32_t* crange, const PipeBuffers& bf, const RParams& p, bool next,
                                        bool run, const uint16_t* fkb) {
    if (next) r_geometry_next<STEP, QP, LC>(c, tid, p, r.g);   // r.g holds chunk c - 1
    else r_geometry<STEP, QP, LC>(c, tid, p, r.g);
    if (!run) return;   // uniform: a chunk pass 2 skips (none of its grid points can be kept)
    r_load_disp<STEP, QP, LC>(fdisp, r.g, p, r.dw);
    if constexpr (STEP == 1) r.kb = fkb[c * 256 + tid];   // pass 1's keep1 bits (this lane wrote them)
    // delta words of the chunk's keep1 disparities (pass 1's range), written to
    // LDS at the chunk's start; every index is clamped in range, so the loads
    // are unconditional (whatever crange holds)
    const uint4 cr = *reinterpret_cast<const uint4*>(crange + 4 * c);
    const uint32_t w = pk_max16(pk_max16(cr.x, cr.y), pk_max16(cr.z, cr.w));
    const int dmn = max(0, 255 - (int)(w >> 16)), dmx = (int)(w & 0xFFFFu);
    const int dlo = min(dmn, 256 - kRDN);
    constexpr int per = RCfg<STEP, QP, LC>::QPL * 256;   // quads per chunk
    const int ywb = (fastdiv40(c * per, p.Q_m40) * STEP) >> 5;
    const int ywl = (fastdiv40(min((c + 1) * per, p.frame_quads) - 1, p.Q_m40) * STEP) >> 5;
    // the window staged for the last chunk pass 2 ran still covers this one (same row word, keep1 range inside):
    // no delta loads and no stage writes (8192: DIAGNOSTIC A/B, always reload)
    r.reuse = !ablated(p.ablate, 8192 | 1024) && r.staged && p.dx_words <= 32 && ywl == ywb &&
              ywb == r.ywb && dmn >= r.dlo && dmx < r.dlo + kRDN;
    if (r.reuse) {
        r.narrow = true;
        return;
    }
    r.staged = true;
    r.dlo = dlo;
    r.ywb = ywb;
    r.narrow = !ablated(p.ablate, 1024) && p.dx_words <= 32 && dmx - dlo < kRDN && ywl == ywb;   // 1024: DIAGNOSTIC A/B
    if constexpr (LC) {   // transposed: words dlo >> 5 and the next of x = 4 tid .. 4 tid + 3 and of row 32 ywb + tid
        const int j0 = dlo >> 5, j1 = min(j0 + 1, 7);
        const int nx = 32 * p.dx_words, ny = 32 * p.dy_words;
        const int x4 = min(4 * tid, nx - 4);   // nx is a multiple of 32
        const uint4 a = *reinterpret_cast<const uint4*>(bf.dxT + j0 * nx + x4);
        const uint4 b = *reinterpret_cast<const uint4*>(bf.dxT + j1 * nx + x4);
        r.fx[0] = a.x, r.fx[1] = a.y, r.fx[2] = a.z, r.fx[3] = a.w;
        r.fx2[0] = b.x, r.fx2[1] = b.y, r.fx2[2] = b.z, r.fx2[3] = b.w;
        const int yr = min(32 * ywb + (tid & 31), ny - 1);
        r.fy = bf.dyT[j0 * ny + yr];
        r.fy2 = bf.dyT[j1 * ny + yr];
    } else {
        const int xw = min(tid & 31, p.dx_words - 1);
#pragma unroll
        for (int j = 0; j < kRDN / 8; ++j) r.fx[j] = bf.dxbits[(dlo + 8 * j + (tid >> 5)) * p.dx_words + xw];
        r.fy = bf.dybits[(dlo + (tid & (kRDN - 1))) * p.dy_words + min(ywb, p.dy_words - 1)];
    }
}

// stage the chunk's delta words (loaded by p2_load) into dl: dx word (d, xw) at
// (d - dlo) * kRDxStride + xw, dy word of d at kRDyOff + d - dlo
template <int STEP, int QP, bool LC>
__device__ __forceinline__ void p2_stage_deltas(const P2Regs<STEP, QP, LC>& r, uint32_t* dl) {
    const int tid = threadIdx.x;
    if constexpr (LC) {   // x = 4 tid .. 4 tid + 3: bits dlo .. dlo + 31 of each x's 256-bit row
        const uint32_t sh = (uint32_t)(r.dlo & 31);
        uint4 w;
        w.x = __builtin_amdgcn_alignbit(r.fx2[0], r.fx[0], sh);
        w.y = __builtin_amdgcn_alignbit(r.fx2[1], r.fx[1], sh);
        w.z = __builtin_amdgcn_alignbit(r.fx2[2], r.fx[2], sh);
        w.w = __builtin_amdgcn_alignbit(r.fx2[3], r.fx[3], sh);
        *reinterpret_cast<uint4*>(dl + (tid >> 2) * kRTxGroup + 4 * (tid & 3)) = w;
        if (tid < 32) dl[kRTyOff + tid] = __builtin_amdgcn_alignbit(r.fy2, r.fy, sh);
    } else {
#pragma unroll
        for (int j = 0; j < kRDN / 8; ++j) dl[(8 * j + (tid >> 5)) * kRDxStride + (tid & 31)] = r.fx[j];
        if (tid < kRDN) dl[kRDyOff + tid] = r.fy;
    }
}

// this wave's keep1 disparity range of the chunk as (255 - dmin) << 16 | dmax
// (0 when nothing is kept): byte masks from the keep nibbles, no per-point branch
template <int STEP, int QP, bool LC>
__device__ __forceinline__ uint32_t r_keep_range(const uint32_t (&dw)[RCfg<STEP, QP, LC>::QPL][STEP], uint32_t keep) {
    uint32_t dmn = 255, dmx = 0;
#pragma unroll
    for (int i = 0; i < RCfg<STEP, QP, LC>::QPL; ++i) {
        uint32_t v;   // the quad's 4 disparity bytes, point k at byte k
        if constexpr (STEP == 1) v = dw[i][0];
        else v = __builtin_amdgcn_perm(dw[i][1], dw[i][0], 0x06040200u);
        const uint32_t nib = (keep >> (4 * i)) & 0xFu;
        // bit k -> byte k = 0xFF: v_perm selector 0x0C gives a 0x00 byte, 0x0D a 0xFF byte
        const uint32_t m = __builtin_amdgcn_perm(0u, 0u, ((__umul24(nib, 0x00204081u) & 0x01010101u) + 0x0C0C0C0Cu));
        const uint32_t vx = v & m, vn = v | ~m;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dmx = max(dmx, (vx >> (8 * k)) & 0xFFu);
            dmn = min(dmn, (vn >> (8 * k)) & 0xFFu);
        }
    }
    // max-scan (identity 0) of both halves; lane 63 holds the wave's
    const uint32_t w = wave_scan_dpp(((255u - dmn) << 16) | dmx, pk_max16);
    return __builtin_amdgcn_readlane(w, 63);
}

// pass 1 of one chunk: keep1, valid/kept counts, dense hue binning into hist,
// candidate mark into dirty, keep1 disparity range into crange. Wave-local (no barrier).
template <int STEP, int QP, bool LC>
__device__ __forceinline__ void p1_chunk(const P1Regs<STEP, QP, LC>& r, int c, uint32_t* hist, uint32_t* dirty,
                                         uint32_t* crange, uint32_t* wstage, uint32_t* dump, const RParams& p,
                                         uint32_t& nvalid, uint32_t& nkept, bool any, uint16_t* fkb,
                                         uint32_t keep) {
    const int lane = lane_id();
    nvalid += r_nvalid<STEP, QP, LC>(r.dw, r.g, p);
    // for pass 2 (read back by this lane); a chunk the plane rules out is skipped there, except the last
    if constexpr (STEP == 1)
        if (any || c + 1 == p.nchunks) fkb[c * 256 + threadIdx.x] = (uint16_t)keep;
    if (!any) {   // uniform: the plane rules out every grid point of the chunk: nothing to bin
        if (lane == 0) crange[4 * c + (threadIdx.x >> 6)] = 0u;
        return;
    }
    nkept += __builtin_popcount(keep);
    {
        const uint32_t w = r_keep_range<STEP, QP, LC>(r.dw, keep);
        if (lane == 0) crange[4 * c + (threadIdx.x >> 6)] = w;
    }
    uint32_t pos0;
    bool cand = false;
    // a point is a candidate while its bin holds fewer than hist_thr points (never for hist_thr < 0)
    const uint32_t lim = p.hist_thr < 0 ? 0u : (uint32_t)p.hist_thr;
    constexpr int NPL = 4 * RCfg<STEP, QP, LC>::QPL;   // grid points a lane holds
    // density threshold in eighths (DIAGNOSTIC A/B: ablate bits 15-16 pick 6, 4, 5 or 7; release: 6)
    const uint32_t dense8 = (0x7546u >> (4 * ablate_field(p.ablate, 15, 3))) & 0xFu;
    // DIAGNOSTIC (diagnostic build only, results invalid): 2 no hue binning; 8 the bins without the atomics; 32
    // plain adds (no return) on spread bins (lane + 64 b mod 1000) without the bin arithmetic; 64 the real bins with
    // adds that return nothing (no candidates)
    if (ablated(p.ablate, 2)) {
    } else if (ablated(p.ablate, 8 | 32 | 64)) {
        uint32_t acc = 0;
#pragma unroll
        for (int b = 0; b < NPL; ++b) {
            if (!((keep >> b) & 1u)) continue;
            if (ablated(p.ablate, 8)) acc += r_bin_sel(r_col<STEP, QP, LC>(r.cw[b >> 2], b & 3));
            else if (ablated(p.ablate, 64)) __hip_atomic_fetch_add(&hist[r_bin_sel(r_col<STEP, QP, LC>(r.cw[b >> 2], b & 3))], 1u,
                                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else atomicAdd(&hist[(uint32_t)(lane + 64 * b) % 1000u], 1u);
        }
        if (acc == 0xFFFFFFFFu) hist[0] = acc;   // keeps the bins
    } else if (!ablated(p.ablate, 16384) && wave_sum((uint32_t)__builtin_popcount(keep)) * 8u >= dense8 * 64u * NPL) {
        // uniform: a dense wave (>= 3/4 of its points kept, the road) bins its colours from registers, each lane
        // its own kept points in turn: at most 1/4 of the lanes idle, and no LDS staging writes and reads
        // (16384: DIAGNOSTIC A/B, always stage)
#pragma unroll
        for (int b0 = 0; b0 < NPL; b0 += 4) {
            uint32_t o[4];
#pragma unroll
            for (int b = b0; b < b0 + 4; ++b) {
                o[b - b0] = lim;
                if ((keep >> b) & 1u) o[b - b0] = atomicAdd(&hist[r_bin_sel(r_col<STEP, QP, LC>(r.cw[b >> 2], b & 3))], 1u);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) cand |= o[k] < lim;
        }
    } else {
        const uint32_t wtotal = r_stage_colours_sel<STEP, QP, LC>(keep, r.cw, wstage, dump, pos0);
        for (uint32_t j = lane; j < (ablated(p.ablate, 512) ? 0u : wtotal); j += 4 * kWave) {   // four colours in flight
            uint32_t o[4], cl[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) cl[k] = wstage[min(j + k * kWave, wtotal - 1)];   // the reads first
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[k] = lim;
                if (j + k * kWave < wtotal) o[k] = atomicAdd(&hist[r_bin_sel(cl[k])], 1u);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) cand |= o[k] < lim;
        }
    }
    if (__ballot(cand) && lane == 0) atomicOr(&dirty[c >> 5], 1u << (c & 31));
}

typedef float v4f __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));

// A kept point's LDS descriptor: gx | dx << 11 | gy << 12 | dy << 23 | d << 24
// (grid coordinates < 2048; dx, dy = the back-projection deltas of §2 item 2:
// the int32 (x, y) is (x - dx, y - dy)).
__device__ __forceinline__ uint32_t rdesc(uint32_t d, uint32_t gy, uint32_t gx, uint32_t dx, uint32_t dy) {
    return (d << 24) | (dy << 23) | (gy << 12) | (dx << 11) | gx;
}

// Write outputs [a, b) of the frame from their LDS descriptors (slot = g mod
// the stage size); groups of 4 outputs at 16-byte-aligned positions: lane l
// writes the X, Y, Z, x, y of outputs 4l..4l+3 of its wave's 256-output block,
// one 16-byte non-temporal store per plane, so every store instruction covers
// 1 KiB contiguous. The loop runs over wave blocks, uniform per wave; it reads
// only LDS.
template <int STEP, int QP, bool LC>
__device__ __forceinline__ void p2_write(const uint32_t* stage, uint32_t a, uint32_t b, float* oX, float* oY,
                                         float* oZ, uint32_t* oPxy, const RParams& p) {
    constexpr uint32_t SM = stage_of<QP>() - 1;
    const uint32_t first = a & ~3u;
    const uint32_t groups = (b - first + 3) >> 2;
    const int lane = lane_id();
    for (uint32_t m0 = threadIdx.x & ~63u; m0 < groups; m0 += 256) {   // uniform per wave
        const uint32_t m = m0 + lane;
        if (m >= groups) continue;
        const uint32_t g = first + 4 * m;
        if (ablated(p.ablate, 4096)) {   // DIAGNOSTIC (diagnostic build only, results invalid): the stores alone
            if (g >= a && g + 3 < b) {
                const v4f z = {0.f, 0.f, 0.f, 0.f};
                __builtin_nontemporal_store(z, reinterpret_cast<v4f*>(oX + g));
                __builtin_nontemporal_store(z, reinterpret_cast<v4f*>(oY + g));
                __builtin_nontemporal_store(z, reinterpret_cast<v4f*>(oZ + g));
                __builtin_nontemporal_store((v4i){0, 0, 0, 0}, reinterpret_cast<v4i*>(oPxy + g));
            }
            continue;
        }
        const uint4 u4 = *reinterpret_cast<const uint4*>(&stage[g & SM]);
        const uint32_t u[4] = {u4.x, u4.y, u4.z, u4.w};
        float X[4], Y[4], Z[4];
        int PX[4], PY[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t d = u[e] >> 24;   // a stale slot past b may give rcp(0) = inf: never stored
            const int y = (int)((u[e] >> 12) & 0x7FF) * STEP;
            const int x = (int)(u[e] & 0x7FF) * STEP;
            const float rr = __builtin_amdgcn_rcpf((float)d);
            const float K = p.B32 * rr;
            X[e] = centred(x, p.cw_hi, p.cw_lo) * K;
            Y[e] = centred(y, p.ch_hi, p.ch_lo) * K;
            Z[e] = p.fB32 * rr;
            PX[e] = x - (int)((u[e] >> 11) & 1);
            PY[e] = y - (int)((u[e] >> 23) & 1);
        }
        if (g >= a && g + 3 < b) {
            __builtin_nontemporal_store((v4f){X[0], X[1], X[2], X[3]}, reinterpret_cast<v4f*>(oX + g));
            __builtin_nontemporal_store((v4f){Y[0], Y[1], Y[2], Y[3]}, reinterpret_cast<v4f*>(oY + g));
            __builtin_nontemporal_store((v4f){Z[0], Z[1], Z[2], Z[3]}, reinterpret_cast<v4f*>(oZ + g));
            __builtin_nontemporal_store((v4i){(int)pp_pack(PX[0], PY[0]), (int)pp_pack(PX[1], PY[1]),
                                         (int)pp_pack(PX[2], PY[2]), (int)pp_pack(PX[3], PY[3])},
                                        reinterpret_cast<v4i*>(oPxy + g));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!(g + e >= a && g + e < b)) continue;
                oX[g + e] = X[e];
                oY[g + e] = Y[e];
                oZ[g + e] = Z[e];
                oPxy[g + e] = pp_pack(PX[e], PY[e]);
            }
        }
    }
}

// pass 2 of one chunk: keep2, block scan, descriptor scatter, then the
// chunk's whole output groups. Two barriers. Loads chunk c + 1 into r before
// the stores (PF).
// The road bitmap's marks of one lane (RB: LC, 1024-wide rows): its 16 points are 16 consecutive x = x0 + k of row
// gy (x0 = 16 lane), each marking pixel (x0 + k - dx, gy - dy) (generatePointsAsImage, functions.py:339-344).
// Relative to x0 - 1 a kept point sets bit k + 1 - dx of row gy - dy's 17-bit window; the window is bits 15..31
// of word x0 / 32 (x0 % 32 == 16) or bit 31 of the word before and bits 0..15 (x0 % 32 == 0). Wave w holds one
// row, but row gy - 1 also gets the marks of row gy's wave, so the words are OR-ed (ds_or, no return).
template <class SH>
__device__ __forceinline__ void rb_mark(SH& sh, uint32_t keep, uint32_t bxm, uint32_t bym, int gy, int x0, int Wu) {
    if (!keep) return;
    const uint32_t kb1 = keep & bym, kb0 = keep & ~bym;
    const uint32_t m0 = ((kb0 & ~bxm) << 1) | (kb0 & bxm);   // row gy
    const uint32_t m1 = ((kb1 & ~bxm) << 1) | (kb1 & bxm);   // row gy - 1
    const int w = x0 >> 5;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t m = h ? m1 : m0;
        if (!m) continue;
        const int y = gy - h;
        uint32_t* row = y < 0 ? sh.rwrap : sh.rring + 32 * (y & 7);   // y = -1: numpy's last row
        if (x0 & 16) {
            atomicOr(row + w, m << 15);
        } else {
            atomicOr(row + w, m >> 1);
            if (m & 1u) {   // x0 - 1: the word before, or (x0 = 0) numpy's last column
                const int xl = w > 0 ? x0 - 1 : Wu - 1;
                atomicOr(row + (xl >> 5), 1u << (xl & 31));
            }
        }
    }
}

// Write the road bitmap's rows [*rflushed, upto) to out (frame's rows x 32 words) and clear their ring slots. Each
// thread owns one (slot, word) of the ring for the whole frame (t = 32 * slot + word), so no barrier is needed
// between a flush and the next one; marks reach a slot only in a chunk whose barriers order them after its clear.
// (upto - *rflushed <= 8.)
template <class SH>
__device__ __forceinline__ void rb_flush(SH& sh, uint32_t* out, int& rflushed, int upto, int H) {
    const int t = threadIdx.x, slot = t >> 5, word = t & 31;
    // the row in [rflushed, upto) that this thread's slot holds, if any
    const int y = rflushed + ((slot - rflushed) & 7);
    if (y < upto) {
        uint32_t v = sh.rring[t];
        if (y == H - 1) v |= sh.rwrap[word];
        out[32 * y + word] = v;
        sh.rring[t] = 0u;
    }
    rflushed = upto;
}

template <int STEP, int QP, bool LC, bool PF, bool RB, class SH>
__device__ __forceinline__ void p2_chunk(P2Regs<STEP, QP, LC>& r, int c, bool more, const uint32_t* hist,
                                         const uint32_t* dirty, SH& sh, uint32_t* wstage,
                                         const uint8_t* fdisp, const uint8_t* fbgr, const RLean& L,
                                         const FramePlane* Lp, const PipeBuffers& bf, float* oX, float* oY,
                                         float* oZ, uint32_t* oPxy,
                                         uint32_t& running, uint32_t& flushed, bool next_run, const uint16_t* fkb,
                                         const RParams& p) {
    constexpr int QPL = RCfg<STEP, QP, LC>::QPL;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    uint32_t keep;
    if constexpr (STEP == 1) keep = r.kb;
    else keep = r_keep1<STEP, QP, LC>(r.dw, r.g, L, Lp, p.Wg);   // chunks pass 2 runs: not ruled out, or the last
    // this chunk's delta words into LDS, read by its scatter after the next
    // barrier (every wave has finished chunk c - 1's scatter)
    uint32_t* dl = sh.dlt;
    if (!r.reuse) p2_stage_deltas<STEP, QP, LC>(r, dl);
    const int dlo = r.dlo;
    const bool narrow = r.narrow;
    const bool dirty_c = !ablated(p.ablate, 16) && ((dirty[c >> 5] >> (c & 31)) & 1);   // 16: no chunk re-binned
    if (dirty_c) {   // uniform: candidate chunk (rare)
        uint32_t cw[QPL][RCfg<STEP, QP, LC>::CW];
        r_load_bgr<STEP, QP, LC>(fbgr, r.g, p, cw);
        __syncthreads();   // every wave is done writing the previous chunk: sh.stage is free
        uint32_t pos0;
        const uint32_t wtotal = r_stage_colours_sel<STEP, QP, LC>(keep, cw, wstage, sh.dump + tid, pos0);
        for (uint32_t j = lane; j < wtotal; j += kWave) {
            const uint32_t bin = r_bin_sel(wstage[j]);
            wstage[j] = (int64_t)hist[bin] > (int64_t)p.hist_thr ? 1u : 0u;
        }
        uint32_t pos = pos0;
#pragma unroll
        for (int b = 0; b < 4 * QPL; ++b) {
            if (keep & (1u << b)) {
                if (!wstage[pos]) keep &= ~(1u << b);
                ++pos;
            }
        }
    }
    uint64_t cnt = 0, inc;
    const auto add = [](uint32_t a, uint32_t b) { return a + b; };
    if constexpr (LC) {   // raster order is lane order: one 32-bit scan of the lane's count (in field 0)
        cnt = (uint64_t)__builtin_popcount(keep);
        inc = (uint64_t)wave_scan_dpp((uint32_t)cnt, add);
    } else {
#pragma unroll
        for (int i = 0; i < QPL; ++i) cnt += (uint64_t)__builtin_popcount((keep >> (4 * i)) & 0xF) << (16 * i);
        // the four 16-bit row counts never carry (<= 256 each): two 32-bit DPP scans
        inc = (uint64_t)wave_scan_dpp((uint32_t)cnt, add) | ((uint64_t)wave_scan_dpp((uint32_t)(cnt >> 32), add) << 32);
    }
    if (lane == 63) sh.wtot[wave] = inc;
    __syncthreads();
    uint64_t wbase = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint64_t v = sh.wtot[w];
        wbase += (w < wave) ? v : 0ull;
        tot += v;
    }
    const uint64_t excl = wbase + inc - cnt;
    // LDS slot of output g = g mod kRStage. Outputs [flushed, running) are the
    // previous chunk's unwritten tail (< 32, restored from sh.red), so every
    // group of 4 written below is whole and the writes start on a 128-byte line. If this chunk's
    // points would wrap onto that tail (almost every point kept), the tail is
    // written first as a partial group (uniform, rare).
    const uint32_t T = LC ? (uint32_t)tot
                          : (uint32_t)((tot >> 0) & 0xFFFF) + (uint32_t)((tot >> 16) & 0xFFFF) +
                                (uint32_t)((tot >> 32) & 0xFFFF) + (uint32_t)((tot >> 48) & 0xFFFF);
    if (tid < (int)(running - flushed)) sh.stage[(flushed + tid) & (stage_of<QP>() - 1)] = sh.red[tid];   // the tail
    if (T > (uint32_t)stage_of<QP>() - (running - flushed)) {   // uniform
        p2_write<STEP, QP, LC>(sh.stage, flushed, running, oX, oY, oZ, oPxy, p);
        flushed = running;
        // the scatter below wraps onto the slots just written out: every wave must have read them first
        // (without this barrier the other waves' scatter raced wave 0's read of the tail)
        __syncthreads();
    }
    // descriptors (rdesc) with the back-projection delta bits of each point,
    // branch-free: a slot that is not kept writes to this lane's dump word
    uint32_t rowbase = running;
    uint32_t olc = running + (uint32_t)excl;   // LC: the lane's outputs are one run
    // LC, narrow: the lane's one row's transposed dy word (bit dd = the dy bit of d = dlo + dd)
    const uint32_t tyl = (LC && narrow) ? dl[kRTyOff + (((uint32_t)max(r.g.gy[0], 0) * STEP) & 31u)] : 0u;
    uint32_t bxm = 0u, bym = 0u;   // RB: the lane's delta bits, bit 4 i + k
#pragma unroll
    for (int i = 0; i < QPL; ++i) {
        uint32_t o = LC ? olc : rowbase + (uint32_t)((excl >> (16 * i)) & 0xFFFF);
        rowbase += (uint32_t)((tot >> (16 * i)) & 0xFFFF);
        const uint32_t gy = (uint32_t)max(r.g.gy[i], 0), y = gy * STEP;
        uint32_t dv[4], bx[4], by[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) dv[k] = r_d<STEP, QP, LC>(r.dw[i], k);
        if (narrow && LC) {   // uniform; transposed stage: the lane's 16 x are 4 quads of one row (x0 % 16 == 0)
            const uint32_t x0 = 4u * (uint32_t)r.g.q[0];
            const uint4 tw = *reinterpret_cast<const uint4*>(dl + (x0 >> 4) * kRTxGroup + 4 * i);
            const uint32_t t4[4] = {tw.x, tw.y, tw.z, tw.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t dd = min(dv[k] - (uint32_t)dlo, (uint32_t)kRDN - 1);   // clamp: slots not kept
                bx[k] = (t4[k] >> dd) & 1u;
                by[k] = (tyl >> dd) & 1u;
            }
        } else if (narrow) {   // uniform: every kept d in [dlo, dlo + kRDN), the chunk's rows in word ywb
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t dd = min(dv[k] - (uint32_t)dlo, (uint32_t)kRDN - 1);   // clamp: slots not kept
                const uint32_t x = (uint32_t)(4 * r.g.q[i] + k) * STEP;
                bx[k] = (dl[dd * kRDxStride + (x >> 5)] >> (x & 31)) & 1u;
                by[k] = (dl[kRDyOff + dd] >> (y & 31)) & 1u;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t x = (uint32_t)(4 * r.g.q[i] + k) * STEP;
                const uint32_t xw = min(x >> 5, (uint32_t)p.dx_words - 1);   // pad columns
                bx[k] = (bf.dxbits[dv[k] * p.dx_words + xw] >> (x & 31)) & 1u;
                by[k] = (bf.dybits[dv[k] * p.dy_words + (y >> 5)] >> (y & 31)) & 1u;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t bit = (keep >> (4 * i + k)) & 1u;
            *(bit ? &sh.stage[o & (stage_of<QP>() - 1)] : sh.dump + tid) =
                rdesc(dv[k], gy, (uint32_t)(4 * r.g.q[i] + k), bx[k], by[k]);
            o += bit;
            if constexpr (RB) {
                bxm |= bx[k] << (4 * i + k);
                bym |= by[k] << (4 * i + k);
            }
        }
        olc = o;
    }
    if constexpr (RB) {   // LC, step 1: the lane's 16 points are x0 .. x0 + 15 of row gy
        static_assert(!RB || (LC && STEP == 1 && QPL == 4), "the road bitmap needs lane-contiguous step-1 quads");
        rb_mark(sh, keep, bxm, bym, r.g.gy[0], 4 * r.g.q[0], bf.rb_Wu);
    }
    if (PF && more) p2_load<STEP, QP, LC>(r, c + 1, tid, fdisp, sh.crange, bf, p, true, next_run, fkb);   // in flight before the stores
    __syncthreads();
    running += T;
    // write whole 128-byte lines: outputs up to a multiple of 32 (X, Y, Z: 32 floats a line; P: 16 pairs),
    // the rest (< 32) carried to the next chunk; the last chunk flushes its tail
    const uint32_t upto = more ? (running & ~31u) : running;
    // keep the new tail (< 32 descriptors) out of sh.stage's way: the next
    // chunk's dirty path may reuse sh.stage before its scatter restores them
    if (tid < (int)(running - upto)) sh.red[tid] = sh.stage[(upto + tid) & (stage_of<QP>() - 1)];
    if (upto > flushed) {
        p2_write<STEP, QP, LC>(sh.stage, flushed, upto, oX, oY, oZ, oPxy, p);
        flushed = upto;
    }
}

// ---------------------------------------------------------------------------
// One frame's two passes as workgroup-level device functions. pass 1 leaves
// the histogram and dirty bits in LDS and the valid/kept counts in sh.red.
// ---------------------------------------------------------------------------
template <int QP>
struct FusedShared {
    uint32_t hist[kRBins];
    uint32_t dirty[maxchunks_of<QP>() / 32];
    uint64_t wtot[4];
    uint32_t red[32];   // pass 1: valid/kept counts per wave; pass 2: the carried output tail (< 32)
    uint32_t stage[stage_of<QP>()];
    uint32_t dump[256];   // pass 1: one slot per lane for the colours of points that are not kept
    // pass 1 -> pass 2: per chunk and wave, the keep1 disparity range as
    // (255 - dmin) << 16 | dmax (0 = no kept point)
    alignas(16) uint32_t crange[maxchunks_of<QP>() * 4];
    uint32_t dlt[kRDeltaWords];   // pass 2: the chunk's delta words (scatter lookups)
    uint32_t cany[8];             // per chunk: can the frame's plane keep any of its grid points
    // pass 2 with the road bitmap (RB): image rows being marked, row y in slot y & 7 (32 words of 32 pixels);
    // marks for row -1 (numpy's last row) wait in rwrap until row H - 1 is written
    uint32_t rring[8 * 32];
    uint32_t rwrap[32];
};
static_assert(sizeof(FusedShared<4>) <= 32768, "5 workgroups per CU (160 KiB LDS), as many as 93 VGPRs allow");

// sh.cany bit c: can the plane keep some grid point of chunk c (rows_keepable
// over the chunk's rows)? One lane per chunk (nchunks <= 256), one ballot per wave.
template <int STEP, int QP, bool LC>
__device__ __forceinline__ void chunk_keepable_bits(FusedShared<QP>& sh, const FramePlane* Lp, const RParams& p) {
    constexpr int per = RCfg<STEP, QP, LC>::QPL * 256;   // quads per chunk
    const int c = threadIdx.x;
    bool k = false;
    const FramePlane L = *Lp;
    if (c < p.nchunks && L.valid) {
        const int gy0 = fastdiv40(c * per, p.Q_m40);
        const int gy1 = fastdiv40(min((c + 1) * per, p.frame_quads) - 1, p.Q_m40);
        k = rows_keepable(L, gy0, gy1, p.Wg, STEP);
    }
    const uint64_t m = __ballot(k);
    if (lane_id() == 0) {
        sh.cany[2 * (c >> 6)] = (uint32_t)m;
        sh.cany[2 * (c >> 6) + 1] = (uint32_t)(m >> 32);
    }
}

template <int QP>
__device__ __forceinline__ bool chunk_any(const FusedShared<QP>& sh, int c) {   // uniform
    return __builtin_amdgcn_readfirstlane((sh.cany[c >> 5] >> (c & 31)) & 1u) != 0;
}

template <int STEP, int QP, bool LC, bool PF1 = false>
__device__ __forceinline__ void frame_pass1(int frame, FusedShared<QP>& sh, const PipeBuffers& bf,
                                            const RLean& L, const FramePlane* Lp,
                                            const RParams& p) {
    constexpr int WREGION = 64 * RCfg<STEP, QP, LC>::QPL * 4;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const uint8_t* fdisp = bf.disp + (int64_t)frame * p.frame_px;
    const uint8_t* fbgr = bf.bgr + (int64_t)frame * p.frame_px * 3;
    uint32_t* wstage = sh.stage + wave * WREGION;
    for (int i = tid; i < kRBins; i += 256) sh.hist[i] = 0;
    if (tid < maxchunks_of<QP>() / 32) sh.dirty[tid] = 0;
    chunk_keepable_bits<STEP, QP, LC>(sh, Lp, p);
    __syncthreads();
    uint32_t nvalid = 0, nkept = 0;
    uint16_t* fkb = bf.kbits + (int64_t)frame * p.nchunks * 256;   // step 1: keep1 bits per chunk and lane
    const int n1 = ablated(p.ablate, 128) ? 0 : p.nchunks;   // ablate: DIAGNOSTIC ONLY
    if constexpr (PF1) {   // chunk c + 1's loads in flight while chunk c is binned (pass 1 stores nothing)
        P1Regs<STEP, QP, LC> r1;
        if (n1 > 0) p1_load<STEP, QP, LC>(r1, 0, tid, fdisp, fbgr, p, false, chunk_any(sh, 0));
        for (int c = 0; c < n1; ++c) {
            P1Regs<STEP, QP, LC> cur = r1;
            // keep1 before chunk c + 1's loads are issued: its rare fp64 path then
            // runs with one chunk's registers live, not two
            const bool any = chunk_any(sh, c);
            const uint32_t keep = any ? r_keep1<STEP, QP, LC>(cur.dw, cur.g, L, Lp, p.Wg) : 0u;
            if (c + 1 < n1) p1_load<STEP, QP, LC>(r1, c + 1, tid, fdisp, fbgr, p, true, chunk_any(sh, c + 1));
            p1_chunk<STEP, QP, LC>(cur, c, sh.hist, sh.dirty, sh.crange, wstage, sh.dump + tid, p, nvalid, nkept,
                               any, fkb, keep);
        }
    } else {
        for (int c = 0; c < n1; ++c) {
            P1Regs<STEP, QP, LC> r1;
            const bool any = chunk_any(sh, c);
            p1_load<STEP, QP, LC>(r1, c, tid, fdisp, fbgr, p, false, any);
            const uint32_t keep = any ? r_keep1<STEP, QP, LC>(r1.dw, r1.g, L, Lp, p.Wg) : 0u;
            p1_chunk<STEP, QP, LC>(r1, c, sh.hist, sh.dirty, sh.crange, wstage, sh.dump + tid, p, nvalid, nkept, any, fkb,
                               keep);
        }
    }
    nvalid = wave_sum(nvalid);
    nkept = wave_sum(nkept);
    if (lane == 0) {
        sh.red[wave] = nvalid;
        sh.red[4 + wave] = nkept;
    }
    __syncthreads();   // histogram, dirty bits, counts complete
}

template <int STEP, int QP, bool LC, bool PF, bool RB>
__device__ __forceinline__ void frame_pass2(int frame, FusedShared<QP>& sh, const PipeBuffers& bf,
                                            const RLean& L, const FramePlane* Lp,
                                            const RParams& p) {
    constexpr int WREGION = 64 * RCfg<STEP, QP, LC>::QPL * 4;
    const int tid = threadIdx.x, wave = tid >> 6;
    const uint8_t* fdisp = bf.disp + (int64_t)frame * p.frame_px;
    const uint8_t* fbgr = bf.bgr + (int64_t)frame * p.frame_px * 3;
    uint32_t* wstage = sh.stage + wave * WREGION;
    float* oX = bf.ox + (int64_t)frame * bf.ofs;
    float* oY = bf.oy + (int64_t)frame * bf.ofs;
    float* oZ = bf.oz + (int64_t)frame * bf.ofs;
    uint32_t* oPxy = bf.pxy + (int64_t)frame * bf.cap;
    uint32_t running = 0, flushed = 0;
    const int n2 = ablated(p.ablate, 256) ? 0 : p.nchunks;
    // a chunk in which pass 1 kept no point (its keep1 range is 0 in every wave;
    // always so where the plane rules the chunk out) adds no output and is
    // skipped, loads included; the last chunk always runs (it flushes the tail)
    const auto run = [&](int c) {
        const uint4 cr = *reinterpret_cast<const uint4*>(sh.crange + 4 * c);
        return c + 1 == n2 || (cr.x | cr.y | cr.z | cr.w) != 0u;
    };
    const uint16_t* fkb = bf.kbits + (int64_t)frame * p.nchunks * 256;
    // RB: the road bitmap's rows, written as they become final (chunk c + 1 can still mark row 4 (c + 1) - 1)
    uint32_t* frb = RB ? bf.rbits + (int64_t)frame * bf.rb_H * 32 : nullptr;
    int rflushed = 0;
    if constexpr (RB) {
        sh.rring[tid] = 0u;
        if (tid < 32) sh.rwrap[tid] = 0u;
        __syncthreads();
    }
    constexpr int RPC = RB ? 4 : 1;   // RB: grid rows per chunk (1024 quads of 256 a row)
    P2Regs<STEP, QP, LC> r2;
    r2.staged = false;
    if (PF && n2 > 0) p2_load<STEP, QP, LC>(r2, 0, tid, fdisp, sh.crange, bf, p, false, run(0), fkb);
    for (int c = 0; c < n2; ++c) {
        if (!PF) p2_load<STEP, QP, LC>(r2, c, tid, fdisp, sh.crange, bf, p, c > 0, run(c), fkb);
        if (!run(c)) {   // uniform; c + 1 < n2 here
            if (PF) p2_load<STEP, QP, LC>(r2, c + 1, tid, fdisp, sh.crange, bf, p, true, run(c + 1), fkb);
            if constexpr (RB) rb_flush(sh, frb, rflushed, RPC * (c + 1) - 1, bf.rb_H);
            continue;
        }
        p2_chunk<STEP, QP, LC, PF, RB>(r2, c, c + 1 < n2, sh.hist, sh.dirty, sh, wstage, fdisp, fbgr, L, Lp, bf, oX, oY,
                                       oZ, oPxy,
                                       running, flushed, c + 1 < n2 && run(c + 1), fkb, p);
        if constexpr (RB) {   // after the chunk's last barrier: its marks are in the ring
            if (c + 1 < n2) {
                rb_flush(sh, frb, rflushed, RPC * (c + 1) - 1, bf.rb_H);
            } else {   // the frame's last chunk: every remaining row, row H - 1 with the wrapped marks
                while (rflushed < bf.rb_H) rb_flush(sh, frb, rflushed, min(rflushed + 8, bf.rb_H), bf.rb_H);
            }
        }
    }
    if (tid == 0) bf.counts[4 * (int64_t)frame + 2] = running;
}

// ---------------------------------------------------------------------------
// One workgroup = one frame: pass 1 over all chunks, then pass 2 (grid = frames).
// The frame's plane: bf.planes[frame * bf.plane_stride] (device memory).
// ---------------------------------------------------------------------------
template <int STEP, int QP, bool LC, bool PF, bool PF1, bool RB>
__device__ __forceinline__ void fused_body(const PipeBuffers& bf, const RParams& p,
                                           FusedShared<QP>& sh) {
    const int tid = threadIdx.x;
    const int frame = blockIdx.x;
    const FramePlane* Lp = bf.planes + (int64_t)frame * bf.plane_stride;
    const RLean L{Lp->al32, Lp->bb32, Lp->b032, Lp->tn32, Lp->g32};
    // DIAGNOSTIC A/B (diagnostic build; outputs unchanged): ablate bits 20-30 = a start delay in us per slot group,
    // workgroup w of the first round waiting (w / 256) x that, so the five workgroups a CU holds do not run pass 1
    // and pass 2 in phase (the phase-lock probe)
    if (const uint32_t us = ablate_field(p.ablate, 20, 0xFFFu); us && blockIdx.x < 5 * 256) {
        const uint64_t t0 = wall_clock64(), wait = (uint64_t)(blockIdx.x >> 8) * us * 100u;   // 100 MHz ticks
        while (wall_clock64() - t0 < wait) __builtin_amdgcn_s_sleep(32);
    }
    frame_pass1<STEP, QP, LC, PF1>(frame, sh, bf, L, Lp, p);
    // pass 2 (store-bound) issues ahead of other workgroups' pass-1 waves on the SIMD: -0.2 to -0.4 %
    // (5.78 vs 5.80 ms, 6.81 vs 6.82 with per-frame planes; ten and eight in-process alternations)
    __builtin_amdgcn_s_setprio(2);
    uint32_t* gh = bf.hist + (int64_t)frame * kBins;
    for (int b = tid; b < kBins; b += 256) gh[b] = b < kRBins ? sh.hist[b] : 0u;
    if (tid == 0) {
        int64_t* cn = bf.counts + 4 * (int64_t)frame;
        cn[0] = (int64_t)sh.red[0] + sh.red[1] + sh.red[2] + sh.red[3];
        cn[1] = (int64_t)sh.red[4] + sh.red[5] + sh.red[6] + sh.red[7];
    }
    frame_pass2<STEP, QP, LC, PF, RB>(frame, sh, bf, L, Lp, p);
}

template <int STEP, int QP, bool LC, bool PF, bool PF1 = false, bool RB = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5))) void resident_fused_kernel(PipeBuffers bf, RParams p) {
    __shared__ FusedShared<QP> sh;
    fused_body<STEP, QP, LC, PF, PF1, RB>(bf, p, sh);
}

bool resident_supported(const KParams& p) {   // frame_quads <= 2^20: every QP's chunk count fits its dirty bits
    return (p.step == 1 || p.step == 2) && p.pitch <= 2048 && p.Hg <= 2048 &&   // rdesc: 11-bit coordinates
           resident_chunks_per_frame(p, 4) <= kRMaxChunks && p.frame_px * 3 < (1ll << 31);
}

// lane-contiguous quads (r_qi) for step 1 when a lane's 4 quads are one aligned
// 16-byte run of a row; SVX_RES_LC=0 keeps the slot-major order (A/B knob)
static bool resident_lane_quads(const KParams& kp) {
    const char* v = svx_knob("SVX_RES_LC");   // read per call (tools/prof.py ab --env)
    const bool on = !(v && v[0] == '0');
    return on && kp.step == 1 && kp.Q % 4 == 0 && kp.W % 16 == 0 && kp.frame_px % 16 == 0;
}

bool resident_road_bits_supported(const KParams& p) {   // 1024-wide rows: 4 grid rows a chunk, 32 words a row
    return resident_supported(p) && p.step == 1 && p.W == 1024 && p.Q == 256 && p.H <= 1024 && p.Hg >= 1 &&
           resident_lane_quads(p);
}

static RParams resident_params(const KParams& kp, int qpl) {
    RParams p;
    p.W = kp.W;
    p.Wg = kp.Wg;
    p.Q = kp.Q;
    p.pitch = kp.pitch;
    p.frame_quads = kp.frame_quads;
    p.nchunks = resident_chunks_per_frame(kp, qpl);
    p.drow = 256 * qpl / kp.Q;
    p.dq = 256 * qpl % kp.Q;
    p.hist_thr = kp.hist_thr;
    p.dx_words = kp.dx_words;
    p.dy_words = kp.dy_words;
    p.ablate = kp.ablate;
    p.Q_m40 = kp.Q_m40;
    p.frame_px = kp.frame_px;
    p.B32 = kp.B32;
    p.fB32 = kp.fB32;
    p.cw_hi = kp.cw_hi;
    p.cw_lo = kp.cw_lo;
    p.ch_hi = kp.ch_hi;
    p.ch_lo = kp.ch_lo;
    return p;
}

// A host plane into device memory, stream-ordered (no host buffer outlives the call).
__global__ void store_plane_kernel(FramePlane v, FramePlane* __restrict__ dst) {
    if (threadIdx.x == 0) *dst = v;
}

hipError_t launch_store_plane(const FramePlane& v, FramePlane* dst, hipStream_t s) {
    hipLaunchKernelGGL(store_plane_kernel, dim3(1), dim3(64), 0, s, v, dst);
    return hipGetLastError();
}

// b.planes must be set (device planes; one for every frame with plane_stride 0). kname (nullable): the
// launched instance's name as rocprofv3 prints it, so a PMC profile can be matched to the kernel that was timed.
hipError_t launch_pipeline_resident(const KParams& kp, const PipeBuffers& b, int frames,
                                    bool prefetch, hipStream_t s, bool prefetch1, const char** kname) {
    if (frames <= 0) return hipSuccess;
    if (!resident_supported(kp) || !b.planes) return hipErrorInvalidValue;
    const dim3 grid(frames), block(256);
    const char* name = nullptr;
#define SVX_RESIDENT(ST, QP, LC, PF, PF1, RB, SIG)                                                          \
    do {                                                                                                    \
        hipLaunchKernelGGL((resident_fused_kernel<ST, QP, LC, PF, PF1, RB>), grid, block, 0, s, b, p);    \
        name = "svx::resident_fused_kernel<" SIG ">";                                                       \
    } while (0)
    if (b.rbits) {   // the road bitmap too (resident_road_bits_supported)
        if (!resident_road_bits_supported(kp) || !resident_lane_quads(kp) || b.rb_H != kp.H) return hipErrorInvalidValue;
        const RParams p = resident_params(kp, 4);
        if (prefetch1) SVX_RESIDENT(1, 4, true, true, true, true, "1, 4, true, true, true, true");
        else if (prefetch) SVX_RESIDENT(1, 4, true, true, false, true, "1, 4, true, true, false, true");
        else SVX_RESIDENT(1, 4, true, false, false, true, "1, 4, true, false, false, true");
    } else if (kp.step == 1 && resident_lane_quads(kp)) {
        const RParams p = resident_params(kp, 4);
        if (prefetch1) SVX_RESIDENT(1, 4, true, true, true, false, "1, 4, true, true, true, false");
        else if (prefetch) SVX_RESIDENT(1, 4, true, true, false, false, "1, 4, true, true, false, false");
        else SVX_RESIDENT(1, 4, true, false, false, false, "1, 4, true, false, false, false");
    } else if (kp.step == 1) {
        const RParams p = resident_params(kp, 4);
        if (prefetch1) SVX_RESIDENT(1, 4, false, true, true, false, "1, 4, false, true, true, false");
        else if (prefetch) SVX_RESIDENT(1, 4, false, true, false, false, "1, 4, false, true, false, false");
        else SVX_RESIDENT(1, 4, false, false, false, false, "1, 4, false, false, false, false");
    } else {
        const RParams p = resident_params(kp, 2);
        if (prefetch1) SVX_RESIDENT(2, 2, false, true, true, false, "2, 2, false, true, true, false");
        else if (prefetch) SVX_RESIDENT(2, 2, false, true, false, false, "2, 2, false, true, false, false");
        else SVX_RESIDENT(2, 2, false, false, false, false, "2, 2, false, false, false, false");
    }
#undef SVX_RESIDENT
    if (kname) *kname = name;
    return hipGetLastError();
}

}  // namespace svx
