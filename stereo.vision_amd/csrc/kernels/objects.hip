// The obstacle list (gfx950): the 8-connected components of a packed obstacle bitmap, with area, box, first pixel,
// coordinate sums and the disparity's count, maximum and lower median (include/svx.h, sv_obstacle_list). Integers
// only. Bitmaps have morph.hip's layout: rows of WW = ceil(W / 32) words, pixel x at bit x & 31 of word x >> 5; the
// last word's pad bits are masked off as it is read, so nothing outside the frame is touched whatever they hold.
//
// The unit of work is a SEGMENT: a maximal run of set bits inside one word, found by ctz on the word. A run of the
// row is its segments chained over the word boundaries. A segment that starts at bit s of word w in row y is NODE
// y * 16 WW + 16 w + (s >> 1): two segments of a word never start in the same even / odd pair, so a word has 16 node
// slots, and node order is the raster order of the segments' first pixels. A segment that starts at bit 0 behind a
// set bit 31 continues a run: its parent starts as the node of the segment before it; every other node starts as
// its own parent. Segment [a, b] of row y touches the pieces of row y - 1 in [a - 1, b + 1] (8-connectivity), which
// lie in that row's words w - 1 (bit 31), w and w + 1 (bit 0): every step reads a word and its neighbours, so no
// thread walks a long run, and a full row costs what an empty one costs.
//
//  * obstacle_list_kernel — a workgroup of four waves takes a frame, then the frame a grid further on, through one
//    scratch slot (svx_objects_host.h: a parent and an area table of H x 16 WW int32; only the entries of the
//    frame's own nodes are ever read, and those are written first, so the slot is never cleared). A thread takes
//    every 256th word in each of five sweeps, with a workgroup barrier between them:
//      1. nodes: parent and area 0 of every segment; an empty frame ends here;
//      2. unions: union-find over the nodes as the speckle filter's (sgbm.hip: path halving, the larger root hooked
//         under the smaller by compare-and-swap), so a component's root is its first pixel's node;
//      3. areas: a read-only root walk per segment, the segment's length added at the root (a thread sums what it
//         adds to one root in a row), and the node pointed straight at its root;
//      4. selection: a root with area >= min_area counts, and its key area << 32 | ~first goes down a list of cap
//         LDS words by atomic maxima, each slot keeping the largest key that passed and handing the smaller on; the
//         slots end as the cap largest keys in order whatever the interleaving. A key below the last slot is dropped
//         at once (the slots only grow). The listed roots' area entries are then overwritten with -(slot + 1);
//      5. listed components only: box, sums, disparity count and maximum by LDS atomics into the slot's record,
//         the disparities into the slot's 256-bin histogram (cap KB of LDS, bin-major so the medians' scan has no
//         bank conflicts); then a lane per slot scans its histogram for the lower median and writes the entry.
//    Box, sums and disparity are reduced in sweep 5, not at every root: a record a node would be six times the
//    scratch, and only the listed components' are ever read.
#include <limits.h>

#include "../svx_objects.h"

namespace svx {

// The tables are read and written through agent-scope atomics: the area table takes atomic adds, which the L2
// performs, and a plain load could be served by a line the CU read before them.
__device__ __forceinline__ int ob_ld(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ob_st(int32_t* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sgbm.hip's cc_find / cc_root / cc_unite over the node table
__device__ __forceinline__ int ob_find(int32_t* par, int x) {
    int p = ob_ld(par + x);
    while (p != x) {
        const int gp = ob_ld(par + p);
        if (gp != p) ob_st(par + x, gp);   // path halving
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ int ob_root(const int32_t* par, int x) {   // read-only: once the unions are done
    int p = ob_ld(par + x);
    while (p != x) {
        x = p;
        p = ob_ld(par + x);
    }
    return x;
}

__device__ __forceinline__ void ob_unite(int32_t* par, int a, int b) {
    a = ob_find(par, a);
    b = ob_find(par, b);
    while (a != b) {
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicCAS(par + b, b, a);
        if (old == b) break;
        b = old;   // b was hooked meanwhile: climb from its new parent
        a = ob_find(par, a);
        b = ob_find(par, b);
    }
}

// the first bit of the segment of v that holds the set bit p
__device__ __forceinline__ int seg_start(uint32_t v, int p) {
    const uint32_t z = ~v & ((1u << p) - 1u);
    return z ? 32 - __builtin_clz(z) : 0;
}

// f(s, e) for every segment [s, e] of v, lowest first
template <class F>
__device__ __forceinline__ void for_segments(uint32_t v, F f) {
    while (v) {
        const int s = __builtin_ctz(v);
        const uint32_t t = ~(v >> s);   // (the zeros shifted in end a segment that reaches bit 31)
        const int e = s + (t ? __builtin_ctz(t) : 32) - 1;
        f(s, e);
        v = e >= 31 ? 0u : v & (0xFFFFFFFFu << (e + 1));
    }
}

__global__ __launch_bounds__(256) void obstacle_list_kernel(const uint32_t* __restrict__ bits, int frames, int H, int W,
                                                            int WW, const uint8_t* __restrict__ disp,
                                                            int64_t disp_frame_bytes, int disp_ld, int min_area,
                                                            int cap, int32_t* __restrict__ par_all,
                                                            int32_t* __restrict__ area_all,
                                                            sv_obstacle* __restrict__ out, int32_t* __restrict__ n_out) {
    extern __shared__ uint32_t ob_hist[];   // 256 bins x cap slots, bin-major (with a disparity only)
    __shared__ unsigned long long top[kObjMaxCap], sx[kObjMaxCap], sy[kObjMaxCap];
    __shared__ int bx0[kObjMaxCap], by0[kObjMaxCap], bx1[kObjMaxCap], by1[kObjMaxCap], snd[kObjMaxCap],
        sdmax[kObjMaxCap];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int HW = 16 * WW, nw = H * WW;
    const uint32_t tail = (W & 31) ? (1u << (W & 31)) - 1u : 0xFFFFFFFFu;
    int32_t* par = par_all + (size_t)blockIdx.x * (size_t)H * HW;
    int32_t* area = area_all + (size_t)blockIdx.x * (size_t)H * HW;

    for (int64_t f = blockIdx.x; f < frames; f += gridDim.x) {
        const uint32_t* src = bits + f * nw;
        const auto word = [&](int y, int w) {
            const uint32_t v = src[y * WW + w];
            return w == WW - 1 ? v & tail : v;
        };
        if (tid < kObjMaxCap) {
            top[tid] = 0;
            sx[tid] = 0;
            sy[tid] = 0;
            bx0[tid] = INT_MAX;
            by0[tid] = INT_MAX;
            bx1[tid] = -1;
            by1[tid] = -1;
            snd[tid] = 0;
            sdmax[tid] = 0;
        }
        if (tid == 0) s_n = 0;

        // 1. nodes
        int any = 0;
        for (int i = tid; i < nw; i += 256) {
            const int y = i / WW, w = i - y * WW;
            const uint32_t v = word(y, w);
            if (!v) continue;
            any = 1;
            const uint32_t pv = (w > 0 && (v & 1u)) ? word(y, w - 1) : 0u;
            const int base = y * HW + 16 * w;
            for_segments(v, [&](int s, int) {
                const int node = base + (s >> 1);
                const int p = (s == 0 && (pv >> 31)) ? base - 16 + (seg_start(pv, 31) >> 1) : node;
                ob_st(par + node, p);
                ob_st(area + node, 0);
            });
        }
        if (!__syncthreads_or(any)) {   // (the same for the whole workgroup)
            if (tid == 0) n_out[f] = 0;
            continue;
        }

        // 2. unions with the row above
        for (int i = tid + WW; i < nw; i += 256) {
            const int y = i / WW, w = i - y * WW;
            const uint32_t v = word(y, w);
            if (!v) continue;
            const uint32_t pw = word(y - 1, w);
            const uint32_t pl = (w > 0 && (v & 1u)) ? word(y - 1, w - 1) : 0u;
            const uint32_t pr = (w + 1 < WW && (v >> 31)) ? word(y - 1, w + 1) : 0u;
            if (!(pw | (pl >> 31) | (pr & 1u))) continue;
            const int base = y * HW + 16 * w, pbase = base - HW;
            for_segments(v, [&](int s, int e) {
                const int node = base + (s >> 1);
                const int lo = max(s - 1, 0), hi = min(e + 1, 31);
                uint32_t m = pw & (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo);
                while (m) {   // a piece of the window is part of one segment of the row above
                    const int p = __builtin_ctz(m);
                    ob_unite(par, node, pbase + (seg_start(pw, p) >> 1));
                    const uint32_t t = ~(m >> p);
                    const int pe = p + (t ? __builtin_ctz(t) : 32) - 1;
                    m = pe >= 31 ? 0u : m & (0xFFFFFFFFu << (pe + 1));
                }
                // the neighbour words' corner bits, unless the run they belong to was met in pw
                if (s == 0 && (pl >> 31) && !(pw & 1u)) ob_unite(par, node, pbase - 16 + (seg_start(pl, 31) >> 1));
                if (e == 31 && (pr & 1u) && !(pw >> 31)) ob_unite(par, node, pbase + 16);
            });
        }
        __syncthreads();

        // 3. areas; every node pointed at its root (a final value: walkers see an ancestor or the root either way)
        {
            int acc_root = -1, acc = 0;
            for (int i = tid; i < nw; i += 256) {
                const int y = i / WW, w = i - y * WW;
                const uint32_t v = word(y, w);
                if (!v) continue;
                const int base = y * HW + 16 * w;
                for_segments(v, [&](int s, int e) {
                    const int node = base + (s >> 1);
                    const int r = ob_root(par, node);
                    if (r != node) ob_st(par + node, r);
                    if (r != acc_root) {
                        if (acc) atomicAdd(area + acc_root, acc);
                        acc_root = r;
                        acc = 0;
                    }
                    acc += e - s + 1;
                });
            }
            if (acc) atomicAdd(area + acc_root, acc);
        }
        __syncthreads();

        // 4. the roots of at least min_area pixels: their number, and the cap largest keys
        for (int i = tid; i < nw; i += 256) {
            const int y = i / WW, w = i - y * WW;
            const uint32_t v = word(y, w);
            if (!v) continue;
            const int base = y * HW + 16 * w;
            for_segments(v, [&](int s, int) {
                const int node = base + (s >> 1);
                if (ob_ld(par + node) != node) return;
                const int a = ob_ld(area + node);
                if (a < min_area) return;
                atomicAdd(&s_n, 1);
                const uint32_t first = (uint32_t)(y * W + 32 * w + s);
                unsigned long long key = ((unsigned long long)(uint32_t)a << 32) | (0xFFFFFFFFu - first);
                if (key < __hip_atomic_load(&top[cap - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;
                for (int j = 0; j < cap && key; ++j) {
                    const unsigned long long old = atomicMax(&top[j], key);
                    if (old < key) key = old;
                }
            });
        }
        __syncthreads();
        const int n = s_n, L = min(n, cap);
        if (tid < L) {
            const uint32_t first = 0xFFFFFFFFu - (uint32_t)top[tid];
            const int y = (int)first / W, x = (int)first - y * W;
            ob_st(area + y * HW + (x >> 1), -(tid + 1));
        }
        if (disp)
            for (int i = tid; i < 256 * cap; i += 256) ob_hist[i] = 0;
        __syncthreads();

        // 5. the listed components' records
        const uint8_t* dfr = disp ? disp + f * disp_frame_bytes : nullptr;
        for (int i = tid; i < nw; i += 256) {
            const int y = i / WW, w = i - y * WW;
            const uint32_t v = word(y, w);
            if (!v) continue;
            const int base = y * HW + 16 * w;
            for_segments(v, [&](int s, int e) {
                const int a = ob_ld(area + ob_ld(par + base + (s >> 1)));
                if (a >= 0) return;
                const int slot = -a - 1, xa = 32 * w + s, xb = 32 * w + e, cnt = e - s + 1;
                atomicMin(&bx0[slot], xa);
                atomicMax(&bx1[slot], xb);
                atomicMin(&by0[slot], y);
                atomicMax(&by1[slot], y);
                atomicAdd(&sx[slot], (unsigned long long)((xa + xb) * cnt / 2));
                atomicAdd(&sy[slot], (unsigned long long)(y * cnt));
                if (dfr) {
                    const uint8_t* row = dfr + (int64_t)y * disp_ld;
                    int nd = 0, dm = 0;
                    for (int x = xa; x <= xb; ++x) {
                        const int d = row[x];
                        if (d) {
                            ++nd;
                            dm = max(dm, d);
                            atomicAdd(&ob_hist[d * cap + slot], 1u);
                        }
                    }
                    if (nd) {
                        atomicAdd(&snd[slot], nd);
                        atomicMax(&sdmax[slot], dm);
                    }
                }
            });
        }
        __syncthreads();

        // the lower median of a slot's nd values: the first bin at which the running count passes (nd - 1) / 2
        if (tid < L) {
            const int nd = snd[tid];
            int dmed = 0;
            if (nd > 0) {
                const uint32_t want = (uint32_t)((nd - 1) / 2 + 1);
                uint32_t cum = 0;
                for (int d = 1; d < 256; ++d) {
                    cum += ob_hist[d * cap + tid];
                    if (cum >= want) {
                        dmed = d;
                        break;
                    }
                }
            }
            const uint32_t first = 0xFFFFFFFFu - (uint32_t)top[tid];
            sv_obstacle o;
            o.x0 = bx0[tid];
            o.y0 = by0[tid];
            o.x1 = bx1[tid];
            o.y1 = by1[tid];
            o.area = (int32_t)(top[tid] >> 32);
            o.first = (int32_t)first;
            o.nd = nd;
            o.dmax = sdmax[tid];
            o.dmed = dmed;
            o.reserved = 0;
            o.sx = (int64_t)sx[tid];
            o.sy = (int64_t)sy[tid];
            out[f * cap + tid] = o;
        }
        if (tid == 0) n_out[f] = n;
        __syncthreads();   // the records and the scratch slot are the next frame's
    }
}

hipError_t launch_obstacle_list(const uint32_t* bits, int frames, int H, int W, const uint8_t* disp,
                                int64_t disp_frame_bytes, int disp_ld, int min_area, int cap, void* scratch,
                                sv_obstacle* out, int32_t* n, hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    if (!bits || !scratch || !out || !n || H < 1 || H > 4096 || W < 2 || W > 4096 || min_area < 1 || cap < 1 ||
        cap > kObjMaxCap || (disp && disp_ld < W))
        return hipErrorInvalidValue;
    const ObjLayout l = objects_layout(H, W, frames);
    int32_t* par = static_cast<int32_t*>(scratch);
    int32_t* area = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + l.off_area);
    const size_t lds = disp ? sizeof(uint32_t) * 256 * (size_t)cap : 0;
    hipLaunchKernelGGL(obstacle_list_kernel, dim3((unsigned)l.slots), dim3(256), lds, s, bits, frames, H, W, l.WW, disp,
                       disp_frame_bytes, disp_ld, min_area, cap, par, area, out, n);
    return hipGetLastError();
}

}  // namespace svx
