// The result image (gfx950): stereovision.py:181-209 with drawRoadLine (functions.py:390-394) and drawNormalLine
// (functions.py:424-431), from the batch's BGR and the obstacle stage's outputs (include/svx.h, sv_result_image).
//
// One workgroup of four waves takes a band of 64 rows of a frame.
//  1. Plan: the strokes become per-row pixel intervals in LDS, 16 bytes a row: two runs for the hull's outline
//     (the outline of a convex polygon is its outer offset without its inner erosion, so a row meets it in at most
//     two runs), one for the glyph's line, one for its head. Wave 0 plans the outline, a lane a row: every edge
//     whose rows come within 2 of the lane's row gives one interval, found by bisecting the exact predicate
//     4 D(p; a, b) <= 25 on each side of a pixel that is known to satisfy it (the edge's crossing of the row
//     rounded, or the nearer end's x): D along a row is convex in x. Wave 1 plans the glyph the same way, the
//     line's predicate in 128-bit integers (a tip of 2^31 puts the squared cross product near 2^92).
//  2. Stream: a wave a row, a lane 16 pixels (48 bytes: three 16-byte loads and stores; 8 pixels and 8-byte
//     accesses where the row stride is no multiple of 16 pixels): 0.6 i rounded on every byte, + 102 on G and R of
//     the obstacle pixels (the lane's 16 bits of the obstacle word), then the row's intervals, later layers over
//     earlier ones. A frame without a hull vertex is copied.
// No pixel loops over the edges; all predicates are exact integers.
#include "../svx_result.h"

namespace svx {

namespace {

using i128 = __int128;

constexpr int kBand = 64;

// the plan of a row: closed pixel intervals clipped to the image, empty when lo > hi
struct RowPlan {
    int16_t o0lo, o0hi, o1lo, o1hi;   // the outline's runs
    int16_t llo, lhi;                 // the glyph's line
    int16_t hlo, hhi;                 // the glyph's head
};

// kn * D(p; a, b) <= kd, D the squared distance from p to the closed segment ab (a point when a == b)
template <class T>
__device__ __forceinline__ bool near_segment(T ax, T ay, T bx, T by, T px, T py, int kn, int kd) {
    const T dx = bx - ax, dy = by - ay, wx = px - ax, wy = py - ay;
    const T t = wx * dx + wy * dy, L = dx * dx + dy * dy;
    if (t <= 0) return kn * (wx * wx + wy * wy) <= kd;
    if (t >= L) {
        const T ux = px - bx, uy = py - by;
        return kn * (ux * ux + uy * uy) <= kd;
    }
    const T cr = dx * wy - dy * wx;
    return kn * cr * cr <= kd * L;
}

// floor(num / den), den > 0
__device__ __forceinline__ int64_t floor_div64(int64_t num, int64_t den) {
    const int64_t q = num / den;
    return (num % den < 0) ? q - 1 : q;
}

// The pixels x of row y, 0 <= x < W, with kn * D((x, y); a, b) <= kd, for a row within `reach` rows of the segment
// (reach^2 * kn <= kd < (reach + 1)^2 * kn): false when there is none. The seed x0 satisfies the predicate: inside
// the segment's rows the crossing rounded to the nearest pixel lies within half a pixel of the segment; above or
// below them the nearer end's x is `reach` rows or fewer away.
template <class T>
__device__ bool row_interval(int64_t ax, int64_t ay, int64_t bx, int64_t by, int y, int W, int kn, int kd,
                             int reach, int& lo, int& hi) {
    const int64_t ymin = min(ay, by), ymax = max(ay, by);
    if (y < ymin - reach || y > ymax + reach) return false;
    int64_t x0;
    if (y <= ymin) x0 = ay <= by ? ax : bx;
    else if (y >= ymax) x0 = ay <= by ? bx : ax;
    else {
        int64_t num = (bx - ax) * (y - ay), den = by - ay;   // |num| < 2^48
        if (den < 0) num = -num, den = -den;
        x0 = ax + floor_div64(2 * num + den, 2 * den);
    }
    const int64_t A64 = max((int64_t)0, min(ax, bx) - reach - 1), B64 = min((int64_t)W - 1, max(ax, bx) + reach + 1);
    if (A64 > B64) return false;
    const int A = (int)A64, B = (int)B64;
    const int xs = (int)min(max(x0, (int64_t)A), (int64_t)B);
    const auto pred = [&](int x) { return near_segment<T>((T)ax, (T)ay, (T)bx, (T)by, (T)x, (T)y, kn, kd); };
    // the interval is contiguous and holds x0: when x0 is outside the image, the border pixel decides
    if ((int64_t)xs != x0 && !pred(xs)) return false;
    int l = A, h = xs;
    while (l < h) {
        const int m = (l + h) >> 1;
        if (pred(m)) h = m;
        else l = m + 1;
    }
    lo = l;
    l = xs, h = B;
    while (l < h) {
        const int m = (l + h + 1) >> 1;
        if (pred(m)) l = m;
        else h = m - 1;
    }
    hi = l;
    return true;
}

__device__ __forceinline__ bool touches(int lo, int hi, int rlo, int rhi) {
    return rlo <= rhi && lo <= rhi + 1 && hi >= rlo - 1;
}

// the outline's runs of row y: every edge's interval merged into at most two runs
__device__ void plan_outline(const int32_t* __restrict__ P, int n, int y, int W, RowPlan& r) {
    int r0lo = 1, r0hi = 0, r1lo = 1, r1hi = 0;
    const int E = n >= 3 ? n : 1;
    for (int e = 0; e < E; ++e) {
        const int e1 = e + 1 < n ? e + 1 : 0;
        const int2 a = reinterpret_cast<const int2*>(P)[e], b = reinterpret_cast<const int2*>(P)[e1];
        int lo, hi;
        if (!row_interval<int64_t>(a.x, a.y, b.x, b.y, y, W, 4, 25, 2, lo, hi)) continue;
        if (r0lo > r0hi) {
            r0lo = lo, r0hi = hi;
        } else if (touches(lo, hi, r0lo, r0hi)) {
            r0lo = min(r0lo, lo), r0hi = max(r0hi, hi);
        } else if (touches(lo, hi, r1lo, r1hi)) {
            r1lo = min(r1lo, lo), r1hi = max(r1hi, hi);
        } else if (r1lo > r1hi) {
            r1lo = lo, r1hi = hi;
        } else {   // a third run: not a convex outline (the host entry refuses those); it joins the first
            r0lo = min(r0lo, lo), r0hi = max(r0hi, hi);
        }
        if (touches(r0lo, r0hi, r1lo, r1hi)) {
            r0lo = min(r0lo, r1lo), r0hi = max(r0hi, r1hi);
            r1lo = 1, r1hi = 0;
        }
    }
    r.o0lo = (int16_t)r0lo, r.o0hi = (int16_t)r0hi, r.o1lo = (int16_t)r1lo, r.o1hi = (int16_t)r1hi;
}

// the glyph's line and head in row y
__device__ void plan_glyph(const sv_hull_info& in, int y, int W, RowPlan& r) {
    int llo = 1, lhi = 0, hlo = 1, hhi = 0;
    const int64_t lim = 2147483647;
    if ((in.valid & 2) && in.tipx >= -lim && in.tipx <= lim && in.tipy >= -lim && in.tipy <= lim) {
        int lo, hi;
        if (row_interval<i128>(in.cx, in.cy, in.tipx, in.tipy, y, W, 1, 1, 1, lo, hi)) llo = lo, lhi = hi;
        const int64_t dy = (int64_t)y - in.tipy;
        if (dy >= -7 && dy <= 7) {
            int hw = 0;
            while ((hw + 1) * (hw + 1) + (int)(dy * dy) <= 49) ++hw;
            const int64_t a = max(in.tipx - hw, (int64_t)0), b = min(in.tipx + hw, (int64_t)W - 1);
            if (a <= b) hlo = (int)a, hhi = (int)b;
        }
    }
    r.llo = (int16_t)llo, r.lhi = (int16_t)lhi, r.hlo = (int16_t)hlo, r.hhi = (int16_t)hhi;
}

// rint(0.6 v) of the four bytes of a word: floor((6 v + 5) / 10) = floor((3 v + 2) / 5), and n / 5 =
// (n * 205) >> 10 for n <= 767
__device__ __forceinline__ uint32_t blend4(uint32_t w) {
    const uint32_t b0 = ((3u * (w & 255u) + 2u) * 205u) >> 10;
    const uint32_t b1 = ((3u * ((w >> 8) & 255u) + 2u) * 205u) >> 10;
    const uint32_t b2 = ((3u * ((w >> 16) & 255u) + 2u) * 205u) >> 10;
    const uint32_t b3 = ((3u * (w >> 24) + 2u) * 205u) >> 10;
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// a chunk of PX pixels: three vectors V of its 3 PX / 4 words (kept in registers: no array is indexed by a variable)
template <int PX>
struct Chunk;
template <>
struct Chunk<16> {
    using V = uint4;
    static __device__ __forceinline__ void unpack(const V& v, uint32_t* w) {
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    }
    static __device__ __forceinline__ V pack(const uint32_t* w) { return make_uint4(w[0], w[1], w[2], w[3]); }
};
template <>
struct Chunk<8> {
    using V = uint2;
    static __device__ __forceinline__ void unpack(const V& v, uint32_t* w) { w[0] = v.x, w[1] = v.y; }
    static __device__ __forceinline__ V pack(const uint32_t* w) { return make_uint2(w[0], w[1]); }
};

// the three bytes of pixel k of a chunk (NW words), as a window of the two words they lie in
template <int NW>
__device__ __forceinline__ void pixel_window(const uint32_t (&w)[NW], int k, uint64_t& win, int& wi, int& sh) {
    wi = (3 * k) >> 2;
    sh = ((3 * k) & 3) * 8;
    win = (uint64_t)w[wi] | (wi + 1 < NW ? (uint64_t)w[wi + 1] << 32 : 0ull);
}
template <int NW>
__device__ __forceinline__ void pixel_store(uint32_t (&w)[NW], uint64_t win, int wi) {
    w[wi] = (uint32_t)win;
    if (wi + 1 < NW) w[wi + 1] = (uint32_t)(win >> 32);
}

template <int PX>
__global__ __launch_bounds__(256) void result_kernel(const uint8_t* __restrict__ bgr, int64_t frame_bytes, int ld3,
                                                     const uint32_t* __restrict__ obst,
                                                     const int32_t* __restrict__ pts, int64_t pts_stride,
                                                     const sv_hull_info* __restrict__ info, int H, int W, int bands,
                                                     uint8_t* __restrict__ out) {
    using V = typename Chunk<PX>::V;
    constexpr int NW = PX * 3 / 4;   // words of a chunk
    constexpr int NV = 3;            // vectors of a chunk
    __shared__ RowPlan plan[kBand];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t frame = blockIdx.x / bands;
    const int band = blockIdx.x - (int)frame * bands;
    const int y0 = band * kBand, rows = min(kBand, H - y0);
    const sv_hull_info in = info[frame];
    const int n = in.n;

    if (n > 0) {
        if (wv == 0 && lane < rows) plan_outline(pts + frame * pts_stride, n, y0 + lane, W, plan[lane]);
        if (wv == 1 && lane < rows) plan_glyph(in, y0 + lane, W, plan[lane]);
    }
    __syncthreads();

    const int WW = (W + 31) >> 5, Wp = ld3 / 3;
    const int chunks = Wp / PX;
    for (int r = wv; r < rows; r += 4) {
        const int y = y0 + r;
        const int64_t ro = frame * frame_bytes + (int64_t)y * ld3;
        const V* src = reinterpret_cast<const V*>(bgr + ro);
        V* dst = reinterpret_cast<V*>(out + ro);
        const uint32_t* orow = obst + (frame * H + y) * WW;
        for (int c = lane; c < chunks; c += 64) {
            V v[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) v[k] = src[NV * c + k];
            uint32_t w[NW];
#pragma unroll
            for (int k = 0; k < NV; ++k) Chunk<PX>::unpack(v[k], w + k * (NW / NV));
            if (n > 0) {
                const int x0 = c * PX;
                const uint32_t ob = (orow[x0 >> 5] >> (x0 & 31)) & ((1u << PX) - 1u);
#pragma unroll
                for (int k = 0; k < NW; ++k) w[k] = blend4(w[k]);
                if (ob) {
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        if ((ob >> k) & 1u) {
                            uint64_t win;
                            int wi, sh;
                            pixel_window<NW>(w, k, win, wi, sh);
                            win += (uint64_t)0x666600u << sh;   // G and R + 102: at most 255, no carry
                            pixel_store<NW>(w, win, wi);
                        }
                    }
                }
                const RowPlan p = plan[r];
                const int x1 = x0 + PX - 1;
                const bool any = (p.o0lo <= x1 && p.o0hi >= x0) || (p.o1lo <= x1 && p.o1hi >= x0) ||
                                 (p.llo <= x1 && p.lhi >= x0) || (p.hlo <= x1 && p.hhi >= x0);
                if (any) {
#pragma unroll
                    for (int k = 0; k < PX; ++k) {
                        const int x = x0 + k;
                        uint32_t col = 0xFFFFFFFFu;
                        if ((x >= p.o0lo && x <= p.o0hi) || (x >= p.o1lo && x <= p.o1hi)) col = 0xFF0000u;   // red
                        if (x >= p.llo && x <= p.lhi) col = 204u | (185u << 8) | (22u << 16);
                        if (x >= p.hlo && x <= p.hhi) col = 214u | (195u << 8) | (32u << 16);
                        if (col != 0xFFFFFFFFu) {
                            uint64_t win;
                            int wi, sh;
                            pixel_window<NW>(w, k, win, wi, sh);
                            win = (win & ~((uint64_t)0xFFFFFFu << sh)) | ((uint64_t)col << sh);
                            pixel_store<NW>(w, win, wi);
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) dst[NV * c + k] = Chunk<PX>::pack(w + k * (NW / NV));
        }
    }
}

}  // namespace

hipError_t launch_result(const uint8_t* bgr, int64_t frame_bytes, int ld3, const uint32_t* obst, const int32_t* pts,
                         int64_t pts_stride, const sv_hull_info* info, int frames, int H, int W, uint8_t* out,
                         hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    const int Wp = (W + 7) / 8 * 8;
    if (!bgr || !obst || !pts || !info || !out || H < 1 || H > kResultMaxH || W < 2 || W > kResultMaxW ||
        ld3 != 3 * Wp || frame_bytes < (int64_t)H * ld3 || frame_bytes % 8 != 0 || pts_stride < 0)
        return hipErrorInvalidValue;
    const auto al = [&](uintptr_t m) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(bgr), b = reinterpret_cast<uintptr_t>(out);
        return ((a | b | (uintptr_t)frame_bytes) & m) == 0;
    };
    if (!al(7) || (reinterpret_cast<uintptr_t>(pts) & 7u) != 0 || (pts_stride & 1) != 0) return hipErrorInvalidValue;
    const int bands = (H + kBand - 1) / kBand;
    const int64_t blocks = (int64_t)frames * bands;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    if (Wp % 16 == 0 && al(15))
        hipLaunchKernelGGL(result_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, s, bgr, frame_bytes, ld3, obst, pts,
                           pts_stride, info, H, W, bands, out);
    else
        hipLaunchKernelGGL(result_kernel<8>, dim3((unsigned)blocks), dim3(256), 0, s, bgr, frame_bytes, ld3, obst, pts,
                           pts_stride, info, H, W, bands, out);
    return hipGetLastError();
}

}  // namespace svx
