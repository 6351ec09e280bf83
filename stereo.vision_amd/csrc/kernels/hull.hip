// The obstacle stage (gfx950): stereovision.py:170-189 and functions.py:396-421 on the cleaned road bitmap.
//
// Per frame: the convex hull of the set pixels (strict vertices), the hull filled as a bitmap, the obstacles
// (hull & ~cleaned), the centre of the hull's exact minimum enclosing circle and the tip of the road-normal glyph
// drawn from it (include/svx.h, sv_road_obstacles). Bitmaps have morph.hip's layout: rows of WW = ceil(W / 32)
// words, pixel x at bit x & 31 of word x >> 5, pad bits zero.
//
//  * road_hull_kernel — one workgroup of four waves per frame, the frame's state in LDS (12 bytes a row):
//      1. row extremes: a group of G lanes (G = the row's loads, 16 bytes each where the row is a multiple of four
//         words, rounded up to a power of two, at most 64) takes a row, a lane the ctz / clz of its words, min / max
//         over the group by xor shuffles -> L[y], R[y] (-1: empty row); four rows' loads are in flight at a time;
//      2. the two chains: the hull of a bitmap is the hull of its rows' extreme pixels, the left chain over
//         (L[y], y) and the right chain over (R[y], y). One lane per chain (lane 0 of waves 0 and 1) runs the
//         monotone-chain scan down the rows with its stack in LDS and the stack's top two in registers;
//      3. spans: a lane per row finds the chain edge that covers the row by bisection and takes
//         [ceil(xl), floor(xr)] in integers (floor division, right for negative numerators);
//      4. one lane (wave 3's first) computes the circle and the glyph tip while the other waves write the words of
//         the hull mask and the obstacles, whole words, 16 bytes a lane where the row length allows.
//  * min_circle_kernel — the circle alone, of a caller's points (getCenterPoint).
//
// The circle: its centre is a rational (px / q, py / q) with q > 0, and its squared radius rn / q^2; p and q fit
// 64 bits (|q| < 2^26 for image coordinates), the containment test (q x - px)^2 + (q y - py)^2 <= rn is done in
// 128-bit integers, and nothing is divided but p by q at the end. The iteration is deterministic: the basis (at
// most three points) starts as vertex 0; the point farthest outside the current circle (lowest index among equals)
// joins, and the new circle is the smallest one through it and some of the basis that holds the rest of the
// basis: a diametral circle, or the circumcircle of a non-obtuse triangle. The radius grows strictly, so it ends,
// with the one minimum enclosing circle whichever of several possible supports it ends on.
#include <limits.h>

#include "../svx_hull.h"

namespace svx {

using i128 = __int128;

struct Circle {
    int64_t px, py, q;   // centre (px / q, py / q), q > 0
    i128 rn;             // squared radius x q^2
};

__device__ __forceinline__ i128 sq128(int64_t v) { return (i128)v * v; }

__device__ __forceinline__ i128 circle_dist2(const Circle& c, int x, int y) {
    return sq128(c.q * x - c.px) + sq128(c.q * y - c.py);
}

// the circle with a-b as a diameter
__device__ __forceinline__ Circle circle_of2(int ax, int ay, int bx, int by) {
    Circle c;
    c.px = (int64_t)ax + bx;
    c.py = (int64_t)ay + by;
    c.q = 2;
    const int64_t dx = (int64_t)ax - bx, dy = (int64_t)ay - by;
    c.rn = (i128)(dx * dx + dy * dy);
    return c;
}

// the circumcircle of a, b, c; false when they are collinear or the triangle is obtuse (then the circumcircle is
// not the smallest circle around the three)
__device__ __forceinline__ bool circle_of3(int ax, int ay, int bx_, int by_, int cx_, int cy_, Circle& o) {
    const int64_t bx = (int64_t)bx_ - ax, by = (int64_t)by_ - ay, cx = (int64_t)cx_ - ax, cy = (int64_t)cy_ - ay;
    int64_t d = 2 * (bx * cy - by * cx);
    if (d == 0) return false;
    if (bx * cx + by * cy < 0 || bx * (bx - cx) + by * (by - cy) < 0 || cx * (cx - bx) + cy * (cy - by) < 0)
        return false;
    const int64_t b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
    int64_t nx = cy * b2 - by * c2, ny = bx * c2 - cx * b2;
    if (d < 0) {
        d = -d;
        nx = -nx;
        ny = -ny;
    }
    o.px = ax * d + nx;
    o.py = ay * d + ny;
    o.q = d;
    o.rn = sq128(nx) + sq128(ny);
    return true;
}

// The minimum enclosing circle of the n >= 1 points get(i, x, y) (see the head of the file). false: the
// iteration's bound was reached or no circle through the new point held the basis (neither happens in exact
// arithmetic; the bound keeps a fault elsewhere from spinning here).
template <class Get>
__device__ bool min_circle(int n, Get get, Circle& c) {
    int b0x, b0y, b1x = 0, b1y = 0, b2x = 0, b2y = 0, nb = 1;
    get(0, b0x, b0y);
    c.px = b0x;
    c.py = b0y;
    c.q = 1;
    c.rn = 0;
    for (int it = 0; it < 4 * n + 64; ++it) {
        int far = -1;
        i128 dmax = c.rn;
        for (int i = 0; i < n; ++i) {
            int x, y;
            get(i, x, y);
            const i128 d = circle_dist2(c, x, y);
            if (d > dmax) {
                dmax = d;
                far = i;
            }
        }
        if (far < 0) return true;
        int px, py;
        get(far, px, py);
        Circle t;
        // a diametral circle through p and one of the basis that holds the others
        if (t = circle_of2(px, py, b0x, b0y), (nb < 2 || circle_dist2(t, b1x, b1y) <= t.rn) &&
                                                   (nb < 3 || circle_dist2(t, b2x, b2y) <= t.rn)) {
            nb = 2;
        } else if (nb >= 2 && (t = circle_of2(px, py, b1x, b1y), circle_dist2(t, b0x, b0y) <= t.rn &&
                                                                     (nb < 3 || circle_dist2(t, b2x, b2y) <= t.rn))) {
            b0x = b1x, b0y = b1y;
            nb = 2;
        } else if (nb >= 3 && (t = circle_of2(px, py, b2x, b2y),
                               circle_dist2(t, b0x, b0y) <= t.rn && circle_dist2(t, b1x, b1y) <= t.rn)) {
            b0x = b2x, b0y = b2y;
            nb = 2;
        // the circumcircle of p and two of the basis that holds the third
        } else if (nb >= 2 && circle_of3(px, py, b0x, b0y, b1x, b1y, t) &&
                   (nb < 3 || circle_dist2(t, b2x, b2y) <= t.rn)) {
            b2x = b1x, b2y = b1y;
            nb = 3;
        } else if (nb >= 3 && circle_of3(px, py, b0x, b0y, b2x, b2y, t) && circle_dist2(t, b1x, b1y) <= t.rn) {
            nb = 3;
        } else if (nb >= 3 && circle_of3(px, py, b1x, b1y, b2x, b2y, t) && circle_dist2(t, b0x, b0y) <= t.rn) {
            b0x = b1x, b0y = b1y;
            nb = 3;
        } else {
            return false;
        }
        // the basis: b0 (, b2 when nb = 3), and p in b1
        b1x = px, b1y = py;
        c = t;
    }
    return false;
}

// floor(num / den), den > 0
__device__ __forceinline__ int floor_div(int num, int den) {
    const int q = num / den;
    return (num % den < 0) ? q - 1 : q;
}

// Where the chain S (n packed vertices x | y << 16, y increasing) crosses row y, S[0].y <= y <= S[n - 1].y:
// ceil of the crossing for the left chain, floor for the right one.
template <bool LEFT>
__device__ __forceinline__ int chain_cross(const uint32_t* S, int n, int y) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {   // the last vertex at or above the row
        const int mid = (lo + hi + 1) >> 1;
        if ((int)(S[mid] >> 16) <= y) lo = mid;
        else hi = mid - 1;
    }
    if (lo == n - 1) {
        if (n == 1) return (int)(S[0] & 0xFFFFu);
        lo = n - 2;
    }
    const uint32_t a = S[lo], b = S[lo + 1];
    const int ax = (int)(a & 0xFFFFu), ay = (int)(a >> 16), bx = (int)(b & 0xFFFFu), by = (int)(b >> 16);
    const int num = (bx - ax) * (y - ay), den = by - ay;
    return ax + (LEFT ? -floor_div(-num, den) : floor_div(num, den));
}

// bits lo..hi of the row, as they fall into word w
__device__ __forceinline__ uint32_t span_word(int lo, int hi, int w) {
    const int a = max(lo - 32 * w, 0), b = min(hi - 32 * w, 31);
    return a <= b ? ((0xFFFFFFFFu >> (31 - b)) & (0xFFFFFFFFu << a)) : 0u;
}

// getNormalVectorLine((cx, cy), abc, disparity) (functions.py:396-416) in the reference's operation order (the
// file is built without contraction); false where the reference raises or a result does not fit an int64
__device__ bool glyph_tip(const HullPlane& p, int cx, int cy, uint8_t d8, int64_t& tx, int64_t& ty) {
    if (d8 == 0) return false;   // ZeroDivisionError
    double Z = p.fB / (double)d8;
    const double X = (((double)cx - p.cw) * Z) / p.f;
    const double Y = (((double)cy - p.ch) * Z) / p.f;
    double newY = Y - 0.7;
    double newX = X + 0.0;
    const double d = __builtin_sqrt(p.a * p.a + p.b * p.b + p.c * p.c);
    Z = d - ((p.a * newX) + (p.b * newY));
    newX = ((newX * p.f) / Z) + p.cw;
    newY = ((newY * p.f) / Z) + p.ch;
    // int() raises on inf and nan; |v| < 2^63 so that the truncation fits
    if (!(__builtin_fabs(newX) < 0x1p63) || !(__builtin_fabs(newY) < 0x1p63)) return false;
    tx = (int64_t)newX;
    ty = (int64_t)newY;
    return true;
}

// Eight waves a SIMD (63 VGPRs; the circle's 128-bit terms spill 20 bytes a lane): 2,048 workgroups resident, so a
// batch of 4,096 frames is two full rounds. Measured 0.42 against 0.47 ms a batch at seven waves (68 VGPRs, no spill).
__global__ __launch_bounds__(256, 8) void road_hull_kernel(const uint32_t* __restrict__ cleaned, int H, int W, int WW,
                                                        int G, const uint8_t* __restrict__ disp,
                                                        int64_t disp_frame_bytes, int disp_ld,
                                                        const FramePlane* __restrict__ planes, int plane_stride,
                                                        HullPlane shared, int32_t* __restrict__ pts,
                                                        uint32_t* __restrict__ mask, uint32_t* __restrict__ obst,
                                                        sv_hull_info* __restrict__ info, int vec) {
    extern __shared__ __align__(16) unsigned char hull_lds[];
    int* hdr = reinterpret_cast<int*>(hull_lds);              // left / right chain lengths
    uint32_t* SL = reinterpret_cast<uint32_t*>(hull_lds + 16);   // the chains' stacks: x | y << 16
    uint32_t* SR = SL + H;
    int16_t* L = reinterpret_cast<int16_t*>(SR + H);          // row extremes, later the rows' spans
    int16_t* R = L + H;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t frame = blockIdx.x;
    const int64_t fo = frame * H * WW;
    const uint32_t* src = cleaned + fo;
    // 1. row extremes (every lane of a wave makes the same trips; four rows' loads are in flight before the first
    // is used)
    {
        const int rpw = 64 / G, sub = lane & (G - 1), slot = wv * rpw + lane / G, rows = 4 * rpw;
        const auto reduce_store = [&](int y, int mn, int mx) {
            for (int o = G >> 1; o; o >>= 1) {
                mn = min(mn, __shfl_xor(mn, o));
                mx = max(mx, __shfl_xor(mx, o));
            }
            if (y < H && sub == 0) {
                mx = min(mx, W - 1);   // pad bits are zero; a set one could not leave the frame either
                L[y] = (int16_t)(mx < 0 ? -1 : mn);
                R[y] = (int16_t)mx;
            }
        };
        if (vec) {   // 16 bytes a lane: G lanes cover the row's WW / 4 quads
            const int Q = WW / 4;
            const uint4* src4 = reinterpret_cast<const uint4*>(src);
            for (int base = 0; base < H; base += 4 * rows) {
                uint4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int y = base + u * rows + slot;
                    v[u] = (y < H && sub < Q) ? src4[y * Q + sub] : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint64_t lo = (uint64_t)v[u].x | ((uint64_t)v[u].y << 32);
                    const uint64_t hi = (uint64_t)v[u].z | ((uint64_t)v[u].w << 32);
                    int mn = INT_MAX, mx = -1;
                    if (lo | hi) {
                        mn = 128 * sub + (lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll(hi));
                        mx = 128 * sub + (hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo));
                    }
                    reduce_store(base + u * rows + slot, mn, mx);
                }
            }
        } else {     // a word a lane: G lanes stride over the row's true word count
            for (int base = 0; base < H; base += rows) {
                const int y = base + slot;
                int mn = INT_MAX, mx = -1;
                if (y < H)
                    for (int w = sub; w < WW; w += G) {
                        const uint32_t v = src[y * WW + w];
                        if (v) {
                            mn = min(mn, 32 * w + __builtin_ctz(v));
                            mx = max(mx, 32 * w + 31 - __builtin_clz(v));
                        }
                    }
                reduce_store(y, mn, mx);
            }
        }
    }
    __syncthreads();
    sv_hull_info res = {0, 0, 0, 0, 0, 0};
    // 2. the chains: the vertex below the stack's top stays while it lies strictly outside the line from the one
    // under it to the new point
    if (tid == 0 || tid == 64) {
        const bool left = tid == 0;
        const int16_t* X = left ? L : R;
        uint32_t* S = left ? SL : SR;
        int n = 0, ax = 0, ay = 0, bx = 0, by = 0;   // S[n - 2], S[n - 1]
        int xn = X[0];
        for (int y = 0; y < H; ++y) {
            const int x = xn;
            if (y + 1 < H) xn = X[y + 1];
            if (x < 0) continue;
            while (n >= 2) {
                const int cr = (bx - ax) * (y - ay) - (by - ay) * (x - ax);
                if (left ? cr < 0 : cr > 0) break;
                --n;
                bx = ax;
                by = ay;
                if (n >= 2) {
                    const uint32_t v = S[n - 2];
                    ax = (int)(v & 0xFFFFu);
                    ay = (int)(v >> 16);
                }
            }
            S[n++] = (uint32_t)x | ((uint32_t)y << 16);
            ax = bx;
            ay = by;
            bx = x;
            by = y;
        }
        hdr[left ? 0 : 1] = n;
    }
    __syncthreads();
    const int nl = hdr[0], nr = hdr[1];
    int rhi = 0;

    if (nl > 0) {   // (the same for the whole workgroup; nr > 0 too)
        const int yt = (int)(SL[0] >> 16), yb = (int)(SL[nl - 1] >> 16);   // the first and last row with a pixel

        // 3. the rows' spans
        for (int y = tid; y < H; y += 256) {
            int lo = 1, hi = 0;
            if (y >= yt && y <= yb) {
                lo = chain_cross<true>(SL, nl, y);
                hi = min(chain_cross<false>(SR, nr, y), W - 1);
            }
            L[y] = (int16_t)lo;
            R[y] = (int16_t)hi;
        }
        __syncthreads();

        // the vertices in order: down the left chain, then up the right chain without the ends the chains share
        rhi = nr - 1 - (SR[nr - 1] == SL[nl - 1] ? 1 : 0);
        const int rlo = SR[0] == SL[0] ? 1 : 0;
        const int n = nl + max(0, rhi - rlo + 1);
        const auto vert = [&](int i, int& x, int& y) {
            const uint32_t v = i < nl ? SL[i] : SR[rhi - (i - nl)];
            x = (int)(v & 0xFFFFu);
            y = (int)(v >> 16);
        };
        for (int i = tid; i < n; i += 256) {
            int x, y;
            vert(i, x, y);
            reinterpret_cast<int2*>(pts + frame * 4 * H)[i] = make_int2(x, y);
        }

        // 4. the circle and the glyph tip
        if (tid == 192) {
            res.n = n;
            Circle c;
            if (min_circle(n, vert, c)) {
                res.cx = (int32_t)(c.px / c.q);
                res.cy = (int32_t)(c.py / c.q);
                res.valid = 1;
                HullPlane pl = shared;
                if (planes) {
                    const FramePlane& fp = planes[frame * plane_stride];
                    pl.a = fp.a, pl.b = fp.b, pl.c = fp.c, pl.f = fp.f, pl.fB = fp.fB, pl.cw = fp.cw, pl.ch = fp.ch;
                    pl.valid = fp.valid;
                }
                if (disp && pl.valid && res.cx >= 0 && res.cx < W && res.cy >= 0 && res.cy < H) {
                    const uint8_t d8 = disp[frame * disp_frame_bytes + (int64_t)res.cy * disp_ld + res.cx];
                    int64_t tx = 0, ty = 0;
                    if (glyph_tip(pl, res.cx, res.cy, d8, tx, ty)) {
                        res.tipx = tx;
                        res.tipy = ty;
                        res.valid |= 2;
                    }
                }
            }
        }
    } else {
        for (int y = tid; y < H; y += 256) {   // an empty frame: empty spans
            L[y] = 1;
            R[y] = 0;
        }
        __syncthreads();
    }
    if (tid == 192) info[frame] = res;

    // the words of the hull mask and of the obstacles
    if (!mask && !obst) return;
    if (vec) {
        const int nq = H * WW / 4;   // WW % 4 == 0: a quad of words stays in its row
        const uint4* src4 = reinterpret_cast<const uint4*>(src);
        for (int i0 = tid; i0 < nq; i0 += 4 * 256) {   // four loads in flight
            uint4 c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + 256 * u;
                c[u] = (obst && i < nq) ? src4[i] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + 256 * u;
                if (i >= nq) break;
                const int y = 4 * i / WW, w = 4 * i - y * WW;
                const int lo = L[y], hi = R[y];
                uint4 m;
                m.x = span_word(lo, hi, w);
                m.y = span_word(lo, hi, w + 1);
                m.z = span_word(lo, hi, w + 2);
                m.w = span_word(lo, hi, w + 3);
                if (mask) reinterpret_cast<uint4*>(mask + fo)[i] = m;
                if (obst)
                    reinterpret_cast<uint4*>(obst + fo)[i] =
                        make_uint4(m.x & ~c[u].x, m.y & ~c[u].y, m.z & ~c[u].z, m.w & ~c[u].w);
            }
        }
    } else {
        const int nw = H * WW;
        for (int i = tid; i < nw; i += 256) {
            const int y = i / WW, w = i - y * WW;
            const uint32_t m = span_word(L[y], R[y], w);
            if (mask) mask[fo + i] = m;
            if (obst) obst[fo + i] = m & ~src[i];
        }
    }
}

hipError_t launch_road_hull(const uint32_t* cleaned, int frames, int H, int W, const uint8_t* disp,
                            int64_t disp_frame_bytes, int disp_ld, const FramePlane* planes, int plane_stride,
                            const HullPlane& shared, int32_t* pts, uint32_t* mask, uint32_t* obst, sv_hull_info* info,
                            hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    if (!cleaned || !pts || !info || H < 1 || H > kHullMaxH || W < 2 || W > 4096 || (disp && disp_ld < W))
        return hipErrorInvalidValue;
    const int WW = (W + 31) / 32;
    const auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const int vec = WW % 4 == 0 && a16(cleaned) && a16(mask) && a16(obst);
    const int per_row = vec ? WW / 4 : WW;   // loads a row: 16 bytes a lane, else a word a lane
    int G = 1;                               // lanes a row
    while (G < per_row && G < 64) G <<= 1;
    const size_t lds = 16 + 12 * (size_t)H;
    hipLaunchKernelGGL(road_hull_kernel, dim3((unsigned)frames), dim3(256), lds, s, cleaned, H, W, WW, G, disp,
                       disp_frame_bytes, disp_ld, planes, plane_stride, shared, pts, mask, obst, info, vec);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void min_circle_kernel(const int32_t* __restrict__ pts, int n,
                                                        int32_t* __restrict__ out) {
    if (threadIdx.x != 0) return;
    Circle c;
    const bool ok = min_circle(n, [&](int i, int& x, int& y) { x = pts[2 * i], y = pts[2 * i + 1]; }, c);
    out[0] = ok ? (int32_t)(c.px / c.q) : 0;
    out[1] = ok ? (int32_t)(c.py / c.q) : 0;
    out[2] = ok ? 1 : 0;
}

hipError_t launch_min_circle(const int32_t* pts, int64_t n, int32_t* out, hipStream_t s) {
    if (!pts || !out || n < 1 || n > kCircleMaxPoints) return hipErrorInvalidValue;
    hipLaunchKernelGGL(min_circle_kernel, dim3(1), dim3(64), 0, s, pts, (int)n, out);
    return hipGetLastError();
}

}  // namespace svx
