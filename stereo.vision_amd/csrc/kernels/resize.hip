// General-scale bilinear resize of 8-bit pictures (gfx950): cv2.resize's INTER_LINEAR path as tests/tile_numpy.py
// restates it (resize_linear_u8), for resizeImage and batchImages (functions.py:452-501). The coefficient tables
// come from the host (svx_resize_host.h, resize_fill_tables): per destination column the two source columns sx, sx1
// and their 11-bit coefficients a0, a1, per destination row sy, sy1, b0, b1. Per output byte, in int32:
//   r0  = src[sy ][sx] * a0 + src[sy ][sx1] * a1
//   r1  = src[sy1][sx] * a0 + src[sy1][sx1] * a1
//   out = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
// which stays within 0 .. 255 (a0 + a1 and b0 + b1 are 2048 up to the two roundings), so nothing saturates.
//
// A workgroup takes 16 output rows of one image, a wave four of them: the rows' sy, sy1, b0, b1 are wave-uniform
// and read once, lanes run along the row, and a lane reads its columns' table entries once for its wave's four rows.
//  - PX = 1: an output pixel per lane from byte loads, byte stores. Every shape.
//  - PX = 4: four output pixels per lane: the table entries from 16- and 8-byte loads, the pixels stored as 4 bytes
//    (grey) or 12 (BGR). dw % 4 == 0 and a 4-byte aligned destination (svx_resize.h). The source is gathered by bytes.
//  - WIN (PX = 4, grey source, 4-byte aligned source rows): a lane's eight samples of a source row come from one
//    16-byte window of it, at the 4-byte boundary below its first column: a byte-pair select (v_perm_b32) puts
//    src[sx] and src[sx + 1] into the halves of a word, and one 16-bit dot product with (a0, a1) is the horizontal
//    pass. src[sx + 1] stands in for src[sx1]: they differ only where sx is the last column, and there a1 = 0. The
//    windows of the wave's four rows are all requested before the first is used: with a row's loads waited for one
//    after the other the kernel ran at the memory's latency. A lane whose samples do not fit the
//    window (a scale above about 3), or whose window would end past the last byte of the source (src_end), gathers
//    by bytes as above: the choice is per lane and changes no result.
// No array is indexed by a variable: every index is a constant after unrolling. No LDS.
#include "../svx_resize.h"

namespace svx {

namespace {

constexpr int kRows = 16;          // output rows of a workgroup
constexpr int kRowsPerWave = 4;    // ... of each of its four waves, consecutive: their source rows are neighbours

struct ResizeTabs {
    const int32_t *xs0, *xs1;
    const int16_t *xa0, *xa1;
    const int32_t *ys0, *ys1;
    const int16_t *yb0, *yb1;
};

// the vertical pass over the two rows' horizontal sums. Nothing is negative, r >> 4 <= 255 * 2049 >> 4 and
// b <= 2048 fit 24 bits and their product 32, so the full-rate 24-bit multiply gives the int32 product.
__device__ __forceinline__ uint32_t vertical(uint32_t r0, uint32_t r1, uint32_t b0, uint32_t b1) {
    return ((__umul24(b0, r0 >> 4) >> 16) + (__umul24(b1, r1 >> 4) >> 16) + 2u) >> 2;
}

__device__ __forceinline__ uint32_t blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, uint32_t a0,
                                          uint32_t a1, uint32_t b0, uint32_t b1) {
    return vertical(__umul24(p00, a0) + __umul24(p01, a1), __umul24(p10, a0) + __umul24(p11, a1), b0, b1);
}

// 16 bytes at a 4-byte boundary
struct __attribute__((aligned(4))) Window {
    uint32_t w0, w1, w2, w3;
};

typedef unsigned short ushort2_t __attribute__((ext_vector_type(2)));

// src[o] * a0 + src[o + 1] * a1 for the byte offset o = 4 j + rem (j = 0 .. 2) into the window: sel picks the two
// bytes out of words j and j + 1 into the halves of a word, coef holds a0 | a1 << 16
__device__ __forceinline__ uint32_t window_pass(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t j,
                                                uint32_t sel, uint32_t coef) {
    const uint32_t lo = j == 0 ? w0 : j == 1 ? w1 : w2;
    const uint32_t hi = j == 0 ? w1 : j == 1 ? w2 : w3;
    const uint32_t pair = __builtin_amdgcn_perm(hi, lo, sel);
    return __builtin_amdgcn_udot2(__builtin_bit_cast(ushort2_t, pair), __builtin_bit_cast(ushort2_t, coef), 0u, false);
}

// a lane's PX pixels of one output row, gathered by bytes
template <int PX, int SC, int DC>
__device__ __forceinline__ void gather_row(const uint8_t* p0, const uint8_t* p1, const uint32_t (&sx)[PX],
                                           const uint32_t (&sx1)[PX], const uint32_t (&a0)[PX],
                                           const uint32_t (&a1)[PX], uint32_t b0, uint32_t b1, uint32_t (&px)[PX]) {
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        uint32_t v = 0;
#pragma unroll
        for (int ch = 0; ch < SC; ++ch) {
            const uint32_t o0 = SC * sx[j] + ch, o1 = SC * sx1[j] + ch;
            v |= blend(p0[o0], p0[o1], p1[o0], p1[o1], a0[j], a1[j], b0, b1) << (8 * ch);
        }
        px[j] = (SC == 1 && DC == 3) ? v * 0x010101u : v;
    }
}

// ... stored: px holds B | G << 8 | R << 16, or the grey byte
template <int PX, int DC>
__device__ __forceinline__ void store_row(uint8_t* o, const uint32_t (&px)[PX]) {
    if constexpr (PX == 4 && DC == 1) {
        *reinterpret_cast<uint32_t*>(o) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    } else if constexpr (PX == 4) {
        *reinterpret_cast<uint3*>(o) =
            make_uint3(px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8));
    } else if constexpr (DC == 1) {
        o[0] = (uint8_t)px[0];
    } else {
        o[0] = (uint8_t)px[0], o[1] = (uint8_t)(px[0] >> 8), o[2] = (uint8_t)(px[0] >> 16);
    }
}

template <int PX, int SC, int DC, bool WIN>
__global__ __launch_bounds__(256) void resize_linear_kernel(const ResizeArgs a, const ResizeTabs t, int row_blocks) {
    static_assert((PX == 1 || PX == 4) && (SC == 1 || SC == 3) && (DC == 1 || DC == 3) && DC >= SC, "instances");
    static_assert(!WIN || (PX == 4 && SC == 1), "the window form: four grey pixels a lane");
    constexpr int R = kRowsPerWave;
    // the wave's number through readfirstlane: the rows' table entries and pointers are then scalar, and every
    // load and store is a scalar base plus a lane's 32-bit offset
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t frame = blockIdx.x / row_blocks;
    const int rb = blockIdx.x - (int)frame * row_blocks;
    const int y0 = rb * kRows + wv * R;
    if (y0 >= a.dh) return;
    const uint8_t* src = a.src + frame * a.src_frame;
    uint8_t* dst = a.dst + a.dst_off + frame * a.dst_frame;
    // the wave's rows, read once; a row past the last one repeats it and is not stored
    const uint8_t *p0[R], *p1[R];
    uint8_t* orow[R];
    uint32_t b0[R], b1[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int y = min(y0 + r, a.dh - 1);
        b0[r] = (uint32_t)t.yb0[y], b1[r] = (uint32_t)t.yb1[y];
        p0[r] = src + (int64_t)t.ys0[y] * a.src_ld;
        p1[r] = src + (int64_t)t.ys1[y] * a.src_ld;
        orow[r] = dst + (int64_t)y * a.dst_ld;
    }
    // the bytes from the wave's last source row (sy1 does not decrease with y) to the end of the source: a window
    // must end within them. It does, but for the last lanes of the last image's last rows.
    const int64_t left = a.src_end - p1[R - 1];
    const uint32_t room = left > 0x7FFFFFFF ? 0x7FFFFFFFu : (uint32_t)left;
    for (uint32_t x0 = lane * PX; x0 < (uint32_t)a.dw; x0 += 64 * PX) {
        uint32_t sx[PX], sx1[PX], a0[PX], a1[PX];   // columns 0 .. 8191, coefficients 0 .. 2048
        if constexpr (PX == 4) {
            const uint4 u = *reinterpret_cast<const uint4*>(t.xs0 + x0);
            const uint4 v = *reinterpret_cast<const uint4*>(t.xs1 + x0);
            const uint2 c = *reinterpret_cast<const uint2*>(t.xa0 + x0);   // no sign to extend
            const uint2 d = *reinterpret_cast<const uint2*>(t.xa1 + x0);
            sx[0] = u.x, sx[1] = u.y, sx[2] = u.z, sx[3] = u.w;
            sx1[0] = v.x, sx1[1] = v.y, sx1[2] = v.z, sx1[3] = v.w;
            a0[0] = c.x & 0xFFFFu, a0[1] = c.x >> 16, a0[2] = c.y & 0xFFFFu, a0[3] = c.y >> 16;
            a1[0] = d.x & 0xFFFFu, a1[1] = d.x >> 16, a1[2] = d.y & 0xFFFFu, a1[3] = d.y >> 16;
        } else {
            sx[0] = t.xs0[x0], sx1[0] = t.xs1[x0], a0[0] = t.xa0[x0], a1[0] = t.xa1[x0];
        }
        bool windowed = false;
        if constexpr (WIN) {
            // the window starts at column wx; pixel j's pair of bytes lies in words wj[j], wj[j] + 1 at the bytes
            // wsel[j] names (0x0c: a zero byte)
            const uint32_t wx = sx[0] & ~3u;
            windowed = sx[3] - wx <= 14u && wx + 16u <= room;   // sx[3] + 1 within the 16 bytes, and they exist
            if (windowed) {
                uint32_t wj[PX], wsel[PX], wcoef[PX];
#pragma unroll
                for (int j = 0; j < PX; ++j) {
                    const uint32_t o = sx[j] - wx;
                    wj[j] = min(o >> 2, 2u);
                    const uint32_t rem = o - 4u * wj[j];
                    wsel[j] = rem | 0x0c00u | ((rem + 1u) << 16) | 0x0c000000u;
                    wcoef[j] = a0[j] | (a1[j] << 16);
                }
                // every row's loads before the first use: one round trip for the four rows. Words, not structures:
                // an array of structures is an array in scratch.
                uint32_t u0[R], u1[R], u2[R], u3[R], v0[R], v1[R], v2[R], v3[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const Window u = *reinterpret_cast<const Window*>(p0[r] + wx);
                    const Window v = *reinterpret_cast<const Window*>(p1[r] + wx);
                    u0[r] = u.w0, u1[r] = u.w1, u2[r] = u.w2, u3[r] = u.w3;
                    v0[r] = v.w0, v1[r] = v.w1, v2[r] = v.w2, v3[r] = v.w3;
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    uint32_t px[PX];
#pragma unroll
                    for (int j = 0; j < PX; ++j) {
                        const uint32_t g =
                            vertical(window_pass(u0[r], u1[r], u2[r], u3[r], wj[j], wsel[j], wcoef[j]),
                                     window_pass(v0[r], v1[r], v2[r], v3[r], wj[j], wsel[j], wcoef[j]), b0[r], b1[r]);
                        px[j] = DC == 3 ? g * 0x010101u : g;
                    }
                    if (y0 + r < a.dh) store_row<PX, DC>(orow[r] + (uint32_t)DC * x0, px);
                }
            }
        }
        if (!windowed) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                uint32_t px[PX];
                gather_row<PX, SC, DC>(p0[r], p1[r], sx, sx1, a0, a1, b0[r], b1[r], px);
                if (y0 + r < a.dh) store_row<PX, DC>(orow[r] + (uint32_t)DC * x0, px);
            }
        }
    }
}

template <int PX, int SC, int DC, bool WIN = false>
void launch_instance(const ResizeArgs& a, const ResizeTabs& t, int row_blocks, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL((resize_linear_kernel<PX, SC, DC, WIN>), dim3(blocks), dim3(256), 0, s, a, t, row_blocks);
}

template <int PX>
void launch_channels(const ResizeArgs& a, const ResizeTabs& t, int row_blocks, unsigned blocks, hipStream_t s) {
    if (a.sc == 3) launch_instance<PX, 3, 3>(a, t, row_blocks, blocks, s);
    else if (a.dc == 3) launch_instance<PX, 1, 3>(a, t, row_blocks, blocks, s);
    else launch_instance<PX, 1, 1>(a, t, row_blocks, blocks, s);
}

void launch_window(const ResizeArgs& a, const ResizeTabs& t, int row_blocks, unsigned blocks, hipStream_t s) {
    if (a.dc == 3) launch_instance<4, 1, 3, true>(a, t, row_blocks, blocks, s);
    else launch_instance<4, 1, 1, true>(a, t, row_blocks, blocks, s);
}

}  // namespace

hipError_t launch_resize_linear(const ResizeArgs& a0, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    ResizeArgs a = a0;
    if (resize_check_shape(a.sh, a.sw, a.dh, a.dw) || !a.src || !a.dst || !a.tables) return hipErrorInvalidValue;
    if ((a.sc != 1 && a.sc != 3) || (a.dc != 1 && a.dc != 3) || a.dc < a.sc) return hipErrorInvalidValue;
    if (a.src_ld < a.sw * a.sc || a.dst_ld < a.dw * a.dc || a.src_frame < 0 || a.dst_frame < 0 || a.dst_off < 0)
        return hipErrorInvalidValue;
    if (reinterpret_cast<uintptr_t>(a.tables) & 15u) return hipErrorInvalidValue;
    const ResizeTableLayout l = resize_table_layout(a.dh, a.dw);
    ResizeTabs t;
    t.xs0 = reinterpret_cast<const int32_t*>(a.tables + l.xs0);
    t.xs1 = reinterpret_cast<const int32_t*>(a.tables + l.xs1);
    t.xa0 = reinterpret_cast<const int16_t*>(a.tables + l.xa0);
    t.xa1 = reinterpret_cast<const int16_t*>(a.tables + l.xa1);
    t.ys0 = reinterpret_cast<const int32_t*>(a.tables + l.ys0);
    t.ys1 = reinterpret_cast<const int32_t*>(a.tables + l.ys1);
    t.yb0 = reinterpret_cast<const int16_t*>(a.tables + l.yb0);
    t.yb1 = reinterpret_cast<const int16_t*>(a.tables + l.yb1);
    const int row_blocks = (a.dh + kRows - 1) / kRows;
    const int64_t blocks = (int64_t)n * row_blocks;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    const bool quad = a.dw % 4 == 0 && a.dw >= kResizeQuadMin &&
                      ((reinterpret_cast<uintptr_t>(a.dst) + (uintptr_t)a.dst_off) & 3u) == 0 && a.dst_frame % 4 == 0 &&
                      a.dst_ld % 4 == 0;
    // the last byte of the last image's last row, + 1: no window is read past it
    a.src_end = a.src + (int64_t)(n - 1) * a.src_frame + (int64_t)(a.sh - 1) * a.src_ld + (int64_t)a.sw * a.sc;
    const bool window = quad && a.sc == 1 && a.sw <= kResizeWindowScale * a.dw &&
                        (reinterpret_cast<uintptr_t>(a.src) & 3u) == 0 && a.src_frame % 4 == 0 && a.src_ld % 4 == 0;
    if (window) launch_window(a, t, row_blocks, (unsigned)blocks, s);
    else if (quad) launch_channels<4>(a, t, row_blocks, (unsigned)blocks, s);
    else launch_channels<1>(a, t, row_blocks, (unsigned)blocks, s);
    return hipGetLastError();
}

}  // namespace svx
