// The image tile (gfx950): batchImages (functions.py:452-499) for the five pictures of stereovision.py:216, all of
// the frame's size, so that resizeImage is a copy (include/svx.h, sv_image_tile):
//   stack = vstack(hstack(Disparity, ImageRoadMap), hstack(RoadImage, FilteredRoadImage))      2 H x 2 W
//   tile  = hstack(resize(stack, 1 / 4), resize(Result, 1 / 2))                                 H / 2 x W
// Both resizes are means of four samples rounded half up: of columns 4 dx + 1, 4 dx + 2 of rows 4 dy + 1, 4 dy + 2 of
// the stack, and of the 2 x 2 block of the result. With H and W multiples of 4 an output pixel lies in one picture.
//
// A wave takes an output row: its W / 4 pixels of the left picture and W / 4 of the right one of its half of the
// stack (the top half for dy < H / 4), and its W / 2 pixels of the result. imageRoadMap is not read: its quadrant
// is the BGR with (0, 255, 0) where the road picture is set, painted as the samples are taken. The road picture and
// the cleaned one come as u8 or as bitmaps (svx_tile.h); a bitmap word of two rows holds eight output pixels, the
// mask 0x66666666.
//  - W % 16 == 0 and 16-byte aligned rows: a lane takes 16 source pixels of every picture of its row from 16-byte
//    loads along the two source rows: 2 x 16 grey bytes, 2 x 48 BGR bytes or half a bitmap word a row for each of
//    the stack's two pictures (4 output pixels each, a 12-byte store), 2 x 48 bytes of the result (8 output pixels,
//    three 8-byte stores). The samples stay in registers; every index is a constant after unrolling (no array
//    indexed by a variable: DESIGN §7.8).
//  - other shapes (W % 4 == 0): a lane makes one output pixel at a time from byte loads.
#include "../svx_tile.h"

namespace svx {

namespace {

constexpr int kRows = 16;   // output rows of a workgroup: four waves, four rows each

__device__ __forceinline__ uint32_t mean4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return (a + b + c + d + 2u) >> 2;
}

// byte i of a run of bytes held as words
template <int N>
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[N], int i) {
    return (w[i >> 2] >> ((i & 3) * 8)) & 255u;
}

// NV 16-byte vectors from p
template <int NV>
__device__ __forceinline__ void load16(const uint8_t* p, uint32_t (&w)[4 * NV]) {
    const uint4* v = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const uint4 t = v[k];
        w[4 * k] = t.x, w[4 * k + 1] = t.y, w[4 * k + 2] = t.z, w[4 * k + 3] = t.w;
    }
}

// four pixels (B | G << 8 | R << 16) as 12 bytes
__device__ __forceinline__ void pack4(const uint32_t* p, uint32_t* w) {
    w[0] = p[0] | (p[1] << 24);
    w[1] = (p[1] >> 8) | (p[2] << 16);
    w[2] = (p[2] >> 16) | (p[3] << 8);
}

// ... at dst (4-byte aligned)
__device__ __forceinline__ void store4(uint8_t* dst, const uint32_t (&p)[4]) {
    uint32_t w[3];
    pack4(p, w);
    *reinterpret_cast<uint3*>(dst) = make_uint3(w[0], w[1], w[2]);
}

// eight pixels as 24 bytes at dst (8-byte aligned)
__device__ __forceinline__ void store8(uint8_t* dst, const uint32_t (&p)[8]) {
    uint32_t w[6];
    pack4(p, w);
    pack4(p + 4, w + 3);
    uint2* d = reinterpret_cast<uint2*>(dst);
    d[0] = make_uint2(w[0], w[1]);
    d[1] = make_uint2(w[2], w[3]);
    d[2] = make_uint2(w[4], w[5]);
}

// a grey picture's four output pixels from 16 bytes of its two rows
__device__ __forceinline__ void grey4(const uint8_t* r1, const uint8_t* r2, uint32_t (&p)[4]) {
    uint32_t a[4], b[4];
    load16<1>(r1, a);
    load16<1>(r2, b);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        p[j] = mean4(byte_of(a, 4 * j + 1), byte_of(a, 4 * j + 2), byte_of(b, 4 * j + 1), byte_of(b, 4 * j + 2)) *
               0x010101u;
}

// the same from 16 bits of a bitmap word of each row: k of the four samples set give (255 k + 2) >> 2
__device__ __forceinline__ void bits4(uint32_t m1, uint32_t m2, uint32_t (&p)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t k = __popc((m1 >> (4 * j)) & 6u) + __popc((m2 >> (4 * j)) & 6u);
        p[j] = ((255u * k + 2u) >> 2) * 0x010101u;
    }
}

// the sampled pixels of 16 bytes of a u8 row as bitmap bits (4 j + 1 and 4 j + 2: the others are not read)
__device__ __forceinline__ uint32_t sampled_mask(const uint8_t* r) {
    uint32_t a[4], m = 0;
    load16<1>(r, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m |= (byte_of(a, 4 * j + 1) ? 1u : 0u) << (4 * j + 1);
        m |= (byte_of(a, 4 * j + 2) ? 1u : 0u) << (4 * j + 2);
    }
    return m;
}

// imageRoadMap's four output pixels from 48 bytes of the BGR's two rows and the road picture's bits
__device__ __forceinline__ void map4(const uint8_t* r1, const uint8_t* r2, uint32_t m1, uint32_t m2,
                                     uint32_t (&p)[4]) {
    uint32_t a[12], b[12];
    load16<3>(r1, a);
    load16<3>(r2, b);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool f0 = (m1 >> (4 * j + 1)) & 1u, f1 = (m1 >> (4 * j + 2)) & 1u;
        const bool f2 = (m2 >> (4 * j + 1)) & 1u, f3 = (m2 >> (4 * j + 2)) & 1u;
        uint32_t v = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t green = ch == 1 ? 255u : 0u;   // (0, 255, 0)
            const uint32_t s = mean4(f0 ? green : byte_of(a, 12 * j + 3 + ch), f1 ? green : byte_of(a, 12 * j + 6 + ch),
                                     f2 ? green : byte_of(b, 12 * j + 3 + ch), f3 ? green : byte_of(b, 12 * j + 6 + ch));
            v |= s << (8 * ch);
        }
        p[j] = v;
    }
}

// the result's eight output pixels from 48 bytes of its two rows
__device__ __forceinline__ void result8(const uint8_t* r0, const uint8_t* r1, uint32_t (&p)[8]) {
    uint32_t a[12], b[12];
    load16<3>(r0, a);
    load16<3>(r1, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t v = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            v |= mean4(byte_of(a, 6 * j + ch), byte_of(a, 6 * j + 3 + ch), byte_of(b, 6 * j + ch),
                       byte_of(b, 6 * j + 3 + ch))
                 << (8 * ch);
        p[j] = v;
    }
}

// two rows of a picture of 0 and 255: bytes, or words of a bitmap when b1 is set
struct MaskRows {
    const uint8_t *u1, *u2;
    const uint32_t *b1, *b2;
};

__device__ __forceinline__ MaskRows mask_rows(const TilePlane& u8, const TilePlane& bits, int64_t frame, int y) {
    MaskRows r{nullptr, nullptr, nullptr, nullptr};
    if (bits.p) {
        r.b1 = static_cast<const uint32_t*>(bits.p) + frame * bits.frame + (int64_t)y * bits.ld;
        r.b2 = r.b1 + bits.ld;
    } else {
        r.u1 = static_cast<const uint8_t*>(u8.p) + frame * u8.frame + (int64_t)y * u8.ld;
        r.u2 = r.u1 + u8.ld;
    }
    return r;
}

// pixel x of row k (0, 1) as a byte
__device__ __forceinline__ uint32_t mask_value(const MaskRows& r, int k, int x) {
    if (r.b1) {
        const uint32_t* row = k ? r.b2 : r.b1;
        return ((row[x >> 5] >> (x & 31)) & 1u) ? 255u : 0u;
    }
    const uint8_t* row = k ? r.u2 : r.u1;
    return row[x];
}

// the 16 pixels of chunk c of row k as bitmap bits (of a u8 row: the sampled ones)
__device__ __forceinline__ uint32_t mask_bits(const MaskRows& r, int k, int c) {
    if (r.b1) {
        const uint32_t* row = k ? r.b2 : r.b1;
        return (row[c >> 1] >> (16 * (c & 1))) & 0xFFFFu;
    }
    const uint8_t* row = k ? r.u2 : r.u1;
    return sampled_mask(row + 16 * c);
}

__device__ __forceinline__ void mask4(const MaskRows& r, int c, uint32_t (&p)[4]) {
    if (r.b1) bits4(mask_bits(r, 0, c), mask_bits(r, 1, c), p);
    else grey4(r.u1 + 16 * c, r.u2 + 16 * c, p);
}

template <bool VEC>
__global__ __launch_bounds__(256) void tile_kernel(const TileArgs a, int row_blocks, uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t frame = blockIdx.x / row_blocks;
    const int rb = blockIdx.x - (int)frame * row_blocks;
    const int H = a.H, W = a.W, H2 = H >> 1, H4 = H >> 2, W2 = W >> 1, W4 = W >> 2;
    const uint8_t* disp = static_cast<const uint8_t*>(a.disp.p) + frame * a.disp.frame;
    const uint8_t* bgr = static_cast<const uint8_t*>(a.bgr.p) + frame * a.bgr.frame;
    const uint8_t* res = static_cast<const uint8_t*>(a.res.p) + frame * a.res.frame;
    for (int r = wv; r < kRows; r += 4) {
        const int dy = rb * kRows + r;
        if (dy >= H2) break;
        uint8_t* orow = out + (frame * H2 + dy) * (3 * (int64_t)W);
        const bool top = dy < H4;
        const int y1 = 4 * (top ? dy : dy - H4) + 1;   // the stack's two rows, in their pictures: y1, y1 + 1
        const MaskRows road = mask_rows(a.road, a.rbits, frame, y1);
        const MaskRows clean = mask_rows(a.clean, a.cbits, frame, y1);
        const uint8_t* d1 = disp + (int64_t)y1 * a.disp.ld;
        const uint8_t* d2 = d1 + a.disp.ld;
        const uint8_t* c1 = bgr + (int64_t)y1 * a.bgr.ld;
        const uint8_t* c2 = c1 + a.bgr.ld;
        const uint8_t* r0 = res + (int64_t)(2 * dy) * a.res.ld;
        const uint8_t* r1 = r0 + a.res.ld;
        if constexpr (VEC) {
            // chunk c: 16 source pixels of the stack's two pictures (4 output pixels each) and of the result (8)
            for (int c = lane; c < (W >> 4); c += 64) {
                uint32_t p[4], q[4], t[8];
                if (top) {
                    grey4(d1 + 16 * c, d2 + 16 * c, p);
                    map4(c1 + 48 * c, c2 + 48 * c, mask_bits(road, 0, c), mask_bits(road, 1, c), q);
                } else {
                    mask4(road, c, p);
                    mask4(clean, c, q);
                }
                result8(r0 + 48 * c, r1 + 48 * c, t);
                store4(orow + 12 * c, p);
                store4(orow + 3 * W4 + 12 * c, q);
                store8(orow + 3 * W2 + 24 * c, t);
            }
        } else {
            for (int x = lane; x < W; x += 64) {
                uint32_t v;
                if (x >= W2) {
                    const uint8_t* s0 = r0 + 6 * (x - W2);
                    const uint8_t* s1 = r1 + 6 * (x - W2);
                    v = mean4(s0[0], s0[3], s1[0], s1[3]) | (mean4(s0[1], s0[4], s1[1], s1[4]) << 8) |
                        (mean4(s0[2], s0[5], s1[2], s1[5]) << 16);
                } else {
                    const bool right = x >= W4;
                    const int sx = 4 * (right ? x - W4 : x) + 1;   // the two columns: sx, sx + 1
                    if (top && !right) {
                        v = mean4(d1[sx], d1[sx + 1], d2[sx], d2[sx + 1]) * 0x010101u;
                    } else if (top) {
                        const bool f0 = mask_value(road, 0, sx), f1 = mask_value(road, 0, sx + 1);
                        const bool f2 = mask_value(road, 1, sx), f3 = mask_value(road, 1, sx + 1);
                        const uint8_t* s1 = c1 + 3 * sx;
                        const uint8_t* s2 = c2 + 3 * sx;
                        v = 0;
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            const uint32_t green = ch == 1 ? 255u : 0u;
                            v |= mean4(f0 ? green : s1[ch], f1 ? green : s1[3 + ch], f2 ? green : s2[ch],
                                       f3 ? green : s2[3 + ch])
                                 << (8 * ch);
                        }
                    } else {
                        const MaskRows& m = right ? clean : road;
                        v = mean4(mask_value(m, 0, sx), mask_value(m, 0, sx + 1), mask_value(m, 1, sx),
                                  mask_value(m, 1, sx + 1)) *
                            0x010101u;
                    }
                }
                uint8_t* o = orow + 3 * x;
                o[0] = (uint8_t)v, o[1] = (uint8_t)(v >> 8), o[2] = (uint8_t)(v >> 16);
            }
        }
    }
}

}  // namespace

hipError_t launch_tile(const TileArgs& a, int frames, uint8_t* out, hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    const int H = a.H, W = a.W, WW = (W + 31) / 32;
    if (H < 4 || H > kTileMaxH || W < 4 || W > kTileMaxW || H % 4 || W % 4 || !out) return hipErrorInvalidValue;
    const auto u8_ok = [](const TilePlane& t, int row) { return t.p && t.ld >= row && t.frame >= 0; };
    if (!u8_ok(a.disp, W) || !u8_ok(a.bgr, 3 * W) || !u8_ok(a.res, 3 * W)) return hipErrorInvalidValue;
    if (!(a.rbits.p ? u8_ok(a.rbits, WW) : u8_ok(a.road, W))) return hipErrorInvalidValue;
    if (!(a.cbits.p ? u8_ok(a.cbits, WW) : u8_ok(a.clean, W))) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(a.rbits.p) | reinterpret_cast<uintptr_t>(a.cbits.p)) & 3u)
        return hipErrorInvalidValue;
    const auto al16 = [](const TilePlane& t) {
        return ((reinterpret_cast<uintptr_t>(t.p) | (uintptr_t)t.frame | (uintptr_t)t.ld) & 15u) == 0;
    };
    const bool vec = W % 16 == 0 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0 && al16(a.disp) && al16(a.bgr) &&
                     al16(a.res) && (a.rbits.p || al16(a.road)) && (a.cbits.p || al16(a.clean));
    const int row_blocks = (H / 2 + kRows - 1) / kRows;
    const int64_t blocks = (int64_t)frames * row_blocks;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    if (vec)
        hipLaunchKernelGGL(tile_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, a, row_blocks, out);
    else
        hipLaunchKernelGGL(tile_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, a, row_blocks, out);
    return hipGetLastError();
}

}  // namespace svx
