// Road-image clean-up (gfx950): the morphology of sanitiseRoadImage (functions.py:346-358) on packed bits.
//
// The reference cleans the road image with four OpenCV calls before it walks the non-zero pixels: a 9 x 9 close,
// two 9 x 9 erosions (= one 17 x 17 erosion), an AND with road_threshold_mask != 0 and a second 9 x 9 close;
// ParticleCleansing after them changes nothing. With OpenCV's default morphology borders a pixel
// outside the image is clear for a dilation and set for an erosion: the border never sets or clears a pixel.
//
// The image is a bitmap here, 32 pixels a word, pixel x of a row at bit x & 31 of word x >> 5 (the layout of the
// resident pipeline's road bitmap, PipeBuffers::rbits); a row takes WW = ceil(W / 32) words, and the pad bits of
// its last word are zero in every bitmap in memory.
//
//  * morph_pack_kernel   — u8 image -> bitmap (non-zero = set): 4 pixels a lane, 8 lanes a word.
//  * morph_clean_kernel  — the four operations. One workgroup per band of rows of one frame; the band and a
//                          24-row halo on each side (4 + 4 + 8 + 4 + 4, the chain's vertical reach) sit in LDS in
//                          two planes that ping-pong through ten passes. Every rectangle is separable: a pass
//                          along the rows (a word and its two neighbours as two 64-bit windows, shifted and
//                          combined in log steps: offsets 0..1, 0..3, (0..7,) 0..r), then one along the columns
//                          (a lane takes 8 rows of one word column, reads 8 + 2r rows once and combines them in
//                          log steps in registers). Each pass computes only the rows a later pass still needs,
//                          so the halo shrinks 24 -> 20 -> 16 -> 8 -> 4 -> 0. Rows above or below the frame are
//                          "outside" (skipped by the column passes), never the neighbouring frame's rows.
//  * morph_unpack_kernel — bitmap -> u8 image of 0 / 255 (for the widths the bitmap road pass does not take).
#include <algorithm>

#include "../svx_morph.h"

namespace svx {

constexpr int kMorphHalo = 24;    // rows of halo on each side of a band: 4 + 4 + 8 + 4 + 4
constexpr int kMorphStrip = 8;    // rows a lane produces in a column pass

// One word of a row pass by radius R: bit x of the result = OR (dilate) / AND (erode) of bits x - R .. x + R of
// the row, from the word and its neighbours (outside the row: 0 for a dilation, all ones for an erosion). The
// 64-bit window a spreads towards higher x (its high word is the result's share), b towards lower x (its low
// word); what the shifts bring in at the windows' far ends travels at most R <= 8 bits and never reaches them.
template <bool ERODE, int R>
__device__ __forceinline__ uint32_t morph_hword(uint32_t prev, uint32_t cur, uint32_t next) {
    static_assert(R == 4 || R == 8, "radius 4 or 8");
    const auto op = [](uint64_t x, uint64_t y) { return ERODE ? (x & y) : (x | y); };
    uint64_t a = (uint64_t)prev | ((uint64_t)cur << 32);
    uint64_t b = (uint64_t)cur | ((uint64_t)next << 32);
    a = op(a, a << 1);   // offsets 0..1
    b = op(b, b >> 1);
    a = op(a, a << 2);   // 0..3
    b = op(b, b >> 2);
    if (R == 8) {
        a = op(a, a << 4);   // 0..7
        b = op(b, b >> 4);
    }
    a = op(a, a << 1);   // 0..R
    b = op(b, b >> 1);
    return (uint32_t)op(a >> 32, b & 0xFFFFFFFFull);
}

// Geometry of one workgroup's band, shared by the passes. LDS row i holds frame row y0 + i.
struct MorphBand {
    int WW, LR;        // words a row; LDS rows of a plane
    int y0, H;         // frame row of LDS row 0; rows of the frame
    int tx, ty, TX, TY;   // the lane's word column and row slot; the workgroup covers TX word columns x TY rows
    uint32_t pad;      // the pad bits of a row's last word (0 when W % 32 == 0)
};

// Row pass over LDS rows [ilo, ihi): src -> dst.
template <bool ERODE, int R>
__device__ __forceinline__ void morph_rows(const MorphBand& g, const uint32_t* __restrict__ src,
                                           uint32_t* __restrict__ dst, int ilo, int ihi) {
    const uint32_t ident = ERODE ? 0xFFFFFFFFu : 0u;
    for (int i = ilo + g.ty; i < ihi; i += g.TY) {
        const uint32_t* row = src + i * g.WW;
        for (int w = g.tx; w < g.WW; w += g.TX) {
            uint32_t prev = w > 0 ? row[w - 1] : ident;
            uint32_t cur = row[w];
            uint32_t next = w + 1 < g.WW ? row[w + 1] : ident;
            if (ERODE) {   // the pad bits lie outside the row: set into an erosion
                if (w == g.WW - 1) cur |= g.pad;
                if (w + 1 == g.WW - 1) next |= g.pad;
            }
            uint32_t r = morph_hword<ERODE, R>(prev, cur, next);
            if (w == g.WW - 1) r &= ~g.pad;   // and zero in every stored bitmap
            dst[i * g.WW + w] = r;
        }
    }
}

// Column pass: LDS rows [ilo, ihi) of dst (LDS, or with OUT the frame's rows in global memory) = OR / AND of src
// rows i - R .. i + R that lie inside the frame; with mask != nullptr the result is ANDed with the mask's words.
template <bool ERODE, int R, bool OUT>
__device__ __forceinline__ void morph_cols(const MorphBand& g, const uint32_t* __restrict__ src,
                                           uint32_t* __restrict__ dst, int ilo, int ihi,
                                           const uint32_t* __restrict__ mask) {
    constexpr int S = kMorphStrip, N = S + 2 * R;
    const uint32_t ident = ERODE ? 0xFFFFFFFFu : 0u;
    const auto op = [](uint32_t x, uint32_t y) { return ERODE ? (x & y) : (x | y); };
    const int strips = (ihi - ilo + S - 1) / S;
    for (int s = g.ty; s < strips; s += g.TY) {
        const int i0 = ilo + s * S;
        for (int w = g.tx; w < g.WW; w += g.TX) {
            uint32_t v[N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const int i = i0 - R + k, y = g.y0 + i;
                v[k] = (i >= 0 && i < g.LR && y >= 0 && y < g.H) ? src[i * g.WW + w] : ident;
            }
            uint32_t p[N];   // p[k] = v[k] .. v[k + span - 1] combined, span 2, 4, 8(, 16)
#pragma unroll
            for (int k = 0; k + 1 < N; ++k) p[k] = op(v[k], v[k + 1]);
#pragma unroll
            for (int k = 0; k + 3 < N; ++k) p[k] = op(p[k], p[k + 2]);
#pragma unroll
            for (int k = 0; k + 7 < N; ++k) p[k] = op(p[k], p[k + 4]);
            if (R == 8) {
#pragma unroll
                for (int k = 0; k + 15 < N; ++k) p[k] = op(p[k], p[k + 8]);
            }
#pragma unroll
            for (int t = 0; t < S; ++t) {
                const int i = i0 + t, y = g.y0 + i;
                if (i >= ihi) break;
                uint32_t r = op(p[t], v[t + 2 * R]);   // rows i - R .. i + R
                if (mask && y >= 0 && y < g.H) r &= mask[(int64_t)y * g.WW + w];
                if (OUT) {
                    if (y >= 0 && y < g.H) dst[(int64_t)y * g.WW + w] = r;
                } else {
                    dst[i * g.WW + w] = r;
                }
            }
        }
    }
}

// in / out: frames x H x WW words; mask: H x WW words or nullptr (all ones). Workgroup (frame, band): frame rows
// [band * B, min(H, band * B + B)); LDS: two planes of (B + 48) x WW words. ltx = log2(TX), TX * TY = 256.
__global__ __launch_bounds__(256) void morph_clean_kernel(const uint32_t* __restrict__ in,
                                                          const uint32_t* __restrict__ mask,
                                                          uint32_t* __restrict__ out, int H, int WW, uint32_t pad,
                                                          int B, int ltx) {
    extern __shared__ uint32_t morph_lds[];
    const int frame = blockIdx.x, r0 = blockIdx.y * B;
    if (r0 >= H) return;   // uniform
    const int Bc = min(B, H - r0);
    MorphBand g;
    g.WW = WW;
    g.LR = B + 2 * kMorphHalo;
    g.y0 = r0 - kMorphHalo;
    g.H = H;
    g.TX = 1 << ltx;
    g.TY = 256 >> ltx;
    g.tx = threadIdx.x & (g.TX - 1);
    g.ty = threadIdx.x >> ltx;
    g.pad = pad;
    uint32_t* const P0 = morph_lds;
    uint32_t* const P1 = morph_lds + g.LR * WW;
    const uint32_t* fin = in + (int64_t)frame * H * WW;
    uint32_t* fout = out + (int64_t)frame * H * WW;
    // rows r0 - 24 .. r0 + Bc + 24 of the frame (zero outside it: those rows are never combined)
    const int rows = Bc + 2 * kMorphHalo;
    for (int i = g.ty; i < rows; i += g.TY) {
        const int y = g.y0 + i;
        for (int w = g.tx; w < WW; w += g.TX) P0[i * WW + w] = (y >= 0 && y < H) ? fin[(int64_t)y * WW + w] : 0u;
    }
    __syncthreads();
    // rows still needed with a halo of m: LDS rows [24 - m, 24 + Bc + m)
#define SVX_MORPH_LO(m) (kMorphHalo - (m))
#define SVX_MORPH_HI(m) (kMorphHalo + Bc + (m))
    // 1. close by 9 x 9: dilate radius 4, erode radius 4
    morph_rows<false, 4>(g, P0, P1, SVX_MORPH_LO(24), SVX_MORPH_HI(24));
    __syncthreads();
    morph_cols<false, 4, false>(g, P1, P0, SVX_MORPH_LO(20), SVX_MORPH_HI(20), nullptr);
    __syncthreads();
    morph_rows<true, 4>(g, P0, P1, SVX_MORPH_LO(20), SVX_MORPH_HI(20));
    __syncthreads();
    morph_cols<true, 4, false>(g, P1, P0, SVX_MORPH_LO(16), SVX_MORPH_HI(16), nullptr);
    __syncthreads();
    // 2. erode by 9 x 9 twice = radius 8; 3. AND with the mask
    morph_rows<true, 8>(g, P0, P1, SVX_MORPH_LO(16), SVX_MORPH_HI(16));
    __syncthreads();
    morph_cols<true, 8, false>(g, P1, P0, SVX_MORPH_LO(8), SVX_MORPH_HI(8), mask);
    __syncthreads();
    // 4. close by 9 x 9
    morph_rows<false, 4>(g, P0, P1, SVX_MORPH_LO(8), SVX_MORPH_HI(8));
    __syncthreads();
    morph_cols<false, 4, false>(g, P1, P0, SVX_MORPH_LO(4), SVX_MORPH_HI(4), nullptr);
    __syncthreads();
    morph_rows<true, 4>(g, P0, P1, SVX_MORPH_LO(4), SVX_MORPH_HI(4));
    __syncthreads();
    // the band's rows, to the frame: LDS row i is frame row y0 + i, so dst is indexed by the frame row
    morph_cols<true, 4, true>(g, P1, fout, SVX_MORPH_LO(0), SVX_MORPH_HI(0), nullptr);
#undef SVX_MORPH_LO
#undef SVX_MORPH_HI
}

// Rows of a band for an image of WW words a row: 24 KB a plane (48 KB a workgroup, three per CU) where that
// leaves a band of 32 rows or more, else 32 KB a plane (W = 4096: 64 rows, a band of 16); the frame's rows are
// then spread evenly over the bands.
static int morph_band_rows(int H, int W) {
    const int WW = (W + 31) / 32;
    int rows = 6144 / WW;
    if (rows < 2 * kMorphHalo + 32) rows = 8192 / WW;
    const int bmax = std::max(1, rows - 2 * kMorphHalo);
    const int nb = (H + bmax - 1) / bmax;
    return nb > 0 ? (H + nb - 1) / nb : 1;
}

hipError_t launch_morph_clean(const uint32_t* in, const uint32_t* mask, uint32_t* out, int frames, int H, int W,
                              hipStream_t s) {
    if (frames <= 0 || H <= 0) return hipSuccess;
    if (W < 2 || W > 4096) return hipErrorInvalidValue;
    const int WW = (W + 31) / 32;
    const int B = morph_band_rows(H, W), nb = (H + B - 1) / B;
    const size_t lds = sizeof(uint32_t) * 2 * (size_t)(B + 2 * kMorphHalo) * WW;
    if (lds > 65536 || nb > 65535) return hipErrorInvalidValue;
    int ltx = 0;
    while ((1 << ltx) < WW && ltx < 7) ++ltx;   // TX = the power of two >= WW (<= 128)
    const uint32_t pad = W % 32 ? 0xFFFFFFFFu << (W % 32) : 0u;
    hipLaunchKernelGGL(morph_clean_kernel, dim3((unsigned)frames, (unsigned)nb), dim3(256), lds, s, in, mask, out, H,
                       WW, pad, B, ltx);
    return hipGetLastError();
}

// img: frames images of H rows at a stride of ld bytes (ld % 4 == 0, frame f at img + f * frame_bytes, 4-byte
// aligned), Wu pixels a row -> bits: frames x H x WW words. A lane takes 4 pixels (one word of the image), the 8
// lanes of a bitmap word combine their nibbles (every lane of the wave takes part in the shuffles).
__global__ __launch_bounds__(256) void morph_pack_kernel(const uint8_t* __restrict__ img, int64_t frame_bytes, int ld,
                                                         int Wu, int H, uint32_t* __restrict__ bits, int WW) {
    const int frame = blockIdx.y;
    const int G = WW * 8;   // lanes a row
    const int64_t idx = blockIdx.x * 256ll + threadIdx.x;
    const int64_t row = idx / G;
    const int gq = (int)(idx - row * G), x0 = 4 * gq;
    uint32_t v = 0;
    if (row < H && x0 < ld) v = *reinterpret_cast<const uint32_t*>(img + frame * frame_bytes + row * ld + x0);
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (((v >> (8 * k)) & 0xFFu) != 0 && x0 + k < Wu) word |= 1u << (4 * (gq & 7) + k);
    word |= (uint32_t)__shfl_xor((int)word, 1);
    word |= (uint32_t)__shfl_xor((int)word, 2);
    word |= (uint32_t)__shfl_xor((int)word, 4);
    if ((gq & 7) == 0 && row < H) bits[((int64_t)frame * H + row) * WW + (gq >> 3)] = word;
}

hipError_t launch_morph_pack(const uint8_t* img, int64_t frame_bytes, int ld, int Wu, int H, int frames,
                             uint32_t* bits, hipStream_t s) {
    if (frames <= 0 || H <= 0) return hipSuccess;
    if (Wu < 1 || Wu > 4096 || ld < Wu || ld % 4 || frame_bytes % 4 || (reinterpret_cast<uintptr_t>(img) & 3u) ||
        frames > 65535)
        return hipErrorInvalidValue;
    const int WW = (Wu + 31) / 32;
    const int64_t lanes = (int64_t)H * WW * 8;   // a multiple of 8: the 8 lanes of a word share a wave
    hipLaunchKernelGGL(morph_pack_kernel, dim3((unsigned)((lanes + 255) / 256), (unsigned)frames), dim3(256), 0, s,
                       img, frame_bytes, ld, Wu, H, bits, WW);
    return hipGetLastError();
}

// bits (frames x H x WW words) -> img: frames x H rows at a stride of ld bytes (ld % 4 == 0, ld <= 32 WW), 255 at
// every set pixel, 0 elsewhere (the stride's pad columns too: their bits are zero). A lane writes 4 pixels.
__global__ __launch_bounds__(256) void morph_unpack_kernel(const uint32_t* __restrict__ bits, int H, int WW, int ld,
                                                           uint8_t* __restrict__ img) {
    const int frame = blockIdx.y;
    const int G = ld / 4;
    const int64_t idx = blockIdx.x * 256ll + threadIdx.x;
    const int64_t row = idx / G;
    if (row >= H) return;
    const int gq = (int)(idx - row * G);
    const uint32_t word = bits[((int64_t)frame * H + row) * WW + (gq >> 3)];
    const uint32_t nib = (word >> (4 * (gq & 7))) & 0xFu;
    // bit k of the nibble -> byte k = 0xFF
    const uint32_t px = ((nib * 0x00204081u) & 0x01010101u) * 0xFFu;
    *reinterpret_cast<uint32_t*>(img + ((int64_t)frame * H + row) * ld + 4 * gq) = px;
}

hipError_t launch_morph_unpack(const uint32_t* bits, int frames, int H, int Wu, int ld, uint8_t* img, hipStream_t s) {
    if (frames <= 0 || H <= 0) return hipSuccess;
    const int WW = (Wu + 31) / 32;
    if (Wu < 1 || Wu > 4096 || ld < Wu || ld % 4 || ld > 32 * WW || (reinterpret_cast<uintptr_t>(img) & 3u) ||
        frames > 65535)
        return hipErrorInvalidValue;
    const int64_t lanes = (int64_t)H * (ld / 4);
    hipLaunchKernelGGL(morph_unpack_kernel, dim3((unsigned)((lanes + 255) / 256), (unsigned)frames), dim3(256), 0, s,
                       bits, H, WW, ld, img);
    return hipGetLastError();
}

}  // namespace svx
