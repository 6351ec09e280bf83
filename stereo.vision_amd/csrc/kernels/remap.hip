// Remap of 8-bit pictures through OpenCV's fixed-point map pair (gfx950): cv2.remap's INTER_LINEAR path with
// BORDER_CONSTANT 0 as tests/rectify_numpy.py restates it (remap), for the stereo rectification. Per
// destination pixel the map gives the source position (sx, sy) and the fraction fy * 32 + fx; per channel, in int32:
//   S(i, j) = src[sy + j][sx + i] inside the source, else 0
//   out = (w00 S(0,0) + w10 S(1,0) + w01 S(0,1) + w11 S(1,1) + 16384) >> 15
//   w00 = 32 (32 - fx)(32 - fy), w10 = 32 fx (32 - fy), w01 = 32 (32 - fx) fy, w11 = 32 fx fy     (their sum is 32768)
// so nothing saturates: the sum is at most 255 * 32768 + 16384.
//
// The destination is walked as one run of dh * dw pixels: a workgroup takes 256 * PX neighbouring pixels of one eye
// and up to kFramesPerBlock pictures of the stack, one after the other. A lane reads the map entries of its PX pixels
// once and keeps the offset of tap (0, 0), the four weights and the four in-bounds bits in registers for all of its
// pictures: the map (6 bytes a pixel against 6 or 2 moved per picture) is read once per workgroup, not per picture.
//  - PX = 1: a pixel per lane, byte stores. Every shape.
//  - PX = 4: four pixels per lane: the map entries from a 16- and an 8-byte load, the pixels stored as 4 bytes (grey)
//    or 12 (BGR). dw % 4 == 0 (svx_rectify.h), so the four lie in one row and every store is 4-byte aligned.
// The taps are gathered by bytes. A tap outside the source is 0 and no load is issued for it: a lane with a pixel
// that has one takes the guarded form for its four pixels, the others the plain one (in a real rectification that is
// the waves along the border). Both index from tap (0, 0)'s address, the picture's base plus a signed 32-bit offset:
// the other taps are a constant or a row away, so a lane carries one offset a pixel round the loop and not twelve.
// No array is indexed by a variable: every index is a constant after unrolling. No LDS.
#include "../svx_rectify.h"

namespace svx {

namespace {

constexpr int kFramesPerBlock = 64;   // pictures a workgroup walks with its map entries in registers

// px holds B | G << 8 | R << 16, or the grey byte
template <int PX, int C>
__device__ __forceinline__ void store_px(uint8_t* o, const uint32_t (&px)[PX]) {
    if constexpr (PX == 4 && C == 1) {
        *reinterpret_cast<uint32_t*>(o) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    } else if constexpr (PX == 4) {
        *reinterpret_cast<uint3*>(o) =
            make_uint3(px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8));
    } else if constexpr (C == 1) {
        o[0] = (uint8_t)px[0];
    } else {
        o[0] = (uint8_t)px[0], o[1] = (uint8_t)(px[0] >> 8), o[2] = (uint8_t)(px[0] >> 16);
    }
}

// the weights are at most 32768 and a sample 255: the 24-bit multiply-add gives the int32 sum
__device__ __forceinline__ uint32_t blend(uint32_t s00, uint32_t s10, uint32_t s01, uint32_t s11, uint32_t w00,
                                          uint32_t w10, uint32_t w01, uint32_t w11) {
    return (__umul24(w00, s00) + __umul24(w10, s10) + __umul24(w01, s01) + __umul24(w11, s11) + 16384u) >> 15;
}

template <int PX, int C>
__global__ __launch_bounds__(256) void remap_kernel(const RemapArgs a, int strips) {
    static_assert((PX == 1 || PX == 4) && (C == 1 || C == 3), "instances");
    const int eye = blockIdx.x >= (unsigned)strips ? 1 : 0;   // uniform
    const uint32_t strip = blockIdx.x - (unsigned)(eye * strips);
    const uint32_t npx = (uint32_t)a.dh * (uint32_t)a.dw;     // at most 2^26
    const uint32_t q0 = (strip * 256u + threadIdx.x) * PX;
    if (q0 >= npx) return;                                    // PX = 4: npx % 4 == 0, so q0 + 3 < npx too
    const uint8_t* __restrict__ src = eye ? a.src[1] : a.src[0];
    uint8_t* __restrict__ dst = eye ? a.dst[1] : a.dst[0];
    const int16_t* xy = eye ? a.xy[1] : a.xy[0];
    const uint16_t* frac = eye ? a.frac[1] : a.frac[0];
    // the lane's map entries, read once: (sx, sy) as the halves of a word, the fraction as a half-word
    uint32_t exy[PX], efr[PX];
    if constexpr (PX == 4) {
        const uint4 u = *reinterpret_cast<const uint4*>(xy + 2 * (size_t)q0);
        const uint2 v = *reinterpret_cast<const uint2*>(frac + q0);
        exy[0] = u.x, exy[1] = u.y, exy[2] = u.z, exy[3] = u.w;
        efr[0] = v.x & 0xFFFFu, efr[1] = v.x >> 16, efr[2] = v.y & 0xFFFFu, efr[3] = v.y >> 16;
    } else {
        exy[0] = *reinterpret_cast<const uint32_t*>(xy + 2 * (size_t)q0);
        efr[0] = frac[q0];
    }
    const uint32_t row = (uint32_t)a.sw * C;   // bytes of a source row: at most 24576
    int32_t o0[PX];
    uint32_t w00[PX], w10[PX], w01[PX], w11[PX], in[PX];
    uint32_t all_in = 15u;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const int sx = (int)(int16_t)(exy[j] & 0xFFFFu), sy = (int)exy[j] >> 16;
        const uint32_t fx = efr[j] & 31u, fy = (efr[j] >> 5) & 31u;
        w00[j] = 32u * (32u - fx) * (32u - fy), w10[j] = 32u * fx * (32u - fy);
        w01[j] = 32u * (32u - fx) * fy, w11[j] = 32u * fx * fy;
        const bool x0 = (uint32_t)sx < (uint32_t)a.sw, x1 = (uint32_t)(sx + 1) < (uint32_t)a.sw;
        const bool y0 = (uint32_t)sy < (uint32_t)a.sh, y1 = (uint32_t)(sy + 1) < (uint32_t)a.sh;
        in[j] = (x0 && y0 ? 1u : 0u) | (x1 && y0 ? 2u : 0u) | (x0 && y1 ? 4u : 0u) | (x1 && y1 ? 8u : 0u);
        all_in &= in[j];
        // |sy * sw + sx| * 3 < 2^30: no overflow; negative where tap (0, 0) lies before the picture's first byte
        o0[j] = (sy * a.sw + sx) * C;
    }
    const int64_t sframe = (int64_t)a.sh * a.sw * C, dframe = (int64_t)npx * C;
    const int f0 = blockIdx.y * kFramesPerBlock, f1 = min(a.n, f0 + kFramesPerBlock);
    const uint32_t oq = q0 * C;
    for (int f = f0; f < f1; ++f) {
        // the picture's bases through readfirstlane: scalar, and made anew each time round, so that every load is
        // that base plus a lane's 32-bit offset. As pointers stepped from picture to picture, each of the 48 taps
        // got a 64-bit address of its own to carry round the loop (190 VGPRs, two waves a SIMD, in a build of that
        // form that is not kept). This steers one compiler's address selection and changes no result: after a ROCm
        // upgrade look at the kernel's VGPR count again (DESIGN §7.15's table) before trusting it.
        const int64_t fu = __builtin_amdgcn_readfirstlane(f);
        const uint8_t* __restrict__ p = src + fu * sframe;
        uint8_t* __restrict__ o = dst + fu * dframe + oq;
        uint32_t px[PX];
        if (all_in == 15u) {
            // every pixel's samples are requested before the first is used: one round trip a picture, not one a pixel
            uint32_t s0[PX][2 * C], s1[PX][2 * C];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                const uint8_t* t0 = p + o0[j];
                const uint8_t* t1 = t0 + row;
#pragma unroll
                for (int k = 0; k < 2 * C; ++k) s0[j][k] = t0[k], s1[j][k] = t1[k];
            }
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                uint32_t v = 0;
#pragma unroll
                for (int ch = 0; ch < C; ++ch)
                    v |= blend(s0[j][ch], s0[j][C + ch], s1[j][ch], s1[j][C + ch], w00[j], w10[j], w01[j], w11[j])
                         << (8 * ch);
                px[j] = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                // tap (0, 0)'s address is formed, not read, where that tap lies outside the picture: up to 8e8 bytes
                // either side of it, so formally pointer arithmetic outside the allocation. On this target a global
                // pointer is a flat 64-bit number and the sum cannot wrap; only taps whose bit is set are read.
                const uint8_t* t0 = p + o0[j];
                const uint8_t* t1 = t0 + row;
                uint32_t v = 0;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    uint32_t s00 = 0, s10 = 0, s01 = 0, s11 = 0;
                    if (in[j] & 1u) s00 = t0[ch];
                    if (in[j] & 2u) s10 = t0[C + ch];
                    if (in[j] & 4u) s01 = t1[ch];
                    if (in[j] & 8u) s11 = t1[C + ch];
                    v |= blend(s00, s10, s01, s11, w00[j], w10[j], w01[j], w11[j]) << (8 * ch);
                }
                px[j] = v;
            }
        }
        store_px<PX, C>(o, px);
    }
}

template <int PX, int C>
void launch_instance(const RemapArgs& a, int strips, dim3 grid, hipStream_t s) {
    hipLaunchKernelGGL((remap_kernel<PX, C>), grid, dim3(256), 0, s, a, strips);
}

}  // namespace

hipError_t launch_remap(const RemapArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.eyes < 1 || a.eyes > 2 || (a.channels != 1 && a.channels != 3)) return hipErrorInvalidValue;
    if (a.sh < 1 || a.sh > kRemapMaxDim || a.sw < 1 || a.sw > kRemapMaxDim || remap_check_dst(a.dh, a.dw))
        return hipErrorInvalidValue;
    bool quad = a.dw % 4 == 0 && a.dw >= kRemapQuadMin;
    for (int e = 0; e < a.eyes; ++e) {
        if (!a.src[e] || !a.dst[e] || !a.xy[e] || !a.frac[e]) return hipErrorInvalidValue;
        if (reinterpret_cast<uintptr_t>(a.xy[e]) & 3u || reinterpret_cast<uintptr_t>(a.frac[e]) & 1u)
            return hipErrorInvalidValue;
        quad = quad && (reinterpret_cast<uintptr_t>(a.xy[e]) & 15u) == 0 &&
               (reinterpret_cast<uintptr_t>(a.frac[e]) & 7u) == 0 && (reinterpret_cast<uintptr_t>(a.dst[e]) & 3u) == 0;
    }
    const int64_t npx = (int64_t)a.dh * a.dw;
    const int per_block = 256 * (quad ? 4 : 1);
    const int strips = (int)((npx + per_block - 1) / per_block);
    const int chunks = (a.n + kFramesPerBlock - 1) / kFramesPerBlock;
    if (chunks > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(strips * a.eyes), (unsigned)chunks);
    if (quad) {
        if (a.channels == 3) launch_instance<4, 3>(a, strips, grid, s);
        else launch_instance<4, 1>(a, strips, grid, s);
    } else {
        if (a.channels == 3) launch_instance<1, 3>(a, strips, grid, s);
        else launch_instance<1, 1>(a, strips, grid, s);
    }
    return hipGetLastError();
}

}  // namespace svx
