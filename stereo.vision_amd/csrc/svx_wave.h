// Wave64 primitives of the SGBM and batched-RANSAC kernels (gfx950): the LDS hand-off point, DPP moves, readlane
// and the six-step DPP scan, for 32- and 64-bit values. Every lane must be active in the DPP forms.
// (svx_device.h's wave_scan_dpp / wave_sum remain a second spelling of the u32 ladder: that header is hashed into
// sv_source_id, so it folds in here the next time those sources change for a measured reason.)
#pragma once
#include <stdint.h>

namespace svx {

// A wave's lanes hand data to each other through LDS with no workgroup
// barrier. The hardware keeps one wave's LDS operations in order, but the
// compiler reasons per lane (lane i's store to mt[j] never aliases lane i's
// load of mt[j - 35]) and may move loads above earlier stores: every hand-off
// between lanes goes through this point (a compiler memory barrier + LDS wait).
__device__ __forceinline__ void wave_lds_sync() { __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// One DPP move (control CTL, row mask RM): a lane whose source is outside its row, the wave or the row mask reads
// `identity`. A 64-bit value moves as two halves under the same control. One VALU op a half, no LDS round trip.
template <int CTL, int RM = 0xf, class T>
__device__ __forceinline__ T dpp_move(T v, T identity) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32- and 64-bit values");
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, identity),
                                                                 __builtin_bit_cast(int, v), CTL, RM, 0xf, false));
    } else {
        const uint64_t u = __builtin_bit_cast(uint64_t, v), id = __builtin_bit_cast(uint64_t, identity);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)id, (int)(uint32_t)u, CTL, RM, 0xf, false);
        const uint32_t hi =
            (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(id >> 32), (int)(uint32_t)(u >> 32), CTL, RM, 0xf, false);
        return __builtin_bit_cast(T, (uint64_t)hi << 32 | lo);
    }
}

// Lane `src`'s value read by every lane (src uniform across the wave: a scalar read).
template <class T>
__device__ __forceinline__ T wave_readlane(T v, int src) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32- and 64-bit values");
    if constexpr (sizeof(T) == 4) {
        return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
    } else {
        const uint64_t u = __builtin_bit_cast(uint64_t, v);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, src);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), src);
        return __builtin_bit_cast(T, (uint64_t)hi << 32 | lo);
    }
}

// Inclusive scan over the wave under op (identity as given): row_shr 1/2/4/8, then row_bcast 15 and 31; lane 63
// ends with the wave's total. wave_scan2 runs two chains interleaved, so each step's input was written two
// instructions earlier.
template <int CTL, int RM, class T, class Op>
__device__ __forceinline__ void wave_scan_step(T& v, T identity, Op op) {
    v = op(v, dpp_move<CTL, RM>(v, identity));
}
template <class T, class Op>
__device__ __forceinline__ T wave_scan(T v, T identity, Op op) {
    wave_scan_step<0x111, 0xf>(v, identity, op);   // row_shr:1
    wave_scan_step<0x112, 0xf>(v, identity, op);   // row_shr:2
    wave_scan_step<0x114, 0xf>(v, identity, op);   // row_shr:4
    wave_scan_step<0x118, 0xf>(v, identity, op);   // row_shr:8
    wave_scan_step<0x142, 0xa>(v, identity, op);   // row_bcast:15
    wave_scan_step<0x143, 0xc>(v, identity, op);   // row_bcast:31
    return v;
}
template <class T, class Op>
__device__ __forceinline__ void wave_scan2(T& a, T& b, T identity, Op op) {
    wave_scan_step<0x111, 0xf>(a, identity, op), wave_scan_step<0x111, 0xf>(b, identity, op);
    wave_scan_step<0x112, 0xf>(a, identity, op), wave_scan_step<0x112, 0xf>(b, identity, op);
    wave_scan_step<0x114, 0xf>(a, identity, op), wave_scan_step<0x114, 0xf>(b, identity, op);
    wave_scan_step<0x118, 0xf>(a, identity, op), wave_scan_step<0x118, 0xf>(b, identity, op);
    wave_scan_step<0x142, 0xa>(a, identity, op), wave_scan_step<0x142, 0xa>(b, identity, op);
    wave_scan_step<0x143, 0xc>(a, identity, op), wave_scan_step<0x143, 0xc>(b, identity, op);
}

}  // namespace svx
