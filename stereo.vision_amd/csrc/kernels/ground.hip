// The ground grid (gfx950): the obstacle bitmap and the cleaned road bitmap of a frame laid out on the ground plane,
// a count a cell each, the nearest occupied row of every column and four totals (include/svx.h, sv_ground_grid).
// Integers only: where a pixel (d, x) lands is looked up in the host-made mapping (svx_ground_host.h:
// cell[d * W + x] = iz * nx + ix, -1 outside the grid). Bitmaps have morph.hip's layout: rows of WW = ceil(W / 32)
// words, pixel x at bit x & 31 of word x >> 5; the last word's pad bits are masked off as it is read, as objects.hip
// does.
//
//  * ground_grid_kernel — a workgroup of kGroundThreads takes a frame, then the frame a grid further on. The frame's
//    two planes of nx nz uint32 counts (obst, then road) live in LDS: cleared, filled by LDS atomic adds, and written
//    out whole with 16-byte stores (8-byte ones for an odd number of cells), so no cell is touched in memory twice and
//    nothing but the outputs is written. A thread takes every kGroundThreads-th bitmap word: it reads the obstacle
//    word and the cleaned word and goes on when both are zero without touching the disparity; else it reads the
//    word's 32 disparity bytes 8 at a time, all four loads in flight (a group of 8 without a set bit reads the
//    word's first group again, so nothing is read past the row's stride), then a group's eight cells, all eight
//    look-ups in flight (the walk is bound by the latency of these dependent loads, not by their bytes), and walks
//    the group's set bits in registers.
//    Neighbouring pixels of a row very often share (classes, cell) — the disparity is piecewise constant and a cell
//    spans many columns — so a run of equal (classes, cell) inside the word becomes one atomic add a plane, not one
//    a pixel. After a barrier a lane per column walks its cells upward for `nearest`, the four totals are summed
//    over the wave by DPP (svx_wave.h) and over the waves through LDS behind the planes.
#include "../svx_ground.h"
#include "../svx_wave.h"

namespace svx {

constexpr int kGroundThreads = 512;   // eight waves: at two workgroups a CU (64 KB of planes each) four waves a SIMD
constexpr int kGroundWaves = kGroundThreads / 64;

__global__ __launch_bounds__(kGroundThreads) void ground_grid_kernel(
    const uint32_t* __restrict__ obits, const uint32_t* __restrict__ cbits, int frames, int H, int W,
    const uint8_t* __restrict__ disp, int64_t disp_frame_bytes, int disp_ld, const int16_t* __restrict__ map_cell,
    int nx, int nz, int min_count, uint32_t* __restrict__ out) {
    // the two planes (2 nx nz words, rounded up to 16 bytes), then kGroundWaves x 4 totals (all LDS dynamic, so the
    // base stays 16-byte aligned)
    extern __shared__ __align__(16) uint32_t gr_lds[];
    const int tid = threadIdx.x;
    const int WW = (W + 31) >> 5, ncell = nx * nz, nw = H * WW;
    const int plane_words = (2 * ncell + 3) & ~3;
    uint32_t* part = gr_lds + plane_words;
    const int step_y = kGroundThreads / WW, step_w = kGroundThreads - step_y * WW;

    for (int64_t f = blockIdx.x; f < frames; f += gridDim.x) {
        for (int i = tid; i < plane_words / 4; i += kGroundThreads)
            reinterpret_cast<uint4*>(gr_lds)[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();

        const uint32_t* osrc = obits + f * nw;
        const uint32_t* csrc = cbits ? cbits + f * nw : nullptr;
        const uint8_t* dfr = disp + f * disp_frame_bytes;
        // obstacle pixels in the grid, with d > 0 outside it, with d == 0; road pixels in the grid
        int n_in = 0, n_out = 0, n_zero = 0, n_road = 0;
        // word i = tid + k kGroundThreads is word w of row y, stepped without a division
        int y = tid / WW, w = tid - y * WW;
        for (int i = tid; i < nw; i += kGroundThreads, y += step_y, w += step_w) {
            if (w >= WW) {
                w -= WW;
                ++y;
            }
            uint32_t o = osrc[i], c = csrc ? csrc[i] : 0u;
            if (w == WW - 1) {
                const uint32_t tail = (W & 31) ? (1u << (W & 31)) - 1u : 0xFFFFFFFFu;
                o &= tail;
                c &= tail;
            }
            const uint32_t m = o | c;
            if (!m) continue;
            const int xw = 32 * w;
            const uint8_t* row = dfr + (int64_t)y * disp_ld + xw;
            uint64_t q[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)   // a set bit lies inside the frame, so its group lies inside the row's stride;
                                          // a group without one reads the word's first group again (selects, no branch)
                q[g] = *reinterpret_cast<const uint64_t*>(row + (((m >> (8 * g)) & 0xFFu) ? 8 * g : 0));
            int run_key = -1, run_n = 0;   // classes << 13 | cell: bit 13 obstacle, bit 14 road
            const auto flush = [&]() {
                if (run_n) {
                    if (run_key & (1 << 13)) atomicAdd(&gr_lds[run_key & 8191], (uint32_t)run_n);
                    if (run_key & (1 << 14)) atomicAdd(&gr_lds[ncell + (run_key & 8191)], (uint32_t)run_n);
                }
            };
#pragma unroll 1
            for (int g = 0; g < 4; ++g) {   // (one copy of the body: unrolled four times it runs out of SGPRs)
                const uint32_t mg = (m >> (8 * g)) & 0xFFu;
                if (!mg) continue;
                const uint64_t qg = g < 2 ? (g == 0 ? q[0] : q[1]) : (g == 2 ? q[2] : q[3]);
                const uint32_t og = (o >> (8 * g)) & 0xFFu, cg = (c >> (8 * g)) & 0xFFu;
                const int x0 = xw + 8 * g;
                uint64_t lo = 0, hi = 0;   // the group's eight cells as int16s, four a register pair
                uint32_t live = 0;         // the group's set pixels with d > 0
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const int d = (int)((qg >> (8 * p)) & 0xFFu);
                    const bool on = ((mg >> p) & 1u) && d;
                    live |= (uint32_t)on << p;
                    const uint64_t v = (uint16_t)map_cell[on ? d * W + x0 + p : 0];   // (entry 0 for the others)
                    if (p < 4)
                        lo |= v << (16 * p);
                    else
                        hi |= v << (16 * (p - 4));
                }
                n_zero += __builtin_popcount(og & ~live);
                while (live) {
                    const int p = __builtin_ctz(live);
                    live &= live - 1u;
                    const int cell = (int)(int16_t)((p < 4 ? lo : hi) >> (16 * (p & 3)));
                    const int ob = (int)((og >> p) & 1u), cb = (int)((cg >> p) & 1u);
                    if (cell < 0) {
                        n_out += ob;
                        continue;
                    }
                    n_in += ob;
                    n_road += cb;
                    const int key = cell | (ob << 13) | (cb << 14);
                    if (key != run_key) {
                        flush();
                        run_key = key;
                        run_n = 0;
                    }
                    ++run_n;
                }
            }
            flush();
        }
        // the totals: over the wave (every lane is active here), then lane 63's of the waves
        const auto add = [](int a, int b) { return a + b; };
        wave_scan2(n_in, n_out, 0, add);
        wave_scan2(n_zero, n_road, 0, add);
        if ((tid & 63) == 63) {
            uint32_t* p = part + 4 * (tid >> 6);
            p[0] = (uint32_t)n_in;
            p[1] = (uint32_t)n_out;
            p[2] = (uint32_t)n_zero;
            p[3] = (uint32_t)n_road;
        }
        __syncthreads();

        // GroundLayout: every frame's planes, then every frame's nearest, then every frame's info
        uint32_t* dst = out + f * 2 * ncell;   // 8 ncell bytes a frame: 16-byte aligned when ncell is even
        int32_t* nearest = reinterpret_cast<int32_t*>(out) + (int64_t)frames * 2 * ncell + f * nx;
        int32_t* info = reinterpret_cast<int32_t*>(out) + (int64_t)frames * (2 * ncell + nx) + f * 4;
        if (!(ncell & 1)) {
            for (int i = tid; i < ncell / 2; i += kGroundThreads)
                reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(gr_lds)[i];
        } else {
            for (int i = tid; i < ncell; i += kGroundThreads)
                reinterpret_cast<uint2*>(dst)[i] = reinterpret_cast<const uint2*>(gr_lds)[i];
        }
        for (int ix = tid; ix < nx; ix += kGroundThreads) {
            int first = -1;
            for (int iz = 0; iz < nz; ++iz)
                if (gr_lds[iz * nx + ix] >= (uint32_t)min_count) {
                    first = iz;
                    break;
                }
            nearest[ix] = first;
        }
        if (tid < 4) {
            uint32_t t = 0;
            for (int k = 0; k < kGroundWaves; ++k) t += part[4 * k + tid];
            info[tid] = (int32_t)t;
        }
        __syncthreads();   // the planes and the totals are the next frame's
    }
}

hipError_t launch_ground_grid(const uint32_t* obits, const uint32_t* cbits, int frames, int H, int W,
                              const uint8_t* disp, int64_t disp_frame_bytes, int disp_ld, const int16_t* map_cell,
                              int nx, int nz, int min_count, uint32_t* out, hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    if (!obits || !disp || !map_cell || !out || H < 1 || H > 4096 || W < 2 || W > 4096 ||
        nx < 1 || nz < 1 || (int64_t)nx * nz > kGroundMaxCells || min_count < 1 || disp_ld < W || (disp_ld & 7) ||
        (disp_frame_bytes & 7) || (reinterpret_cast<uintptr_t>(disp) & 7) ||
        (reinterpret_cast<uintptr_t>(out) & 15))
        return hipErrorInvalidValue;
    const size_t lds = sizeof(uint32_t) * (size_t)(((2 * nx * nz + 3) & ~3) + 4 * kGroundWaves);
    if (lds > 64 * 1024) {   // dynamic LDS above 64 KiB needs the per-kernel opt-in (on the current device)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ground_grid_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const int slots = frames < kGroundMaxSlots ? frames : kGroundMaxSlots;
    hipLaunchKernelGGL(ground_grid_kernel, dim3((unsigned)slots), dim3(kGroundThreads), lds, s, obits, cbits, frames,
                       H, W, disp, disp_frame_bytes, disp_ld, map_cell, nx, nz, min_count, out);
    return hipGetLastError();
}

}  // namespace svx
