// Host-only part of the ground grid's runtime (rt_ground.hip): the argument checks of sv_ground_grid, the layout of
// its results and the mapping the kernel looks up. No HIP in here, so that tools/ground_host_check.cpp can run it
// under the host sanitizers without a device (by hand, on the development machine) and tests/test_ground_cpu.py can
// compare the mapping with the oracle's.
#pragma once
#include <cmath>
#include <stddef.h>
#include <stdint.h>

#include "../../include/svx.h"

namespace svx {

constexpr int kGroundMaxCells = 8192;   // two uint32 planes of the cells are 64 KB of LDS: two workgroups a CU
constexpr int kGroundMaxSlots = 1024;   // workgroups of a launch, each taking every slots-th frame

inline sv_grid ground_default_grid() { return sv_grid{-8.0, 0.0, 0.25, 64, 128}; }

// nullptr when the grid is in range, else what is wrong with it
inline const char* ground_check_grid(const sv_grid& g) {
    if (!std::isfinite(g.cell) || !(g.cell > 0)) return "cell finite and > 0";
    if (!std::isfinite(g.x0) || !std::isfinite(g.z0)) return "x0 and z0 finite";
    if (g.nx < 1 || g.nz < 1) return "nx >= 1, nz >= 1";
    if ((int64_t)g.nx * (int64_t)g.nz > kGroundMaxCells) return "nx * nz <= 8192";
    return nullptr;
}

inline const char* ground_check_camera(const sv_camera& c) {
    if (!std::isfinite(c.f) || !(c.f > 0) || !std::isfinite(c.B) || !(c.B > 0)) return "camera f and B finite and > 0";
    return nullptr;
}

inline const char* ground_check_shape(int H, int W) {
    if (H < 1 || H > 4096) return "1 <= H <= 4096";
    if (W < 2 || W > 4096) return "2 <= W <= 4096";
    return nullptr;
}

// nullptr when sv_ground_grid's arguments are in range (grid: the caller's, or null for the default)
inline const char* ground_check_args(const void* obstacles, const void* disp, int H, int W, const sv_camera* cam,
                                     const sv_grid* grid, int min_count, const void* obst, const void* nearest,
                                     const void* info) {
    if (!obstacles || !disp || !cam || !obst || !nearest || !info)
        return "null obstacle image, disparity, camera, obst, nearest or info";
    if (const char* why = ground_check_shape(H, W)) return why;
    if (grid)
        if (const char* why = ground_check_grid(*grid)) return why;
    if (min_count < 1) return "min_count >= 1";
    return ground_check_camera(*cam);
}

// A launch's results: every frame's two planes (obst then road, 2 nx nz words a frame), then every frame's nearest
// profile (nx words a frame, so all of them leave in one copy), then every frame's info (4 words). Offsets in words.
struct GroundLayout {
    size_t cells = 0;                       // nx nz
    size_t off_nearest = 0, off_info = 0;   // the planes at 0
    size_t bytes = 0;                       // frames x (2 nx nz + nx + 4) x 4
};

inline GroundLayout ground_layout(const sv_grid& g, int frames) {
    GroundLayout l;
    const size_t F = frames > 0 ? (size_t)frames : 0;
    l.cells = (size_t)g.nx * (size_t)g.nz;
    l.off_nearest = 2 * l.cells * F;
    l.off_info = l.off_nearest + (size_t)g.nx * F;
    l.bytes = sizeof(uint32_t) * (l.off_info + 4 * F);
    return l;
}

// The mapping is the full table: ix[d * W + x] for every disparity value d and pixel column x, and iz[d], each the
// cell index or -1 outside the grid (row d = 0 is all -1: no depth). Every value is computed on its own in float64 in
// the reference's order, so the table is the semantics' own statement with nothing derived from monotonicity; the
// kernel's look-up is one 2-byte load a pixel at an address that rises with x inside a run of equal d; and its size
// follows from W alone (512 KB at W = 1024, 2 MB at 4096: L2-resident), where the per-d thresholds (256 x (nx + 1))
// grow with the grid to 4 MB at nx = 8192 and need a search at every run start. The device holds the two folded into
// one table of the same size, cell[d * W + x] = iz[d] * nx + ix[d * W + x] (< 8192), or -1 where either is -1.
inline size_t ground_map_bytes(int W) { return sizeof(int16_t) * 256 * (size_t)W; }   // the cell table

inline int16_t ground_index(double v, double origin, double cell, int n) {
    const double q = std::floor((v - origin) / cell);
    return (q >= 0.0 && q < (double)n) ? (int16_t)q : (int16_t)-1;   // compared as doubles; a NaN is outside
}

// ix: 256 x W entries, iz: 256 entries. false (nothing written) for arguments out of range.
inline bool ground_fill_mapping(const sv_camera& cam, const sv_grid& g, int W, int16_t* ix, int16_t* iz) {
    if (!ix || !iz || W < 2 || W > 4096 || ground_check_grid(g) || ground_check_camera(cam)) return false;
    iz[0] = -1;
    for (int x = 0; x < W; ++x) ix[x] = -1;
    const double fb = cam.f * cam.B;
    for (int d = 1; d < 256; ++d) {
        const double Z = fb / (double)d;
        iz[d] = ground_index(Z, g.z0, g.cell, g.nz);
        int16_t* row = ix + (size_t)d * W;
        for (int x = 0; x < W; ++x) {
            const double X = (((double)x - cam.cw) * Z) / cam.f;
            row[x] = ground_index(X, g.x0, g.cell, g.nx);
        }
    }
    return true;
}

// cell: 256 x W entries from ground_fill_mapping's ix and iz of a grid of nx columns
inline void ground_fold_cells(const int16_t* ix, const int16_t* iz, int W, int nx, int16_t* cell) {
    for (int d = 0; d < 256; ++d)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)d * W + x;
            cell[i] = (iz[d] < 0 || ix[i] < 0) ? (int16_t)-1 : (int16_t)((int)iz[d] * nx + (int)ix[i]);
        }
}

}  // namespace svx
