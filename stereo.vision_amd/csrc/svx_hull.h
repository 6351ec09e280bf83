// Host-side launchers of kernels/hull.hip: the obstacle stage (stereovision.py:170-189, functions.py:396-421) on
// bitmaps. (A header of its own, like svx_morph.h: svx_launch.h is part of the sources sv_source_id hashes.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svx.h"
#include "svx_device.h"
#include "svx_hull_host.h"   // kHullMaxH: the limit, defined once where the host checks read it

namespace svx {

constexpr int kHullMaxCoord = 16383;  // |x|, |y| of launch_min_circle's points: its 64-bit centre terms hold
constexpr int kCircleMaxPoints = 8192;   // points launch_min_circle takes: one lane, n distance tests an exchange

// What the glyph tip needs of a plane and the camera (functions.py:396-416); valid = 0: no plane.
struct HullPlane {
    double a, b, c, f, fB, cw, ch;
    uint32_t valid;
};

// cleaned: frames x H x WW words (svx_morph.h's bitmap layout, pad bits zero), 2 <= W <= 4096, 1 <= H <= kHullMaxH.
// Per frame (include/svx.h, sv_road_obstacles): pts = the hull's strict vertices as int32 (x, y) pairs, frame f's
// at pts + f * 4 * H (room for 2 H pairs); mask / obst (each nullable) = the filled hull and hull & ~cleaned, frames
// x H x WW words; info[f] = vertex count, circle centre, glyph tip and the valid bits.
// disp (nullable): the frames' u8 disparity, frame f at disp + f * disp_frame_bytes, rows at a stride of disp_ld.
// Frame f's plane is planes[f * plane_stride] when planes is not null, else `shared`.
// One workgroup per frame.
hipError_t launch_road_hull(const uint32_t* cleaned, int frames, int H, int W, const uint8_t* disp,
                            int64_t disp_frame_bytes, int disp_ld, const FramePlane* planes, int plane_stride,
                            const HullPlane& shared, int32_t* pts, uint32_t* mask, uint32_t* obst, sv_hull_info* info,
                            hipStream_t s);

// The exact minimum enclosing circle of 1 <= n <= kCircleMaxPoints int32 (x, y) pairs with |x|, |y| <=
// kHullMaxCoord, on one lane: out[0..1] = its centre truncated toward zero, out[2] = 1 (0 when the iteration found no
// circle).
hipError_t launch_min_circle(const int32_t* pts, int64_t n, int32_t* out, hipStream_t s);

}  // namespace svx
