// Host-side launcher of kernels/result.hip: the result image (stereovision.py:181-209, functions.py:390-394,
// :424-431) from the BGR and the obstacle stage's outputs. (A header of its own, like svx_hull.h: svx_launch.h is
// part of the sources sv_source_id hashes.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svx.h"
#include "svx_result_host.h"   // kResultMaxH, kResultMaxW, kResultMaxCoord, kResultMaxVerts: the limits, defined once
                               // where the host checks read them

namespace svx {

// bgr, out: frames x H rows of ld3 = 3 * round_up(W, 8) bytes, frame f at + f * frame_bytes; out must not overlap
// bgr. obst: frames x H x ceil(W / 32) words (svx_morph.h's layout, pad bits zero). pts: frame f's n int32 (x, y)
// pairs at pts + f * pts_stride, a convex polygon in outline order (include/svx.h, sv_result_image); info[f]: n,
// centre, tip and the valid bits. Both buffers 8-byte aligned, frame_bytes % 8 == 0 (16 and 16 take the wide path
// when round_up(W, 8) is a multiple of 16). One workgroup per band of 64 rows of a frame.
hipError_t launch_result(const uint8_t* bgr, int64_t frame_bytes, int ld3, const uint32_t* obst, const int32_t* pts,
                         int64_t pts_stride, const sv_hull_info* info, int frames, int H, int W, uint8_t* out,
                         hipStream_t s);

}  // namespace svx
