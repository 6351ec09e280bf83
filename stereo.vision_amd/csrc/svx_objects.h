// Host-side launcher of kernels/objects.hip: the obstacle list (include/svx.h, sv_obstacle_list) of packed obstacle
// bitmaps. (A header of its own, like svx_hull.h: svx_launch.h is part of the sources sv_source_id hashes.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svx.h"
#include "svx_objects_host.h"

namespace svx {

// bits: frames x H x WW words (svx_morph.h's bitmap layout; pad bits are ignored), 2 <= W <= 4096, 1 <= H <= 4096.
// disp (nullable): the frames' u8 disparity, frame f at disp + f * disp_frame_bytes, rows at a stride of disp_ld.
// scratch: objects_layout(H, W, frames).bytes, 4-byte aligned; nothing in it need be initialised.
// out: frames x cap entries, frame f's list at out + f * cap, its first min(n[f], cap) entries written;
// n[f] = the frame's components of at least min_area pixels. 1 <= cap <= kObjMaxCap, min_area >= 1.
// objects_layout's `slots` workgroups, each taking every slots-th frame.
hipError_t launch_obstacle_list(const uint32_t* bits, int frames, int H, int W, const uint8_t* disp,
                                int64_t disp_frame_bytes, int disp_ld, int min_area, int cap, void* scratch,
                                sv_obstacle* out, int32_t* n, hipStream_t s);

}  // namespace svx
