// Host-side launcher of kernels/ground.hip: the ground grid (include/svx.h, sv_ground_grid) of packed obstacle and
// road bitmaps. (A header of its own, like svx_objects.h: svx_launch.h is part of the sources sv_source_id hashes.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svx.h"
#include "svx_ground_host.h"

namespace svx {

// obits, cbits (nullable): frames x H x WW words (svx_morph.h's bitmap layout; pad bits are ignored), 2 <= W <= 4096,
// 1 <= H <= 4096. disp: the frames' u8 disparity, frame f at disp + f * disp_frame_bytes, rows at a stride of disp_ld;
// disp, disp_frame_bytes and disp_ld are multiples of 8 and disp_ld >= W (a bitmap word's bytes are read 8 at a time,
// never past the row's stride). map_cell: 256 x W int16 (ground_fold_cells for this W and grid). nx, nz: the
// grid's, nx nz <= kGroundMaxCells. out: ground_layout(grid, frames).bytes, 16-byte aligned: frames x 2 nx nz words (frame f's
// obst plane, then its road plane), then nearest, frames x nx, then info, frames x 4. At most kGroundMaxSlots workgroups, each taking every
// slots-th frame; 8 nx nz bytes of LDS a workgroup.
hipError_t launch_ground_grid(const uint32_t* obits, const uint32_t* cbits, int frames, int H, int W,
                              const uint8_t* disp, int64_t disp_frame_bytes, int disp_ld, const int16_t* map_cell,
                              int nx, int nz, int min_count, uint32_t* out, hipStream_t s);

}  // namespace svx
