// Host-side launcher of kernels/tile.hip: batchImages' five-picture tile (functions.py:452-499 as stereovision.py:216
// calls it) from the disparity, the BGR, the road picture, the cleaned road picture and the result image. (A header
// of its own, like svx_result.h: svx_launch.h is part of the sources sv_source_id hashes.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svx.h"
#include "svx_tile_host.h"   // kTileMaxH, kTileMaxW: the limits, defined once where the host checks read them

namespace svx {

// A picture of `frames` frames: frame f at + f * frame (bytes for a u8 picture, words for a bitmap), its rows ld
// apart (bytes or words).
struct TilePlane {
    const void* p;
    int64_t frame;
    int ld;
};

// The five pictures of H x W (multiples of 4, 4 .. 4096). disp: u8, ld >= W; bgr, res: 3 bytes a pixel, ld >= 3 W.
// The road picture and the cleaned one come as u8 (road, clean: ld >= W; the map quadrant paints where road != 0,
// the two quadrants average the bytes as they are) or, when the bitmap's pointer is set, as bitmaps in svx_morph.h's
// layout (rbits, cbits: ld >= ceil(W / 32) words, pad bits zero; a set bit is a pixel of 255), which give the same
// bytes for pictures of 0 and 255.
struct TileArgs {
    TilePlane disp, bgr, road, clean, rbits, cbits, res;
    int H, W;
};

// out: frames x H / 2 rows of 3 W bytes, packed (frame f at + f * 3 W H / 2), overlapping no input. One wave per
// output row. With W % 16 == 0, every u8 pointer, frame stride and row stride a multiple of 16 and out a multiple of
// 8, a lane takes 16 source pixels of every picture from 16-byte loads; other shapes take an output pixel per lane.
hipError_t launch_tile(const TileArgs& a, int frames, uint8_t* out, hipStream_t s);

}  // namespace svx
