// Host-side launcher of kernels/resize.hip: cv2.resize's 8-bit INTER_LINEAR path at any scale, from the coefficient
// tables of svx_resize_host.h. (A header of its own, like svx_tile.h: svx_launch.h is part of the sources
// sv_source_id hashes.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svx.h"
#include "svx_resize_host.h"   // kResizeMaxSrc, kResizeMaxDst, ResizeTableLayout

namespace svx {

// n images of sh x sw, sc (1 or 3) bytes a pixel: image f at src + f * src_frame, its rows src_ld bytes apart; n
// images of dh x dw, dc bytes a pixel: image f's first pixel at dst + dst_off + f * dst_frame, its rows dst_ld apart,
// so that a destination can be a quadrant of a stack or a half of a tile. dc >= sc; a 1-channel source into a
// 3-channel destination repeats the byte (COLOR_GRAY2BGR). tables: a device block laid out by
// resize_table_layout(dh, dw) and filled by resize_fill_tables(.., sh, sw, dh, dw): the kernel reads every source
// index from it and checks none.
struct ResizeArgs {
    const uint8_t* src;
    int64_t src_frame;
    int src_ld, sh, sw, sc;
    uint8_t* dst;
    int64_t dst_off, dst_frame;
    int dst_ld, dh, dw, dc;
    const uint8_t* tables;
    const uint8_t* src_end;   // set by the launcher: one past the last source byte of the n images
};

// One wave per four output rows, lanes along the row. With dw % 4 == 0, dw >= kResizeQuadMin and the destination's
// first pixel, row stride and frame stride multiples of 4 bytes a lane makes four output pixels and stores them as
// 4 or 12 bytes; other shapes take an output pixel per lane and store bytes. A four-pixel lane of a grey source
// whose first pixel, row stride and frame stride are multiples of 4 bytes, at a scale sw / dw of at most
// kResizeWindowScale, reads its samples of a source row as one 16-byte window instead of eight bytes.
constexpr int kResizeQuadMin = 128;
constexpr int kResizeWindowScale = 3;
hipError_t launch_resize_linear(const ResizeArgs& a, int n, hipStream_t s);

}  // namespace svx
