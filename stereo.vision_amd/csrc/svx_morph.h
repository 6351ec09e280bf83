// Host-side launchers of kernels/morph.hip: sanitiseRoadImage's morphology (functions.py:346-358) on bitmaps.
// (A header of its own: svx_launch.h is part of the sources sv_source_id hashes for K1 and the resident pipeline,
// whose committed PMC profiles count only for a library built from the same sources.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svx {

// Bitmaps: rows of WW = ceil(W / 32) words, pixel x at bit x & 31 of word x >> 5 (PipeBuffers::rbits' layout), the
// last word's pad bits zero.
// in -> out (frames x H x WW words each): close 9 x 9, erode 17 x 17, AND mask (H x WW words; nullptr: all ones),
// close 9 x 9, with OpenCV's default borders (include/svx.h, sv_sanitise_road). 2 <= W <= 4096. One workgroup per
// band of rows of a frame.
hipError_t launch_morph_clean(const uint32_t* in, const uint32_t* mask, uint32_t* out, int frames, int H, int W,
                              hipStream_t s);
// u8 images (frame f at img + f * frame_bytes, rows of Wu pixels at a stride of ld bytes, ld % 4 == 0) -> bitmaps
// (non-zero = set), and back: 255 at every set pixel, 0 elsewhere, pad columns of the stride included.
hipError_t launch_morph_pack(const uint8_t* img, int64_t frame_bytes, int ld, int Wu, int H, int frames,
                             uint32_t* bits, hipStream_t s);
hipError_t launch_morph_unpack(const uint32_t* bits, int frames, int H, int Wu, int ld, uint8_t* img, hipStream_t s);

}  // namespace svx
