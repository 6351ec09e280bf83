// Host-side launchers of kernels/jpeg.hip: the baseline JPEG stream of the MJPG recording (loop.py:49-54,82-89;
// DESIGN §7.11) of a run of BGR pictures on the device. (A header of its own, like svx_tile.h: svx_launch.h is part
// of the sources sv_source_id hashes.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svx.h"
#include "svx_jpeg_host.h"

namespace svx {

// The scratch of a chunk of frames (svx_jpeg_host.h, jpeg_work_layout).
struct JpegWork {
    int16_t* coef;    // frames x MCU rows x MCUs a row x 6 blocks x 64, zig-zag order
    uint2* lane;      // frames x MCU rows x 64: a lane's first bit | the next lane's first byte << 24, its first byte
    int32_t* ilen;    // frames x MCU rows: an interval's bytes, stuffed
    int32_t* ioff;    // ... and where they start in the frame's stream
};

// `frames` pictures of h x w (1 .. 4096), picture f at img + f * frame_stride, rows ld >= 3 w bytes apart, into
// out + f * cap: the stream of DESIGN §7.11 when it fits in cap bytes, and sizes[f] = its length; else nothing is
// written for that frame and sizes[f] = minus the length it needs. jc: the device copy of jpeg_build(h, w, quality).
// Three kernels and a scan, none of which waits for another workgroup: the transform (colour, 4:2:0, DCT, quantiser,
// zig-zag: int16 coefficients in MCU order), the size pass (a wave per restart interval: every lane's bits, the
// stuffed bytes), the scan of a frame's intervals, the write pass.
hipError_t launch_jpeg(const uint8_t* img, int64_t frame_stride, int ld, int h, int w, int frames, const JpegConst* jc,
                       const JpegWork& wk, uint8_t* out, int64_t cap, int32_t* sizes, hipStream_t s);

// offsets[0 .. frames]: the exclusive sums of max(sizes[f], 0); packed + offsets[f]: frame f's stream from its slot
// (overflowed frames contribute nothing).
hipError_t launch_jpeg_pack(const int32_t* sizes, int frames, const uint8_t* slots, int64_t cap, int64_t* offsets,
                            uint8_t* packed, hipStream_t s);

}  // namespace svx
