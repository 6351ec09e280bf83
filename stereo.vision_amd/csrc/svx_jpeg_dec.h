// Host-side launcher of kernels/jpeg_dec.hip: the baseline JPEG decoder of the MJPG playback, from
// packed streams on the device to BGR pictures on the device. (A header of its own, like svx_jpeg.h: svx_launch.h is
// part of the sources sv_source_id hashes.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svx.h"
// the interval walk of svx_jpeg_dec_host.h runs on the host (tools/jpeg_decode_host_check.cpp) and in the kernel
#define SVX_JPEG_HD __host__ __device__
#include "svx_jpeg_dec_host.h"

namespace svx {

// The scratch of a chunk of frames (svx_jpeg_dec_host.h, jpeg_dec_work_layout).
struct JpegDecWork {
    int16_t* coef;     // frames x MCUs x 6 blocks x 64, zig-zag order, quantised (the encoder's layout)
    uint8_t* chroma;   // frames x {Cb, Cr} x 8 MCU rows x 8 MCUs a row: the chroma samples of the padded picture
    int32_t* first;    // frames x maxi: an interval's first byte in its stream (first[0] < 0: the RSTn are wrong)
    int32_t* end;      // ... and the byte behind its last
};

// `frames` streams of h x w pictures, stream f the fr[f].len bytes at packed + fr[f].at with the tables
// tabs / quant[fr[f].tab] and at most maxi intervals, into out + f * frame_stride (rows ld >= 3 w bytes apart) as
// BGR, and status[f] = 0 or a JpegDecStatus (the picture of such a frame is unspecified, and written only inside
// its own h rows of 3 w bytes). Four kernels, none of which waits for another workgroup: the marker scan (a
// workgroup a frame: the RSTn positions compacted in order, their count and sequence checked), the entropy walk (a
// lane an interval: int16 coefficients through LDS), the chroma planes (a lane a block: dequantiser, slow-integer
// IDCT) and the picture (luma IDCT, h2v2 triangle filter, colour). ev (nullable): five events recorded around them.
hipError_t launch_jpeg_decode(const uint8_t* packed, const JpegDecFrame* fr, const JpegDecTables* tabs,
                              const JpegDecQuant* quant, int frames, int h, int w, int maxi, const JpegDecWork& wk,
                              uint8_t* out, int64_t frame_stride, int64_t ld, int32_t* status, hipStream_t s,
                              hipEvent_t* ev);

}  // namespace svx
