// Host-side launcher of kernels/remap.hip: cv2.remap's 8-bit INTER_LINEAR path through a fixed-point map pair
// (svx_rectify_host.h), for one picture stack or for the two eyes of a batch in one launch. (A header of its own, like
// svx_resize.h: svx_launch.h is part of the sources sv_source_id hashes.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/svx.h"
#include "svx_rectify_host.h"   // kRemapMaxDim

namespace svx {

// `eyes` (1 or 2) stacks of n packed pictures of sh x sw x channels (1 or 3) bytes, picture f of eye e at
// src[e] + f * sh * sw * channels, each remapped through its eye's map (xy[e]: dh x dw x 2 int16, frac[e]: dh x dw
// uint16, every entry < 1024: the kernel checks none) into n packed pictures of dh x dw x channels at dst[e]. No
// destination may overlap a source. The maps are device memory, xy 16-byte and frac 8-byte aligned; dst 4-byte.
struct RemapArgs {
    const uint8_t* src[2];
    uint8_t* dst[2];
    const int16_t* xy[2];
    const uint16_t* frac[2];
    int eyes, n, sh, sw, channels, dh, dw;
};

// A lane owns its destination pixels for every picture of its chunk of the stack and keeps their map entries in
// registers. With dw % 4 == 0 and dw >= kRemapQuadMin a lane makes four neighbouring pixels and stores them as 4 or 12
// bytes; other shapes take a pixel per lane and store bytes.
constexpr int kRemapQuadMin = 128;
hipError_t launch_remap(const RemapArgs& a, hipStream_t s);

}  // namespace svx
