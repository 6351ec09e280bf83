// Host-only part of the image tile's runtime (rt_road.hip): the shape and argument checks of sv_image_tile and
// sv_batch_tile, the size of a batch's tile buffer and the layout of the device buffer that stages a host call's
// result image and holds its tile. No HIP in here, so that tools/tile_host_check.cpp can run it under the host
// sanitizers without a device (by hand, on the development machine only).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace svx {

constexpr int kTileMaxH = 4096;   // rows of a frame
constexpr int kTileMaxW = 4096;   // pixels of a row

// nullptr when a frame of H x W has a tile, else what is wrong with the shape: the quadrants of the stack meet on
// output-pixel boundaries only when H and W are multiples of 4
inline const char* tile_check_shape(int H, int W) {
    if (H < 4 || H > kTileMaxH || H % 4) return "H a multiple of 4, 4 <= H <= 4096";
    if (W < 4 || W > kTileMaxW || W % 4) return "W a multiple of 4, 4 <= W <= 4096";
    return nullptr;
}

// bytes of a frame's tile: H / 2 rows of 3 W bytes, packed
inline size_t tile_frame_bytes(int H, int W) { return (size_t)(H / 2) * 3 * (size_t)W; }

// whether [a, a + na) and [b, b + nb) share a byte
inline bool tile_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// nullptr when sv_image_tile's arguments are in range, else what is wrong with them
inline const char* tile_check_args(const void* disparity, const void* bgr, const void* road, const void* cleaned,
                                   const void* result, int H, int W, const void* out) {
    if (!disparity || !bgr || !road || !cleaned || !result || !out) return "null image";
    if (const char* why = tile_check_shape(H, W)) return why;
    const size_t px = (size_t)H * (size_t)W, ob = tile_frame_bytes(H, W);
    if (tile_overlap(out, ob, disparity, px) || tile_overlap(out, ob, bgr, 3 * px) || tile_overlap(out, ob, road, px) ||
        tile_overlap(out, ob, cleaned, px) || tile_overlap(out, ob, result, 3 * px))
        return "out overlaps an input";
    return nullptr;
}

// sv_image_tile's device buffer: the staged result image (H rows of ld3 bytes) | the tile, both 16-byte aligned.
// The disparity, the BGR and the two road pictures are staged in the device's buffers of their own, the u8 ones at
// `pitch`, the BGR at ld3.
struct TileLayout {
    int pitch = 0, ld3 = 0;   // u8 staging stride (W rounded up to 8); bytes of a BGR row at that stride
    size_t img = 0;           // bytes of a BGR image at ld3
    size_t off_res = 0, off_out = 0, bytes = 0;
};

inline TileLayout tile_layout(int H, int W) {
    TileLayout l;
    const auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    l.pitch = (W + 7) / 8 * 8;
    l.ld3 = 3 * l.pitch;
    l.img = up16((size_t)H * (size_t)l.ld3);
    l.off_res = 0;
    l.off_out = l.img;
    l.bytes = l.off_out + up16(tile_frame_bytes(H, W));
    return l;
}

}  // namespace svx
