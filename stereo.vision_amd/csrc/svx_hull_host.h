// Host-only part of the obstacle stage's runtime (rt_road.hip): the argument checks of sv_road_obstacles and the
// layout of the device buffer that holds a call's bitmaps, vertices and results. No HIP in here, so that
// tools/hull_host_check.cpp can run it under the host sanitizers without a device (by hand, on the development
// machine only).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svx.h"

namespace svx {

constexpr int kHullMaxH = 4096;   // rows of a frame the hull kernel takes (12 bytes of LDS a row)

// nullptr when sv_road_obstacles' arguments are in range, else what is wrong with them
inline const char* hull_check_args(const void* cleaned, const void* cam, int H, int W, const void* hull_pts,
                                   int64_t cap, const void* info) {
    if (!cleaned || !cam || !info) return "null cleaned image, camera or info";
    if (H < 1 || H > kHullMaxH) return "1 <= H <= 4096";
    if (W < 2 || W > 4096) return "2 <= W <= 4096";
    if (cap < 0 || (cap > 0 && !hull_pts)) return "cap < 0, or cap > 0 without hull_pts";
    return nullptr;
}

// One allocation: in | mask | obst bitmaps (frames x H x WW words each, every part 16-byte aligned; `in` only
// with with_in: the batch reads the clean-up's own bitmaps), the vertices (frames x 2 H int32 pairs), the infos.
struct HullLayout {
    int pitch = 0, WW = 0;             // u8 staging stride (W rounded up to 8); words a bitmap row
    size_t px = 0, words = 0;          // bytes of a staged u8 frame; words of a frame's bitmap
    size_t off_in = 0, off_mask = 0, off_obst = 0, off_pts = 0, off_info = 0, bytes = 0;
};

inline HullLayout hull_layout(int H, int W, int frames, bool with_in) {
    HullLayout l;
    const auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    l.pitch = (W + 7) / 8 * 8;
    l.WW = (W + 31) / 32;
    l.px = (size_t)H * (size_t)l.pitch;
    l.words = (size_t)H * (size_t)l.WW;
    const size_t bits = up16(sizeof(uint32_t) * l.words * (size_t)frames);
    l.off_in = 0;
    l.off_mask = with_in ? bits : 0;
    l.off_obst = l.off_mask + bits;
    l.off_pts = l.off_obst + bits;
    l.off_info = l.off_pts + up16(sizeof(int32_t) * 4 * (size_t)H * (size_t)frames);
    l.bytes = l.off_info + sizeof(sv_hull_info) * (size_t)frames;
    return l;
}

}  // namespace svx
