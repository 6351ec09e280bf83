// Host-only part of the result image's runtime (rt_road.hip): the argument checks of sv_result_image and the layout
// of the device buffer that holds a call's image, obstacle bitmap, vertices and info. No HIP in here, so that
// tools/result_host_check.cpp can run it under the host sanitizers without a device (by hand, on the development
// machine only).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svx.h"

namespace svx {

constexpr int kResultMaxH = 4096;        // rows of a frame
constexpr int kResultMaxW = 4096;        // pixels of a row
constexpr int kResultMaxCoord = 16383;   // |x|, |y| of a hull vertex and of the centre: the outline's terms fit 64 bits
constexpr int kResultMaxVerts = 8192;    // vertices of a frame (the obstacle stage writes at most 2 H)

// how often the sign of the non-zero values of d(0) .. d(n - 1) changes around the ring
template <class F>
inline int ring_sign_changes(int64_t n, F d) {
    int first = 0, last = 0, changes = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t v = d(i);
        const int s = v > 0 ? 1 : v < 0 ? -1 : 0;
        if (!s) continue;
        if (!first) first = s;
        if (last && s != last) ++changes;
        last = s;
    }
    if (first && last != first) ++changes;
    return changes;
}

// Whether the n >= 3 vertices are a convex polygon in outline order (either orientation; collinear and repeated
// vertices allowed): every turn has the same sign, and the ring goes once around (x and y each change direction at
// most twice).
inline bool result_is_convex_ring(const int32_t* p, int64_t n) {
    const auto dx = [&](int64_t i) { return (int64_t)p[2 * ((i + 1) % n)] - p[2 * i]; };
    const auto dy = [&](int64_t i) { return (int64_t)p[2 * ((i + 1) % n) + 1] - p[2 * i + 1]; };
    bool pos = false, neg = false;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t j = (i + 1) % n;
        const int64_t cr = dx(i) * dy(j) - dy(i) * dx(j);
        pos |= cr > 0;
        neg |= cr < 0;
    }
    if (pos && neg) return false;
    return ring_sign_changes(n, dx) <= 2 && ring_sign_changes(n, dy) <= 2;
}

// nullptr when sv_result_image's arguments are in range, else what is wrong with them
inline const char* result_check_args(const void* bgr, const void* obstacles, const int32_t* hull_pts, int64_t n,
                                     const sv_hull_info* info, int H, int W, const void* out) {
    if (!bgr || !obstacles || !out) return "null image";
    if (H < 1 || H > kResultMaxH) return "1 <= H <= 4096";
    if (W < 2 || W > kResultMaxW) return "2 <= W <= 4096";
    if (n < 0 || n > kResultMaxVerts || (n > 0 && !hull_pts)) return "0 <= n <= 8192, hull_pts with n > 0";
    for (int64_t i = 0; i < 2 * n; ++i)
        if (hull_pts[i] < -kResultMaxCoord || hull_pts[i] > kResultMaxCoord) return "|vertex| <= 16383";
    if (n >= 3 && !result_is_convex_ring(hull_pts, n)) return "hull_pts is no convex polygon in outline order";
    if (info && (info->valid & 2) &&
        (info->cx < -kResultMaxCoord || info->cx > kResultMaxCoord || info->cy < -kResultMaxCoord ||
         info->cy > kResultMaxCoord))
        return "|centre| <= 16383";
    return nullptr;
}

// One allocation: the result image (H rows of ld3 bytes) | the obstacle bitmap (H x WW words) | the vertices | the
// info, every part 16-byte aligned. The BGR and the obstacles' bytes are staged in buffers of their own.
struct ResultLayout {
    int pitch = 0, ld3 = 0, WW = 0;    // u8 staging stride (W rounded up to 8); bytes a BGR row; words a bitmap row
    size_t img = 0;                    // bytes of an image at the stride
    size_t off_out = 0, off_bits = 0, off_pts = 0, off_info = 0, bytes = 0;
};

inline ResultLayout result_layout(int H, int W, int64_t n) {
    ResultLayout l;
    const auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    l.pitch = (W + 7) / 8 * 8;
    l.ld3 = 3 * l.pitch;
    l.WW = (W + 31) / 32;
    l.img = up16((size_t)H * (size_t)l.ld3);
    l.off_out = 0;
    l.off_bits = l.img;
    l.off_pts = l.off_bits + up16(sizeof(uint32_t) * (size_t)H * (size_t)l.WW);
    l.off_info = l.off_pts + up16(sizeof(int32_t) * 2 * (size_t)(n > 0 ? n : 1));
    l.bytes = l.off_info + sizeof(sv_hull_info);
    return l;
}

}  // namespace svx
