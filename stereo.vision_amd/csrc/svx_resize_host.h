// Host-only part of the general-scale bilinear resize (rt_resize.hip): cv2.resize's 8-bit INTER_LINEAR coefficient
// tables (sv_resize_coefficients), the layout of the table block the kernel reads, the argument checks of
// sv_resize_linear_u8 and the plan of sv_images_tile (batchImages, functions.py:456-501, for one to five pictures).
// No HIP in here, so that tools/resize_host_check.cpp can run it under the host sanitizers without a device (by
// hand, on the development machine only).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace svx {

constexpr int kResizeMaxSrc = 8192;   // rows or pixels of a source: the stack of two 4096-wide pictures is one
constexpr int kResizeMaxDst = 4096;   // rows or pixels of a destination
constexpr int kResizeCoefBits = 11;   // OpenCV's INTER_RESIZE_COEF_BITS

// The table of one axis, tests/tile_numpy._coefficients literally: per destination index the source index, the
// clamped next one and the two int16 coefficients of 11-bit fixed point, each rounded half to even in float32
// (rintf under the default rounding mode). The source coordinate is evaluated in double and rounded to float32
// once (the unit is built with -ffp-contract=off); both coefficients are computed, as OpenCV computes them:
// 1.f - f is itself rounded when f < 0.5, so c0 is not 2048 - c1. false when dn or sn is outside 1 .. 8192.
inline bool resize_coefficients(int dn, int sn, int32_t* s0, int32_t* s1, int16_t* c0, int16_t* c1) {
    if (dn < 1 || dn > kResizeMaxSrc || sn < 1 || sn > kResizeMaxSrc || !s0 || !s1 || !c0 || !c1) return false;
    const double scale = 1.0 / ((double)dn / sn);
    for (int dx = 0; dx < dn; ++dx) {
        float f = (float)((dx + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        if (s < 0) s = 0, f = 0.f;
        if (s >= sn - 1) s = sn - 1, f = 0.f;
        s0[dx] = s;
        s1[dx] = s + 1 < sn - 1 ? s + 1 : sn - 1;
        c0[dx] = (int16_t)rintf((1.f - f) * (float)(1 << kResizeCoefBits));
        c1[dx] = (int16_t)rintf(f * (float)(1 << kResizeCoefBits));
    }
    return true;
}

// The table block of one resize in device memory: the x axis' four tables, then the y axis', every table at a
// multiple of 16 bytes (the entries of an axis are rounded up to 8).
struct ResizeTableLayout {
    size_t xs0 = 0, xs1 = 0, xa0 = 0, xa1 = 0, ys0 = 0, ys1 = 0, yb0 = 0, yb1 = 0, bytes = 0;
};

inline ResizeTableLayout resize_table_layout(int dh, int dw) {
    ResizeTableLayout l;
    const size_t nx = ((size_t)dw + 7) / 8 * 8, ny = ((size_t)dh + 7) / 8 * 8;
    l.xs0 = 0;
    l.xs1 = l.xs0 + 4 * nx;
    l.xa0 = l.xs1 + 4 * nx;
    l.xa1 = l.xa0 + 2 * nx;
    l.ys0 = l.xa1 + 2 * nx;
    l.ys1 = l.ys0 + 4 * ny;
    l.yb0 = l.ys1 + 4 * ny;
    l.yb1 = l.yb0 + 2 * ny;
    l.bytes = l.yb1 + 2 * ny;
    return l;
}

// fills a block of resize_table_layout(dh, dw).bytes bytes (16-byte aligned) for sh x sw -> dh x dw
inline bool resize_fill_tables(uint8_t* block, int sh, int sw, int dh, int dw) {
    if (!block || dh < 1 || dh > kResizeMaxDst || dw < 1 || dw > kResizeMaxDst) return false;
    const ResizeTableLayout l = resize_table_layout(dh, dw);
    for (size_t i = 0; i < l.bytes; ++i) block[i] = 0;
    return resize_coefficients(dw, sw, reinterpret_cast<int32_t*>(block + l.xs0),
                               reinterpret_cast<int32_t*>(block + l.xs1), reinterpret_cast<int16_t*>(block + l.xa0),
                               reinterpret_cast<int16_t*>(block + l.xa1)) &&
           resize_coefficients(dh, sh, reinterpret_cast<int32_t*>(block + l.ys0),
                               reinterpret_cast<int32_t*>(block + l.ys1), reinterpret_cast<int16_t*>(block + l.yb0),
                               reinterpret_cast<int16_t*>(block + l.yb1));
}

// nullptr when a resize of sh x sw to dh x dw is built, else what is wrong with the shapes
inline const char* resize_check_shape(int sh, int sw, int dh, int dw) {
    if (sh < 1 || sh > kResizeMaxSrc || sw < 1 || sw > kResizeMaxSrc) return "source dimensions in 1 .. 8192";
    if (dh < 1 || dh > kResizeMaxDst || dw < 1 || dw > kResizeMaxDst) return "destination dimensions in 1 .. 4096";
    return nullptr;
}

// whether [a, a + na) and [b, b + nb) share a byte
inline bool resize_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// nullptr when sv_resize_linear_u8's arguments are in range, else what is wrong with them
inline const char* resize_check_args(const void* src, int n, int sh, int sw, int channels, const void* dst, int dh,
                                     int dw) {
    if (!src || !dst) return "null image";
    if (n < 1) return "n >= 1";
    if (channels != 1 && channels != 3) return "channels 1 or 3";
    if (const char* why = resize_check_shape(sh, sw, dh, dw)) return why;
    const size_t sb = (size_t)n * sh * sw * channels, db = (size_t)n * dh * dw * channels;
    if (sb > ((size_t)1 << 40) || db > ((size_t)1 << 40)) return "n images of at most 2^40 bytes";
    if (resize_overlap(src, sb, dst, db)) return "dst overlaps src";
    return nullptr;
}

// ---- batchImages of `count` pictures at size (H, W) ----------------------------------------------------------------
// The stack of the pictures resized to H x W (BGR), and what its final resize writes:
//   count 1: no stack; the resized picture is the output, H x W
//   count 2: hstack(0, 1), H x 2 W; fx = fy = 0.5 -> H / 2 x W (H even)
//   count 3: vstack(hstack(0, 1), hstack(2, 2)), 2 H x 2 W; 0.5 -> H x W
//   count 4: vstack(hstack(0, 1), hstack(2, 3)); 0.5 -> H x W
//   count 5: the same stack at 0.25 -> H / 2 x W / 2, beside picture 4 at 0.5 -> H / 2 x W / 2 (H and W even)
// The final resize is built only where the stack's size is an exact multiple of the scale: elsewhere OpenCV takes
// its scale from fx and not from the rounded dsize, and its scale-2 area path has a tail restated nowhere.
struct ImagesTilePlan {
    int count = 0, H = 0, W = 0;
    int stack_h = 0, stack_w = 0;   // 0 x 0 for count 1
    int left_h = 0, left_w = 0;     // the stack's resize (count 1: the picture's own)
    int out_h = 0, out_w = 0;
    int quadrants = 0;              // pictures placed in the stack; quadrant q at row (q / 2) H, column (q % 2) W
    int pic_of[4] = {0, 1, 2, 3};   // the picture of each quadrant (count 3: 2 twice)
};

// nullptr and the plan, else what is wrong with count, H or W
inline const char* images_tile_plan(int count, int H, int W, ImagesTilePlan* p) {
    if (count < 1 || count > 5) return "1 to 5 pictures";
    if (H < 1 || H > kResizeMaxDst || W < 1 || W > kResizeMaxDst) return "H and W in 1 .. 4096";
    if ((count == 2 || count == 5) && H % 2) return "H even for 2 or 5 pictures";
    if (count == 5 && W % 2) return "W even for 5 pictures";
    ImagesTilePlan q;
    q.count = count, q.H = H, q.W = W;
    if (count == 1) {
        q.left_h = q.out_h = H, q.left_w = q.out_w = W;
    } else if (count == 2) {
        q.quadrants = 2, q.stack_h = H, q.stack_w = 2 * W;
        q.left_h = q.out_h = H / 2, q.left_w = q.out_w = W;
    } else {
        q.quadrants = 4, q.stack_h = 2 * H, q.stack_w = 2 * W;
        if (count == 3) q.pic_of[3] = 2;
        if (count == 5) q.left_h = q.out_h = H / 2, q.left_w = W / 2, q.out_w = W;
        else q.left_h = q.out_h = H, q.left_w = q.out_w = W;
    }
    if (p) *p = q;
    return nullptr;
}

}  // namespace svx
