// Host-only part of the stereo rectification (rt_rectify.hip): the maker of OpenCV's fixed-point map
// pair (sv_rectify_map: initUndistortRectifyMap with m1type = CV_16SC2, as tests/rectify_numpy.py restates it) and
// the argument checks of sv_remap_u8 and sv_batch_rectify_maps. No HIP in here, so
// that tools/rectify_host_check.cpp can run it under the host sanitizers without a device (by hand, on the
// development machine only). Every unit that includes it is built with -ffp-contract=off: the oracle's float64
// operations are restated one by one, in its order, and the two agree bit for bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace svx {

constexpr int kRemapMaxDim = 8192;                // rows or pixels of a source or a destination
constexpr int kRemapFracEnd = 1024;               // a frac entry is fy * 32 + fx, 0 <= fx, fy < 32
constexpr double kRectIuMin = -32768.0 * 32.0;    // 32 x the coordinate, clamped so that it >> 5 fits int16
constexpr double kRectIuMax = 32767.0 * 32.0 + 31.0;

// nullptr when dh x dw is a map's shape, else what is wrong with it
inline const char* remap_check_dst(int dh, int dw) {
    if (dh < 1 || dh > kRemapMaxDim || dw < 1 || dw > kRemapMaxDim) return "destination dimensions in 1 .. 8192";
    return nullptr;
}

// nullptr when every frac entry of a dh x dw map is below 1024 (the kernel takes fx and fy from it unchecked)
inline const char* remap_check_frac(const uint16_t* frac, int dh, int dw) {
    const size_t n = (size_t)dh * dw;
    for (size_t i = 0; i < n; ++i)
        if (frac[i] >= kRemapFracEnd) return "a frac entry >= 1024 (fy * 32 + fx, 5 bits each)";
    return nullptr;
}

// whether [a, a + na) and [b, b + nb) share a byte
inline bool remap_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// nullptr when sv_remap_u8's arguments are in range, else what is wrong with them. Reads the whole frac map.
inline const char* remap_check_args(const void* src, int n, int sh, int sw, int channels, const int16_t* xy,
                                    const uint16_t* frac, int dh, int dw, const void* dst) {
    if (!src || !dst || !xy || !frac) return "null image or map";
    if (n < 1) return "n >= 1";
    if (channels != 1 && channels != 3) return "channels 1 or 3";
    if (sh < 1 || sh > kRemapMaxDim || sw < 1 || sw > kRemapMaxDim) return "source dimensions in 1 .. 8192";
    if (const char* why = remap_check_dst(dh, dw)) return why;
    const size_t sb = (size_t)n * sh * sw * channels, db = (size_t)n * dh * dw * channels;
    if (sb > ((size_t)1 << 40) || db > ((size_t)1 << 40)) return "n images of at most 2^40 bytes";
    if (remap_overlap(src, sb, dst, db)) return "dst overlaps src";
    return remap_check_frac(frac, dh, dw);
}

// inv = adj(M) / det(M), every product and difference written once (tests/rectify_numpy.inverse_3x3's order). false
// for a zero or non-finite determinant.
inline bool rectify_inverse(const double* M, double* inv) {
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    const double A00 = e * i - f * h, A01 = c * h - b * i, A02 = b * f - c * e;
    const double A10 = f * g - d * i, A11 = a * i - c * g, A12 = c * d - a * f;
    const double A20 = d * h - e * g, A21 = b * g - a * h, A22 = a * e - b * d;
    const double det = (a * A00 + b * A10) + c * A20;
    if (!isfinite(det) || det == 0.0) return false;
    inv[0] = A00 / det, inv[1] = A01 / det, inv[2] = A02 / det;
    inv[3] = A10 / det, inv[4] = A11 / det, inv[5] = A12 / det;
    inv[6] = A20 / det, inv[7] = A21 / det, inv[8] = A22 / det;
    return true;
}

// 32 x a map coordinate as the integer the map stores: rint (half to even under the default rounding mode), clamped;
// a non-finite value becomes the lower bound
inline int32_t rectify_fix(double t) {
    const double r = rint(32.0 * t);
    if (!isfinite(r)) return (int32_t)kRectIuMin;
    return (int32_t)(r < kRectIuMin ? kRectIuMin : r > kRectIuMax ? kRectIuMax : r);
}

// nullptr and the dh x dw map (xy: dh x dw x 2 int16 (sx, sy); frac: dh x dw uint16 fy * 32 + fx), else what is wrong.
// K9: the raw camera (fx, fy, u0, v0 are read); D8: k1, k2, p1, p2, k3, k4, k5, k6; R9: the rectifying rotation; P9:
// the new camera matrix. Nothing is written when it refuses.
inline const char* rectify_fill_map(const double* K9, const double* D8, const double* R9, const double* P9, int dh,
                                    int dw, int16_t* xy, uint16_t* frac) {
    if (!K9 || !D8 || !R9 || !P9 || !xy || !frac) return "null pointer";
    if (const char* why = remap_check_dst(dh, dw)) return why;
    double M[9], inv[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            M[3 * i + j] = (P9[3 * i] * R9[j] + P9[3 * i + 1] * R9[3 + j]) + P9[3 * i + 2] * R9[6 + j];
    if (!rectify_inverse(M, inv)) return "P R is singular or not finite";
    const double fxk = K9[0], fyk = K9[4], u0 = K9[2], v0 = K9[5];
    const double k1 = D8[0], k2 = D8[1], p1 = D8[2], p2 = D8[3], k3 = D8[4], k4 = D8[5], k5 = D8[6], k6 = D8[7];
    for (int iy = 0; iy < dh; ++iy) {
        const double v = (double)iy;
        for (int ix = 0; ix < dw; ++ix) {
            const double u = (double)ix;
            const double X = (inv[0] * u + inv[1] * v) + inv[2];
            const double Y = (inv[3] * u + inv[4] * v) + inv[5];
            const double W = (inv[6] * u + inv[7] * v) + inv[8];
            const double x = X / W, y = Y / W;
            const double r2 = x * x + y * y;
            const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xy2 = 2.0 * x * y;
            const double xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x * x);
            const double yd = (y * kr + p1 * (r2 + 2.0 * y * y)) + p2 * xy2;
            const int32_t iu = rectify_fix(fxk * xd + u0), iv = rectify_fix(fyk * yd + v0);
            const size_t at = (size_t)iy * dw + ix;
            xy[2 * at] = (int16_t)(iu >> 5);
            xy[2 * at + 1] = (int16_t)(iv >> 5);
            frac[at] = (uint16_t)((iv & 31) * 32 + (iu & 31));
        }
    }
    return nullptr;
}

}  // namespace svx
