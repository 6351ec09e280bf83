// Stand-alone program over the rectification's host code (stereo.vision_amd/csrc/svx_rectify_host.h): the maker of the
// fixed-point map pair and the argument checks of sv_remap_u8.
//   rectify_host_check K(9) D(8) R(9) P(9) dh dw   writes the map to stdout, raw little-endian: xy (dh x dw x 2 int16,
//                                                  (sx, sy)), then frac (dh x dw uint16). Exit status 2 (and
//                                                  "refused: ..." on stderr) when the model or the shape is refused
//   rectify_host_check                             the self-check below; "rectify host check ok" and status 0
// tests/test_rectify_cpu.py compiles it with the host compiler and compares the first form with the oracle's, every
// entry. It is also what the host sanitizers run, by hand on the development machine after a change to
// svx_rectify_host.h:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/rectify_host_check.cpp -o x && ./x && ./x 800 0 511.5 0 776 271.5 0 0 1  -0.3 0 0 0 0 0 0 0
//       1 0 0 0 1 0 0 0 1  800 0 511.5 0 776 271.5 0 0 1  544 1024 | wc -c
// It touches no device: every map is written into host allocations of exactly the map's size.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../stereo.vision_amd/csrc/svx_rectify_host.h"

using namespace svx;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);      \
            ++failures;                                              \
        }                                                            \
    } while (0)

struct Model {
    double K[9], D[8], R[9], P[9];
};

static Model identity_model(double f, double u0, double v0) {
    Model m{};
    const double K[9] = {f, 0, u0, 0, f, v0, 0, 0, 1};
    for (int i = 0; i < 9; ++i) m.K[i] = m.P[i] = K[i], m.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    return m;
}

static bool fill(const Model& m, int dh, int dw, std::vector<int16_t>& xy, std::vector<uint16_t>& frac) {
    xy.assign((size_t)dh * dw * 2, 0x5555);   // exactly the map's sizes
    frac.assign((size_t)dh * dw, 0x5555);
    return rectify_fill_map(m.K, m.D, m.R, m.P, dh, dw, xy.data(), frac.data()) == nullptr;
}

static int self_check() {
    std::vector<int16_t> xy;
    std::vector<uint16_t> frac;
    const int shapes[][2] = {{1, 1}, {2, 70}, {13, 17}, {390, 889}, {544, 1024}, {1, 8192}, {8192, 1}};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // K = P, R = I, D = 0: the identity map
    for (const auto& s : shapes) {
        const Model m = identity_model(0.8 * s[1] + 1.0, (s[1] - 1) / 2.0, (s[0] - 1) / 2.0);
        CHECK(fill(m, s[0], s[1], xy, frac));
        bool ok = true;
        for (int y = 0; y < s[0]; ++y)
            for (int x = 0; x < s[1]; ++x) {
                const size_t at = (size_t)y * s[1] + x;
                ok = ok && xy[2 * at] == x && xy[2 * at + 1] == y && frac[at] == 0;
            }
        CHECK(ok);
    }
    // the new camera's u0 moved by + 2.5: the source column is x - 2.5, so sx = x - 3 and fx = 16
    {
        Model m = identity_model(400.0, 35.0, 6.0);
        m.P[2] += 2.5;
        CHECK(fill(m, 13, 70, xy, frac));
        bool ok = true;
        for (int y = 0; y < 13; ++y)
            for (int x = 0; x < 70; ++x) {
                const size_t at = (size_t)y * 70 + x;
                ok = ok && xy[2 * at] == x - 3 && xy[2 * at + 1] == y && frac[at] == 16;
            }
        CHECK(ok);
    }
    // every model below: frac < 1024 everywhere, whatever the coordinates do (strong distortion, a camera that looks
    // along the image plane, coefficients that make the denominator cross zero, a huge focal length)
    {
        Model ms[5];
        for (auto& m : ms) m = identity_model(800.0, 511.5, 271.5);
        ms[0].D[0] = -0.3;
        ms[1].D[0] = -40.0, ms[1].D[5] = -25.0, ms[1].D[2] = 0.5, ms[1].D[3] = -0.5;
        const double c = std::cos(1.5), s = std::sin(1.5);
        ms[2].R[0] = c, ms[2].R[2] = s, ms[2].R[6] = -s, ms[2].R[8] = c;
        ms[3].K[0] = 1e300, ms[3].K[4] = 1e300, ms[3].D[0] = 1e300;
        ms[4].P[0] = 1e-3, ms[4].P[4] = 1e-3;
        for (const auto& m : ms)
            for (const auto& sh : shapes) {
                CHECK(fill(m, sh[0], sh[1], xy, frac));
                CHECK(remap_check_frac(frac.data(), sh[0], sh[1]) == nullptr);
            }
        // non-finite coordinates become the lower bound: (-32768, -32768), frac 0
        Model bad = identity_model(800.0, 511.5, 271.5);
        bad.K[2] = nan;
        bad.K[5] = inf;
        CHECK(fill(bad, 2, 3, xy, frac));
        CHECK(xy[0] == -32768 && xy[1] == -32768 && frac[0] == 0 && xy[10] == -32768 && frac[5] == 0);
        bad = identity_model(800.0, 511.5, 271.5);
        bad.K[2] = 1e9;    // beyond int16: clamped to the upper bound, 32767 and fx = 31
        bad.K[5] = -1e9;
        CHECK(fill(bad, 1, 1, xy, frac));
        CHECK(xy[0] == 32767 && xy[1] == -32768 && frac[0] == 31);
    }
    // refusals write nothing
    {
        Model m = identity_model(800.0, 511.5, 271.5);
        std::vector<int16_t> a(8, 77);
        std::vector<uint16_t> b(4, 77);
        Model sing = m;
        sing.P[0] = 0.0;                           // det(P R) = 0
        CHECK(rectify_fill_map(sing.K, sing.D, sing.R, sing.P, 2, 2, a.data(), b.data()) != nullptr);
        sing = m;
        for (double& r : sing.R) r = 0.0;
        CHECK(rectify_fill_map(sing.K, sing.D, sing.R, sing.P, 2, 2, a.data(), b.data()) != nullptr);
        sing = m;
        sing.P[4] = nan;
        CHECK(rectify_fill_map(sing.K, sing.D, sing.R, sing.P, 2, 2, a.data(), b.data()) != nullptr);
        sing.P[4] = inf;
        CHECK(rectify_fill_map(sing.K, sing.D, sing.R, sing.P, 2, 2, a.data(), b.data()) != nullptr);
        const int dims[][2] = {{0, 2}, {2, 0}, {-1, 2}, {8193, 1}, {1, 8193}, {2147483647, 2147483647}};
        for (const auto& d : dims) CHECK(rectify_fill_map(m.K, m.D, m.R, m.P, d[0], d[1], a.data(), b.data()) != nullptr);
        CHECK(rectify_fill_map(nullptr, m.D, m.R, m.P, 2, 2, a.data(), b.data()) != nullptr);
        CHECK(rectify_fill_map(m.K, nullptr, m.R, m.P, 2, 2, a.data(), b.data()) != nullptr);
        CHECK(rectify_fill_map(m.K, m.D, nullptr, m.P, 2, 2, a.data(), b.data()) != nullptr);
        CHECK(rectify_fill_map(m.K, m.D, m.R, nullptr, 2, 2, a.data(), b.data()) != nullptr);
        CHECK(rectify_fill_map(m.K, m.D, m.R, m.P, 2, 2, nullptr, b.data()) != nullptr);
        CHECK(rectify_fill_map(m.K, m.D, m.R, m.P, 2, 2, a.data(), nullptr) != nullptr);
        bool untouched = true;
        for (int16_t v : a) untouched = untouched && v == 77;
        for (uint16_t v : b) untouched = untouched && v == 77;
        CHECK(untouched);
        CHECK(rectify_fill_map(m.K, m.D, m.R, m.P, 2, 2, a.data(), b.data()) == nullptr);
    }
    // the inverse: closed form of a diagonal matrix, and M inv(M) of a rotation
    {
        const double Dg[9] = {2, 0, 0, 0, 4, 0, 0, 0, 0.5};
        double inv[9];
        CHECK(rectify_inverse(Dg, inv));
        CHECK(inv[0] == 0.5 && inv[4] == 0.25 && inv[8] == 2.0 && inv[1] == 0.0 && inv[5] == 0.0);
        const double Z[9] = {1, 2, 3, 2, 4, 6, 0, 0, 1};
        CHECK(!rectify_inverse(Z, inv));
    }
    // sv_remap_u8's checks
    {
        uint8_t src[64] = {}, dst[64] = {};
        int16_t mxy[32] = {};
        uint16_t mfr[16] = {};
        CHECK(remap_check_args(src, 1, 4, 4, 1, mxy, mfr, 4, 4, dst) == nullptr);
        CHECK(remap_check_args(src, 1, 4, 4, 3, mxy, mfr, 4, 4, dst) == nullptr);
        CHECK(remap_check_args(nullptr, 1, 4, 4, 1, mxy, mfr, 4, 4, dst) != nullptr);
        CHECK(remap_check_args(src, 1, 4, 4, 1, nullptr, mfr, 4, 4, dst) != nullptr);
        CHECK(remap_check_args(src, 1, 4, 4, 1, mxy, nullptr, 4, 4, dst) != nullptr);
        CHECK(remap_check_args(src, 1, 4, 4, 1, mxy, mfr, 4, 4, nullptr) != nullptr);
        CHECK(remap_check_args(src, 0, 4, 4, 1, mxy, mfr, 4, 4, dst) != nullptr);
        for (int ch : {0, 2, 4}) CHECK(remap_check_args(src, 1, 4, 4, ch, mxy, mfr, 4, 4, dst) != nullptr);
        CHECK(remap_check_args(src, 1, 0, 4, 1, mxy, mfr, 4, 4, dst) != nullptr);
        CHECK(remap_check_args(src, 1, 4, 8193, 1, mxy, mfr, 4, 4, dst) != nullptr);
        CHECK(remap_check_args(src, 1, 4, 4, 1, mxy, mfr, 0, 4, dst) != nullptr);
        CHECK(remap_check_args(src, 1, 4, 4, 1, mxy, mfr, 4, 8193, dst) != nullptr);   // refused before frac is read
        CHECK(remap_check_args(src, 1, 4, 4, 1, mxy, mfr, 4, 4, src) != nullptr);
        CHECK(remap_check_args(src, 1, 4, 4, 1, mxy, mfr, 4, 4, src + 15) != nullptr);
        CHECK(remap_check_args(src, 1, 4, 4, 1, mxy, mfr, 4, 4, src + 16) == nullptr);
        mfr[15] = 1023;
        CHECK(remap_check_args(src, 1, 4, 4, 1, mxy, mfr, 4, 4, dst) == nullptr);
        mfr[15] = 1024;
        CHECK(remap_check_args(src, 1, 4, 4, 1, mxy, mfr, 4, 4, dst) != nullptr);
    }
    if (failures) return 1;
    std::printf("rectify host check ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return self_check();
    if (argc != 38) {
        std::fprintf(stderr, "usage: %s [K(9) D(8) R(9) P(9) dh dw]\n", argv[0]);
        return 64;
    }
    Model m{};
    int at = 1;
    for (double& v : m.K) v = std::strtod(argv[at++], nullptr);
    for (double& v : m.D) v = std::strtod(argv[at++], nullptr);
    for (double& v : m.R) v = std::strtod(argv[at++], nullptr);
    for (double& v : m.P) v = std::strtod(argv[at++], nullptr);
    const long dh = std::strtol(argv[at++], nullptr, 10), dw = std::strtol(argv[at++], nullptr, 10);
    if (dh < 1 || dh > kRemapMaxDim || dw < 1 || dw > kRemapMaxDim) {
        std::fprintf(stderr, "refused: destination dimensions in 1 .. 8192\n");
        return 2;
    }
    std::vector<int16_t> xy((size_t)dh * dw * 2);
    std::vector<uint16_t> frac((size_t)dh * dw);
    if (const char* why = rectify_fill_map(m.K, m.D, m.R, m.P, (int)dh, (int)dw, xy.data(), frac.data())) {
        std::fprintf(stderr, "refused: %s\n", why);
        return 2;
    }
    if (std::fwrite(xy.data(), sizeof(int16_t), xy.size(), stdout) != xy.size()) return 1;
    if (std::fwrite(frac.data(), sizeof(uint16_t), frac.size(), stdout) != frac.size()) return 1;
    return 0;
}
