// Stand-alone check of the result image's host code (stereo.vision_amd/csrc/svx_result_host.h): the argument checks
// of sv_result_image (ranges, the convex-ring test) and the layout of the device buffer, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/result_host_check.cpp -o x && ./x
// It touches no device: every part of a layout is written to its last byte in a host allocation of the layout's
// size, the way the kernel and the copies fill the device one. Run it by hand on the development machine after a
// change to svx_result_host.h; it is part of no test and is never run on a GPU machine.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../stereo.vision_amd/csrc/svx_result_host.h"

using namespace svx;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);      \
            ++failures;                                              \
        }                                                            \
    } while (0)

static void check_layout(int H, int W, int64_t n) {
    const ResultLayout l = result_layout(H, W, n);
    const size_t bits = sizeof(uint32_t) * (size_t)H * l.WW, pts = sizeof(int32_t) * 2 * (size_t)n;
    CHECK(l.WW == (W + 31) / 32 && l.pitch >= W && l.pitch % 8 == 0 && l.pitch < W + 8 && l.pitch <= 32 * l.WW);
    CHECK(l.ld3 == 3 * l.pitch && l.img >= (size_t)H * l.ld3 && l.img % 16 == 0);
    CHECK(l.off_out == 0 && l.off_bits >= l.img && l.off_pts >= l.off_bits + bits && l.off_info >= l.off_pts + pts);
    CHECK(l.off_bits % 16 == 0 && l.off_pts % 16 == 0 && l.off_info % 16 == 0);
    CHECK(l.bytes == l.off_info + sizeof(sv_hull_info));
    std::vector<unsigned char> buf(l.bytes);   // every part, to its last byte
    std::memset(buf.data() + l.off_out, 1, (size_t)H * l.ld3);
    std::memset(buf.data() + l.off_bits, 2, bits);
    int32_t* p = reinterpret_cast<int32_t*>(buf.data() + l.off_pts);
    for (int64_t i = 0; i < 2 * n; ++i) p[i] = (int32_t)i;
    *reinterpret_cast<sv_hull_info*>(buf.data() + l.off_info) = sv_hull_info{(int32_t)n, 1, 2, 3, 4, 5};
    CHECK(buf[0] == 1 && buf[(size_t)H * l.ld3 - 1] == 1 && buf[l.off_bits] == 2 && buf[l.off_bits + bits - 1] == 2);
    if (n > 0) CHECK(p[0] == 0 && p[2 * n - 1] == (int32_t)(2 * n - 1));
    CHECK(reinterpret_cast<const sv_hull_info*>(buf.data() + l.off_info)->tipy == 5);
}

int main() {
    static_assert(sizeof(sv_hull_info) == 32, "sv_hull_info: four int32 and two int64");
    unsigned char img[4] = {0, 0, 0, 0};
    sv_hull_info info = {0, 1, 1, 3, 7, 7};
    const int32_t tri[] = {1, 1, 1, 3, 6, 3};
    CHECK(result_check_args(img, img, tri, 3, &info, 4, 8, img) == nullptr);
    CHECK(result_check_args(img, img, tri, 3, nullptr, 4, 8, img) == nullptr);
    CHECK(result_check_args(img, img, nullptr, 0, nullptr, 1, 2, img) == nullptr);
    CHECK(result_check_args(img, img, tri, 1, &info, 4096, 4096, img) == nullptr);
    CHECK(result_check_args(nullptr, img, tri, 3, &info, 4, 8, img) != nullptr);
    CHECK(result_check_args(img, nullptr, tri, 3, &info, 4, 8, img) != nullptr);
    CHECK(result_check_args(img, img, tri, 3, &info, 4, 8, nullptr) != nullptr);
    CHECK(result_check_args(img, img, nullptr, 3, &info, 4, 8, img) != nullptr);
    CHECK(result_check_args(img, img, tri, -1, &info, 4, 8, img) != nullptr);
    CHECK(result_check_args(img, img, tri, 8193, &info, 4, 8, img) != nullptr);   // refused before a vertex is read
    CHECK(result_check_args(img, img, tri, 3, &info, 0, 8, img) != nullptr);
    CHECK(result_check_args(img, img, tri, 3, &info, 4097, 8, img) != nullptr);
    CHECK(result_check_args(img, img, tri, 3, &info, 4, 1, img) != nullptr);
    CHECK(result_check_args(img, img, tri, 3, &info, 4, 4097, img) != nullptr);
    CHECK(result_check_args(img, img, tri, 3, &info, 2147483647, 2147483647, img) != nullptr);
    const int32_t far[] = {1, 1, 1, 3, 16384, 3}, neg[] = {1, 1, 1, -16384, 6, 3};
    const int32_t edge[] = {-16383, 0, 0, 16383, 16383, 0};
    CHECK(result_check_args(img, img, far, 3, &info, 4, 8, img) != nullptr);
    CHECK(result_check_args(img, img, neg, 3, &info, 4, 8, img) != nullptr);
    CHECK(result_check_args(img, img, edge, 3, &info, 4, 8, img) == nullptr);
    sv_hull_info off = {0, 20000, 1, 3, 7, 7};
    CHECK(result_check_args(img, img, tri, 3, &off, 4, 8, img) != nullptr);
    off.valid = 1;   // no glyph: the centre is not read
    CHECK(result_check_args(img, img, tri, 3, &off, 4, 8, img) == nullptr);
    // the convex-ring test: either orientation, any start, collinear and repeated vertices; dents, bow ties and
    // rings that go round twice are refused
    const int32_t sq[] = {0, 0, 0, 5, 5, 5, 5, 0}, sq_r[] = {5, 0, 5, 5, 0, 5, 0, 0};
    const int32_t col[] = {0, 0, 0, 2, 0, 5, 5, 5, 5, 5, 5, 0}, line3[] = {0, 0, 4, 4, 2, 2};
    const int32_t dent[] = {0, 0, 6, 0, 3, 1, 6, 3, 0, 3}, bow[] = {0, 0, 5, 5, 5, 0, 0, 5};
    const int32_t star[] = {3, 0, 5, 3, 0, 1, 6, 1, 1, 3}, zig[] = {0, 0, 10, 10, 2, 2, 8, 8};
    const int32_t flat[] = {0, 3, 9, 3, 2, 3, 7, 3};
    CHECK(result_is_convex_ring(sq, 4) && result_is_convex_ring(sq_r, 4) && result_is_convex_ring(col, 6));
    CHECK(result_is_convex_ring(line3, 3) && result_is_convex_ring(edge, 3));
    CHECK(!result_is_convex_ring(dent, 5) && !result_is_convex_ring(bow, 4) && !result_is_convex_ring(star, 5));
    CHECK(!result_is_convex_ring(zig, 4) && !result_is_convex_ring(flat, 4));
    std::vector<int32_t> ring(2 * 8192);       // the largest ring: a vertex a row down the left side and up the right
    for (int i = 0; i < 4096; ++i) {
        ring[2 * i] = 0, ring[2 * i + 1] = i;
        ring[2 * (8191 - i)] = 4095, ring[2 * (8191 - i) + 1] = i;
    }
    CHECK(result_check_args(img, img, ring.data(), 8192, &info, 4096, 4096, img) == nullptr);
    const int shapes[][2] = {{1, 2}, {1, 33}, {40, 70}, {64, 96}, {390, 889}, {544, 1024}, {17, 4096}, {4096, 2},
                             {4096, 4096}, {3, 31}, {3, 32}, {5, 65}};
    for (const auto& s : shapes)
        for (int64_t n : {0, 1, 2, 7, 8192}) check_layout(s[0], s[1], n);
    if (failures) return 1;
    std::printf("result host check ok\n");
    return 0;
}
