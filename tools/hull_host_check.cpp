// Stand-alone check of the obstacle stage's host code (stereo.vision_amd/csrc/svx_hull_host.h): the argument checks
// of sv_road_obstacles and the layout of the device buffer, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/hull_host_check.cpp -o x && ./x
// It touches no device: every part of a layout is written to its last byte in a host allocation of the layout's
// size, the way the kernel and the copies fill the device one. Run it by hand on the development machine after a
// change to svx_hull_host.h; it is part of no test and is never run on a GPU machine.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../stereo.vision_amd/csrc/svx_hull_host.h"

using namespace svx;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);      \
            ++failures;                                              \
        }                                                            \
    } while (0)

static void check_layout(int H, int W, int frames, bool with_in) {
    const HullLayout l = hull_layout(H, W, frames, with_in);
    const size_t bits = sizeof(uint32_t) * l.words * (size_t)frames;
    const size_t pts = sizeof(int32_t) * 4 * (size_t)H * (size_t)frames;
    CHECK(l.WW == (W + 31) / 32 && l.pitch >= W && l.pitch % 8 == 0 && l.pitch < W + 8 && l.pitch <= 32 * l.WW);
    CHECK(l.words == (size_t)H * l.WW && l.px == (size_t)H * l.pitch);
    CHECK(l.off_in == 0 && (with_in ? l.off_mask >= bits : l.off_mask == 0));
    CHECK(l.off_obst >= l.off_mask + bits && l.off_pts >= l.off_obst + bits && l.off_info >= l.off_pts + pts);
    CHECK(l.off_mask % 16 == 0 && l.off_obst % 16 == 0 && l.off_pts % 16 == 0 && l.off_info % 16 == 0);
    CHECK(l.bytes == l.off_info + sizeof(sv_hull_info) * (size_t)frames);
    std::vector<unsigned char> buf(l.bytes);   // every part, to its last byte
    if (with_in) std::memset(buf.data() + l.off_in, 1, bits);
    std::memset(buf.data() + l.off_mask, 2, bits);
    std::memset(buf.data() + l.off_obst, 3, bits);
    for (int f = 0; f < frames; ++f) {         // a frame's vertices: 2 H pairs at pts + f * 4 H
        int32_t* p = reinterpret_cast<int32_t*>(buf.data() + l.off_pts) + 4 * (size_t)H * f;
        for (int i = 0; i < 2 * H; ++i) p[2 * i] = p[2 * i + 1] = i;
        sv_hull_info* info = reinterpret_cast<sv_hull_info*>(buf.data() + l.off_info) + f;
        *info = sv_hull_info{2 * H, 1, 2, 3, 4, 5};
    }
    // the parts did not overwrite each other
    CHECK(buf[l.off_mask] == 2 && buf[l.off_mask + bits - 1] == 2 && buf[l.off_obst] == 3 &&
          buf[l.off_obst + bits - 1] == 3);
    if (with_in) CHECK(buf[0] == 1 && buf[bits - 1] == 1);
    const sv_hull_info* last = reinterpret_cast<const sv_hull_info*>(buf.data() + l.off_info) + (frames - 1);
    CHECK(last->n == 2 * H && last->tipy == 5);
    const int32_t* p0 = reinterpret_cast<const int32_t*>(buf.data() + l.off_pts);
    CHECK(p0[0] == 0 && p0[4 * (size_t)H * frames - 1] == 2 * H - 1);
}

int main() {
    static_assert(sizeof(sv_hull_info) == 32, "sv_hull_info: four int32 and two int64");
    unsigned char img[4] = {0, 0, 0, 0};
    sv_camera cam = {1.0, 1.0, 0.0, 0.0};
    sv_hull_info info;
    int32_t pts[4];
    CHECK(hull_check_args(img, &cam, 1, 2, pts, 2, &info) == nullptr);
    CHECK(hull_check_args(img, &cam, 4096, 4096, nullptr, 0, &info) == nullptr);
    CHECK(hull_check_args(nullptr, &cam, 1, 2, pts, 2, &info) != nullptr);
    CHECK(hull_check_args(img, nullptr, 1, 2, pts, 2, &info) != nullptr);
    CHECK(hull_check_args(img, &cam, 1, 2, pts, 2, nullptr) != nullptr);
    CHECK(hull_check_args(img, &cam, 0, 2, pts, 2, &info) != nullptr);
    CHECK(hull_check_args(img, &cam, -5, 2, pts, 2, &info) != nullptr);
    CHECK(hull_check_args(img, &cam, 4097, 2, pts, 2, &info) != nullptr);
    CHECK(hull_check_args(img, &cam, 1, 1, pts, 2, &info) != nullptr);
    CHECK(hull_check_args(img, &cam, 1, 4097, pts, 2, &info) != nullptr);
    CHECK(hull_check_args(img, &cam, 1, 2, pts, -1, &info) != nullptr);
    CHECK(hull_check_args(img, &cam, 1, 2, nullptr, 2, &info) != nullptr);
    CHECK(hull_check_args(img, &cam, 2147483647, 2147483647, pts, 2, &info) != nullptr);
    const int shapes[][2] = {{1, 2}, {1, 33}, {40, 70}, {64, 96}, {390, 889}, {544, 1024}, {17, 4096}, {4096, 2},
                             {4096, 4096}, {3, 31}, {3, 32}, {5, 65}};
    for (const auto& s : shapes)
        for (int frames : {1, 2, 5}) {
            if ((long long)s[0] * s[1] * frames > (64ll << 20)) continue;
            check_layout(s[0], s[1], frames, true);
            check_layout(s[0], s[1], frames, false);
        }
    check_layout(544, 1024, 64, false);
    // the largest batch the flagship runs: sizes in size_t, nothing wraps (no allocation)
    const HullLayout big = hull_layout(4096, 4096, 65535, true);
    CHECK(big.bytes > big.off_info && big.off_info > big.off_pts && big.off_pts > big.off_obst &&
          big.off_obst > big.off_mask && big.off_mask == sizeof(uint32_t) * 4096ull * 128ull * 65535ull);
    if (failures) return 1;
    std::printf("hull host check ok\n");
    return 0;
}
