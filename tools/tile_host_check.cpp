// Stand-alone check of the image tile's host code (stereo.vision_amd/csrc/svx_tile_host.h): the shape and argument
// checks of sv_image_tile / sv_batch_tile, the size of a tile and the layout of the host entry's device buffer, for
// the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/tile_host_check.cpp -o x && ./x
// It touches no device: every part of a layout is written to its last byte in a host allocation of the layout's
// size, the way the copies and the kernel fill the device one. Run it by hand on the development machine after a
// change to svx_tile_host.h; it is part of no test and is never run on a GPU machine.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../stereo.vision_amd/csrc/svx_tile_host.h"

using namespace svx;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);      \
            ++failures;                                              \
        }                                                            \
    } while (0)

static void check_layout(int H, int W) {
    const TileLayout l = tile_layout(H, W);
    const size_t tile = tile_frame_bytes(H, W);
    CHECK(tile == (size_t)(H / 2) * 3 * (size_t)W);
    CHECK(l.pitch >= W && l.pitch % 8 == 0 && l.pitch < W + 8 && l.ld3 == 3 * l.pitch);
    CHECK(l.img >= (size_t)H * l.ld3 && l.img % 16 == 0);
    CHECK(l.off_res == 0 && l.off_out >= l.img && l.off_out % 16 == 0 && l.bytes >= l.off_out + tile);
    std::vector<unsigned char> buf(l.bytes);   // both parts, to their last byte
    std::memset(buf.data() + l.off_res, 1, (size_t)H * l.ld3);
    std::memset(buf.data() + l.off_out, 2, tile);
    CHECK(buf[0] == 1 && buf[(size_t)H * l.ld3 - 1] == 1 && buf[l.off_out] == 2 && buf[l.off_out + tile - 1] == 2);
}

int main() {
    CHECK(tile_check_shape(4, 4) == nullptr && tile_check_shape(544, 1024) == nullptr);
    CHECK(tile_check_shape(4096, 4096) == nullptr && tile_check_shape(40, 76) == nullptr);
    CHECK(tile_check_shape(390, 889) != nullptr && tile_check_shape(390, 888) != nullptr);
    CHECK(tile_check_shape(392, 889) != nullptr && tile_check_shape(0, 8) != nullptr && tile_check_shape(8, 0) != nullptr);
    CHECK(tile_check_shape(4100, 8) != nullptr && tile_check_shape(8, 4100) != nullptr);
    CHECK(tile_check_shape(-4, 8) != nullptr && tile_check_shape(8, -4) != nullptr);
    CHECK(tile_check_shape(2147483644, 2147483644) != nullptr && tile_check_shape(2, 2) != nullptr);
    // sv_image_tile's arguments: 8 x 8 pictures side by side in one allocation
    const int H = 8, W = 8;
    const size_t px = (size_t)H * W;
    std::vector<unsigned char> mem(9 * px + tile_frame_bytes(H, W));
    unsigned char *disp = mem.data(), *bgr = disp + px, *road = bgr + 3 * px, *clean = road + px, *res = clean + px;
    unsigned char* out = res + 3 * px;
    CHECK(tile_check_args(disp, bgr, road, clean, res, H, W, out) == nullptr);
    CHECK(tile_check_args(disp, bgr, road, road, res, H, W, out) == nullptr);      // inputs may share memory
    CHECK(tile_check_args(nullptr, bgr, road, clean, res, H, W, out) != nullptr);
    CHECK(tile_check_args(disp, nullptr, road, clean, res, H, W, out) != nullptr);
    CHECK(tile_check_args(disp, bgr, nullptr, clean, res, H, W, out) != nullptr);
    CHECK(tile_check_args(disp, bgr, road, nullptr, res, H, W, out) != nullptr);
    CHECK(tile_check_args(disp, bgr, road, clean, nullptr, H, W, out) != nullptr);
    CHECK(tile_check_args(disp, bgr, road, clean, res, H, W, nullptr) != nullptr);
    CHECK(tile_check_args(disp, bgr, road, clean, res, 6, W, out) != nullptr);
    CHECK(tile_check_args(disp, bgr, road, clean, res, H, 10, out) != nullptr);
    CHECK(tile_check_args(disp, bgr, road, clean, res, 0, W, out) != nullptr);
    CHECK(tile_check_args(disp, bgr, road, clean, res, H, 4100, out) != nullptr);
    // out over the last byte of an input, over its first, and just clear of both
    CHECK(tile_check_args(disp, bgr, road, clean, res, H, W, res + 3 * px - 1) != nullptr);
    CHECK(tile_check_args(disp, bgr, road, clean, res, H, W, disp) != nullptr);
    CHECK(tile_check_args(disp, bgr, road, clean, res, H, W, bgr + 1) != nullptr);
    CHECK(tile_check_args(disp, bgr, road, clean, res, H, W, clean + px - 1) != nullptr);
    CHECK(tile_check_args(bgr, bgr, bgr, bgr, bgr, H, W, out) == nullptr);
    CHECK(tile_overlap(disp, 4, disp + 3, 4) && !tile_overlap(disp, 4, disp + 4, 4) && !tile_overlap(disp + 4, 4, disp, 4));
    const int shapes[][2] = {{4, 4}, {8, 12}, {40, 76}, {64, 96}, {72, 1024}, {544, 1024}, {4, 4096}, {4096, 4},
                             {4096, 4096}, {12, 36}, {20, 2064}};
    for (const auto& s : shapes) check_layout(s[0], s[1]);
    if (failures) return 1;
    std::printf("tile host check ok\n");
    return 0;
}
