// Stand-alone check of the general-scale resize's host code (stereo.vision_amd/csrc/svx_resize_host.h): the
// coefficient tables, the layout of the table block the kernel reads, the argument checks of sv_resize_linear_u8 and
// the plan of sv_images_tile, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/resize_host_check.cpp -o x && ./x
// It touches no device: every table is written into a host allocation of exactly the layout's size, the way the
// upload fills the device one, and every source index a table holds is checked against the source it was made for,
// since the kernel checks none. Run it by hand on the development machine after a change to svx_resize_host.h; it is
// part of no test and is never run on a GPU machine.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../stereo.vision_amd/csrc/svx_resize_host.h"

using namespace svx;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);      \
            ++failures;                                              \
        }                                                            \
    } while (0)

static void check_axis(int dn, int sn) {
    std::vector<int32_t> s0(dn), s1(dn);   // exactly dn entries each: a write past them is the sanitizer's to find
    std::vector<int16_t> c0(dn), c1(dn);
    CHECK(resize_coefficients(dn, sn, s0.data(), s1.data(), c0.data(), c1.data()));
    bool ok = true;
    for (int i = 0; i < dn; ++i) {
        ok = ok && s0[i] >= 0 && s0[i] <= sn - 1 && s1[i] >= s0[i] && s1[i] <= sn - 1 && s1[i] - s0[i] <= 1;
        ok = ok && c0[i] >= 0 && c0[i] <= 2048 && c1[i] >= 0 && c1[i] <= 2048 && c0[i] + c1[i] >= 2047 &&
             c0[i] + c1[i] <= 2049;
        if (i) ok = ok && s0[i] >= s0[i - 1];
    }
    CHECK(ok);
    if (dn == sn) {   // the identity: every index its own, every weight whole
        for (int i = 0; i < dn; ++i) ok = ok && s0[i] == i && c0[i] == 2048 && c1[i] == 0;
        CHECK(ok);
    }
}

static void check_tables(int sh, int sw, int dh, int dw) {
    const ResizeTableLayout l = resize_table_layout(dh, dw);
    CHECK(l.xs0 == 0 && l.xs1 >= l.xs0 + 4 * (size_t)dw && l.xa0 >= l.xs1 + 4 * (size_t)dw);
    CHECK(l.xa1 >= l.xa0 + 2 * (size_t)dw && l.ys0 >= l.xa1 + 2 * (size_t)dw && l.ys1 >= l.ys0 + 4 * (size_t)dh);
    CHECK(l.yb0 >= l.ys1 + 4 * (size_t)dh && l.yb1 >= l.yb0 + 2 * (size_t)dh && l.bytes >= l.yb1 + 2 * (size_t)dh);
    for (size_t off : {l.xs0, l.xs1, l.xa0, l.xa1, l.ys0, l.ys1, l.yb0, l.yb1, l.bytes}) CHECK(off % 16 == 0);
    std::vector<uint8_t> block(l.bytes);
    CHECK(resize_fill_tables(block.data(), sh, sw, dh, dw));
    const int32_t* xs1 = reinterpret_cast<const int32_t*>(block.data() + l.xs1);
    const int32_t* ys1 = reinterpret_cast<const int32_t*>(block.data() + l.ys1);
    bool ok = true;
    for (int i = 0; i < dw; ++i) ok = ok && xs1[i] >= 0 && xs1[i] < sw;
    for (int i = 0; i < dh; ++i) ok = ok && ys1[i] >= 0 && ys1[i] < sh;
    CHECK(ok);
}

int main() {
    for (int dn = 1; dn <= 40; ++dn)
        for (int sn = 1; sn <= 40; ++sn) check_axis(dn, sn);
    const int axes[][2] = {{1024, 889}, {544, 390}, {889, 1024}, {390, 544}, {4095, 4096}, {4096, 8192}, {8192, 1},
                           {1, 8192}, {8192, 8192}};
    for (const auto& a : axes) check_axis(a[0], a[1]);
    {   // half to even: 3 -> 2 samples at 0.25 and 1.25: f = 0.25 -> 512 / 1536; the closed ramp of tile_numpy's test
        int32_t s0[6], s1[6];
        int16_t c0[6], c1[6];
        CHECK(resize_coefficients(6, 3, s0, s1, c0, c1));
        CHECK(s0[0] == 0 && c0[0] == 2048 && c1[0] == 0);                  // -0.25: clamped
        CHECK(s0[1] == 0 && s1[1] == 1 && c0[1] == 1536 && c1[1] == 512);  // 0.25
        CHECK(s0[5] == 2 && s1[5] == 2 && c0[5] == 2048 && c1[5] == 0);    // 2.25: clamped
        CHECK(!resize_coefficients(0, 3, s0, s1, c0, c1) && !resize_coefficients(3, 0, s0, s1, c0, c1));
        CHECK(!resize_coefficients(8193, 3, s0, s1, c0, c1) && !resize_coefficients(3, 8193, s0, s1, c0, c1));
        CHECK(!resize_coefficients(-1, 3, s0, s1, c0, c1) && !resize_coefficients(3, 3, nullptr, s1, c0, c1));
        CHECK(!resize_coefficients(3, 3, s0, s1, c0, nullptr));
    }
    const int shapes[][4] = {{1, 1, 1, 1}, {1, 1, 5, 7}, {2, 3, 7, 5}, {13, 17, 5, 4}, {390, 889, 544, 1024},
                             {544, 1024, 390, 889}, {3, 4096, 2, 4095}, {2, 8192, 2, 4096}, {8192, 8192, 4096, 4096},
                             {1088, 2048, 272, 512}};
    for (const auto& s : shapes) check_tables(s[0], s[1], s[2], s[3]);
    std::vector<uint8_t> small(64);
    CHECK(!resize_fill_tables(small.data(), 8, 8, 0, 4) && !resize_fill_tables(small.data(), 8, 8, 4, 4097));
    CHECK(!resize_fill_tables(nullptr, 8, 8, 4, 4));
    // sv_resize_linear_u8's arguments
    std::vector<uint8_t> mem(4096);
    uint8_t *src = mem.data(), *dst = mem.data() + 1024;
    CHECK(resize_check_args(src, 1, 8, 8, 1, dst, 5, 7) == nullptr && resize_check_args(src, 3, 8, 8, 3, dst, 16, 16) == nullptr);
    CHECK(resize_check_args(nullptr, 1, 8, 8, 1, dst, 5, 7) != nullptr && resize_check_args(src, 1, 8, 8, 1, nullptr, 5, 7) != nullptr);
    CHECK(resize_check_args(src, 0, 8, 8, 1, dst, 5, 7) != nullptr && resize_check_args(src, -1, 8, 8, 1, dst, 5, 7) != nullptr);
    CHECK(resize_check_args(src, 1, 8, 8, 2, dst, 5, 7) != nullptr && resize_check_args(src, 1, 8, 8, 0, dst, 5, 7) != nullptr);
    CHECK(resize_check_args(src, 1, 0, 8, 1, dst, 5, 7) != nullptr && resize_check_args(src, 1, 8, 8193, 1, dst, 5, 7) != nullptr);
    CHECK(resize_check_args(src, 1, 8, 8, 1, dst, 0, 7) != nullptr && resize_check_args(src, 1, 8, 8, 1, dst, 5, 4097) != nullptr);
    CHECK(resize_check_args(src, 1, 8, 8, 1, src + 63, 4, 4) != nullptr && resize_check_args(src, 1, 8, 8, 1, src + 64, 4, 4) == nullptr);
    CHECK(resize_check_args(src + 16, 1, 8, 8, 1, src, 4, 4) == nullptr && resize_check_args(src + 15, 1, 8, 8, 1, src, 4, 4) != nullptr);
    CHECK(resize_check_args(src, 2147483647, 8192, 8192, 3, dst, 4096, 4096) != nullptr);   // the byte counts do not wrap
    // the plan of batchImages
    ImagesTilePlan p;
    CHECK(images_tile_plan(1, 7, 9, &p) == nullptr && p.out_h == 7 && p.out_w == 9 && p.quadrants == 0);
    CHECK(images_tile_plan(2, 8, 9, &p) == nullptr && p.out_h == 4 && p.out_w == 9 && p.stack_h == 8 && p.stack_w == 18);
    CHECK(images_tile_plan(3, 7, 9, &p) == nullptr && p.out_h == 7 && p.out_w == 9 && p.pic_of[3] == 2 && p.stack_h == 14);
    CHECK(images_tile_plan(4, 7, 9, &p) == nullptr && p.out_h == 7 && p.pic_of[3] == 3 && p.quadrants == 4);
    CHECK(images_tile_plan(5, 6, 10, &p) == nullptr && p.out_h == 3 && p.out_w == 10 && p.left_h == 3 && p.left_w == 5);
    CHECK(images_tile_plan(5, 4096, 4096, &p) == nullptr && p.stack_h == 8192 && p.stack_w == 8192);
    CHECK(resize_check_shape(p.stack_h, p.stack_w, p.left_h, p.left_w) == nullptr);
    CHECK(images_tile_plan(2, 7, 8, &p) != nullptr && images_tile_plan(5, 8, 9, &p) != nullptr && images_tile_plan(5, 7, 8, &p) != nullptr);
    CHECK(images_tile_plan(0, 8, 8, &p) != nullptr && images_tile_plan(6, 8, 8, &p) != nullptr);
    CHECK(images_tile_plan(1, 0, 8, &p) != nullptr && images_tile_plan(1, 8, 4097, &p) != nullptr);
    CHECK(images_tile_plan(4, 8, 8, nullptr) == nullptr);
    if (failures) return 1;
    std::printf("resize host check ok\n");
    return 0;
}
