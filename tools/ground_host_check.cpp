// Stand-alone program over the ground grid's host code (stereo.vision_amd/csrc/svx_ground_host.h): the mapping the
// kernel looks up, the argument checks of sv_ground_grid and the layout of its results.
//   ground_host_check f B cw x0 z0 cell nx nz W     writes the mapping to stdout as raw little-endian int16: ix for
//                                                   every (d, x), d = 0..255 outer, x = 0..W-1 inner, then iz for
//                                                   every d, then the folded table the device holds, cell for
//                                                   every (d, x); -1 = outside the grid. Exit status 2 (and
//                                                   "refused: ..." on stderr) when the checks refuse the camera,
//                                                   the grid or W
//   ground_host_check                               the self-check below; "ground host check ok" and status 0
// tests/test_ground_cpu.py compiles it with the host compiler and compares the first form with the oracle's. It is
// also what the host sanitizers run, by hand on the development machine after a change to svx_ground_host.h:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       tools/ground_host_check.cpp -o x && ./x && ./x 399.9745178222656 0.2090607502 474.5 -8 0 0.25 64 128 1024 | wc -c
// It touches no device: every table is written into a host allocation of exactly the table's size, the way the
// upload fills the device one, and every index a table holds is checked against the grid it was made for, since
// the kernel checks none.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../stereo.vision_amd/csrc/svx_ground_host.h"

using namespace svx;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);      \
            ++failures;                                              \
        }                                                            \
    } while (0)

static void check_mapping(const sv_camera& cam, const sv_grid& g, int W) {
    std::vector<int16_t> ix((size_t)256 * W), iz(256);   // exactly the tables' sizes
    CHECK(ground_fill_mapping(cam, g, W, ix.data(), iz.data()));
    bool ok = iz[0] == -1;
    for (int d = 0; d < 256; ++d) {
        ok = ok && iz[d] >= -1 && iz[d] < g.nz;
        if (d > 1 && iz[d] >= 0 && iz[d - 1] >= 0) ok = ok && iz[d] <= iz[d - 1];   // nearer with d
        int last = -1;
        for (int x = 0; x < W; ++x) {
            const int v = ix[(size_t)d * W + x];
            ok = ok && v >= -1 && v < g.nx && (d > 0 || v == -1);
            if (v >= 0) {
                ok = ok && v >= last;   // non-decreasing in x
                last = v;
            }
        }
    }
    CHECK(ok);
    std::vector<int16_t> cell((size_t)256 * W);
    ground_fold_cells(ix.data(), iz.data(), W, g.nx, cell.data());
    for (int d = 0; d < 256; ++d)
        for (int x = 0; x < W; ++x) {
            const size_t i = (size_t)d * W + x;
            const int v = cell[i];   // what the kernel indexes its planes with
            ok = ok && v >= -1 && v < g.nx * g.nz && ((v < 0) == (ix[i] < 0 || iz[d] < 0));
            if (v >= 0) ok = ok && v / g.nx == iz[d] && v % g.nx == ix[i];
        }
    CHECK(ok);
}

static int self_check() {
    const sv_camera cams[] = {{399.9745178222656, 0.2090607502, 474.5, 262.0}, {401.25, 0.21, 36.0003, 22.0002},
                              {1203.9, 0.075, 100.00004, 47.99997}, {612.7, 0.12, -35.4, 700.9},
                              {401.25, 0.21, 500.3, 250.7}, {400.0, 0.25, 474.5, 262.0}};
    const sv_grid grids[] = {ground_default_grid(), {-8.0, 0.0, 16.0, 1, 1}, {-8.0, 0.0, 0.01, 8192, 1},
                             {-0.5, 0.0, 0.01, 1, 8192}, {1e6, 1e6, 0.25, 64, 128}, {0.0, 0.0, 0.25, 64, 128},
                             {-8.0, 0.0, 0.01, 64, 128}, {-1e300, -1e300, 1e-300, 3, 5}};
    const int widths[] = {2, 70, 889, 1024, 4096};
    for (const auto& c : cams)
        for (const auto& g : grids)
            for (int W : widths) check_mapping(c, g, W);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // closed forms: f B = 100 exactly, so d = 200 is Z = 0.5, on a cell edge at cell 0.25
    {
        const sv_camera c{400.0, 0.25, 474.5, 262.0};
        const sv_grid g = ground_default_grid();
        std::vector<int16_t> ix((size_t)256 * 1024), iz(256);
        CHECK(ground_fill_mapping(c, g, 1024, ix.data(), iz.data()));
        CHECK(iz[200] == 2 && iz[100] == 4 && iz[3] == -1 && iz[4] == 100);
        CHECK(ix[(size_t)200 * 1024 + 394] == 31);   // X = (394 - 474.5) * 0.5 / 400 = -0.100625
        sv_grid g0 = g;
        g0.x0 = 0.0;
        CHECK(ground_fill_mapping(c, g0, 1024, ix.data(), iz.data()));
        CHECK(ix[(size_t)200 * 1024 + 394] == -1 && ix[(size_t)200 * 1024 + 475] == 0);
    }
    // the checks
    sv_grid g = ground_default_grid();
    CHECK(ground_check_grid(g) == nullptr);
    for (double bad : {0.0, -0.25, inf, nan}) {
        sv_grid b = g;
        b.cell = bad;
        CHECK(ground_check_grid(b) != nullptr);
    }
    for (double bad : {inf, -inf, nan}) {
        sv_grid b = g;
        b.x0 = bad;
        CHECK(ground_check_grid(b) != nullptr);
        b = g;
        b.z0 = bad;
        CHECK(ground_check_grid(b) != nullptr);
    }
    const int dims[][3] = {{0, 1, 0}, {1, 0, 0}, {-1, 4, 0}, {8193, 1, 0}, {1, 8193, 0}, {4097, 2, 0}, {65536, 65536, 0},
                           {2147483647, 2147483647, 0}, {8192, 1, 1}, {1, 8192, 1}, {64, 128, 1}, {1, 1, 1}};
    for (const auto& d : dims) {
        sv_grid b = g;
        b.nx = d[0];
        b.nz = d[1];
        CHECK((ground_check_grid(b) == nullptr) == (d[2] == 1));
    }
    sv_camera cam{399.9745178222656, 0.2090607502, 474.5, 262.0};
    CHECK(ground_check_camera(cam) == nullptr);
    for (double bad : {0.0, -1.0, inf, nan}) {
        sv_camera c = cam;
        c.f = bad;
        CHECK(ground_check_camera(c) != nullptr);
        c = cam;
        c.B = bad;
        CHECK(ground_check_camera(c) != nullptr);
    }
    int mem[8];
    const void* p = mem;
    CHECK(ground_check_args(p, p, 40, 70, &cam, nullptr, 1, p, p, p) == nullptr);
    CHECK(ground_check_args(p, p, 40, 70, &cam, &g, 1, p, p, p) == nullptr);
    CHECK(ground_check_args(nullptr, p, 40, 70, &cam, &g, 1, p, p, p) != nullptr);
    CHECK(ground_check_args(p, nullptr, 40, 70, &cam, &g, 1, p, p, p) != nullptr);
    CHECK(ground_check_args(p, p, 40, 70, nullptr, &g, 1, p, p, p) != nullptr);
    CHECK(ground_check_args(p, p, 40, 70, &cam, &g, 1, nullptr, p, p) != nullptr);
    CHECK(ground_check_args(p, p, 40, 70, &cam, &g, 1, p, nullptr, p) != nullptr);
    CHECK(ground_check_args(p, p, 40, 70, &cam, &g, 1, p, p, nullptr) != nullptr);
    CHECK(ground_check_args(p, p, 0, 70, &cam, &g, 1, p, p, p) != nullptr);
    CHECK(ground_check_args(p, p, 4097, 70, &cam, &g, 1, p, p, p) != nullptr);
    CHECK(ground_check_args(p, p, 40, 1, &cam, &g, 1, p, p, p) != nullptr);
    CHECK(ground_check_args(p, p, 40, 4097, &cam, &g, 1, p, p, p) != nullptr);
    CHECK(ground_check_args(p, p, 40, 70, &cam, &g, 0, p, p, p) != nullptr);
    // refused mappings write nothing (null tables would be the sanitizer's to find)
    sv_grid big = g;
    big.nx = 8193;
    big.nz = 1;
    CHECK(!ground_fill_mapping(cam, big, 70, nullptr, nullptr));
    std::vector<int16_t> ix((size_t)256 * 70), iz(256);
    CHECK(!ground_fill_mapping(cam, big, 70, ix.data(), iz.data()));
    CHECK(!ground_fill_mapping(cam, g, 1, ix.data(), iz.data()) && !ground_fill_mapping(cam, g, 4097, ix.data(), iz.data()));
    // the layout: frames x (2 nx nz + nx + 4) words
    const GroundLayout l = ground_layout(g, 4096);
    CHECK(l.cells == 8192 && l.off_nearest == (size_t)2 * 8192 * 4096 && l.off_info == l.off_nearest + (size_t)64 * 4096);
    CHECK(l.bytes == (size_t)4096 * (2 * 8192 + 64 + 4) * 4);
    CHECK(ground_map_bytes(1024) == (size_t)512 * 1024);
    if (failures) return 1;
    std::printf("ground host check ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return self_check();
    if (argc != 10) {
        std::fprintf(stderr, "usage: %s [f B cw x0 z0 cell nx nz W]\n", argv[0]);
        return 64;
    }
    const sv_camera cam{std::strtod(argv[1], nullptr), std::strtod(argv[2], nullptr), std::strtod(argv[3], nullptr), 0.0};
    const sv_grid g{std::strtod(argv[4], nullptr), std::strtod(argv[5], nullptr), std::strtod(argv[6], nullptr),
                    (int32_t)std::strtol(argv[7], nullptr, 10), (int32_t)std::strtol(argv[8], nullptr, 10)};
    const long W = std::strtol(argv[9], nullptr, 10);
    const char* why = ground_check_grid(g);
    if (!why) why = ground_check_camera(cam);
    if (!why && (W < 2 || W > 4096)) why = "2 <= W <= 4096";
    if (why) {
        std::fprintf(stderr, "refused: %s\n", why);
        return 2;
    }
    std::vector<int16_t> ix((size_t)256 * W), iz(256);
    if (!ground_fill_mapping(cam, g, (int)W, ix.data(), iz.data())) return 2;
    if (std::fwrite(ix.data(), sizeof(int16_t), ix.size(), stdout) != ix.size()) return 1;
    if (std::fwrite(iz.data(), sizeof(int16_t), iz.size(), stdout) != iz.size()) return 1;
    std::vector<int16_t> cell((size_t)256 * W);
    ground_fold_cells(ix.data(), iz.data(), (int)W, g.nx, cell.data());
    if (std::fwrite(cell.data(), sizeof(int16_t), cell.size(), stdout) != cell.size()) return 1;
    return 0;
}
