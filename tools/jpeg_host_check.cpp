// Stand-alone check of the JPEG encoder's host code (stereo.vision_amd/csrc/svx_jpeg_host.h): the argument checks of
// sv_jpeg_encode, the capacity bound, the tables the kernels read (quantiser words, Huffman codes), the header's
// segments and the layout of a chunk's device scratch, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp -o x && ./x
// It touches no device: every part of a layout is written to its last byte in a host allocation of the layout's
// size. Run it by hand on the development machine after a change to svx_jpeg_host.h; it is part of no test and is
// never run on a GPU machine.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../stereo.vision_amd/csrc/svx_jpeg_host.h"

using namespace svx;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);      \
            ++failures;                                              \
        }                                                            \
    } while (0)

// the header's segments in order, their lengths adding up to header_len
static void check_header(int h, int w, int quality) {
    JpegConst c;
    jpeg_build(h, w, quality, &c);
    CHECK(c.header_len == 629 && c.header_len <= kJpegHeaderMax);
    const uint8_t* p = c.header;
    CHECK(p[0] == 0xFF && p[1] == 0xD8);
    const int want[10] = {0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA};
    int i = 2;
    for (int k = 0; k < 10; ++k) {
        CHECK(i + 4 <= c.header_len && p[i] == 0xFF && p[i + 1] == want[k]);
        const int n = p[i + 2] << 8 | p[i + 3];
        if (want[k] == 0xC0) CHECK((p[i + 5] << 8 | p[i + 6]) == h && (p[i + 7] << 8 | p[i + 8]) == w);
        if (want[k] == 0xDD) CHECK((p[i + 4] << 8 | p[i + 5]) == jpeg_mcu_cols(w));
        if (want[k] == 0xDB)
            for (int z = 0; z < 64; ++z) CHECK(p[i + 5 + z] >= 1);
        i += 2 + n;
    }
    CHECK(i == c.header_len);
    // the quantiser words: r | q << 21, and the multiply-and-shift is the division for every |c| < 2^14
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            const uint32_t e = c.quant[t][k], q = e >> 21, r = e & 0x1FFFFFu;
            const int base = t ? jpeg_tables::kChroma[k] : jpeg_tables::kLuma[k];
            CHECK((int)q == jpeg_quant_entry(base, quality) && q >= 1 && q <= 255 && r == (1u << 20) / q + 1);
            for (uint32_t a = 0; a < (1u << 14); a += (k == 0 ? 1 : 37)) {
                const uint64_t prod = (uint64_t)((a + 4 * q) >> 3) * r;
                CHECK(prod < (1ull << 32) && (prod >> 20) == (a + ((8 * q) >> 1)) / (8 * q));
            }
        }
    // the Huffman codes: every symbol of a table has a code of 1 .. 16 bits, no code is all ones, Kraft's sum < 1
    const int dc_syms = 12;
    for (int t = 0; t < 2; ++t) {
        double kraft = 0;
        for (int s = 0; s < dc_syms; ++s) {
            const uint32_t len = c.dc[t][s] >> 16, code = c.dc[t][s] & 0xFFFF;
            CHECK(len >= 1 && len <= 16 && code < (1u << len) - 1);
            kraft += 1.0 / (double)(1u << len);
        }
        CHECK(kraft < 1.0);
        int n = 0;
        kraft = 0;
        for (int s = 0; s < 256; ++s) {
            const uint32_t len = c.ac[t][s] >> 16, code = c.ac[t][s] & 0xFFFF;
            if (!len) continue;
            ++n;
            CHECK(len <= 16 && code < (1u << len) - 1);
            kraft += 1.0 / (double)(1u << len);
        }
        CHECK(n == 162 && kraft < 1.0);
        CHECK(c.ac[t][0x00] >> 16 && c.ac[t][0xF0] >> 16);
        for (int run = 0; run < 16; ++run)
            for (int size = 1; size <= 10; ++size) CHECK(c.ac[t][run << 4 | size] >> 16);
    }
}

static void check_layout(int h, int w, int frames) {
    const JpegWorkLayout l = jpeg_work_layout(h, w, frames);
    const size_t mr = (size_t)jpeg_mcu_rows(h), mc = (size_t)jpeg_mcu_cols(w), f = (size_t)frames;
    CHECK(l.off_coef == 0 && l.off_lane >= f * mr * mc * 768 && l.off_ilen >= l.off_lane + f * mr * 512);
    CHECK(l.off_ioff >= l.off_ilen + f * mr * 4 && l.bytes >= l.off_ioff + f * mr * 4);
    CHECK(l.off_lane % 16 == 0 && l.off_ilen % 16 == 0 && l.off_ioff % 16 == 0);
    CHECK(l.bytes <= f * (jpeg_work_frame_bytes(h, w) + 64));
    std::vector<unsigned char> buf(l.bytes);
    std::memset(buf.data() + l.off_coef, 1, f * mr * mc * 768);
    std::memset(buf.data() + l.off_lane, 2, f * mr * 512);
    std::memset(buf.data() + l.off_ilen, 3, f * mr * 4);
    std::memset(buf.data() + l.off_ioff, 4, f * mr * 4);
    CHECK(buf[l.off_lane - 1] != 2 && buf[l.off_lane] == 2 && buf[l.off_ilen] == 3 && buf[l.off_ioff + f * mr * 4 - 1] == 4);
}

int main() {
    unsigned char px[4] = {0, 0, 0, 0}, out[4];
    long long size = 0;
    CHECK(jpeg_check_args(px, 1, 1, 3, 75, out, 4, &size) == nullptr);
    CHECK(jpeg_check_args(px, 4096, 4096, 3 * 4096, 1, out, 0, &size) == nullptr);
    CHECK(jpeg_check_args(nullptr, 1, 1, 3, 75, out, 4, &size) != nullptr);
    CHECK(jpeg_check_args(px, 1, 1, 3, 75, nullptr, 4, &size) != nullptr);
    CHECK(jpeg_check_args(px, 1, 1, 3, 75, out, 4, nullptr) != nullptr);
    CHECK(jpeg_check_args(px, 0, 1, 3, 75, out, 4, &size) != nullptr && jpeg_check_args(px, 1, 0, 3, 75, out, 4, &size) != nullptr);
    CHECK(jpeg_check_args(px, 4097, 1, 3, 75, out, 4, &size) != nullptr);
    CHECK(jpeg_check_args(px, 1, 4097, 3 * 4097, 75, out, 4, &size) != nullptr);
    CHECK(jpeg_check_args(px, 1, 1, 2, 75, out, 4, &size) != nullptr && jpeg_check_args(px, 1, 1, 3, 0, out, 4, &size) != nullptr);
    CHECK(jpeg_check_args(px, 1, 1, 3, 101, out, 4, &size) != nullptr && jpeg_check_args(px, 1, 1, 3, 75, out, -1, &size) != nullptr);
    CHECK(jpeg_check_args(px, 2147483647, 2147483647, 3, 75, out, 4, &size) != nullptr);
    CHECK(jpeg_bound(0, 1) == 0 && jpeg_bound(1, 4097) == 0 && jpeg_bound(-1, -1) == 0);
    CHECK(jpeg_bound(1, 1) == 640 + 2 * 1244 + 2 && jpeg_bound(16, 16) == jpeg_bound(1, 1) && jpeg_bound(17, 16) > jpeg_bound(16, 16));
    CHECK(jpeg_bound(4096, 4096) == 640 + 256ll * (2 * 1244ll * 256 + 2) && jpeg_bound(4096, 4096) < (1ll << 31));
    CHECK(jpeg_quant_entry(16, 50) == 16 && jpeg_quant_entry(16, 100) == 1 && jpeg_quant_entry(99, 1) == 255);
    CHECK(jpeg_quant_entry(16, 75) == 8 && jpeg_quant_entry(17, 30) == (17 * 166 + 50) / 100);
    CHECK(jpeg_default_cap(272, 1024) == 272 * 1024 * 3 / 2 && jpeg_default_cap(2, 2) == 2048);
    const int shapes[][2] = {{1, 1}, {8, 8}, {17, 33}, {36, 1024}, {272, 1024}, {4096, 4096}};
    for (const auto& s : shapes)
        for (int q : {1, 30, 49, 50, 75, 100}) check_header(s[0], s[1], q);
    const int lay[][3] = {{1, 1, 1}, {17, 33, 3}, {36, 1024, 5}, {272, 1024, 7}, {4096, 4096, 1}, {20, 76, 2}};
    for (const auto& s : lay) check_layout(s[0], s[1], s[2]);
    if (failures) return 1;
    std::printf("jpeg host check ok\n");
    return 0;
}
