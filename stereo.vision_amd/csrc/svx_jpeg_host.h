// Host-only part of the MJPG recording's JPEG encoder (rt_jpeg.hip; loop.py:49-54,82-89): the argument checks, the
// capacity bound, the quantisation and Huffman tables the kernels read, and the stream's header, assembled once per
// (h, w, quality). No HIP in here, so that tools/jpeg_host_check.cpp can run it under the host sanitizers without a
// device (by hand, on the development machine only). The stream is defined in DESIGN §7.11 and restated in
// tests/jpeg_numpy.py.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace svx {

constexpr int kJpegMaxDim = 4096;      // rows and columns of a picture
constexpr int kJpegHeaderMax = 640;    // SOI .. SOS of this encoder is 629 bytes
// Worst case of one MCU before stuffing: a DC code and its bits are at most 9 + 11 (luma) and 11 + 11 (chroma)
// bits, each of the 63 AC coefficients at most a 16-bit code and 10 value bits (|AC| <= 1023 at q = 1), so
// 4 (20 + 63 * 26) + 2 (22 + 63 * 26) = 9952 bits = 1244 bytes exactly.
constexpr int kJpegMcuMaxBytes = 1244;
constexpr int kJpegRecipShift = 20;

// What the kernels read, copied to the device as it stands.
struct JpegConst {
    // per table (0 luma, 1 chroma) and natural position: r | q << 21 with r = floor(2^20 / q) + 1, so that the
    // quantiser's (|c| + 4 q) / (8 q) is (((|c| + 4 q) >> 3) * r) >> 20 in 32 bits (tests/test_jpeg_cpu.py proves it
    // for every |c| < 2^14 and every q)
    uint32_t quant[2][64];
    uint32_t dc[2][12];     // code | length << 16 by size category
    uint32_t ac[2][256];    // code | length << 16 by run << 4 | size
    int32_t header_len;
    uint8_t header[kJpegHeaderMax];
};

namespace jpeg_tables {
// Annex K.1, K.2 (natural order)
constexpr uint8_t kLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                               14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                               18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// natural index of zig-zag position k
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.3 - K.6: BITS (code lengths 1..16) and HUFFVAL (as hex)
constexpr uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
constexpr uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr char kDcVals[] = "000102030405060708090a0b";
constexpr char kAcLumaVals[] =
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f0"
    "2433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a"
    "92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa";
constexpr char kAcChromaVals[] =
    "000102031104052131061241510761711322328108144291a1b1c109233352f0"
    "156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a828384858687"
    "88898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa";

inline int hex_digit(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
// the n symbols of a hex string
inline int hex_vals(const char* hex, uint8_t* out) {
    int n = 0;
    for (; hex[2 * n] && hex[2 * n + 1]; ++n) out[n] = (uint8_t)(hex_digit(hex[2 * n]) * 16 + hex_digit(hex[2 * n + 1]));
    return n;
}
}  // namespace jpeg_tables

// the IJG quality rule on an Annex K entry
inline int jpeg_quant_entry(int base, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (base * scale + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}

inline int jpeg_mcu_rows(int h) { return (h + 15) / 16; }
inline int jpeg_mcu_cols(int w) { return (w + 15) / 16; }

// A capacity no stream of this definition exceeds: the header, and for every restart interval (an MCU row) its
// MCUs' worst code lengths (kJpegMcuMaxBytes each, a whole number of bytes), every byte of them stuffed, and the two
// bytes of the RSTn or EOI behind it. 0 for dimensions outside 1 .. 4096.
inline int64_t jpeg_bound(int h, int w) {
    if (h < 1 || h > kJpegMaxDim || w < 1 || w > kJpegMaxDim) return 0;
    return kJpegHeaderMax + (int64_t)jpeg_mcu_rows(h) * (2 * (int64_t)kJpegMcuMaxBytes * jpeg_mcu_cols(w) + 2);
}

// nullptr when sv_jpeg_encode's arguments are in range, else what is wrong with them
inline const char* jpeg_check_args(const void* bgr, int h, int w, int64_t ld, int quality, const void* out,
                                   int64_t cap, const void* size) {
    if (!bgr || !out || !size) return "null pointer";
    if (h < 1 || h > kJpegMaxDim || w < 1 || w > kJpegMaxDim) return "1 <= h, w <= 4096";
    if (quality < 1 || quality > 100) return "1 <= quality <= 100";
    if (ld < 3 * (int64_t)w) return "ld >= 3 w bytes";
    if (cap < 0) return "cap >= 0";
    return nullptr;
}

namespace jpeg_detail {
struct Writer {
    uint8_t* p;
    int n = 0, cap;
    void byte(int v) {
        if (n < cap) p[n] = (uint8_t)v;
        ++n;
    }
    void be16(int v) { byte(v >> 8), byte(v & 255); }
    void marker(int m, int payload) { byte(0xFF), byte(m), be16(payload + 2); }
};

// Annex C: the codes of a table in the order of its symbols; code | length << 16 at out[symbol]
inline void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) out[vals[k++]] = code++ | (uint32_t)len << 16;
        code <<= 1;
    }
}
}  // namespace jpeg_detail

// The tables and the header of an h x w stream at `quality` (arguments in range). Header: SOI, JFIF APP0, DQT x 2,
// SOF0 (Y 2 x 2 on table 0, Cb and Cr 1 x 1 on table 1), DHT x 4, DRI = MCUs a row, SOS.
inline void jpeg_build(int h, int w, int quality, JpegConst* c) {
    using namespace jpeg_tables;
    memset(c, 0, sizeof *c);
    uint8_t q[2][64];
    for (int i = 0; i < 64; ++i) {
        q[0][i] = (uint8_t)jpeg_quant_entry(kLuma[i], quality);
        q[1][i] = (uint8_t)jpeg_quant_entry(kChroma[i], quality);
        for (int t = 0; t < 2; ++t) c->quant[t][i] = ((1u << kJpegRecipShift) / q[t][i] + 1) | (uint32_t)q[t][i] << 21;
    }
    uint8_t dcv[12], acl[162], acc[162];
    hex_vals(kDcVals, dcv);
    hex_vals(kAcLumaVals, acl);
    hex_vals(kAcChromaVals, acc);
    const uint8_t* bits[4] = {kDcLumaBits, kAcLumaBits, kDcChromaBits, kAcChromaBits};
    const uint8_t* vals[4] = {dcv, acl, dcv, acc};
    const int count[4] = {12, 162, 12, 162};
    const int ids[4] = {0x00, 0x10, 0x01, 0x11};
    jpeg_detail::huff_codes(bits[0], vals[0], c->dc[0]);
    jpeg_detail::huff_codes(bits[2], vals[2], c->dc[1]);
    jpeg_detail::huff_codes(bits[1], vals[1], c->ac[0]);
    jpeg_detail::huff_codes(bits[3], vals[3], c->ac[1]);
    jpeg_detail::Writer o{c->header, 0, kJpegHeaderMax};
    o.byte(0xFF), o.byte(0xD8);
    o.marker(0xE0, 14);
    for (const char* s = "JFIF"; *s; ++s) o.byte(*s);
    o.byte(0), o.byte(1), o.byte(1), o.byte(0), o.be16(1), o.be16(1), o.byte(0), o.byte(0);
    for (int t = 0; t < 2; ++t) {
        o.marker(0xDB, 65);
        o.byte(t);
        for (int k = 0; k < 64; ++k) o.byte(q[t][kZigzag[k]]);
    }
    o.marker(0xC0, 15);
    o.byte(8), o.be16(h), o.be16(w), o.byte(3);
    o.byte(1), o.byte(0x22), o.byte(0);
    o.byte(2), o.byte(0x11), o.byte(1);
    o.byte(3), o.byte(0x11), o.byte(1);
    for (int t = 0; t < 4; ++t) {
        o.marker(0xC4, 17 + count[t]);
        o.byte(ids[t]);
        for (int i = 0; i < 16; ++i) o.byte(bits[t][i]);
        for (int i = 0; i < count[t]; ++i) o.byte(vals[t][i]);
    }
    o.marker(0xDD, 2);
    o.be16(jpeg_mcu_cols(w));
    o.marker(0xDA, 10);
    o.byte(3), o.byte(1), o.byte(0x00), o.byte(2), o.byte(0x11), o.byte(3), o.byte(0x11), o.byte(0), o.byte(63), o.byte(0);
    c->header_len = o.n;
}

// ---- the device scratch of a chunk of frames (kernels/jpeg.hip), all 16-byte aligned ----
struct JpegWorkLayout {
    size_t off_coef = 0, off_lane = 0, off_ilen = 0, off_ioff = 0, bytes = 0;
};
// bytes of one frame's scratch: int16 coefficients in MCU order (3 B a pixel of the padded picture), two words a
// lane of every interval's wave, an interval's length and offset
inline size_t jpeg_work_frame_bytes(int h, int w) {
    const size_t mr = (size_t)jpeg_mcu_rows(h), mc = (size_t)jpeg_mcu_cols(w);
    return mr * mc * 768 + mr * (64 * 8 + 8);
}
inline JpegWorkLayout jpeg_work_layout(int h, int w, int frames) {
    const size_t mr = (size_t)jpeg_mcu_rows(h), mc = (size_t)jpeg_mcu_cols(w), f = (size_t)frames;
    const auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    JpegWorkLayout l;
    l.off_coef = 0;
    l.off_lane = up16(f * mr * mc * 768);
    l.off_ilen = l.off_lane + up16(f * mr * 64 * 8);
    l.off_ioff = l.off_ilen + up16(f * mr * 4);
    l.bytes = l.off_ioff + up16(f * mr * 4);
    return l;
}

// the default slot of a batch's streams: half the raw picture (noise at quality 75 takes 0.20 of it), at least the
// header and a little
inline int64_t jpeg_default_cap(int h, int w) {
    const int64_t half = (int64_t)h * w * 3 / 2;
    return half < 2048 ? 2048 : (half + 15) / 16 * 16;
}

}  // namespace svx
