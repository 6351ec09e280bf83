// Stand-alone check of the JPEG decoder's host code (stereo.vision_amd/csrc/svx_jpeg_dec_host.h): the segment parser,
// the Huffman decode tables, the interval ranges, the entropy walk of an interval (the function the entropy kernel
// runs a lane an interval) and the layout of a chunk's device scratch, for the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_decode_host_check.cpp -o x && ./x
// Inputs: valid streams built here (this project's encoder tables, Annex K without DHT, several restart intervals),
// every prefix of one of them, a few thousand single-byte corruptions from a fixed seed, and the malformed scans of
// tests/test_jpeg_decode_cpu.py (a scan cut in the middle, a missing RST, swapped RST indices, a code outside the
// table). Every stream is copied into an allocation of exactly its size, so a read past it is an error, and the
// walk writes its blocks into an allocation of exactly the interval's coefficients. It touches no device. Run it by
// hand on the development machine after a change to svx_jpeg_dec_host.h; it is part of no test and is never run on a
// GPU machine.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#define SVX_JPEG_HD
#include "../stereo.vision_amd/csrc/svx_jpeg_dec_host.h"

using namespace svx;

static int failures = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED %s (line %d)\n", #c, __LINE__);      \
            ++failures;                                              \
        }                                                            \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// ---- a small encoder: random coefficients through the Annex K tables, restart interval `ri` MCUs ----
struct BitWriter {
    std::vector<uint8_t>& out;
    uint64_t acc = 0;
    int n = 0;
    void put(uint32_t bits, int len) {
        acc = acc << len | bits;
        n += len;
        while (n >= 8) {
            n -= 8;
            const uint8_t b = (uint8_t)(acc >> n);
            out.push_back(b);
            if (b == 0xFF) out.push_back(0);
        }
    }
    void flush() {
        if (n) put((1u << (8 - n)) - 1u, 8 - n);
    }
};

static int size_of(int v) {
    int a = v < 0 ? -v : v, s = 0;
    while (a) ++s, a >>= 1;
    return s;
}

// the stream of h x w with random coefficients (density: one in `sparse` is non-zero); coef (when not null) gets
// the coefficients, MCU order, zig-zag
static std::vector<uint8_t> make_stream(int h, int w, int quality, int ri, bool with_dht, int sparse,
                                        std::vector<int16_t>* coef) {
    JpegConst c;
    jpeg_build(h, w, quality, &c);
    std::vector<uint8_t> s;
    // the encoder's header, with its DRI replaced and optionally without the DHT segments
    for (int i = 0; i < 2; ++i) s.push_back(c.header[i]);
    for (int i = 2; i < c.header_len;) {
        const int m = c.header[i + 1], n = c.header[i + 2] << 8 | c.header[i + 3];
        if (m == 0xDD) {
            if (ri) {
                const uint8_t dri[6] = {0xFF, 0xDD, 0, 4, (uint8_t)(ri >> 8), (uint8_t)ri};
                s.insert(s.end(), dri, dri + 6);
            }
        } else if (m != 0xC4 || with_dht) {
            s.insert(s.end(), c.header + i, c.header + i + 2 + n);
        }
        i += 2 + n;
    }
    const int mcus = jpeg_mcu_rows(h) * jpeg_mcu_cols(w);
    if (coef) coef->assign((size_t)mcus * 384, 0);
    const int per = ri ? ri : mcus;
    int rst = 0;
    for (int m0 = 0; m0 < mcus; m0 += per) {
        BitWriter bw{s};
        int pred[3] = {0, 0, 0};
        for (int m = m0; m < m0 + per && m < mcus; ++m)
            for (int k = 0; k < 6; ++k) {
                const int comp = k < 4 ? 0 : k - 3, tab = k < 4 ? 0 : 1;
                int blk[64];
                for (int z = 0; z < 64; ++z) blk[z] = rnd() % sparse ? 0 : (int)(rnd() % 2047) - 1023;
                blk[0] = (int)(rnd() % 2047) - 1023;
                if (coef)
                    for (int z = 0; z < 64; ++z) (*coef)[((size_t)m * 6 + k) * 64 + z] = (int16_t)blk[z];
                const int diff = blk[0] - pred[comp];
                pred[comp] = blk[0];
                int sz = size_of(diff);
                bw.put(c.dc[tab][sz] & 0xFFFF, (int)(c.dc[tab][sz] >> 16));
                if (sz) bw.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << sz) - 1u), sz);
                int run = 0;
                for (int z = 1; z < 64; ++z) {
                    if (!blk[z]) {
                        ++run;
                        continue;
                    }
                    for (; run > 15; run -= 16) bw.put(c.ac[tab][0xF0] & 0xFFFF, (int)(c.ac[tab][0xF0] >> 16));
                    sz = size_of(blk[z]);
                    const uint32_t e = c.ac[tab][run << 4 | sz];
                    bw.put(e & 0xFFFF, (int)(e >> 16));
                    bw.put((uint32_t)(blk[z] < 0 ? blk[z] - 1 : blk[z]) & ((1u << sz) - 1u), sz);
                    run = 0;
                }
                if (run) bw.put(c.ac[tab][0] & 0xFFFF, (int)(c.ac[tab][0] >> 16));
            }
        bw.flush();
        if (m0 + per < mcus) s.push_back(0xFF), s.push_back((uint8_t)(0xD0 + (rst++ & 7)));
    }
    s.push_back(0xFF), s.push_back(0xD9);
    return s;
}

// Parse and walk one stream held in an allocation of exactly its size. Returns the parser's refusal (-1) or the
// frame's status; got (when not null): the coefficients.
static int decode(const std::vector<uint8_t>& stream, std::vector<int16_t>* got) {
    std::unique_ptr<uint8_t[]> buf(new uint8_t[stream.size() ? stream.size() : 1]);
    if (!stream.empty()) std::memcpy(buf.get(), stream.data(), stream.size());
    JpegDecHeader hd;
    JpegDecTables t;
    JpegDecQuant q;
    if (jpeg_dec_parse(buf.get(), (int64_t)stream.size(), &hd, &t, &q)) return -1;
    CHECK(hd.scan_at <= (int)stream.size() && hd.intervals >= 1 && hd.per >= 1);
    const int mcus = jpeg_mcu_rows(hd.h) * jpeg_mcu_cols(hd.w);
    CHECK((int64_t)hd.intervals * hd.per >= mcus && (int64_t)(hd.intervals - 1) * hd.per < mcus);
    std::vector<int32_t> first((size_t)hd.intervals, -7), end((size_t)hd.intervals, -7);
    bool rst_ok = false;
    int status = jpeg_dec_intervals(buf.get(), (int64_t)stream.size(), hd, first.data(), end.data(), &rst_ok);
    if (got) got->assign((size_t)mcus * 384, 0);
    if (!rst_ok) return status;
    for (int k = 0; k < hd.intervals; ++k) {
        CHECK(first[(size_t)k] >= hd.scan_at && first[(size_t)k] <= end[(size_t)k] && end[(size_t)k] <= (int)stream.size());
        const int m0 = k * hd.per, n = std::min(hd.per, mcus - m0);
        // the interval's own coefficients, and nothing else to write into
        std::unique_ptr<int16_t[]> out(new int16_t[(size_t)n * 384]);
        std::memset(out.get(), 0, (size_t)n * 768);
        alignas(16) int16_t blk[64];
        int16_t* o = out.get();
        const auto sink = [o, n](int m, int b, const int16_t* v) {
            CHECK(m >= 0 && m < n && b >= 0 && b < 6);
            std::memcpy(o + ((size_t)m * 6 + b) * 64, v, 128);
        };
        const int rc = jpeg_dec_interval(buf.get() + first[(size_t)k], end[(size_t)k] - first[(size_t)k], t, n, blk, sink);
        CHECK(rc >= 0 && rc <= kJpegDecBadRun);
        status = std::max(status, rc);
        if (got) std::memcpy(got->data() + (size_t)m0 * 384, out.get(), (size_t)n * 768);
    }
    return status;
}

static void check_tables() {
    JpegHuff dc0, ac0, dc1, ac1;
    jpeg_dec_detail::annex_k(&dc0, &ac0, &dc1, &ac1);
    JpegConst c;
    jpeg_build(16, 16, 75, &c);
    // every code of the encoder's tables decodes to its symbol
    const JpegHuff* tabs[4] = {&dc0, &dc1, &ac0, &ac1};
    for (int t = 0; t < 4; ++t)
        for (int sym = 0; sym < (t < 2 ? 12 : 256); ++sym) {
            const uint32_t e = t < 2 ? c.dc[t][sym] : c.ac[t - 2][sym];
            const int len = (int)(e >> 16);
            if (!len) continue;
            uint8_t bytes[4] = {0, 0, 0, 0};
            const uint32_t top = (e & 0xFFFF) << (32 - len);
            // a zero behind a 0xFF is stuffing: keep the codes clear of it by padding with zeros (no code is all ones)
            for (int i = 0; i < 4; ++i) bytes[i] = (uint8_t)(top >> (24 - 8 * i));
            if (bytes[0] == 0xFF || bytes[1] == 0xFF) continue;   // 0xFF 0x00 would be unstuffed
            JpegBitReader r;
            jpeg_bits_init(r, bytes, 4);
            CHECK(jpeg_huff_decode(r, *tabs[t]) == sym);
        }
    // a table whose lengths overflow is refused; one with 256 symbols of length 8 is accepted
    uint8_t bits[16] = {3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, vals[256];
    for (int i = 0; i < 256; ++i) vals[i] = (uint8_t)i;
    JpegHuff h;
    CHECK(!jpeg_dec_detail::build_huff(bits, vals, 3, &h));
    std::memset(bits, 0, 16);
    bits[7] = 255;
    bits[8] = 3;                          // 255 codes of 8 bits leave room for 2 of 9
    CHECK(!jpeg_dec_detail::build_huff(bits, vals, 256, &h));
    bits[8] = 1;
    CHECK(jpeg_dec_detail::build_huff(bits, vals, 256, &h));
}

static void check_layout(int h, int w, int intervals, int frames) {
    const JpegDecWorkLayout l = jpeg_dec_work_layout(h, w, intervals, frames);
    const size_t mcus = (size_t)jpeg_mcu_rows(h) * jpeg_mcu_cols(w), f = (size_t)frames;
    CHECK(l.off_coef == 0 && l.off_chroma >= f * mcus * 768 && l.off_first >= l.off_chroma + f * mcus * 128);
    CHECK(l.off_end >= l.off_first + f * intervals * 4 && l.bytes >= l.off_end + f * intervals * 4);
    CHECK(l.off_chroma % 16 == 0 && l.off_first % 16 == 0 && l.off_end % 16 == 0);
    CHECK(l.bytes <= f * (jpeg_dec_work_frame_bytes(h, w, intervals) + 64));
    std::vector<unsigned char> buf(l.bytes);
    std::memset(buf.data() + l.off_coef, 1, f * mcus * 768);
    std::memset(buf.data() + l.off_chroma, 2, f * mcus * 128);
    std::memset(buf.data() + l.off_first, 3, f * intervals * 4);
    std::memset(buf.data() + l.off_end, 4, f * intervals * 4);
    CHECK(buf[l.off_chroma] == 2 && buf[l.off_first] == 3 && buf[l.off_end + f * intervals * 4 - 1] == 4);
}

int main() {
    check_tables();
    // valid streams: what was coded comes back
    const int shapes[][3] = {{1, 1, 0}, {17, 33, 3}, {40, 76, 5}, {40, 76, 1}, {36, 200, 13}, {48, 48, 0}, {16, 160, 2}};
    for (const auto& sh : shapes)
        for (int with_dht = 0; with_dht < 2; ++with_dht)
            for (int sparse : {1, 3, 20}) {
                std::vector<int16_t> want, got;
                const std::vector<uint8_t> s = make_stream(sh[0], sh[1], 75, sh[2], with_dht != 0, sparse, &want);
                CHECK(decode(s, &got) == 0);
                CHECK(got == want);
            }
    const std::vector<uint8_t> base = make_stream(40, 76, 75, 5, true, 3, nullptr);
    JpegDecHeader hd;
    CHECK(jpeg_dec_parse(base.data(), (int64_t)base.size(), &hd, nullptr, nullptr) == nullptr);
    CHECK(hd.h == 40 && hd.w == 76 && hd.ri == 5 && hd.intervals == 3 && hd.per == 5);
    // every prefix: refused while the header is incomplete, a status (never 0) afterwards
    for (size_t n = 0; n < base.size(); ++n) {
        const std::vector<uint8_t> cut(base.begin(), base.begin() + (long)n);
        const int rc = decode(cut, nullptr);
        if ((int)n < hd.scan_at) CHECK(rc == -1);
        else CHECK(rc > 0);
    }
    // single-byte corruptions from a fixed seed: anything but a fault
    int refused = 0, flagged = 0, clean = 0;
    for (int i = 0; i < 6000; ++i) {
        std::vector<uint8_t> s = base;
        s[rnd() % s.size()] = (uint8_t)rnd();
        const int rc = decode(s, nullptr);
        rc < 0 ? ++refused : rc ? ++flagged : ++clean;
    }
    CHECK(refused > 0 && flagged > 0 && clean > 0);
    // ... and in the scan alone, where the parser does not look
    for (int i = 0; i < 6000; ++i) {
        std::vector<uint8_t> s = base;
        s[(size_t)hd.scan_at + rnd() % (s.size() - (size_t)hd.scan_at)] = (uint8_t)rnd();
        CHECK(decode(s, nullptr) >= 0);
    }
    // the malformed scans of the tests
    {
        std::vector<uint8_t> s(base.begin(), base.begin() + hd.scan_at + (long)(base.size() - (size_t)hd.scan_at) / 2);
        CHECK(decode(s, nullptr) > 0);   // cut in the middle
        std::vector<size_t> rst;
        for (size_t i = (size_t)hd.scan_at; i + 1 < base.size(); ++i)
            if (base[i] == 0xFF && base[i + 1] >= 0xD0 && base[i + 1] <= 0xD7) rst.push_back(i);
        CHECK(rst.size() == 2);
        s = base;
        s.erase(s.begin() + (long)rst[1], s.begin() + (long)rst[1] + 2);
        CHECK(decode(s, nullptr) == kJpegDecRstCount);   // a missing RST (the last: the others are in sequence)
        s = base;
        std::swap(s[rst[0] + 1], s[rst[1] + 1]);
        CHECK(decode(s, nullptr) == kJpegDecRstOrder);   // indices swapped
        s = base;
        for (int i = 0; i < 4; ++i) s[(size_t)hd.scan_at + i] = i & 1 ? 0x00 : 0xFF;   // 16 one-bits: no DC code
        CHECK(decode(s, nullptr) == kJpegDecBadCode);
    }
    // refusals
    {
        std::vector<uint8_t> s = base;
        for (size_t i = 2; i + 1 < (size_t)hd.scan_at; ++i)
            if (s[i] == 0xFF && s[i + 1] == 0xC0) {
                s[i + 1] = 0xC2;
                CHECK(decode(s, nullptr) == -1);
                s[i + 1] = 0xC0;
                s[i + 4] = 12;
                CHECK(decode(s, nullptr) == -1);
                s[i + 4] = 8;
                s[i + 11] = 0x21;
                CHECK(decode(s, nullptr) == -1);
                s[i + 11] = 0x22;
                s[i + 9] = 1;
                CHECK(decode(s, nullptr) == -1);
                break;
            }
    }
    const int lay[][4] = {{1, 1, 1, 1}, {17, 33, 6, 3}, {36, 1024, 3, 5}, {272, 1024, 17, 7}, {4096, 4096, 65536, 1}};
    for (const auto& s : lay) check_layout(s[0], s[1], s[2], s[3]);
    if (failures) return 1;
    std::printf("jpeg decode host check ok (%d refused, %d flagged, %d clean)\n", refused, flagged, clean);
    return 0;
}
