// Host part of the MJPG playback's JPEG decoder (rt_jpeg_dec.hip, kernels/jpeg_dec.hip): the segment
// parser that accepts a stream or refuses it before anything is launched, the Huffman decode tables built from its
// DHT (or Annex K when it has none), the layout of a chunk's device scratch, and the entropy walk of one restart
// interval, which the kernel and tools/jpeg_decode_host_check.cpp share. No HIP in here: the walk is marked
// SVX_JPEG_HD, which the includer defines (empty for a host compiler, __host__ __device__ in svx_jpeg_dec.h), so the
// host check runs all of it under the host sanitizers without a device (by hand, on the development machine only).
// The contract is restated in tests/jpeg_decode_numpy.py.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "svx_jpeg_host.h"

namespace svx {

// a frame's status: 0, or the largest of what its scan and its intervals met
enum JpegDecStatus {
    kJpegDecOk = 0,
    kJpegDecBadCode = 1,    // a code in no table
    kJpegDecBadSize = 2,    // a DC size above 11, an AC size above 10
    kJpegDecBadRun = 3,     // a run that passes coefficient 63
    kJpegDecRstCount = 4,   // not intervals - 1 RSTn markers
    kJpegDecRstOrder = 5,   // RSTn out of sequence
    kJpegDecNoEoi = 6       // the scan ends with the buffer, not with a marker
};

constexpr int kJpegLookBits = 9;

// One Huffman table as the walk reads it: the first kJpegLookBits bits give length << 8 | symbol for the codes that
// short (0: a longer code); longer ones walk maxcode (the largest code of each length, -1: none) and valoff (the
// index of a length's first symbol minus its first code).
struct JpegHuff {
    uint16_t look[1 << kJpegLookBits];
    int32_t maxcode[17];
    int32_t valoff[17];
    uint8_t vals[256];
};

// What the entropy kernel keeps in LDS: the DC and AC tables 0 and 1, and which of them each component uses.
struct JpegDecTables {
    JpegHuff dc[2], ac[2];
    uint8_t td[3], ta[3];
    uint8_t pad[2];
};

// ... and the reconstruction: each component's quantisation table, zig-zag order as in the DQT
struct JpegDecQuant {
    uint16_t q[3][64];
};

// sv_jpeg_desc of include/svx.h plus what the launch needs
struct JpegDecHeader {
    int h = 0, w = 0;
    int ri = 0;            // the restart interval in MCUs, 0: none
    int scan_at = 0;       // the header's length: the first byte of the entropy-coded segment
    int intervals = 0;     // ceil(MCUs / ri), 1 without DRI
    int per = 0;           // MCUs an interval (the last may hold fewer)
};

// A frame of a launch: where its stream lies in the packed bytes, its scan, its tables.
struct JpegDecFrame {
    int64_t at;            // the stream's first byte
    int32_t len;           // its bytes
    int32_t scan_at;
    int32_t intervals, per;
    int32_t tab;           // index of its JpegDecTables / JpegDecQuant
    int32_t pad;
};

namespace jpeg_dec_detail {

// BITS / HUFFVAL -> JpegHuff; false when the code lengths overflow (more codes of a length than it has)
inline bool build_huff(const uint8_t* bits, const uint8_t* vals, int count, JpegHuff* t) {
    memset(t, 0, sizeof *t);
    memcpy(t->vals, vals, (size_t)count);
    int32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int n = bits[len - 1];
        t->valoff[len] = k - code;
        if (code + n > (1 << len)) return false;
        for (int i = 0; i < n; ++i, ++k, ++code)
            if (len <= kJpegLookBits) {
                const int lo = code << (kJpegLookBits - len);
                for (int j = 0; j < (1 << (kJpegLookBits - len)); ++j)
                    t->look[lo + j] = (uint16_t)(len << 8 | vals[k]);
            }
        t->maxcode[len] = n ? code - 1 : -1;
        code <<= 1;
    }
    t->maxcode[0] = -1;
    return true;
}

inline void annex_k(JpegHuff* dc0, JpegHuff* ac0, JpegHuff* dc1, JpegHuff* ac1) {
    using namespace jpeg_tables;
    uint8_t dcv[12], acl[162], acc[162];
    hex_vals(kDcVals, dcv);
    hex_vals(kAcLumaVals, acl);
    hex_vals(kAcChromaVals, acc);
    build_huff(kDcLumaBits, dcv, 12, dc0);
    build_huff(kAcLumaBits, acl, 162, ac0);
    build_huff(kDcChromaBits, dcv, 12, dc1);
    build_huff(kAcChromaBits, acc, 162, ac1);
}

inline const char* sof_name(int m) {
    switch (m) {
        case 0xC1: return "extended sequential coding (SOF1)";
        case 0xC2: return "progressive coding (SOF2)";
        case 0xC3: return "lossless coding (SOF3)";
        case 0xC9: return "arithmetic coding (SOF9)";
        case 0xCA: return "arithmetic progressive coding (SOF10)";
        case 0xCB: return "arithmetic lossless coding (SOF11)";
        case 0xCC: return "arithmetic conditioning (DAC)";
        case 0xC5: case 0xC6: case 0xC7: case 0xCD: case 0xCE: case 0xCF: return "differential (hierarchical) coding";
        default: return nullptr;
    }
}

}  // namespace jpeg_dec_detail

// The header of a stream of n bytes: nullptr and *hd (tabs and quant when not null) filled when it is of the
// accepted kind, else what was met. Reads s[0 .. n) only.
inline const char* jpeg_dec_parse(const uint8_t* s, int64_t n, JpegDecHeader* hd, JpegDecTables* tabs,
                                  JpegDecQuant* quant) {
    using namespace jpeg_dec_detail;
    if (!s || !hd) return "null pointer";
    if (n < 4 || n > (1 << 30)) return "a stream of fewer than 4 bytes or more than 2^30";
    if (s[0] != 0xFF || s[1] != 0xD8) return "no SOI";
    *hd = JpegDecHeader{};
    uint8_t qt[4][64];
    bool have_q[4] = {false, false, false, false}, have_h[2][2] = {{false, false}, {false, false}};
    bool have_sof = false, any_dht = false;
    JpegHuff* huff[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    if (tabs) {
        memset(tabs, 0, sizeof *tabs);
        huff[0][0] = &tabs->dc[0], huff[0][1] = &tabs->dc[1], huff[1][0] = &tabs->ac[0], huff[1][1] = &tabs->ac[1];
    }
    JpegHuff scratch;   // tables are validated even when the caller wants none
    int cid[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    int64_t i = 2;
    for (;;) {
        if (i + 4 > n) return "a header that runs past the buffer";
        if (s[i] != 0xFF) return "bytes that are no marker in the header";
        const int m = s[i + 1];
        if (m == 0xFF) {   // a fill byte
            ++i;
            continue;
        }
        const int64_t len = (int64_t)s[i + 2] << 8 | s[i + 3];
        if (len < 2 || i + 2 + len > n) return "a segment length that runs past the buffer";
        const uint8_t* p = s + i + 4;
        const int np = (int)len - 2;
        if (const char* why = sof_name(m)) return why;
        if (m == 0xC0) {
            if (have_sof) return "two SOF0 segments";
            if (np < 6) return "a short SOF0";
            if (p[0] != 8) return "samples of other than 8 bits";
            hd->h = p[1] << 8 | p[2];
            hd->w = p[3] << 8 | p[4];
            if (p[5] != 3) return "other than three components";
            if (np != 15) return "a SOF0 of the wrong length";
            for (int k = 0; k < 3; ++k) {
                cid[k] = p[6 + 3 * k];
                ctq[k] = p[8 + 3 * k];
                if (p[7 + 3 * k] != (k ? 0x11 : 0x22)) return "sampling factors other than 2x2, 1x1, 1x1 (4:2:0)";
                if (ctq[k] > 3) return "a quantisation table id above 3";
            }
            if (hd->h < 1 || hd->h > kJpegMaxDim || hd->w < 1 || hd->w > kJpegMaxDim) return "h or w outside 1 .. 4096";
            have_sof = true;
        } else if (m == 0xDB) {
            for (int j = 0; j < np; j += 65) {
                if (p[j] >> 4) return "a 16-bit DQT";
                if ((p[j] & 15) > 3 || j + 65 > np) return "a malformed DQT";
                memcpy(qt[p[j] & 15], p + j + 1, 64);
                have_q[p[j] & 15] = true;
            }
        } else if (m == 0xC4) {
            for (int j = 0; j < np;) {
                if (j + 17 > np) return "a malformed DHT";
                const int tc = p[j] >> 4, th = p[j] & 15;
                int cnt = 0;
                for (int l = 0; l < 16; ++l) cnt += p[j + 1 + l];
                if (tc > 1 || th > 1 || cnt > 256 || j + 17 + cnt > np) return "a malformed DHT";
                if (!build_huff(p + j + 1, p + j + 17, cnt, huff[tc][th] ? huff[tc][th] : &scratch))
                    return "a DHT whose code lengths overflow";
                have_h[tc][th] = true;
                any_dht = true;
                j += 17 + cnt;
            }
        } else if (m == 0xDD) {
            if (np != 2) return "a malformed DRI";
            hd->ri = p[0] << 8 | p[1];
        } else if (m == 0xDA) {
            if (!have_sof) return "SOS before SOF0";
            if (np != 10 || p[0] != 3) return "a scan of other than three components (several scans)";
            if (!any_dht) {   // MJPG frames of other writers: the Annex K tables
                if (tabs) annex_k(&tabs->dc[0], &tabs->ac[0], &tabs->dc[1], &tabs->ac[1]);
                have_h[0][0] = have_h[0][1] = have_h[1][0] = have_h[1][1] = true;
            }
            for (int k = 0; k < 3; ++k) {
                if (p[1 + 2 * k] != cid[k]) return "scan components out of the frame's order";
                const int td = p[2 + 2 * k] >> 4, ta = p[2 + 2 * k] & 15;
                if (td > 1 || ta > 1) return "a Huffman table id above 1";
                if (!have_h[0][td] || !have_h[1][ta]) return "a Huffman table that no DHT defines";
                if (!have_q[ctq[k]]) return "a quantisation table that no DQT defines";
                if (tabs) tabs->td[k] = (uint8_t)td, tabs->ta[k] = (uint8_t)ta;
                if (quant)
                    for (int z = 0; z < 64; ++z) quant->q[k][z] = qt[ctq[k]][z];
            }
            if (p[7] != 0 || p[8] != 63 || p[9] != 0) return "a scan that is not Ss = 0, Se = 63, Ah = Al = 0";
            hd->scan_at = (int)(i + 2 + len);
            const int mcus = jpeg_mcu_rows(hd->h) * jpeg_mcu_cols(hd->w);
            hd->per = hd->ri ? hd->ri : mcus;
            hd->intervals = (mcus + hd->per - 1) / hd->per;
            return nullptr;
        } else if (m == 0xD9) {
            return "EOI before SOS";
        } else if ((m >= 0xD0 && m <= 0xD8) || m == 0x01 || m == 0x00) {
            return "a marker without a segment in the header";
        } else if (m == 0xDC || m == 0xDE || m == 0xDF) {
            return "DNL or hierarchical markers";
        }
        // APPn, COM and the rest: skipped
        i += 2 + len;
    }
}

// ---- the entropy walk of one interval ----
// The bytes [p, p + n) of an interval, most significant bit first; 0xFF 0x00 is one 0xFF, anything else behind a
// 0xFF ends the data, and bits past the end read as zeros. Never reads outside [p, p + n).
struct JpegBitReader {
    const uint8_t* p;
    int n, pos;
    uint64_t acc;   // the next bits at the top
    int cnt;        // how many of them are valid
    uint32_t nxt;   // the four bytes at pos, loaded ahead of their use (valid while pos + 4 <= n)
};

SVX_JPEG_HD inline void jpeg_bits_init(JpegBitReader& r, const uint8_t* p, int n) {
    r.p = p, r.n = n, r.pos = 0, r.acc = 0, r.cnt = 0, r.nxt = 0;
    if (4 <= n) __builtin_memcpy(&r.nxt, p, 4);
}

// at least 32 valid bits (zeros past the end), for a reader that holds fewer than 32. Four bytes from one load where
// none of them is a 0xFF (all but one word in 64 of coded data; the host and the device are little-endian), else
// byte by byte.
SVX_JPEG_HD inline void jpeg_bits_fill(JpegBitReader& r) {
    if (r.pos + 4 <= r.n) {
        const uint32_t w = r.nxt;
        if (!((~w - 0x01010101u) & w & 0x80808080u)) {   // no byte of w is 0xFF
            r.acc |= (uint64_t)__builtin_bswap32(w) << (32 - r.cnt);
            r.cnt += 32;
            r.pos += 4;
            if (r.pos + 4 <= r.n) __builtin_memcpy(&r.nxt, r.p + r.pos, 4);   // used by the next fill
            return;
        }
    }
    while (r.cnt <= 56) {
        uint32_t b = 0;
        if (r.pos < r.n) {
            b = r.p[r.pos++];
            if (b == 0xFFu) {
                if (r.pos < r.n && r.p[r.pos] == 0) {
                    ++r.pos;
                } else {   // a marker, or a 0xFF whose partner is cut off: the data ends here
                    b = 0;
                    r.pos = r.n;
                }
            }
        }
        r.acc |= (uint64_t)b << (56 - r.cnt);
        r.cnt += 8;
    }
    if (r.pos + 4 <= r.n) __builtin_memcpy(&r.nxt, r.p + r.pos, 4);
}

SVX_JPEG_HD inline uint32_t jpeg_bits_peek16(JpegBitReader& r) {
    if (r.cnt < 32) jpeg_bits_fill(r);
    return (uint32_t)(r.acc >> 48);
}
SVX_JPEG_HD inline void jpeg_bits_skip(JpegBitReader& r, int n) {
    r.acc <<= n;
    r.cnt -= n;
}
// n bits (1 .. 16) as the signed value of size category n (F.2.2.1's EXTEND)
SVX_JPEG_HD inline int jpeg_bits_value(JpegBitReader& r, int n) {
    if (r.cnt < 32) jpeg_bits_fill(r);
    const int v = (int)(r.acc >> (64 - n));
    jpeg_bits_skip(r, n);
    return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v;
}

// the next symbol of table t, or -1 for a code it does not hold
SVX_JPEG_HD inline int jpeg_huff_decode(JpegBitReader& r, const JpegHuff& t) {
    const uint32_t v = jpeg_bits_peek16(r);
    const uint32_t e = t.look[v >> (16 - kJpegLookBits)];
    if (e) {
        jpeg_bits_skip(r, (int)(e >> 8));
        return (int)(e & 255u);
    }
    for (int len = kJpegLookBits + 1; len <= 16; ++len) {
        const int32_t code = (int32_t)(v >> (16 - len));
        if (code <= t.maxcode[len]) {
            jpeg_bits_skip(r, len);
            return t.vals[(code + t.valoff[len]) & 255];
        }
    }
    return -1;
}

// `mcus` MCUs (Y00 Y01 Y10 Y11 Cb Cr) of the interval [p, p + n) with tables t, the DC predictors starting at 0.
// Each block is assembled in blk[64] (int16, zig-zag order; the caller's, 16-byte aligned: LDS in the kernel) and handed to
// sink(mcu, block, blk). Returns the status; on an error the blocks not yet decoded are not handed over.
template <class Sink>
SVX_JPEG_HD inline int jpeg_dec_interval(const uint8_t* p, int n, const JpegDecTables& t, int mcus, int16_t* blk,
                                         Sink&& sink) {
    JpegBitReader r;
    jpeg_bits_init(r, p, n);
    blk = static_cast<int16_t*>(__builtin_assume_aligned(blk, 16));
    int pred[3] = {0, 0, 0};
    for (int m = 0; m < mcus; ++m) {
        for (int k = 0; k < 6; ++k) {
            const int c = k < 4 ? 0 : k - 3;
            const JpegHuff& dc = t.dc[t.td[c] & 1];
            const JpegHuff& ac = t.ac[t.ta[c] & 1];
            __builtin_memset(blk, 0, 128);
            int s = jpeg_huff_decode(r, dc);
            if (s < 0) return kJpegDecBadCode;
            if (s > 11) return kJpegDecBadSize;
            if (s) pred[c] += jpeg_bits_value(r, s);
            blk[0] = (int16_t)pred[c];
            for (int z = 1; z < 64;) {
                const int rs = jpeg_huff_decode(r, ac);
                if (rs < 0) return kJpegDecBadCode;
                const int run = rs >> 4;
                s = rs & 15;
                if (s == 0) {
                    if (run != 15) break;   // EOB
                    if (z + 15 > 63) return kJpegDecBadRun;
                    z += 16;
                    continue;
                }
                z += run;
                if (z > 63) return kJpegDecBadRun;
                if (s > 10) return kJpegDecBadSize;
                blk[z++] = (int16_t)jpeg_bits_value(r, s);
            }
            sink(m, k, blk);
        }
    }
    return kJpegDecOk;
}

// The intervals of a scan on the host (what the marker-scan kernel does in parallel): interval k's bytes are
// [first[k], end[k]) of s, RSTn between them in sequence, the last ends at the first other marker. Returns the
// status (the largest of what applies); first / end hold hd.intervals entries and are complete unless the status is
// kJpegDecRstCount or kJpegDecRstOrder (with kJpegDecNoEoi: when rst_ok comes back true).
inline int jpeg_dec_intervals(const uint8_t* s, int64_t n, const JpegDecHeader& hd, int32_t* first, int32_t* end,
                              bool* rst_ok) {
    int k = 0, status = kJpegDecOk;
    bool order = true;
    int64_t i = hd.scan_at, stop = n;
    bool eoi = false;
    if (hd.intervals > 0) first[0] = hd.scan_at;
    for (; i + 1 < n; ++i) {
        if (s[i] != 0xFF) continue;
        const int m = s[i + 1];
        if (m == 0 || m == 0xFF) continue;
        if (m >= 0xD0 && m <= 0xD7) {
            if (m - 0xD0 != (k & 7)) order = false;
            if (k + 1 < hd.intervals) end[k] = (int32_t)i, first[k + 1] = (int32_t)i + 2;
            ++k;
            ++i;
            continue;
        }
        stop = i;
        eoi = true;
        break;
    }
    if (!eoi) status = kJpegDecNoEoi;
    if (k != hd.intervals - 1 || !order) {
        const int bad = order ? kJpegDecRstCount : kJpegDecRstOrder;
        *rst_ok = false;
        return bad > status ? bad : status;
    }
    *rst_ok = true;
    end[hd.intervals - 1] = (int32_t)stop;
    return status;
}

// ---- the device scratch of a chunk of frames (kernels/jpeg_dec.hip), all 16-byte aligned ----
struct JpegDecWorkLayout {
    size_t off_coef = 0, off_chroma = 0, off_first = 0, off_end = 0, bytes = 0;
};
// bytes of one frame's scratch: int16 coefficients in MCU order (768 B an MCU), the Cb and Cr sample planes of the
// padded picture (128 B an MCU), an interval's first byte and its end
inline size_t jpeg_dec_work_frame_bytes(int h, int w, int intervals) {
    const size_t mcus = (size_t)jpeg_mcu_rows(h) * jpeg_mcu_cols(w);
    return mcus * (768 + 128) + (size_t)intervals * 8;
}
inline JpegDecWorkLayout jpeg_dec_work_layout(int h, int w, int intervals, int frames) {
    const size_t mcus = (size_t)jpeg_mcu_rows(h) * jpeg_mcu_cols(w), f = (size_t)frames;
    const auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
    JpegDecWorkLayout l;
    l.off_coef = 0;
    l.off_chroma = up16(f * mcus * 768);
    l.off_first = l.off_chroma + up16(f * mcus * 128);
    l.off_end = l.off_first + up16(f * (size_t)intervals * 4);
    l.bytes = l.off_end + up16(f * (size_t)intervals * 4);
    return l;
}

}  // namespace svx
