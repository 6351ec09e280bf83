// The MJPG recording's JPEG encoder (gfx950): the picture loop.py:49-54,82-89 hands to cv2.VideoWriter, as a baseline
// stream whose entropy-coded bytes are libjpeg's at the same quality (4:2:0, a restart interval an MCU row, the Annex K
// tables; DESIGN §7.11, restated in tests/jpeg_numpy.py). Restart intervals are independent, so no workgroup waits for
// another:
//   transform  a workgroup takes up to 32 MCUs of an MCU row: colour and the 2 x 2 chroma means from two picture rows
//              a lane (16-byte loads where the rows allow) into LDS, then a block a lane: the slow-integer DCT in
//              registers, the quantiser as a multiply and a shift, int16 coefficients in zig-zag and MCU order. A
//              dummy luma block (right of or below the picture) is written as it is coded: the DC of the block before
//              it in the MCU, no AC.
//   size       a wave takes a restart interval, a lane a run of ceil(MCUs / 64) MCUs. Walk 1 gives the lane's bits
//              and its first byte; a wave scan gives where its bits start. Walk 2 packs the bytes whose first bit is
//              the lane's (the last one completed with the next lane's first bits, or with 1-bits at the end of the
//              interval) and counts the 0xFF among them; a second scan gives where the lane writes.
//   scan       a wave per frame: the offsets of its intervals (each followed by RSTn or EOI) and the frame's size.
//   write      walk 3: the same packing, stored with the stuffed zeros at the lane's offset; the header, the markers.
// A frame whose stream is longer than its slot is not written at all (its size comes back negative).
#include "../svx_jpeg.h"
#include "../svx_wave.h"

namespace svx {

namespace {

constexpr int kMcuWg = 32;        // MCUs of a transform workgroup
constexpr int kXformThreads = 192;   // its lanes: 32 MCUs x 6 blocks

// natural index of zig-zag position k (jpeg_tables::kZigzag, for the device)
__device__ const uint8_t kNatOfZig[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                          12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                          58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One pass of the IJG slow-integer forward DCT (Loeffler-Ligtenberg-Moschytz, 13-bit constants) over eight values:
// the row pass keeps 2 extra bits, the column pass takes them out.
template <bool ROWS>
__device__ __forceinline__ void fdct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int n = ROWS ? 11 : 15;
    const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6;
    const int t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if constexpr (ROWS) {
        d0 = (t10 + t11) << 2;
        d4 = (t10 - t11) << 2;
    } else {
        d0 = descale(t10 + t11, 2);
        d4 = descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * 4433;
    d2 = descale(z1 + t13 * 6270, n);
    d6 = descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d7 = descale(u4 + z1 + z3, n);
    d5 = descale(u5 + z2 + z4, n);
    d3 = descale(u6 + z2 + z3, n);
    d1 = descale(u7 + z1 + z4, n);
}

// 16 pixels (B | G << 8 | R << 16) of a picture row from column x0: three 16-byte loads (x0 + 16 <= w, the row
// 16-byte aligned), or bytes with the last column repeated
template <bool VEC>
__device__ __forceinline__ void load_px16(const uint8_t* row, int x0, int w, uint32_t (&px)[16]) {
    if constexpr (VEC) {
        const uint4* v = reinterpret_cast<const uint4*>(row + 3 * x0);
        uint32_t a[13];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint4 t = v[k];
            a[4 * k] = t.x, a[4 * k + 1] = t.y, a[4 * k + 2] = t.z, a[4 * k + 3] = t.w;
        }
        a[12] = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            px[j] = __builtin_amdgcn_alignbyte(a[(3 * j) / 4 + 1], a[(3 * j) / 4], (3 * j) & 3) & 0xFFFFFFu;
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint8_t* p = row + 3 * min(x0 + j, w - 1);
            px[j] = p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
        }
    }
}

__device__ __forceinline__ int px_y(uint32_t p) {
    const int b = p & 255, g = (p >> 8) & 255, r = (p >> 16) & 255;
    return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
}
__device__ __forceinline__ int px_cb(uint32_t p) {
    const int b = p & 255, g = (p >> 8) & 255, r = (p >> 16) & 255;
    return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int px_cr(uint32_t p) {
    const int b = p & 255, g = (p >> 8) & 255, r = (p >> 16) & 255;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// the luma of 16 pixels as 16 bytes
__device__ __forceinline__ uint4 luma16(const uint32_t (&px)[16]) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w[k] = px_y(px[4 * k]) | px_y(px[4 * k + 1]) << 8 | px_y(px[4 * k + 2]) << 16 | px_y(px[4 * k + 3]) << 24;
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the eight 2 x 2 means of Cb and of Cr of two rows of 16 pixels: bias 1 in even output columns, 2 in odd ones
__device__ __forceinline__ void chroma8(const uint32_t (&a)[16], const uint32_t (&b)[16], uint2& cb, uint2& cr) {
    uint32_t u[2] = {0, 0}, v[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int bias = 1 + (j & 1);
        const int sb = px_cb(a[2 * j]) + px_cb(a[2 * j + 1]) + px_cb(b[2 * j]) + px_cb(b[2 * j + 1]);
        const int sr = px_cr(a[2 * j]) + px_cr(a[2 * j + 1]) + px_cr(b[2 * j]) + px_cr(b[2 * j + 1]);
        u[j >> 2] |= (uint32_t)((sb + bias) >> 2) << (8 * (j & 3));
        v[j >> 2] |= (uint32_t)((sr + bias) >> 2) << (8 * (j & 3));
    }
    cb = make_uint2(u[0], u[1]);
    cr = make_uint2(v[0], v[1]);
}

template <bool VEC>
__global__ __launch_bounds__(kXformThreads) void jpeg_transform_kernel(const uint8_t* __restrict__ img,
                                                                       int64_t frame_stride, int ld, int h, int w,
                                                                       int mr, int mc, int chunks,
                                                                       const JpegConst* __restrict__ jc,
                                                                       int16_t* __restrict__ coef) {
    __shared__ __attribute__((aligned(16))) uint8_t sy[16][16 * kMcuWg];
    __shared__ __attribute__((aligned(16))) uint8_t sc[2][8][8 * kMcuWg];
    __shared__ uint32_t sq[2][64];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x % chunks;
    const int r = (blockIdx.x / chunks) % mr;
    const int64_t f = blockIdx.x / (chunks * mr);
    const int m0 = chunk * kMcuWg, nm = min(kMcuWg, mc - m0);
    const uint8_t* pic = img + f * frame_stride;
    if (tid < 128) (&sq[0][0])[tid] = (&jc->quant[0][0])[tid];
    // a lane: two picture rows of an MCU's 16 columns. Luma rows repeat the last row; chroma rows are the means of
    // rows 2 c, 2 c + 1 with only an odd last row repeated, and below chroma row ceil(h / 2) - 1 that row repeats.
    const int clast = (h + 1) / 2 - 1;
    for (int u = tid; u < nm * 8; u += kXformThreads) {
        const int p = u / nm, m = u - p * nm;
        const int x0 = 16 * (m0 + m);
        const int ya = min(16 * r + 2 * p, h - 1), yb = min(16 * r + 2 * p + 1, h - 1);
        const int crow = min(8 * r + p, clast);
        const int ca = 2 * crow, cbw = min(2 * crow + 1, h - 1);
        uint32_t a[16], b[16];
        load_px16<VEC>(pic + (int64_t)ya * ld, x0, w, a);
        load_px16<VEC>(pic + (int64_t)yb * ld, x0, w, b);
        *reinterpret_cast<uint4*>(&sy[2 * p][16 * m]) = luma16(a);
        *reinterpret_cast<uint4*>(&sy[2 * p + 1][16 * m]) = luma16(b);
        if (ca != ya || cbw != yb) {
            load_px16<VEC>(pic + (int64_t)ca * ld, x0, w, a);
            load_px16<VEC>(pic + (int64_t)cbw * ld, x0, w, b);
        }
        uint2 cb, cr;
        chroma8(a, b, cb, cr);
        *reinterpret_cast<uint2*>(&sc[0][p][8 * m]) = cb;
        *reinterpret_cast<uint2*>(&sc[1][p][8 * m]) = cr;
    }
    __syncthreads();
    const int k = tid / kMcuWg, m = tid % kMcuWg;   // block k of MCU m0 + m: Y00 Y01 Y10 Y11 Cb Cr
    if (m >= nm) return;
    // a luma block right of column ceil(w / 8) or below row ceil(h / 8) is a dummy: the DC of the block before it
    // in the MCU, which is the DC of block `src`
    int src = k;
    bool dummy = false;
    if (k >= 1 && k < 4) {
        const bool cold = 2 * (m0 + m) + 1 >= (w + 7) / 8, rowd = 2 * r + 1 >= (h + 7) / 8;
        const int s1 = cold ? 0 : 1;                  // block 1's
        const int s2 = rowd ? s1 : 2;                 // block 2's
        const int s3 = rowd ? s2 : cold ? 2 : 3;      // block 3's
        src = k == 1 ? s1 : k == 2 ? s2 : s3;
        dummy = src != k;
    }
    int d[64];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint2 v = k < 4 ? *reinterpret_cast<const uint2*>(&sy[8 * (src >> 1) + i][16 * m + 8 * (src & 1)])
                              : *reinterpret_cast<const uint2*>(&sc[k - 4][i][8 * m]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[8 * i + j] = (int)((v.x >> (8 * j)) & 255u) - 128;
            d[8 * i + 4 + j] = (int)((v.y >> (8 * j)) & 255u) - 128;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
        fdct8<true>(d[8 * i], d[8 * i + 1], d[8 * i + 2], d[8 * i + 3], d[8 * i + 4], d[8 * i + 5], d[8 * i + 6],
                    d[8 * i + 7]);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        fdct8<false>(d[j], d[8 + j], d[16 + j], d[24 + j], d[32 + j], d[40 + j], d[48 + j], d[56 + j]);
    // (|c| + (8 q >> 1)) / (8 q), sign restored, as ((|c| + 4 q) >> 3) * r >> 20 (svx_jpeg_host.h)
    const int tab = k < 4 ? 0 : 1;
    uint32_t o[32];
#pragma unroll
    for (int z = 0; z < 64; ++z) {
        const int nat = kNatOfZig[z];
        const uint32_t e = sq[tab][nat];
        const int c = d[nat];
        const uint32_t a = (uint32_t)(c < 0 ? -c : c);
        const uint32_t qv = (((a + ((e >> 21) << 2)) >> 3) * (e & 0x1FFFFFu)) >> kJpegRecipShift;
        const uint32_t v = (dummy && z > 0) ? 0u : (uint32_t)(c < 0 ? -(int)qv : (int)qv) & 0xFFFFu;
        if (z & 1) o[z >> 1] |= v << 16;
        else o[z >> 1] = v;
    }
    uint4* dst = reinterpret_cast<uint4*>(coef) + ((((f * mr + r) * mc + m0 + m) * 6 + k) * 8);
#pragma unroll
    for (int g = 0; g < 8; ++g) dst[g] = make_uint4(o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]);
}

// ---- entropy coding: one routine, three walks ----
enum { kWalkBits = 0, kWalkCount = 1, kWalkWrite = 2 };

struct Bits {
    uint64_t acc = 0;      // count, write: the bits not yet in a byte, in the low nacc bits
    int nacc = 0;
    bool skip = false;     // ... the first byte completed is the lane before's
    uint32_t ff = 0;       // count: 0xFF bytes
    uint8_t* p = nullptr;  // write: the next byte, never at or past pend
    uint8_t* pend = nullptr;
    uint32_t total = 0;    // bits: the lane's bits; the first of them (at least 8 once any MCU is coded)
    uint64_t first = 0;
    int nfirst = 0;
};

template <int MODE>
__device__ __forceinline__ void put_byte(Bits& s, uint32_t byte) {
    if (s.skip) {
        s.skip = false;
        return;
    }
    if constexpr (MODE == kWalkCount) {
        s.ff += byte == 255u;
    } else {
        if (s.p < s.pend) *s.p = (uint8_t)byte;
        ++s.p;
        if (byte == 255u) {
            if (s.p < s.pend) *s.p = 0;
            ++s.p;
        }
    }
}

// n <= 27 bits
template <int MODE>
__device__ __forceinline__ void put(Bits& s, uint32_t bits, int n) {
    if constexpr (MODE == kWalkBits) {
        s.total += n;
        if (s.nfirst < 8) {
            s.first = s.first << n | bits;
            s.nfirst += n;
        }
    } else {
        s.acc = s.acc << n | bits;
        s.nacc += n;
        while (s.nacc >= 8) {
            s.nacc -= 8;
            put_byte<MODE>(s, (uint32_t)(s.acc >> s.nacc) & 255u);
        }
    }
}

// the lane's last byte when its bits end inside one: the rest from the next lane's first byte (0xFF at the end of
// the interval: the padding of 1-bits)
template <int MODE>
__device__ __forceinline__ void put_tail(Bits& s, uint32_t next_head) {
    if (s.nacc > 0) put_byte<MODE>(s, (uint32_t)(s.acc << (8 - s.nacc) | next_head >> s.nacc) & 255u);
}

// One MCU: Y00 Y01 Y10 Y11 Cb Cr, each a DC difference (size category, then the bits) and its AC coefficients as
// run / size symbols with ZRL for runs over 15 and EOB when zeros remain. cp: the MCU's 48 vectors of 8 coefficients.
template <int MODE>
__device__ __forceinline__ void walk_mcu(Bits& s, const uint4* __restrict__ cp, int& py, int& pb, int& pr,
                                         const uint32_t (*sdc)[12], const uint32_t (*sac)[256]) {
    for (int k = 0; k < 6; ++k) {
        const int tab = k < 4 ? 0 : 1;
        int run = 0;
        for (int g = 0; g < 8; ++g) {
            const uint4 v = cp[8 * k + g];
            if (g > 0 && (v.x | v.y | v.z | v.w) == 0u) {   // eight zeros (most vectors at the usual qualities)
                run += 8;
                continue;
            }
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                int c = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1)));
                if (j == 0 && g == 0) {
                    const int pred = k < 4 ? py : k == 4 ? pb : pr;
                    const int diff = c - pred;
                    if (k < 4) py = c;
                    else if (k == 4) pb = c;
                    else pr = c;
                    const uint32_t a = (uint32_t)(diff < 0 ? -diff : diff);
                    const int sz = 32 - __clz((int)a);
                    const uint32_t e = sdc[tab][sz];
                    const uint32_t vb = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << sz) - 1u);
                    put<MODE>(s, (e & 0xFFFFu) << sz | vb, (int)(e >> 16) + sz);
                } else if (c == 0) {
                    ++run;
                } else {
                    while (run > 15) {
                        const uint32_t z = sac[tab][0xF0];
                        put<MODE>(s, z & 0xFFFFu, (int)(z >> 16));
                        run -= 16;
                    }
                    const uint32_t a = (uint32_t)(c < 0 ? -c : c);
                    const int sz = 32 - __clz((int)a);
                    const uint32_t e = sac[tab][run << 4 | sz];
                    const uint32_t vb = (uint32_t)(c < 0 ? c - 1 : c) & ((1u << sz) - 1u);
                    put<MODE>(s, (e & 0xFFFFu) << sz | vb, (int)(e >> 16) + sz);
                    run = 0;
                }
            }
        }
        if (run > 0) {
            const uint32_t z = sac[tab][0x00];
            put<MODE>(s, z & 0xFFFFu, (int)(z >> 16));
        }
    }
}

// the Huffman tables into LDS (every lane of the workgroup), then a barrier
__device__ __forceinline__ void load_huff(const JpegConst* __restrict__ jc, uint32_t (*sdc)[12], uint32_t (*sac)[256]) {
    for (int i = threadIdx.x; i < 24; i += blockDim.x) (&sdc[0][0])[i] = (&jc->dc[0][0])[i];
    for (int i = threadIdx.x; i < 512; i += blockDim.x) (&sac[0][0])[i] = (&jc->ac[0][0])[i];
    __syncthreads();
}

// A lane's MCUs [m0, m1) of interval gi and the DC predictors in front of them: 0 at the interval's start, else the
// MCU before's (its last luma block's, a dummy one included: the transform wrote what is coded)
struct LaneRun {
    int m0, m1;
    const uint4* cp;
    int py, pb, pr;
};
__device__ __forceinline__ LaneRun lane_run(const int16_t* __restrict__ coef, int64_t gi, int mc, int lane) {
    LaneRun r;
    const int per = (mc + 63) >> 6;
    r.m0 = min(lane * per, mc);
    r.m1 = min(r.m0 + per, mc);
    const int16_t* base = coef + (gi * mc) * 384;
    r.cp = reinterpret_cast<const uint4*>(base);
    r.py = r.pb = r.pr = 0;
    if (r.m0 > 0 && r.m0 < r.m1) {
        const int16_t* q = base + (int64_t)(r.m0 - 1) * 384;
        r.py = q[3 * 64], r.pb = q[4 * 64], r.pr = q[5 * 64];
    }
    return r;
}

template <int MODE>
__device__ __forceinline__ void walk_run(Bits& s, const LaneRun& r, const uint32_t (*sdc)[12],
                                         const uint32_t (*sac)[256]) {
    int py = r.py, pb = r.pb, pr = r.pr;
    for (int m = r.m0; m < r.m1; ++m) walk_mcu<MODE>(s, r.cp + (int64_t)m * 48, py, pb, pr, sdc, sac);
}

__global__ __launch_bounds__(256) void jpeg_size_kernel(const JpegConst* __restrict__ jc,
                                                        const int16_t* __restrict__ coef, int mc, int64_t intervals,
                                                        uint2* __restrict__ lane_info, int32_t* __restrict__ ilen) {
    __shared__ uint32_t sdc[2][12], sac[2][256];
    load_huff(jc, sdc, sac);
    const int lane = threadIdx.x & 63;
    const int64_t gi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gi >= intervals) return;   // the whole wave
    const LaneRun r = lane_run(coef, gi, mc, lane);
    const auto add = [](uint32_t a, uint32_t b) { return a + b; };
    Bits s;
    walk_run<kWalkBits>(s, r, sdc, sac);
    // an MCU is at least 32 bits, so a lane with MCUs has its first byte; one without reads as the padding
    const uint32_t head = s.nfirst >= 8 ? (uint32_t)(s.first >> (s.nfirst - 8)) & 255u : 255u;
    const uint32_t incl = wave_scan(s.total, 0u, add);
    const uint32_t start = incl - s.total, all_bits = wave_readlane(incl, 63);
    uint32_t next_head = (uint32_t)__shfl_down((int)head, 1);
    if (lane == 63) next_head = 255u;
    Bits t;
    t.nacc = (int)(start & 7u);
    t.skip = t.nacc != 0;
    if (r.m0 < r.m1) {
        walk_run<kWalkCount>(t, r, sdc, sac);
        put_tail<kWalkCount>(t, next_head);
    }
    const uint32_t fincl = wave_scan(t.ff, 0u, add);
    const uint32_t all_ff = wave_readlane(fincl, 63);
    lane_info[gi * 64 + lane] = make_uint2(start | next_head << 24, ((start + 7u) >> 3) + fincl - t.ff);
    if (lane == 0) ilen[gi] = (int32_t)(((all_bits + 7u) >> 3) + all_ff);
}

// a wave per frame: where each interval starts (the header, then every interval and the two bytes of its RSTn or
// EOI) and the frame's size, negative when it does not fit
__global__ __launch_bounds__(256) void jpeg_scan_kernel(const JpegConst* __restrict__ jc,
                                                        const int32_t* __restrict__ ilen, int mr, int frames,
                                                        int64_t cap, int32_t* __restrict__ ioff,
                                                        int32_t* __restrict__ sizes) {
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= frames) return;   // the whole wave
    const auto add = [](int32_t a, int32_t b) { return a + b; };
    int32_t carry = jc->header_len;
    for (int base = 0; base < mr; base += 64) {
        const int i = base + lane;
        const int32_t v = i < mr ? ilen[(int64_t)f * mr + i] + 2 : 0;
        const int32_t incl = wave_scan(v, 0, add);
        if (i < mr) ioff[(int64_t)f * mr + i] = carry + incl - v;
        carry += wave_readlane(incl, 63);
    }
    if (lane == 0) sizes[f] = carry <= cap ? carry : -carry;
}

__global__ __launch_bounds__(256) void jpeg_write_kernel(const JpegConst* __restrict__ jc,
                                                         const int16_t* __restrict__ coef, int mr, int mc,
                                                         int64_t intervals, const uint2* __restrict__ lane_info,
                                                         const int32_t* __restrict__ ilen,
                                                         const int32_t* __restrict__ ioff,
                                                         const int32_t* __restrict__ sizes, uint8_t* __restrict__ out,
                                                         int64_t cap) {
    __shared__ uint32_t sdc[2][12], sac[2][256];
    load_huff(jc, sdc, sac);
    const int lane = threadIdx.x & 63;
    const int64_t gi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gi >= intervals) return;   // the whole wave
    const int64_t f = gi / mr;
    const int r = (int)(gi - f * mr);
    if (sizes[f] < 0) return;      // the frame does not fit its slot: nothing of it is written
    uint8_t* slot = out + f * cap;
    uint8_t* base = slot + ioff[gi];
    const LaneRun run = lane_run(coef, gi, mc, lane);
    const uint2 info = lane_info[gi * 64 + lane];
    Bits s;
    s.nacc = (int)(info.x & 7u);
    s.skip = s.nacc != 0;
    s.p = base + info.y;
    s.pend = slot + cap;
    if (run.m0 < run.m1) {
        walk_run<kWalkWrite>(s, run, sdc, sac);
        put_tail<kWalkWrite>(s, info.x >> 24);
    }
    if (lane == 0) {   // RSTn behind every interval but the last, EOI behind that
        uint8_t* m = base + ilen[gi];
        if (m + 2 <= slot + cap) m[0] = 0xFF, m[1] = (uint8_t)(r == mr - 1 ? 0xD9 : 0xD0 + (r & 7));
    }
    if (r == 0)
        for (int i = lane; i < jc->header_len && i < cap; i += 64) slot[i] = jc->header[i];
}

// the exclusive sums of the frames' sizes (an overflowed frame counts nothing): one wave
__global__ __launch_bounds__(64) void jpeg_offsets_kernel(const int32_t* __restrict__ sizes, int frames,
                                                          int64_t* __restrict__ offsets) {
    const int lane = threadIdx.x;
    const auto add = [](int64_t a, int64_t b) { return a + b; };
    int64_t carry = 0;
    for (int base = 0; base < frames; base += 64) {
        const int i = base + lane;
        const int64_t v = i < frames ? max(sizes[i], 0) : 0;
        const int64_t incl = wave_scan(v, (int64_t)0, add);
        if (i < frames) offsets[i] = carry + incl - v;
        carry += wave_readlane(incl, 63);
    }
    if (lane == 0) offsets[frames] = carry;
}

// frame blockIdx.x's stream from its slot to its place in the packed run, 16 bytes a lane and step
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const int32_t* __restrict__ sizes,
                                                        const int64_t* __restrict__ offsets,
                                                        const uint8_t* __restrict__ slots, int64_t cap,
                                                        uint8_t* __restrict__ packed) {
    const int f = blockIdx.x;
    const int n = max(sizes[f], 0);
    const uint8_t* src = slots + (int64_t)f * cap;
    uint8_t* dst = packed + offsets[f];
    const int stride = 16 * 256 * gridDim.y;
    for (int i = 16 * (blockIdx.y * 256 + threadIdx.x); i < n; i += stride) {
        if (i + 16 <= n) {
            uint4 v;
            __builtin_memcpy(&v, src + i, 16);
            __builtin_memcpy(dst + i, &v, 16);
        } else {
            for (int j = i; j < n; ++j) dst[j] = src[j];
        }
    }
}

}  // namespace

hipError_t launch_jpeg(const uint8_t* img, int64_t frame_stride, int ld, int h, int w, int frames, const JpegConst* jc,
                       const JpegWork& wk, uint8_t* out, int64_t cap, int32_t* sizes, hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    if (!img || !jc || !wk.coef || !wk.lane || !wk.ilen || !wk.ioff || !out || !sizes || cap < 0 || h < 1 ||
        h > kJpegMaxDim || w < 1 || w > kJpegMaxDim || ld < 3 * w || frame_stride < 0)
        return hipErrorInvalidValue;
    const int mr = jpeg_mcu_rows(h), mc = jpeg_mcu_cols(w), chunks = (mc + kMcuWg - 1) / kMcuWg;
    const int64_t intervals = (int64_t)frames * mr, xblocks = intervals * chunks;
    if (xblocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    const bool vec = w % 16 == 0 && ((reinterpret_cast<uintptr_t>(img) | (uintptr_t)frame_stride | (uintptr_t)ld) & 15u) == 0;
    if (vec)
        hipLaunchKernelGGL(jpeg_transform_kernel<true>, dim3((unsigned)xblocks), dim3(kXformThreads), 0, s, img,
                           frame_stride, ld, h, w, mr, mc, chunks, jc, wk.coef);
    else
        hipLaunchKernelGGL(jpeg_transform_kernel<false>, dim3((unsigned)xblocks), dim3(kXformThreads), 0, s, img,
                           frame_stride, ld, h, w, mr, mc, chunks, jc, wk.coef);
    const unsigned iblocks = (unsigned)((intervals + 3) / 4);
    hipLaunchKernelGGL(jpeg_size_kernel, dim3(iblocks), dim3(256), 0, s, jc, wk.coef, mc, intervals, wk.lane, wk.ilen);
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, s, jc, wk.ilen, mr, frames,
                       cap, wk.ioff, sizes);
    hipLaunchKernelGGL(jpeg_write_kernel, dim3(iblocks), dim3(256), 0, s, jc, wk.coef, mr, mc, intervals, wk.lane,
                       wk.ilen, wk.ioff, sizes, out, cap);
    return hipGetLastError();
}

hipError_t launch_jpeg_pack(const int32_t* sizes, int frames, const uint8_t* slots, int64_t cap, int64_t* offsets,
                            uint8_t* packed, hipStream_t s) {
    if (frames <= 0) return hipSuccess;
    if (!sizes || !slots || !offsets || !packed || cap < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(64), 0, s, sizes, frames, offsets);
    const unsigned parts = (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, cap / (16 * 256 * 4)));
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)frames, parts), dim3(256), 0, s, sizes, offsets, slots, cap,
                       packed);
    return hipGetLastError();
}

}  // namespace svx
