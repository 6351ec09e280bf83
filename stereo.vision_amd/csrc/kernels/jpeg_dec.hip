// The MJPG playback's JPEG decoder (gfx950): baseline 4:2:0 streams, as kernels/jpeg.hip writes them or as another
// writer does (any DQT, DHT and DRI; DESIGN §7.12, restated in tests/jpeg_decode_numpy.py), to the BGR pictures
// libjpeg-turbo's default path decodes from them, byte for byte. Restart intervals are independent, so no workgroup
// waits for another:
//   scan     a workgroup takes a frame: 16 bytes of its scan a lane and step, the RSTn found, counted by wave scans
//            and written in order as the intervals' byte ranges; their number and sequence checked; the scan ends
//            at the first other marker (EOI).
//   entropy  a lane takes an interval (svx_jpeg_dec_host.h's walk, the one the host check runs; a wave's lanes span
//            several frames): the Huffman tables in LDS, every block assembled in the lane's 144 bytes of LDS and stored as eight 16-byte
//            vectors, int16 in zig-zag and MCU order (the encoder's scratch layout).
//   chroma   a lane takes a Cb or Cr block: dequantiser, the slow-integer IDCT in registers, samples into the frame's
//            chroma planes (the vertical taps of the upsampling cross MCU rows: 1 B a pixel through scratch against
//            2 B a pixel of coefficients read again, were the neighbour rows recomputed).
//   picture  a workgroup takes up to 32 MCUs of an MCU row: the luma IDCT a lane a block into LDS, the chroma rows
//            with their halo from the planes, then 16 pixels a lane: the h2v2 triangle filter, the colour
//            conversion, BGR stores (16-byte where the rows allow).
// Malformed entropy data sets the frame's status and faults nothing: a lane reads inside its interval's bytes and
// writes inside its interval's coefficients.
#include "../svx_jpeg_dec.h"
#include "../svx_wave.h"

namespace svx {

namespace {

constexpr int kDecMcuWg = 32;          // MCUs of a picture workgroup
constexpr int kDecThreads = 128;       // its lanes: 32 MCUs x 4 luma blocks
constexpr int kDecBlkStride = 72;      // int16 of a lane's block in LDS: 144 bytes, so that 16 lanes' 16-byte reads
                                       // fall on 16 different slots (36 l mod 64 are the multiples of 4)
constexpr int kDecChromaCols = 8 * kDecMcuWg + 2;
constexpr int kNoStop = 0x7FFFFFFF;

// natural index of zig-zag position k (jpeg_tables::kZigzag, for the device; every use is unrolled and folds)
__device__ const uint8_t kDecNat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// One pass of the IJG slow-integer inverse DCT (jidctint, 13-bit constants) over eight values, descaled by N bits:
// 11 for the columns (2 extra bits kept), 18 for the rows.
template <int N>
__device__ __forceinline__ void idct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int r = 1 << (N - 1);
    int z1 = (d2 + d6) * 4433;
    const int t2 = z1 - d6 * 15137, t3 = z1 + d2 * 6270;
    const int t0 = (int)((uint32_t)(d0 + d4) << 13), t1 = (int)((uint32_t)(d0 - d4) << 13);
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    z1 = d7 + d1;
    int z2 = d5 + d3, z3 = d7 + d3, z4 = d5 + d1;
    const int z5 = (z3 + z4) * 9633;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    const int u0 = d7 * 2446 + z1 + z3, u1 = d5 * 16819 + z2 + z4, u2 = d3 * 25172 + z2 + z3,
              u3 = d1 * 12299 + z1 + z4;
    d0 = (t10 + u3 + r) >> N;
    d7 = (t10 - u3 + r) >> N;
    d1 = (t11 + u2 + r) >> N;
    d6 = (t11 - u2 + r) >> N;
    d2 = (t12 + u1 + r) >> N;
    d5 = (t12 - u1 + r) >> N;
    d3 = (t13 + u0 + r) >> N;
    d4 = (t13 - u0 + r) >> N;
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// A block's 64 quantised coefficients (zig-zag) times the table q (zig-zag), through the IDCT: row i's eight
// samples as bytes in rows[i].
__device__ __forceinline__ void block_samples(const uint4* __restrict__ cp, const uint16_t* __restrict__ q,
                                              uint2 (&rows)[8]) {
    int d[64];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const uint4 v = cp[g];
        const uint4 t = reinterpret_cast<const uint4*>(q)[g];
        const uint32_t cw[4] = {v.x, v.y, v.z, v.w}, qw[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = (int)(int16_t)(cw[j >> 1] >> (16 * (j & 1)));
            const int e = (int)((qw[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
            d[kDecNat[8 * g + j]] = c * e;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
        idct8<11>(d[j], d[8 + j], d[16 + j], d[24 + j], d[32 + j], d[40 + j], d[48 + j], d[56 + j]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        idct8<18>(d[8 * i], d[8 * i + 1], d[8 * i + 2], d[8 * i + 3], d[8 * i + 4], d[8 * i + 5], d[8 * i + 6],
                  d[8 * i + 7]);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lo |= (uint32_t)clamp255(d[8 * i + j] + 128) << (8 * j);
            hi |= (uint32_t)clamp255(d[8 * i + 4 + j] + 128) << (8 * j);
        }
        rows[i] = make_uint2(lo, hi);
    }
}

// ---- the marker scan ----
__global__ __launch_bounds__(256) void jpeg_dec_scan_kernel(const uint8_t* __restrict__ packed,
                                                            const JpegDecFrame* __restrict__ fr, int maxi,
                                                            int32_t* __restrict__ first, int32_t* __restrict__ end,
                                                            int32_t* __restrict__ status) {
    __shared__ int wsum[4];
    __shared__ int s_stop, s_order;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t f = blockIdx.x;
    const JpegDecFrame F = fr[f];
    const uint8_t* s = packed + F.at;
    const int n = F.len;
    int32_t* fi = first + f * maxi;
    int32_t* en = end + f * maxi;
    if (tid == 0) s_stop = kNoStop, s_order = 0;
    __syncthreads();
    const auto add = [](int a, int b) { return a + b; };
    int carry = 0, stop = kNoStop;
    for (int base = F.scan_at; base < n && stop == kNoStop; base += 256 * 16) {
        const int i0 = base + 16 * tid;
        uint8_t b[17];
        if (i0 + 17 <= n) {
            uint4 v;
            __builtin_memcpy(&v, s + i0, 16);
            __builtin_memcpy(b, &v, 16);
            b[16] = s[i0 + 16];
        } else {
#pragma unroll
            for (int j = 0; j < 17; ++j) b[j] = i0 + j < n ? s[i0 + j] : (uint8_t)0;   // no marker ends in a zero
        }
        uint32_t rst = 0;
        int other = kNoStop;
#pragma unroll
        for (int j = 15; j >= 0; --j) {
            if (b[j] != 0xFF) continue;
            const int m = b[j + 1];
            if (m >= 0xD0 && m <= 0xD7) rst |= 1u << j;
            else if (m != 0 && m != 0xFF) other = i0 + j;
        }
        if (other != kNoStop) atomicMin(&s_stop, other);
        __syncthreads();
        stop = s_stop;
        // the RSTn in front of the scan's end
        const int lim = stop - i0;   // positions j < lim count
        if (lim < 16) rst &= lim <= 0 ? 0u : (1u << lim) - 1u;
        const int cnt = __popc(rst);
        const int incl = wave_scan(cnt, 0, add);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int k = carry + incl - cnt;
        for (int u = 0; u < wv; ++u) k += wsum[u];
        const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        bool wrong = false;
        while (rst) {
            const int j = __ffs(rst) - 1;
            rst &= rst - 1;
            if ((int)b[j + 1] - 0xD0 != (k & 7)) wrong = true;
            if (k + 1 < F.intervals) en[k] = i0 + j, fi[k + 1] = i0 + j + 2;
            ++k;
        }
        if (wrong) s_order = 1;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) {
        int st = stop == kNoStop ? kJpegDecNoEoi : kJpegDecOk;
        bool ok = true;
        if (carry != F.intervals - 1) st = max(st, (int)kJpegDecRstCount), ok = false;
        if (s_order) st = max(st, (int)kJpegDecRstOrder), ok = false;
        if (ok) {
            fi[0] = F.scan_at;
            en[F.intervals - 1] = min(stop, n);
        } else {
            fi[0] = -1;   // no intervals to walk
        }
        status[f] = st;
    }
}

// ---- the entropy walk ----
// A lane takes interval g = f * maxi + k of the launch (idle where frame f has fewer than k + 1 intervals, or its
// RSTn were wrong), so a wave's lanes span several frames when a frame has fewer than 64. The wave keeps the tables
// of its first frame in LDS; a lane of a frame with other tables reads them from memory (streams of one recording
// share their tables).
__global__ __launch_bounds__(64) void jpeg_dec_entropy_kernel(const uint8_t* __restrict__ packed,
                                                              const JpegDecFrame* __restrict__ fr,
                                                              const JpegDecTables* __restrict__ tabs, int maxi,
                                                              int64_t lanes, int mcus_frame,
                                                              const int32_t* __restrict__ first,
                                                              const int32_t* __restrict__ end,
                                                              int16_t* __restrict__ coef,
                                                              int32_t* __restrict__ status) {
    __shared__ JpegDecTables st;
    __shared__ __attribute__((aligned(16))) int16_t sblk[64][kDecBlkStride];
    const int lane = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * 64;
    const int tab0 = fr[g0 / maxi].tab;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(tabs + tab0);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&st);
        for (int i = lane; i < (int)(sizeof(JpegDecTables) / 4); i += 64) dst[i] = src[i];
    }
    __syncthreads();
    const int64_t g = g0 + lane;
    if (g >= lanes) return;
    const int64_t f = g / maxi;
    const int k = (int)(g - f * maxi);
    const JpegDecFrame F = fr[f];
    if (k >= F.intervals || first[f * maxi] < 0) return;
    // the interval's bytes, inside the stream's scan whatever the scratch holds
    int a = first[g], e = end[g];
    a = min(max(a, F.scan_at), F.len);
    e = min(max(e, a), F.len);
    const int m0 = k * F.per;
    const int mcus = min(F.per, mcus_frame - m0);
    if (mcus <= 0) return;
    uint4* dst = reinterpret_cast<uint4*>(coef + (f * mcus_frame + m0) * 384);
    const auto sink = [dst](int m, int blk, const int16_t* v) {
        const uint4* src = reinterpret_cast<const uint4*>(v);
        uint4* d = dst + (m * 6 + blk) * 8;
#pragma unroll
        for (int u = 0; u < 8; ++u) d[u] = src[u];
    };
    // two copies of the walk, so that the usual one reads its tables with LDS instructions
    const int rc = F.tab == tab0 ? jpeg_dec_interval(packed + F.at + a, e - a, st, mcus, sblk[lane], sink)
                                 : jpeg_dec_interval(packed + F.at + a, e - a, tabs[F.tab], mcus, sblk[lane], sink);
    if (rc) atomicMax(status + f, rc);
}

// ---- the chroma planes ----
__global__ __launch_bounds__(256) void jpeg_dec_chroma_kernel(const JpegDecFrame* __restrict__ fr,
                                                              const JpegDecQuant* __restrict__ quant,
                                                              const int16_t* __restrict__ coef, int mc,
                                                              int mcus_frame, int64_t blocks,
                                                              uint8_t* __restrict__ chroma) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= blocks) return;
    const int c = (int)(u & 1);
    const int64_t fm = u >> 1, f = fm / mcus_frame;
    const int m = (int)(fm - f * mcus_frame), r = m / mc, col = m - r * mc;
    uint2 rows[8];
    block_samples(reinterpret_cast<const uint4*>(coef + (fm * 6 + 4 + c) * 64), quant[fr[f].tab].q[1 + c], rows);
    uint8_t* plane = chroma + (f * 2 + c) * (int64_t)mcus_frame * 64;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        *reinterpret_cast<uint2*>(plane + ((int64_t)(8 * r + i) * mc + col) * 8) = rows[i];
}

// ---- the picture ----
template <bool VEC>
__global__ __launch_bounds__(kDecThreads) void jpeg_dec_picture_kernel(const JpegDecFrame* __restrict__ fr,
                                                                       const JpegDecQuant* __restrict__ quant,
                                                                       const int16_t* __restrict__ coef,
                                                                       const uint8_t* __restrict__ chroma, int h,
                                                                       int w, int mr, int mc, int chunks,
                                                                       uint8_t* __restrict__ out,
                                                                       int64_t frame_stride, int64_t ld) {
    __shared__ __attribute__((aligned(16))) uint8_t sy[16][16 * kDecMcuWg];
    __shared__ uint8_t sc[2][10][kDecChromaCols + 2];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x % chunks;
    const int r = (blockIdx.x / chunks) % mr;
    const int64_t f = blockIdx.x / (chunks * mr);
    const int m0 = chunk * kDecMcuWg, nm = min(kDecMcuWg, mc - m0);
    const int mcus_frame = mr * mc;
    const JpegDecQuant* q = quant + fr[f].tab;
    {   // a lane a luma block: block k of MCU m0 + m
        const int k = tid / kDecMcuWg, m = tid % kDecMcuWg;
        if (m < nm) {
            uint2 rows[8];
            block_samples(reinterpret_cast<const uint4*>(coef + ((f * mcus_frame + (int64_t)r * mc + m0 + m) * 6 + k) * 64),
                          q->q[0], rows);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                *reinterpret_cast<uint2*>(&sy[8 * (k >> 1) + i][16 * m + 8 * (k & 1)]) = rows[i];
        }
    }
    // chroma rows 8 r - 1 .. 8 r + 8 and columns 8 m0 - 1 .. 8 (m0 + nm) of the cropped planes (ceil(h / 2) x
    // ceil(w / 2)), the edges repeated
    const int ch = (h + 1) >> 1, cw = (w + 1) >> 1, ncol = 8 * nm + 2;
    for (int u = tid; u < 2 * 10 * ncol; u += kDecThreads) {
        const int c = u / (10 * ncol), v = u - c * 10 * ncol, rr = v / ncol, cc = v - rr * ncol;
        const int row = min(max(8 * r - 1 + rr, 0), ch - 1), col = min(max(8 * m0 - 1 + cc, 0), cw - 1);
        sc[c][rr][cc] = chroma[(f * 2 + c) * (int64_t)mcus_frame * 64 + (int64_t)row * (8 * mc) + col];
    }
    __syncthreads();
    uint8_t* pic = out + f * frame_stride;
    for (int u = tid; u < nm * 16; u += kDecThreads) {
        const int p = u / nm, m = u - p * nm;
        const int y = 16 * r + p, x0 = 16 * (m0 + m);
        if (y >= h) continue;
        // s = 3 near + far of the ten chroma columns around the MCU's eight
        const int near = 1 + (p >> 1), far = (p & 1) ? near + 1 : near - 1;
        int sb[10], sr[10];
#pragma unroll
        for (int j = 0; j < 10; ++j) {
            sb[j] = 3 * sc[0][near][8 * m + j] + sc[0][far][8 * m + j];
            sr[j] = 3 * sc[1][near][8 * m + j] + sc[1][far][8 * m + j];
        }
        const uint4 yv = *reinterpret_cast<const uint4*>(&sy[p][16 * m]);
        const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
        uint32_t o[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) o[i] = 0;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int c = 1 + (t >> 1);
            const int cb = ((t & 1) ? (3 * sb[c] + sb[c + 1] + 7) >> 4 : (3 * sb[c] + sb[c - 1] + 8) >> 4) - 128;
            const int cr = ((t & 1) ? (3 * sr[c] + sr[c + 1] + 7) >> 4 : (3 * sr[c] + sr[c - 1] + 8) >> 4) - 128;
            const int yy = (int)((yw[t >> 2] >> (8 * (t & 3))) & 255u);
            const uint32_t px[3] = {(uint32_t)clamp255(yy + ((116130 * cb + 32768) >> 16)),
                                    (uint32_t)clamp255(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16)),
                                    (uint32_t)clamp255(yy + ((91881 * cr + 32768) >> 16))};
#pragma unroll
            for (int e = 0; e < 3; ++e) o[(3 * t + e) >> 2] |= px[e] << (8 * ((3 * t + e) & 3));
        }
        uint8_t* dst = pic + (int64_t)y * ld + 3 * x0;
        if constexpr (VEC) {
#pragma unroll
            for (int g = 0; g < 3; ++g)
                reinterpret_cast<uint4*>(dst)[g] = make_uint4(o[4 * g], o[4 * g + 1], o[4 * g + 2], o[4 * g + 3]);
        } else {
            const int nb = 3 * min(16, w - x0);   // > 0: the MCU holds a column of the picture
#pragma unroll
            for (int i = 0; i < 48; ++i)
                if (i < nb) dst[i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
        }
    }
}

}  // namespace

hipError_t launch_jpeg_decode(const uint8_t* packed, const JpegDecFrame* fr, const JpegDecTables* tabs,
                              const JpegDecQuant* quant, int frames, int h, int w, int maxi, const JpegDecWork& wk,
                              uint8_t* out, int64_t frame_stride, int64_t ld, int32_t* status, hipStream_t s,
                              hipEvent_t* ev) {
    if (frames <= 0) return hipSuccess;
    if (!packed || !fr || !tabs || !quant || !wk.coef || !wk.chroma || !wk.first || !wk.end || !out || !status ||
        h < 1 || h > kJpegMaxDim || w < 1 || w > kJpegMaxDim || ld < 3 * (int64_t)w || frame_stride < 0 || maxi < 1)
        return hipErrorInvalidValue;
    const int mr = jpeg_mcu_rows(h), mc = jpeg_mcu_cols(w), chunks = (mc + kDecMcuWg - 1) / kDecMcuWg;
    const int mcus = mr * mc;
    const int64_t lanes = (int64_t)frames * maxi, eblocks = (lanes + 63) / 64, cblocks = (int64_t)frames * mcus * 2;
    const int64_t pblocks = (int64_t)frames * mr * chunks;
    if (eblocks > 0x7FFFFFFF || (cblocks + 255) / 256 > 0x7FFFFFFF || pblocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipError_t e = hipSuccess;
    const auto mark = [&](int i) {
        if (ev && e == hipSuccess) e = hipEventRecord(ev[i], s);
    };
    mark(0);
    hipLaunchKernelGGL(jpeg_dec_scan_kernel, dim3((unsigned)frames), dim3(256), 0, s, packed, fr, maxi, wk.first,
                       wk.end, status);
    mark(1);
    hipLaunchKernelGGL(jpeg_dec_entropy_kernel, dim3((unsigned)eblocks), dim3(64), 0, s, packed, fr, tabs, maxi, lanes,
                       mcus, wk.first, wk.end, wk.coef, status);
    mark(2);
    hipLaunchKernelGGL(jpeg_dec_chroma_kernel, dim3((unsigned)((cblocks + 255) / 256)), dim3(256), 0, s, fr, quant,
                       wk.coef, mc, mcus, cblocks, wk.chroma);
    mark(3);
    const bool vec = w % 16 == 0 && ((reinterpret_cast<uintptr_t>(out) | (uintptr_t)frame_stride | (uintptr_t)ld) & 15u) == 0;
    if (vec)
        hipLaunchKernelGGL(jpeg_dec_picture_kernel<true>, dim3((unsigned)pblocks), dim3(kDecThreads), 0, s, fr, quant,
                           wk.coef, wk.chroma, h, w, mr, mc, chunks, out, frame_stride, ld);
    else
        hipLaunchKernelGGL(jpeg_dec_picture_kernel<false>, dim3((unsigned)pblocks), dim3(kDecThreads), 0, s, fr, quant,
                           wk.coef, wk.chroma, h, w, mr, mc, chunks, out, frame_stride, ld);
    mark(4);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

}  // namespace svx
