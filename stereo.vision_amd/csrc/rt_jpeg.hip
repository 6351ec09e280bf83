// svx runtime: the MJPG recording's JPEG encoder (loop.py:49-54,82-89; kernels/jpeg.hip) as a
// host-picture entry point and as the batch stage behind the image tile, with the pack that lets a batch's streams
// leave the device in one copy.
#include "svx_jpeg.h"
#include "svx_jpeg_host.h"
#include "svx_runtime.h"
#include "svx_tile_host.h"

namespace {

size_t up16(size_t v) { return (v + 15) / 16 * 16; }

JpegWork work_at(char* base, const JpegWorkLayout& l) {
    return JpegWork{reinterpret_cast<int16_t*>(base + l.off_coef), reinterpret_cast<uint2*>(base + l.off_lane),
                    reinterpret_cast<int32_t*>(base + l.off_ilen), reinterpret_cast<int32_t*>(base + l.off_ioff)};
}

int need_jpeg(const sv_batch* b) {
    return b->road_level >= kRoadJpeg ? SV_OK : fail(SV_E_STATE, "no current JPEG streams (sv_batch_jpeg first)");
}

}  // namespace

extern "C" {

int64_t sv_jpeg_bound(int h, int w) { return jpeg_bound(h, w); }

int sv_jpeg_encode(const uint8_t* bgr, int h, int w, int64_t ld, int quality, uint8_t* out, int64_t cap,
                   int64_t* size) {
    if (const char* why = jpeg_check_args(bgr, h, w, ld, quality, out, cap, size))
        return fail(SV_E_ARG, "sv_jpeg_encode: bad arguments (%s)", why);
    *size = 0;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    JpegConst jc;
    jpeg_build(h, w, quality, &jc);
    // const | the picture at a 16-byte row stride | the scratch | the size | the stream (no more than the bound)
    const size_t ld16 = up16(3 * (size_t)w), img = ld16 * (size_t)h;
    const int64_t dcap = std::min(cap, jpeg_bound(h, w));
    const JpegWorkLayout wl = jpeg_work_layout(h, w, 1);
    const size_t off_img = up16(sizeof jc), off_work = off_img + img, off_size = off_work + wl.bytes;
    const size_t off_out = off_size + 16;
    HIP_TRY(d->jpg.ensure(off_out + up16((size_t)dcap)));
    char* base = d->jpg.as<char>();
    HIP_TRY(hipMemcpyAsync(base, &jc, sizeof jc, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpy2DAsync(base + off_img, ld16, bgr, (size_t)ld, 3 * (size_t)w, h, hipMemcpyHostToDevice, s));
    int32_t* dsize = reinterpret_cast<int32_t*>(base + off_size);
    HIP_TRY(launch_jpeg(reinterpret_cast<const uint8_t*>(base + off_img), 0, (int)ld16, h, w, 1,
                        reinterpret_cast<const JpegConst*>(base), work_at(base + off_work, wl),
                        reinterpret_cast<uint8_t*>(base + off_out), dcap, dsize, s));
    int32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, dsize, sizeof n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n < 0) {
        *size = -(int64_t)n;
        return fail(SV_E_CAP, "sv_jpeg_encode: capacity %lld < %lld bytes of stream", (long long)cap, (long long)-n);
    }
    *size = n;
    HIP_TRY(hipMemcpyAsync(out, base + off_out, (size_t)n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_jpeg(sv_batch* b, int quality, int64_t cap_per_frame, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (quality < 1 || quality > 100 || cap_per_frame < 0 || cap_per_frame > 0x7FFFFFFF)
        return fail(SV_E_ARG, "sv_batch_jpeg: 1 <= quality <= 100, 0 <= cap_per_frame < 2^31");
    if (b->road_level < kRoadTile) return fail(SV_E_STATE, "no current image tile (sv_batch_tile first)");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    for (int i = 0; i < 2; ++i)
        if (!b->road_ev[kEvJpeg + i]) HIP_TRY(hipEventCreate(&b->road_ev[kEvJpeg + i]));
    b->road_level = kRoadTile;
    b->jpacked = false;
    const int h = b->H / 2, w = b->Wu;
    const int64_t cap = cap_per_frame ? cap_per_frame : jpeg_default_cap(h, w);
    if (b->jhost.size() != sizeof(JpegConst) || b->jquality != quality) {   // the tables and header of this quality
        HIP_TRY(hipStreamSynchronize(s));   // an earlier copy of the host block has landed
        b->jhost.resize(sizeof(JpegConst));
        jpeg_build(h, w, quality, reinterpret_cast<JpegConst*>(b->jhost.data()));
        HIP_TRY(b->jconst.ensure(sizeof(JpegConst)));
        HIP_TRY(hipMemcpyAsync(b->jconst.p, b->jhost.data(), sizeof(JpegConst), hipMemcpyHostToDevice, s));
        b->jquality = quality;
    }
    // the scratch is 3 B a pixel, the tile's own size: the frames go through it in chunks of at most 1 GiB and half
    // the free memory (what the batch holds of it already counted as free), at least a frame
    if (b->jchunk <= 0) {
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        const size_t slots = (size_t)cap * b->frames;
        const size_t budget = std::min<size_t>((size_t)1 << 30, (fr > slots ? fr - slots : 0) / 2);
        const size_t per = jpeg_work_frame_bytes(h, w) + 64;
        b->jchunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)b->frames, budget / per));
    }
    const JpegWorkLayout wl = jpeg_work_layout(h, w, b->jchunk);
    HIP_TRY(b->jwork.ensure(wl.bytes, false, 0, true));
    HIP_TRY(b->jout.ensure((size_t)cap * b->frames, false, 0, true));
    HIP_TRY(b->jsizes.ensure(sizeof(int32_t) * (size_t)b->frames));
    b->jcap = cap;
    const size_t tile = tile_frame_bytes(b->H, b->Wu);
    const JpegWork wk = work_at(b->jwork.as<char>(), wl);
    HIP_TRY(hipEventRecord(b->road_ev[kEvJpeg], s));
    for (int f0 = 0; f0 < b->frames; f0 += b->jchunk) {
        const int n = std::min(b->jchunk, b->frames - f0);
        HIP_TRY(launch_jpeg(b->timg.as<uint8_t>() + tile * f0, (int64_t)tile, 3 * w, h, w, n, b->jconst.as<JpegConst>(),
                            wk, b->jout.as<uint8_t>() + (size_t)cap * f0, cap, b->jsizes.as<int32_t>() + f0, s));
    }
    HIP_TRY(hipEventRecord(b->road_ev[kEvJpeg + 1], s));
    b->road_level = kRoadJpeg;
    if (sync) HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_jpeg_ms(sv_batch* b, float* ms) {
    if (!b || !ms) return fail(SV_E_ARG, "null batch or ms");
    if (int rc = need_jpeg(b)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipEventSynchronize(b->road_ev[kEvJpeg + 1]));
    HIP_TRY(hipEventElapsedTime(ms, b->road_ev[kEvJpeg], b->road_ev[kEvJpeg + 1]));
    return SV_OK;
}

int sv_batch_jpeg_sizes(sv_batch* b, int32_t* out) {
    if (!b || !out) return fail(SV_E_ARG, "null batch or out");
    if (int rc = need_jpeg(b)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(out, b->jsizes.p, sizeof(int32_t) * (size_t)b->frames, hipMemcpyDeviceToHost));
    return SV_OK;
}

int sv_batch_read_jpeg(sv_batch* b, int frame, uint8_t* out, int64_t cap, int64_t* size) {
    if (!b || !out || !size || cap < 0 || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    *size = 0;
    if (int rc = need_jpeg(b)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    int32_t n = 0;
    HIP_TRY(hipMemcpy(&n, b->jsizes.as<int32_t>() + frame, sizeof n, hipMemcpyDeviceToHost));
    *size = n < 0 ? -(int64_t)n : n;
    if (n < 0)
        return fail(SV_E_CAP, "frame %d's stream of %lld bytes overflowed its slot of %lld", frame, (long long)-n,
                    (long long)b->jcap);
    if (n > cap) return fail(SV_E_CAP, "capacity %lld < %d bytes of stream", (long long)cap, n);
    HIP_TRY(hipMemcpy(out, b->jout.as<uint8_t>() + (size_t)b->jcap * frame, (size_t)n, hipMemcpyDeviceToHost));
    return SV_OK;
}

int sv_batch_jpeg_pack(sv_batch* b, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (int rc = need_jpeg(b)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(b->jpack.ensure((size_t)b->jcap * b->frames, false, 0, true));
    HIP_TRY(b->joffs.ensure(sizeof(int64_t) * ((size_t)b->frames + 1)));
    HIP_TRY(launch_jpeg_pack(b->jsizes.as<int32_t>(), b->frames, b->jout.as<uint8_t>(), b->jcap, b->joffs.as<int64_t>(),
                             b->jpack.as<uint8_t>(), b->stream));
    b->jpacked = true;
    if (sync) HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_read_jpeg_packed(sv_batch* b, uint8_t* out, int64_t cap, int64_t* offsets, int64_t* total) {
    if (!b || !out || !offsets || !total || cap < 0) return fail(SV_E_ARG, "bad args");
    *total = 0;
    if (int rc = need_jpeg(b)) return rc;
    if (!b->jpacked) return fail(SV_E_STATE, "the streams are not packed (sv_batch_jpeg_pack first)");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    std::vector<int64_t> offs((size_t)b->frames + 1);
    HIP_TRY(hipMemcpy(offs.data(), b->joffs.p, sizeof(int64_t) * offs.size(), hipMemcpyDeviceToHost));
    std::copy(offs.begin(), offs.end() - 1, offsets);
    *total = offs.back();
    if (*total > cap) return fail(SV_E_CAP, "capacity %lld < %lld bytes of streams", (long long)cap, (long long)*total);
    if (*total) HIP_TRY(hipMemcpy(out, b->jpack.p, (size_t)*total, hipMemcpyDeviceToHost));
    return SV_OK;
}

}  // extern "C"
