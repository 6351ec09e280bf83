// svx runtime: the general-scale bilinear resize (kernels/resize.hip) as host calls — a picture or n of them
// (resizeImage, functions.py:452-454), batchImages of one to five pictures composed on the device
// (functions.py:456-501) — and as a batch stage: the cleaned disparity at a display size.
#include <cstring>

#include "svx_resize.h"
#include "svx_resize_host.h"
#include "svx_runtime.h"

namespace {

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

extern "C" {

int sv_resize_coefficients(int dn, int sn, int32_t* s0, int32_t* s1, int16_t* c0, int16_t* c1) {
    if (!resize_coefficients(dn, sn, s0, s1, c0, c1))
        return fail(SV_E_ARG, "sv_resize_coefficients: four tables and 1 <= dn, sn <= %d (dn=%d sn=%d)", kResizeMaxSrc,
                    dn, sn);
    return SV_OK;
}

int sv_resize_linear_u8(const uint8_t* src, int n, int sh, int sw, int channels, uint8_t* dst, int dh, int dw) {
    if (const char* why = resize_check_args(src, n, sh, sw, channels, dst, dh, dw))
        return fail(SV_E_ARG, "sv_resize_linear_u8: bad arguments (%s)", why);
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    const ResizeTableLayout tl = resize_table_layout(dh, dw);
    const size_t sf = (size_t)sh * sw * channels, df = (size_t)dh * dw * channels;
    const size_t off_src = up256(tl.bytes), off_dst = off_src + up256(sf * n);
    std::vector<uint8_t> tabs(tl.bytes);
    if (!resize_fill_tables(tabs.data(), sh, sw, dh, dw)) return fail(SV_E_ARG, "sv_resize_linear_u8: bad shapes");
    HIP_TRY(d->rsz.ensure(off_dst + up256(df * n)));
    uint8_t* base = d->rsz.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(base, tabs.data(), tl.bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + off_src, src, sf * n, hipMemcpyHostToDevice, s));
    ResizeArgs a{};
    a.src = base + off_src, a.src_frame = (int64_t)sf, a.src_ld = sw * channels;
    a.sh = sh, a.sw = sw, a.sc = channels;
    a.dst = base + off_dst, a.dst_off = 0, a.dst_frame = (int64_t)df, a.dst_ld = dw * channels;
    a.dh = dh, a.dw = dw, a.dc = channels;
    a.tables = base;
    HIP_TRY(launch_resize_linear(a, n, s));
    HIP_TRY(hipMemcpyAsync(dst, base + off_dst, df * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));   // tabs lives until here
    return SV_OK;
}

int sv_images_tile_shape(int count, int H, int W, int* oh, int* ow) {
    ImagesTilePlan p;
    if (!oh || !ow) return fail(SV_E_ARG, "sv_images_tile_shape: null output");
    if (const char* why = images_tile_plan(count, H, W, &p))
        return fail(SV_E_ARG, "sv_images_tile_shape: not built (%s; count=%d H=%d W=%d)", why, count, H, W);
    *oh = p.out_h, *ow = p.out_w;
    return SV_OK;
}

int sv_images_tile(const sv_picture* pics, int count, int H, int W, uint8_t* out) {
    ImagesTilePlan p;
    if (!pics || !out) return fail(SV_E_ARG, "sv_images_tile: null pictures or out");
    if (const char* why = images_tile_plan(count, H, W, &p))
        return fail(SV_E_ARG, "sv_images_tile: not built (%s; count=%d H=%d W=%d)", why, count, H, W);
    const size_t out_bytes = (size_t)p.out_h * p.out_w * 3;
    for (int i = 0; i < count; ++i) {
        const sv_picture& q = pics[i];
        if (!q.data || (q.channels != 1 && q.channels != 3) || q.h < 1 || q.h > kResizeMaxDst || q.w < 1 ||
            q.w > kResizeMaxDst)
            return fail(SV_E_ARG, "sv_images_tile: picture %d needs data, 1 or 3 channels and dimensions in 1 .. %d", i,
                        kResizeMaxDst);
        if (resize_overlap(out, out_bytes, q.data, (size_t)q.h * q.w * q.channels))
            return fail(SV_E_ARG, "sv_images_tile: out overlaps picture %d", i);
    }
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    // the device block: every resize's tables (one per picture, the stack's, the fifth picture's half) | the staged
    // pictures | the stack | picture 4 at H x W | the output
    size_t tab_off[7] = {}, pic_off[5] = {}, at = 0;
    for (int i = 0; i < count; ++i) tab_off[i] = at, at += up256(resize_table_layout(H, W).bytes);
    const int t_stack = 5, t_half = 6;
    if (count > 1) tab_off[t_stack] = at, at += up256(resize_table_layout(p.left_h, p.left_w).bytes);
    if (count == 5) tab_off[t_half] = at, at += up256(resize_table_layout(H / 2, W / 2).bytes);
    const size_t tab_bytes = at;
    for (int i = 0; i < count; ++i) pic_off[i] = at, at += up256((size_t)pics[i].h * pics[i].w * pics[i].channels);
    const size_t off_stack = at;
    at += up256((size_t)p.stack_h * p.stack_w * 3);
    const size_t off_fifth = at;
    if (count == 5) at += up256((size_t)H * W * 3);
    const size_t off_out = at;
    at += up256(out_bytes);
    std::vector<uint8_t> tabs(tab_bytes);
    bool ok = true;
    for (int i = 0; i < count; ++i) ok = ok && resize_fill_tables(tabs.data() + tab_off[i], pics[i].h, pics[i].w, H, W);
    if (count > 1) ok = ok && resize_fill_tables(tabs.data() + tab_off[t_stack], p.stack_h, p.stack_w, p.left_h, p.left_w);
    if (count == 5) ok = ok && resize_fill_tables(tabs.data() + tab_off[t_half], H, W, H / 2, W / 2);
    if (!ok) return fail(SV_E_ARG, "sv_images_tile: a shape out of range");
    HIP_TRY(d->rsz.ensure(at));
    uint8_t* base = d->rsz.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(base, tabs.data(), tab_bytes, hipMemcpyHostToDevice, s));
    for (int i = 0; i < count; ++i)
        HIP_TRY(hipMemcpyAsync(base + pic_off[i], pics[i].data, (size_t)pics[i].h * pics[i].w * pics[i].channels,
                               hipMemcpyHostToDevice, s));
    // picture i to H x W x 3 at dst + off, rows ld apart (resizeImage, then COLOR_GRAY2BGR)
    const auto place = [&](int i, uint8_t* dst, int64_t off, int ld) {
        ResizeArgs a{};
        a.src = base + pic_off[i], a.src_frame = 0, a.src_ld = pics[i].w * pics[i].channels;
        a.sh = pics[i].h, a.sw = pics[i].w, a.sc = pics[i].channels;
        a.dst = dst, a.dst_off = off, a.dst_frame = 0, a.dst_ld = ld;
        a.dh = H, a.dw = W, a.dc = 3;
        a.tables = base + tab_off[i];
        return launch_resize_linear(a, 1, s);
    };
    if (count == 1) {
        HIP_TRY(place(0, base + off_out, 0, 3 * W));
    } else {
        const int sld = 3 * p.stack_w;
        for (int q = 0; q < p.quadrants; ++q)
            HIP_TRY(place(p.pic_of[q], base + off_stack, (int64_t)(q / 2) * H * sld + (int64_t)(q % 2) * 3 * W, sld));
        ResizeArgs a{};
        a.src = base + off_stack, a.src_ld = sld, a.sh = p.stack_h, a.sw = p.stack_w, a.sc = 3;
        a.dst = base + off_out, a.dst_off = 0, a.dst_ld = 3 * p.out_w, a.dh = p.left_h, a.dw = p.left_w, a.dc = 3;
        a.tables = base + tab_off[t_stack];
        HIP_TRY(launch_resize_linear(a, 1, s));
        if (count == 5) {
            HIP_TRY(place(4, base + off_fifth, 0, 3 * W));
            ResizeArgs r{};
            r.src = base + off_fifth, r.src_ld = 3 * W, r.sh = H, r.sw = W, r.sc = 3;
            r.dst = base + off_out, r.dst_off = 3 * (int64_t)p.left_w, r.dst_ld = 3 * p.out_w, r.dh = H / 2, r.dw = W / 2;
            r.dc = 3;
            r.tables = base + tab_off[t_half];
            HIP_TRY(launch_resize_linear(r, 1, s));
        }
    }
    HIP_TRY(hipMemcpyAsync(out, base + off_out, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));   // tabs lives until here
    return SV_OK;
}

// ---------------------------------------------------------------------------
// the batch: the cleaned disparity at a display size
// ---------------------------------------------------------------------------
int sv_batch_resize_disp(sv_batch* b, int dh, int dw, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (const char* why = resize_check_shape(b->H, b->Wu, dh, dw))
        return fail(SV_E_ARG, "sv_batch_resize_disp: %s (frames of %d x %d to %d x %d)", why, b->H, b->Wu, dh, dw);
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    for (hipEvent_t& e : b->rd_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    b->rdisp_fresh = false;
    const ResizeTableLayout tl = resize_table_layout(dh, dw);
    if (b->rdtab_h != dh || b->rdtab_w != dw) {   // new tables: after whatever still reads the old ones
        std::vector<uint8_t> tabs(tl.bytes);
        if (!resize_fill_tables(tabs.data(), b->H, b->Wu, dh, dw)) return fail(SV_E_ARG, "sv_batch_resize_disp: bad shapes");
        HIP_TRY(hipStreamSynchronize(s));
        b->rdtab_h = b->rdtab_w = 0;
        HIP_TRY(b->rdtab.ensure(tl.bytes));
        HIP_TRY(hipMemcpy(b->rdtab.p, tabs.data(), tl.bytes, hipMemcpyHostToDevice));
        b->rdtab_h = dh, b->rdtab_w = dw;
    }
    const size_t df = (size_t)dh * dw;
    if (b->rdisp.bytes < df * b->frames) HIP_TRY(hipStreamSynchronize(s));   // ensure() frees the old buffer
    HIP_TRY(b->rdisp.ensure(df * b->frames, false, 0, true));
    ResizeArgs a{};
    a.src = b->disp.as<uint8_t>(), a.src_frame = (int64_t)b->H * b->W, a.src_ld = b->W;
    a.sh = b->H, a.sw = b->Wu, a.sc = 1;
    a.dst = b->rdisp.as<uint8_t>(), a.dst_off = 0, a.dst_frame = (int64_t)df, a.dst_ld = dw;
    a.dh = dh, a.dw = dw, a.dc = 1;
    a.tables = b->rdtab.as<uint8_t>();
    HIP_TRY(hipEventRecord(b->rd_ev[0], s));
    HIP_TRY(launch_resize_linear(a, b->frames, s));
    HIP_TRY(hipEventRecord(b->rd_ev[1], s));
    b->rd_h = dh, b->rd_w = dw;
    b->rdisp_fresh = true;
    if (sync) HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_resize_disp_ms(sv_batch* b, float* ms) {
    if (!b || !ms) return fail(SV_E_ARG, "null batch or ms");
    if (!b->rdisp_fresh) return fail(SV_E_STATE, "no current resized disparity (sv_batch_resize_disp first)");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipEventSynchronize(b->rd_ev[1]));
    HIP_TRY(hipEventElapsedTime(ms, b->rd_ev[0], b->rd_ev[1]));
    return SV_OK;
}

int sv_batch_read_resized_disp(sv_batch* b, int frame, uint8_t* out) {
    if (!b || !out || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    if (!b->rdisp_fresh) return fail(SV_E_STATE, "no current resized disparity (sv_batch_resize_disp first)");
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    const size_t bytes = (size_t)b->rd_h * b->rd_w;
    HIP_TRY(hipMemcpy(out, b->rdisp.as<uint8_t>() + bytes * frame, bytes, hipMemcpyDeviceToHost));
    return SV_OK;
}

}  // extern "C"
