// svx runtime: the disparity pre-pass, as host-frame drop-ins and over a batch.
#include "svx_runtime.h"

namespace svx {

int batch_prepass_impl(sv_batch* b, int option, const uint8_t* dprev0) {
    uint8_t* masked = nullptr;
    const uint8_t* mff = nullptr;
    uint8_t* disp = b->disp.as<uint8_t>();
    const uint8_t* in = input_disp(b);   // keep_input: the raw frames, read here and never written
    const int64_t px = (int64_t)b->H * b->W;
    b->rdisp_fresh = false;   // new cleaned frames: a resized disparity is not theirs
    if (option == 1) {
        HIP_TRY(launch_fill_prev(in, disp, masked, mff, dprev0, b->frames, px, b->stream));
    } else {
        if (in != disp) HIP_TRY(hipMemcpyAsync(disp, in, (size_t)px * b->frames, hipMemcpyDeviceToDevice, b->stream));
        if (option == 2) HIP_TRY(launch_fill_mean(disp, masked, mff, b->frames, b->H, b->W, b->Wu, b->stream));
    }
    return SV_OK;
}

}  // namespace svx

extern "C" {

// ---------------------------------------------------------------------------
// disparity pre-pass (functions.py:131-172): host frames, synchronous
// ---------------------------------------------------------------------------
int sv_fill_previous(const uint8_t* disp, const uint8_t* prev, int H, int W, uint8_t* out) {
    if (!disp || !out || H < 0 || W < 0) return fail(SV_E_ARG, "sv_fill_previous: bad arguments");
    if ((int64_t)H * W == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    const int pitch = (W + 3) / 4 * 4;
    if (int rc = upload_u8(d->disp, disp, H, W, pitch, d->stream)) return rc;
    if (prev)
        if (int rc = upload_u8(d->aux, prev, H, W, pitch, d->stream)) return rc;
    HIP_TRY(launch_fill_prev(d->disp.as<uint8_t>(), d->disp.as<uint8_t>(), nullptr, nullptr,
                             prev ? d->aux.as<uint8_t>() : nullptr, 1, (int64_t)H * pitch, d->stream));
    return download_u8(out, d->disp, H, W, pitch, d->stream);
}

int sv_fill_mean(uint8_t* disp, int H, int W) {
    if (!disp || H < 0 || W < 0) return fail(SV_E_ARG, "sv_fill_mean: bad arguments");
    if ((int64_t)H * W == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    const int pitch = (W + 3) / 4 * 4;
    if (int rc = upload_u8(d->disp, disp, H, W, pitch, d->stream)) return rc;
    HIP_TRY(launch_fill_mean(d->disp.as<uint8_t>(), nullptr, nullptr, 1, H, pitch, W, d->stream));
    return download_u8(disp, d->disp, H, W, pitch, d->stream);
}

int sv_mask_disparity(const uint8_t* disp, const uint8_t* mask, int H, int W, uint8_t* out) {
    if (!disp || !mask || !out || H < 0 || W < 0) return fail(SV_E_ARG, "sv_mask_disparity: bad arguments");
    if ((int64_t)H * W == 0) return SV_OK;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    const int pitch = (W + 3) / 4 * 4;
    const int64_t px = (int64_t)H * pitch;
    if (int rc = upload_u8(d->disp, disp, H, W, pitch, d->stream)) return rc;
    if (int rc = upload_u8(d->aux, mask, H, W, pitch, d->stream)) return rc;
    HIP_TRY(d->aux2.ensure((size_t)px));
    HIP_TRY(launch_mask_bytes(d->aux.as<uint8_t>(), d->aux2.as<uint8_t>(), px, d->stream));
    HIP_TRY(launch_mask(d->disp.as<uint8_t>(), d->disp.as<uint8_t>(), d->aux2.as<uint8_t>(), 1, px, d->stream));
    return download_u8(out, d->disp, H, W, pitch, d->stream);
}

int sv_batch_set_mask(sv_batch* b, const uint8_t* mask) {
    if (!b) return fail(SV_E_ARG, "null batch");
    HIP_TRY(hipSetDevice(b->device));
    if (!mask) {
        b->have_mask = false;
        return SV_OK;
    }
    const int64_t px = (int64_t)b->H * b->W;
    HIP_TRY(b->carmask.ensure((size_t)px * 2));
    uint8_t* grey = b->carmask.as<uint8_t>() + px;
    HIP_TRY(hipMemsetAsync(grey, 0, (size_t)px, b->stream));
    HIP_TRY(hipMemcpy2DAsync(grey, b->W, mask, b->Wu, b->Wu, b->H, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(launch_mask_bytes(grey, b->carmask.as<uint8_t>(), px, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    b->have_mask = true;
    // the mask's points on maskpoints' step-2 grid (range(0, H-1, 2) x range(0, W-1, 2)): no frame's masked point
    // count can exceed it, so it sizes the batched RANSAC's launches without reading the counts back (batch_ransac_*)
    int64_t n2 = 0;
    for (int y = 0; y < b->H - 1; y += 2)
        for (int x = 0; x < b->Wu - 1; x += 2) n2 += mask[(int64_t)y * b->Wu + x] != 0;
    b->mask_n2 = n2;
    return SV_OK;
}

int sv_batch_prepass(sv_batch* b, int option, const uint8_t* prev0, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (option < 0 || option > 2) return fail(SV_E_ARG, "prepass option must be 0 (none), 1 (previous) or 2 (mean)");
    HIP_TRY(hipSetDevice(b->device));
    const int64_t px = (int64_t)b->H * b->W;
    // maskDisparity (functions.py:169-172) is not materialised: its only consumer on the device, maskpoints, applies
    // the mask as it reads the cleaned disparity (the fill pass moves 2 B a pixel, not 3); sv_batch_read_disp
    // applies it to the frame it reads back
    const uint8_t* p0 = nullptr;
    if (option == 1 && prev0) {
        HIP_TRY(b->prev0buf.ensure((size_t)px));
        HIP_TRY(hipMemsetAsync(b->prev0buf.p, 0, (size_t)px, b->stream));
        HIP_TRY(hipMemcpy2DAsync(b->prev0buf.p, b->W, prev0, b->Wu, b->Wu, b->H, hipMemcpyHostToDevice, b->stream));
        p0 = b->prev0buf.as<uint8_t>();
    }
    if (int rc = batch_prepass_impl(b, option, p0)) return rc;
    if (sync || prev0) HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_read_disp(sv_batch* b, int frame, uint8_t* disp, uint8_t* masked) {
    if (!b || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    if (masked && !b->have_mask) return fail(SV_E_STATE, "no masked disparity (set a mask first)");
    HIP_TRY(hipSetDevice(b->device));
    const size_t px = (size_t)b->H * b->W;
    uint8_t* mframe = nullptr;
    if (masked) {   // maskDisparity of this frame (the batch does not hold masked copies)
        HIP_TRY(b->rdbuf.ensure(px));
        mframe = b->rdbuf.as<uint8_t>();
        HIP_TRY(launch_mask(b->disp.as<uint8_t>() + px * frame, mframe, b->carmask.as<uint8_t>(), 1, (int64_t)px,
                            b->stream));
    }
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (disp)
        HIP_TRY(hipMemcpy2D(disp, b->Wu, b->disp.as<uint8_t>() + px * frame, b->W, b->Wu, b->H, hipMemcpyDeviceToHost));
    if (masked)
        HIP_TRY(hipMemcpy2D(masked, b->Wu, mframe, b->W, b->Wu, b->H,
                            hipMemcpyDeviceToHost));
    return SV_OK;
}

}  // extern "C"
