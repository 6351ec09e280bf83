// svx runtime: the obstacle list (include/svx.h, sv_obstacle_list; kernels/objects.hip) as a host-frame entry and as
// a side branch of the batch's road chain at the obstacle stage.
#include <cstring>

#include "svx_morph.h"
#include "svx_objects.h"
#include "svx_runtime.h"

extern "C" {

int sv_obstacle_list(const uint8_t* obstacles, const uint8_t* disp, int H, int W, int min_area, sv_obstacle* out,
                     int cap, int32_t* n) {
    if (const char* why = objects_check_args(obstacles, H, W, min_area, out, cap, n))
        return fail(SV_E_ARG, "sv_obstacle_list: bad arguments (%s)", why);
    *n = 0;
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    const ObjLayout l = objects_layout(H, W, 1);
    const int pitch = (W + 7) / 8 * 8;
    const size_t px = (size_t)H * pitch;
    // the bitmap | the entries | the count (each part 16-byte aligned)
    const size_t bits_bytes = (sizeof(uint32_t) * (size_t)H * l.WW + 15) / 16 * 16;
    const size_t list_bytes = sizeof(sv_obstacle) * kObjMaxCap;   // (a multiple of 16)
    HIP_TRY(d->objs.ensure(bits_bytes + list_bytes + 16));
    HIP_TRY(d->objwork.ensure(l.bytes, false, 0, true));
    uint32_t* bits = d->objs.as<uint32_t>();
    sv_obstacle* dlist = reinterpret_cast<sv_obstacle*>(d->objs.as<char>() + bits_bytes);
    int32_t* dn = reinterpret_cast<int32_t*>(d->objs.as<char>() + bits_bytes + list_bytes);
    if (int rc = upload_u8(d->aux, obstacles, H, W, pitch, s)) return rc;
    HIP_TRY(launch_morph_pack(d->aux.as<uint8_t>(), (int64_t)px, pitch, W, H, 1, bits, s));
    const uint8_t* ddisp = nullptr;
    if (disp) {
        if (int rc = upload_u8(d->disp, disp, H, W, pitch, s)) return rc;
        ddisp = d->disp.as<uint8_t>();
    }
    HIP_TRY(launch_obstacle_list(bits, 1, H, W, ddisp, (int64_t)px, pitch, min_area, cap, d->objwork.p, dlist, dn, s));
    int32_t k = 0;
    HIP_TRY(hipMemcpyAsync(&k, dn, sizeof k, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n = k;
    const int len = std::min(k, cap);
    if (len > 0) {
        HIP_TRY(hipMemcpyAsync(out, dlist, sizeof(sv_obstacle) * (size_t)len, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return SV_OK;
}

// SV_E_STATE unless the batch holds the list of its current obstacle stage
static int need_list(const sv_batch* b) {
    return b->road_level >= kRoadObstacles && b->olist_fresh
               ? SV_OK
               : fail(SV_E_STATE, "no current obstacle list (sv_batch_obstacle_list after sv_batch_road_hull first)");
}

int sv_batch_obstacle_list(sv_batch* b, int min_area, int cap, int sync) {
    if (!b) return fail(SV_E_ARG, "null batch");
    if (min_area < 1 || cap < 1 || cap > kObjMaxCap)
        return fail(SV_E_ARG, "sv_batch_obstacle_list: min_area >= 1, 1 <= cap <= 32");
    if (b->road_level < kRoadObstacles)
        return fail(SV_E_STATE, "no current obstacle stage (sv_batch_road_hull first)");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    b->olist_fresh = false;
    b->olist_host_fresh = false;
    hipEvent_t* oev = b->road_ev + kEvObjects;
    for (int i = 0; i < 2; ++i)
        if (!oev[i]) HIP_TRY(hipEventCreate(oev + i));
    const ObjLayout l = objects_layout(b->H, b->Wu, b->frames);
    HIP_TRY(b->owork.ensure(l.bytes, false, 0, true));
    const size_t list_bytes = sizeof(sv_obstacle) * (size_t)cap * b->frames;   // (a multiple of 8)
    HIP_TRY(b->olist.ensure(list_bytes + sizeof(int32_t) * b->frames));
    const HullLayout hl = hull_layout(b->H, b->Wu, b->frames, false);
    HIP_TRY(hipEventRecord(oev[0], s));
    HIP_TRY(launch_obstacle_list(reinterpret_cast<const uint32_t*>(b->hbuf.as<char>() + hl.off_obst), b->frames, b->H,
                                 b->Wu, b->disp.as<uint8_t>(), (int64_t)b->H * b->W, b->W, min_area, cap, b->owork.p,
                                 b->olist.as<sv_obstacle>(),
                                 reinterpret_cast<int32_t*>(b->olist.as<char>() + list_bytes), s));
    HIP_TRY(hipEventRecord(oev[1], s));
    b->olist_cap = cap;
    b->olist_fresh = true;
    if (sync) HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_read_obstacle_list(sv_batch* b, int frame, sv_obstacle* out, int cap, int32_t* n) {
    if (!b || !out || !n || frame < 0 || frame >= b->frames || cap < 1) return fail(SV_E_ARG, "bad args");
    if (int rc = need_list(b)) return rc;
    if (cap > b->olist_cap)
        return fail(SV_E_ARG, "cap %d above the %d of the sv_batch_obstacle_list call", cap, b->olist_cap);
    const size_t list_bytes = sizeof(sv_obstacle) * (size_t)b->olist_cap * b->frames;
    if (!b->olist_host_fresh) {   // every frame's list in one copy; later reads of this call's lists are host reads
        HIP_TRY(hipSetDevice(b->device));
        HIP_TRY(hipStreamSynchronize(b->stream));
        b->olist_host.resize(list_bytes + sizeof(int32_t) * b->frames);
        HIP_TRY(hipMemcpy(b->olist_host.data(), b->olist.p, b->olist_host.size(), hipMemcpyDeviceToHost));
        b->olist_host_fresh = true;
    }
    int32_t k = 0;
    std::memcpy(&k, b->olist_host.data() + list_bytes + sizeof(int32_t) * frame, sizeof k);
    *n = k;
    const int len = std::min(k, cap);
    if (len > 0)
        std::memcpy(out, b->olist_host.data() + sizeof(sv_obstacle) * (size_t)b->olist_cap * frame,
                    sizeof(sv_obstacle) * (size_t)len);
    return SV_OK;
}

int sv_batch_obstacle_list_ms(sv_batch* b, float* ms) {
    if (!b || !ms) return fail(SV_E_ARG, "null batch or ms");
    if (int rc = need_list(b)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    const hipEvent_t* oev = b->road_ev + kEvObjects;
    HIP_TRY(hipEventSynchronize(oev[1]));
    HIP_TRY(hipEventElapsedTime(ms, oev[0], oev[1]));
    return SV_OK;
}

}  // extern "C"
