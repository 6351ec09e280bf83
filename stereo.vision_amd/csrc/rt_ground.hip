// svx runtime: the ground grid (include/svx.h, sv_ground_grid; kernels/ground.hip) as a host-frame entry and as a
// side branch of the batch's road chain at the obstacle stage, and the device's cache of the mapping it looks up.
#include <vector>

#include "svx_ground.h"
#include "svx_morph.h"
#include "svx_runtime.h"

namespace svx {

int ensure_ground_map(Device& d, const sv_camera& cam, const sv_grid& g, int W) {
    GroundMap& m = d.gmap;
    // (the mapping does not depend on ch)
    if (m.valid && m.W == W && m.cam.f == cam.f && m.cam.B == cam.B && m.cam.cw == cam.cw && m.grid.x0 == g.x0 &&
        m.grid.z0 == g.z0 && m.grid.cell == g.cell && m.grid.nx == g.nx && m.grid.nz == g.nz)
        return SV_OK;
    std::vector<int16_t> ix((size_t)256 * W), iz(256), host((size_t)256 * W);
    if (!ground_fill_mapping(cam, g, W, ix.data(), iz.data()))
        return fail(SV_E_ARG, "ground grid: camera, grid or width out of range");
    ground_fold_cells(ix.data(), iz.data(), W, g.nx, host.data());
    if (m.valid) HIP_TRY(hipDeviceSynchronize());   // a launch on another stream may still read the old mapping
    m.valid = false;
    HIP_TRY(m.tab.ensure(ground_map_bytes(W)));
    HIP_TRY(hipMemcpy(m.tab.p, host.data(), ground_map_bytes(W), hipMemcpyHostToDevice));
    m.W = W;
    m.cam = cam;
    m.grid = g;
    m.valid = true;
    return SV_OK;
}

}  // namespace svx

extern "C" {

int sv_ground_grid(const uint8_t* obstacles, const uint8_t* road, const uint8_t* disp, int H, int W,
                   const sv_camera* cam, const sv_grid* grid, int min_count, uint32_t* obst, uint32_t* road_out,
                   int32_t* nearest, int32_t* info) {
    if (const char* why = ground_check_args(obstacles, disp, H, W, cam, grid, min_count, obst, nearest, info))
        return fail(SV_E_ARG, "sv_ground_grid: bad arguments (%s)", why);
    const sv_grid g = grid ? *grid : ground_default_grid();
    Locked L;
    if (int rc = lock_current(L)) return rc;
    Device* d = L.d;
    hipStream_t s = d->stream;
    if (int rc = ensure_ground_map(*d, *cam, g, W)) return rc;
    const int WW = (W + 31) / 32;
    const int pitch = (W + 7) / 8 * 8;
    const size_t px = (size_t)H * pitch;
    // the obstacle bitmap | the road bitmap | the results (each part 16-byte aligned)
    const size_t bits_bytes = (sizeof(uint32_t) * (size_t)H * WW + 15) / 16 * 16;
    const GroundLayout l = ground_layout(g, 1);
    HIP_TRY(d->ground.ensure(2 * bits_bytes + l.bytes));
    uint32_t* obits = d->ground.as<uint32_t>();
    uint32_t* cbits = road ? reinterpret_cast<uint32_t*>(d->ground.as<char>() + bits_bytes) : nullptr;
    uint32_t* out = reinterpret_cast<uint32_t*>(d->ground.as<char>() + 2 * bits_bytes);
    if (int rc = upload_u8(d->aux, obstacles, H, W, pitch, s)) return rc;
    HIP_TRY(launch_morph_pack(d->aux.as<uint8_t>(), (int64_t)px, pitch, W, H, 1, obits, s));
    if (road) {
        if (int rc = upload_u8(d->aux2, road, H, W, pitch, s)) return rc;
        HIP_TRY(launch_morph_pack(d->aux2.as<uint8_t>(), (int64_t)px, pitch, W, H, 1, cbits, s));
    }
    if (int rc = upload_u8(d->disp, disp, H, W, pitch, s)) return rc;
    const int16_t* map = d->gmap.tab.as<int16_t>();
    HIP_TRY(launch_ground_grid(obits, cbits, 1, H, W, d->disp.as<uint8_t>(), (int64_t)px, pitch, map, g.nx,
                               g.nz, min_count, out, s));
    const size_t plane = sizeof(uint32_t) * l.cells;
    HIP_TRY(hipMemcpyAsync(obst, out, plane, hipMemcpyDeviceToHost, s));
    if (road_out) HIP_TRY(hipMemcpyAsync(road_out, out + l.cells, plane, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(nearest, out + l.off_nearest, sizeof(int32_t) * (size_t)g.nx, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(info, out + l.off_info, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

// SV_E_STATE unless the batch holds the grid of its current obstacle stage
static int need_grid(const sv_batch* b) {
    return b->road_level >= kRoadObstacles && b->ggrid_fresh
               ? SV_OK
               : fail(SV_E_STATE, "no current ground grid (sv_batch_ground_grid after sv_batch_road_hull first)");
}

int sv_batch_ground_grid(sv_batch* b, const sv_camera* cam, const sv_grid* grid, int min_count, int sync) {
    if (!b || !cam) return fail(SV_E_ARG, "null batch or camera");
    if (const char* why = ground_check_shape(b->H, b->Wu)) return fail(SV_E_ARG, "sv_batch_ground_grid: %s", why);
    if (grid)
        if (const char* why = ground_check_grid(*grid)) return fail(SV_E_ARG, "sv_batch_ground_grid: %s", why);
    if (min_count < 1) return fail(SV_E_ARG, "sv_batch_ground_grid: min_count >= 1");
    if (const char* why = ground_check_camera(*cam)) return fail(SV_E_ARG, "sv_batch_ground_grid: %s", why);
    if (b->road_level < kRoadObstacles)
        return fail(SV_E_STATE, "no current obstacle stage (sv_batch_road_hull first)");
    const sv_grid g = grid ? *grid : ground_default_grid();
    Locked L;   // the device's mapping cache is shared with the host entry and the device's other batches
    if (int rc = lock_device(b->device, L)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    b->ggrid_fresh = false;
    hipEvent_t* gev = b->road_ev + kEvGround;
    for (int i = 0; i < 2; ++i)
        if (!gev[i]) HIP_TRY(hipEventCreate(gev + i));
    if (int rc = ensure_ground_map(*L.d, *cam, g, b->Wu)) return rc;
    const GroundLayout l = ground_layout(g, b->frames);
    HIP_TRY(b->gbuf.ensure(l.bytes));
    const HullLayout hl = hull_layout(b->H, b->Wu, b->frames, false);
    uint32_t* out = b->gbuf.as<uint32_t>();
    const int16_t* map = L.d->gmap.tab.as<int16_t>();
    HIP_TRY(hipEventRecord(gev[0], s));
    HIP_TRY(launch_ground_grid(reinterpret_cast<const uint32_t*>(b->hbuf.as<char>() + hl.off_obst),
                               b->cbits.as<uint32_t>(), b->frames, b->H, b->Wu, b->disp.as<uint8_t>(),
                               (int64_t)b->H * b->W, b->W, map, g.nx, g.nz, min_count, out, s));
    HIP_TRY(hipEventRecord(gev[1], s));
    b->ggrid = g;
    b->ggrid_fresh = true;
    if (sync) HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_read_ground_grid(sv_batch* b, int frame, uint32_t* obst, uint32_t* road, int32_t* nearest,
                              int32_t* info) {
    if (!b || frame < 0 || frame >= b->frames) return fail(SV_E_ARG, "bad args");
    if (int rc = need_grid(b)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    const GroundLayout l = ground_layout(b->ggrid, b->frames);
    const uint32_t* out = b->gbuf.as<uint32_t>();
    const uint32_t* planes = out + 2 * l.cells * (size_t)frame;
    const size_t plane = sizeof(uint32_t) * l.cells, nx = (size_t)b->ggrid.nx;
    if (obst) HIP_TRY(hipMemcpyAsync(obst, planes, plane, hipMemcpyDeviceToHost, s));
    if (road) HIP_TRY(hipMemcpyAsync(road, planes + l.cells, plane, hipMemcpyDeviceToHost, s));
    if (nearest)
        HIP_TRY(hipMemcpyAsync(nearest, out + l.off_nearest + nx * frame, sizeof(int32_t) * nx, hipMemcpyDeviceToHost,
                               s));
    if (info) HIP_TRY(hipMemcpyAsync(info, out + l.off_info + 4 * (size_t)frame, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SV_OK;
}

int sv_batch_read_ground_nearest(sv_batch* b, int32_t* out) {
    if (!b || !out) return fail(SV_E_ARG, "null batch or output");
    if (int rc = need_grid(b)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    const GroundLayout l = ground_layout(b->ggrid, b->frames);
    HIP_TRY(hipMemcpyAsync(out, b->gbuf.as<uint32_t>() + l.off_nearest,
                           sizeof(int32_t) * (size_t)b->ggrid.nx * b->frames, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return SV_OK;
}

int sv_batch_ground_grid_ms(sv_batch* b, float* ms) {
    if (!b || !ms) return fail(SV_E_ARG, "null batch or ms");
    if (int rc = need_grid(b)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    const hipEvent_t* gev = b->road_ev + kEvGround;
    HIP_TRY(hipEventSynchronize(gev[1]));
    HIP_TRY(hipEventElapsedTime(ms, gev[0], gev[1]));
    return SV_OK;
}

}  // extern "C"
