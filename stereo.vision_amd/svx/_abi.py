"""ctypes binding of libsvx.so (include/svx.h).

The product has exactly one compute path: the hand-written gfx950 kernels in
libsvx.so. If the library is missing or has no device, every call raises —
there is deliberately no CPU fallback.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "_lib", "libsvx.so")

SV_UNIQUE_ID_BYTES = 128


class SvxError(RuntimeError):
    """A libsvx call failed (message from sv_last_error())."""


class Camera(ctypes.Structure):
    _fields_ = [("f", ctypes.c_double), ("B", ctypes.c_double),
                ("cw", ctypes.c_double), ("ch", ctypes.c_double)]


class Plane(ctypes.Structure):
    _fields_ = [("a", ctypes.c_double), ("b", ctypes.c_double), ("c", ctypes.c_double)]


class LoopParams(ctypes.Structure):
    """sv_loop_params (include/svx.h)."""
    _fields_ = [("frames", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("step", ctypes.c_int),
                ("slots", ctypes.c_int), ("source", ctypes.c_int), ("prepass", ctypes.c_int),
                ("trials", ctypes.c_int), ("k", ctypes.c_int), ("seed_base", ctypes.c_uint64),
                ("point_thr", ctypes.c_double), ("hist_thr", ctypes.c_int), ("road", ctypes.c_int)]


class HullInfo(ctypes.Structure):
    """sv_hull_info (include/svx.h)."""
    _fields_ = [("n", ctypes.c_int32), ("cx", ctypes.c_int32), ("cy", ctypes.c_int32), ("valid", ctypes.c_int32),
                ("tipx", ctypes.c_int64), ("tipy", ctypes.c_int64)]


class Obstacle(ctypes.Structure):
    """sv_obstacle (include/svx.h), 56 bytes; OBSTACLE_DTYPE is the same layout for numpy."""
    _fields_ = [(k, ctypes.c_int32) for k in ("x0", "y0", "x1", "y1", "area", "first", "nd", "dmax", "dmed",
                                              "reserved")] + [("sx", ctypes.c_int64), ("sy", ctypes.c_int64)]


OBSTACLE_FIELDS = [(k, "<i4") for k in ("x0", "y0", "x1", "y1", "area", "first", "nd", "dmax", "dmed", "reserved")] \
    + [("sx", "<i8"), ("sy", "<i8")]
OBSTACLE_MAX_CAP = 32


class Grid(ctypes.Structure):
    """sv_grid (include/svx.h), 32 bytes: nz rows of nx square cells of `cell` metres from (x0, z0)."""
    _fields_ = [("x0", ctypes.c_double), ("z0", ctypes.c_double), ("cell", ctypes.c_double),
                ("nx", ctypes.c_int32), ("nz", ctypes.c_int32)]


DEFAULT_GRID = (-8.0, 0.0, 0.25, 64, 128)   # 16 m across, 32 m ahead (include/svx.h, sv_ground_grid)


def as_grid(grid):
    """A Grid from None (the default), a Grid or (x0, z0, cell, nx, nz)."""
    if isinstance(grid, Grid):
        return grid
    x0, z0, cell, nx, nz = DEFAULT_GRID if grid is None else grid
    return Grid(float(x0), float(z0), float(cell), int(nx), int(nz))


class JpegDesc(ctypes.Structure):
    """sv_jpeg_desc (include/svx.h)."""
    _fields_ = [("h", ctypes.c_int32), ("w", ctypes.c_int32), ("restart_interval", ctypes.c_int32),
                ("header_len", ctypes.c_int32)]


class Picture(ctypes.Structure):
    """sv_picture (include/svx.h)."""
    _fields_ = [("data", ctypes.c_void_p), ("h", ctypes.c_int), ("w", ctypes.c_int), ("channels", ctypes.c_int)]


P = ctypes.c_void_p
I = ctypes.c_int
I64 = ctypes.c_int64
D = ctypes.c_double
PI64 = ctypes.POINTER(ctypes.c_int64)
PF = ctypes.POINTER(ctypes.c_float)

# name -> argtypes (restype is int unless listed in _RESTYPE)
SIGNATURES = {
    "sv_version": [],
    "sv_last_error": [],
    "sv_device_count": [ctypes.POINTER(I)],
    "sv_init": [I],
    "sv_project_frame": [P, I, I, I64, P, I64, I, ctypes.POINTER(Camera), P, P, I64, PI64],
    "sv_project_rows": [P, I, I, I64, P, I64, I, ctypes.POINTER(Camera), P, I, I64, PI64],
    "sv_host_alloc": [I64, ctypes.POINTER(P)],
    "sv_host_free": [P],
    "sv_backproject": [P, I64, I64, ctypes.POINTER(Camera), P],
    "sv_pipeline_frame": [P, P, I, I, I, ctypes.POINTER(Camera), ctypes.POINTER(Plane), D, I,
                          P, P, P, P, I64],
    "sv_fill_previous": [P, P, I, I, P],
    "sv_fill_mean": [P, I, I],
    "sv_mask_disparity": [P, P, I, I, P],
    "sv_batch_set_mask": [P, P],
    "sv_batch_prepass": [P, I, P, I],
    "sv_batch_read_disp": [P, I, P, P],
    "sv_road_raster": [P, I64, I, I, P],
    "sv_nonzero_points": [P, I, I, P, I64, PI64],
    "sv_sanitise_road": [P, P, I, I, P, P, I64, PI64],
    "sv_road_obstacles": [P, P, ctypes.POINTER(Plane), I, I, ctypes.POINTER(Camera), P, I64, P, P,
                          ctypes.POINTER(HullInfo)],
    "sv_min_circle_centre": [P, I64, P],
    "sv_obstacle_list": [P, P, I, I, I, P, I, ctypes.POINTER(ctypes.c_int32)],
    "sv_ground_grid": [P, P, P, I, I, ctypes.POINTER(Camera), ctypes.POINTER(Grid), I, P, P, P, P],
    "sv_result_image": [P, P, P, I64, ctypes.POINTER(HullInfo), I, I, P],
    "sv_batch_road_raster": [P, I],
    "sv_batch_nonzero": [P, I],
    "sv_batch_read_road": [P, I, P, P, I64, PI64],
    "sv_batch_road_map": [P, I],
    "sv_batch_road_bits": [P, I],
    "sv_batch_read_road_map": [P, I, P],
    "sv_batch_road_mask": [P, P],
    "sv_batch_road_clean": [P, I],
    "sv_batch_read_road_clean": [P, I, P, P, I64, PI64],
    "sv_batch_road_clean_ms": [P, PF, PF],
    "sv_batch_road_hull": [P, I],
    "sv_batch_read_road_hull": [P, I, P, I64, P, P, ctypes.POINTER(HullInfo)],
    "sv_batch_road_hull_ms": [P, PF],
    "sv_batch_obstacle_list": [P, I, I, I],
    "sv_batch_read_obstacle_list": [P, I, P, I, ctypes.POINTER(ctypes.c_int32)],
    "sv_batch_obstacle_list_ms": [P, PF],
    "sv_batch_ground_grid": [P, ctypes.POINTER(Camera), ctypes.POINTER(Grid), I, I],
    "sv_batch_read_ground_grid": [P, I, P, P, P, P],
    "sv_batch_read_ground_nearest": [P, P],
    "sv_batch_ground_grid_ms": [P, PF],
    "sv_batch_result": [P, I],
    "sv_batch_read_result": [P, I, P],
    "sv_batch_result_ms": [P, PF],
    "sv_image_tile": [P, P, P, P, P, I, I, P],
    "sv_batch_tile": [P, I],
    "sv_batch_read_tile": [P, I, P],
    "sv_batch_tile_ms": [P, PF],
    "sv_jpeg_bound": [I, I],
    "sv_jpeg_encode": [P, I, I, I64, I, P, I64, PI64],
    "sv_batch_jpeg": [P, I, I64, I],
    "sv_batch_jpeg_sizes": [P, P],
    "sv_batch_read_jpeg": [P, I, P, I64, PI64],
    "sv_batch_jpeg_pack": [P, I],
    "sv_batch_read_jpeg_packed": [P, P, I64, P, PI64],
    "sv_batch_jpeg_ms": [P, PF],
    "sv_loop_jpeg": [P, I, I64],
    "sv_jpeg_info": [P, I64, P],
    "sv_jpeg_decode": [P, I64, P, I, I, I64, P],
    "sv_jpeg_decode_many": [I, P, P, I, I, I, P, P],
    "sv_jpeg_decode_stage_ms": [I, PF],
    "sv_batch_decode_bgr_pair": [P, I, I, P, P, P, P, P],
    "sv_batch_decode_ms": [P, PF],
    "sv_batch_read_bgr_pair": [P, I, P, P],
    "sv_resize_coefficients": [I, I, P, P, P, P],
    "sv_resize_linear_u8": [P, I, I, I, I, P, I, I],
    "sv_images_tile_shape": [I, I, I, ctypes.POINTER(I), ctypes.POINTER(I)],
    "sv_images_tile": [ctypes.POINTER(Picture), I, I, I, P],
    "sv_rectify_map": [P, P, P, P, I, I, P, P],
    "sv_remap_u8": [P, I, I, I, I, P, P, I, I, P],
    "sv_batch_rectify_maps": [P, P, P, P, P],
    "sv_batch_rectify": [P, I],
    "sv_batch_rectify_ms": [P, PF],
    "sv_batch_resize_disp": [P, I, I, I],
    "sv_batch_read_resized_disp": [P, I, P],
    "sv_batch_resize_disp_ms": [P, PF],
    "sv_point_errors": [P, I64, I64, P, P],
    "sv_hue_histogram": [P, I64, I64, P, P, P],
    "sv_select_less": [P, I64, D, P, PI64],
    "sv_select_bins": [P, I64, P, P, PI64],
    "sv_ransac_draw": [P, P, I64, I64, I, I, P, P, ctypes.POINTER(I)],
    "sv_ransac": [P, P, I64, I64, I, I, P, P, P, P, P, ctypes.POINTER(I)],
    "sv_batch_ransac": [P, ctypes.POINTER(Camera), ctypes.c_uint64, I64, I, I, I],
    "sv_batch_read_ransac": [P, I, P, P, P, P],
    "sv_batch_read_maskpoints": [P, I, P, I64, PI64],
    "sv_batch_ransac_trace": [P, I],
    "sv_batch_read_ransac_trace": [P, I, P, I64, ctypes.POINTER(I), ctypes.POINTER(I)],
    "sv_batch_create": [I, I, I, I, I, I, I, ctypes.POINTER(P)],
    "sv_batch_destroy": [P],
    "sv_batch_info": [P, P],
    "sv_batch_tune": [P, I, I],
    "sv_batch_synth": [P, I64],
    "sv_batch_upload": [P, I, P, P],
    "sv_batch_project": [P, ctypes.POINTER(Camera), I],
    "sv_batch_pipeline": [P, ctypes.POINTER(Camera), ctypes.POINTER(Plane), D, I, I, I],
    "sv_batch_pipeline_mode": [P, I],
    "sv_batch_pipeline_planes": [P, ctypes.POINTER(Camera), D, I, I, I],
    "sv_batch_pipeline_dev": [P, ctypes.POINTER(Camera), P, D, I, I, I],
    "sv_batch_read_frame_plane": [P, I, P],
    "sv_lut_u8": [P, I64, P, P],
    "sv_grey_equalize": [P, I, I, P],
    "sv_sgbm_compute": [P, P, I, I, P, P],
    "sv_filter_speckles": [P, I, I, I, I, I],
    "sv_disparity": [P, P, I, I, P, I, I, P, P, P],
    "sv_batch_pair_shape": [P, I, I],
    "sv_batch_upload_bgr_pair": [P, I, P, P],
    "sv_batch_synth_bgr_pair": [P, I64],
    "sv_batch_preprocess": [P, P, I],
    "sv_batch_synth_pair": [P, I64],
    "sv_batch_upload_pair": [P, I, P, P],
    "sv_batch_sgbm": [P, P, I, I],
    "sv_batch_sync": [P],
    "sv_batch_last_ms": [P, I, PF],
    "sv_batch_timing": [P, I, ctypes.POINTER(D), PI64],
    "sv_batch_timing_reset": [P],
    "sv_batch_placement": [P, I, PF, I, ctypes.POINTER(I), ctypes.POINTER(I)],
    "sv_batch_kernel_name": [P, I, P, I],
    "sv_source_id": [I, P, I],
    "sv_batch_read_dense": [P, I, P, P, P],
    "sv_batch_read_counts": [P, P],
    "sv_batch_read_hist": [P, I, P],
    "sv_batch_read_points": [P, I, P, P, I64, PI64],
    "sv_batch_digest": [P, ctypes.POINTER(Camera), I, P],
    "sv_hue_lut": [I, P],
    "sv_hue_lut_variant": [I, I, P],
    "sv_delta_tables": [I, I, I, ctypes.POINTER(Camera), P, P],
    "sv_synth_frame": [I, I64, I, I, P, P],
    "sv_png_unfilter": [P, I, I, I, P],
    "sv_gather_rgb_u8": [P, I64, I64, P, I64, P],
    "sv_gather_f64": [P, I64, I64, P, I64, I, I, P],
    "sv_loop_create": [I, ctypes.POINTER(LoopParams), ctypes.POINTER(Camera), P, ctypes.POINTER(P)],
    "sv_loop_destroy": [P],
    "sv_loop_road_mask": [P, P],
    "sv_loop_acquire": [P, ctypes.POINTER(P)],
    "sv_loop_submit": [P, I64, PI64],
    "sv_loop_wait": [P, I64],
    "sv_loop_batch": [P, I64, ctypes.POINTER(P), PI64],
    "sv_loop_timeline": [P, I64, P],
    "sv_comm_unique_id": [P],
    "sv_comm_init": [I, I, P, I, ctypes.POINTER(P)],
    "sv_comm_destroy": [P],
    "sv_comm_init_all": [I, P, P],
    "sv_comm_group_start": [],
    "sv_comm_group_end": [],
    "sv_comm_broadcast_plane": [P, ctypes.POINTER(Plane), I],
    "sv_comm_broadcast_plane_dev": [P, P, ctypes.POINTER(Plane), I, ctypes.POINTER(P)],
    "sv_multi_pipeline": [I, P, P, ctypes.POINTER(Camera), ctypes.POINTER(Plane), I, D, I, I],
    "sv_comm_allreduce_i64": [P, P, I],
}
_RESTYPE = {"sv_version": ctypes.c_char_p, "sv_last_error": ctypes.c_char_p, "sv_jpeg_bound": ctypes.c_int64}

_lib = None


def lib():
    """The loaded libsvx.so (raises ImportError if it was never built)."""
    global _lib
    if _lib is None:
        # SVX_LIB: DIAGNOSTIC A/B only (tools/ab_lib.py times an older build of the
        # library beside this one); symbols that build lacks are left unbound.
        path = os.environ.get("SVX_LIB") or LIB_PATH
        if not os.path.exists(path):
            raise ImportError(f"libsvx.so not found at {path}: build it with "
                              "`python -c 'import __graft_entry__ as g; g.build()'`")
        l = ctypes.CDLL(path)
        for name, args in SIGNATURES.items():
            if path != LIB_PATH and not hasattr(l, name):
                continue
            fn = getattr(l, name)
            fn.argtypes = args
            fn.restype = _RESTYPE.get(name, ctypes.c_int)
        _lib = l
    return _lib


def last_error():
    msg = lib().sv_last_error()
    return msg.decode() if msg else ""


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise SvxError(f"{name} failed ({rc}): {last_error()}")
    return rc


def ptr(a):
    """data pointer of a numpy array (or None)."""
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def device_count():
    n = ctypes.c_int(0)
    rc = lib().sv_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def hull_result(H, W, images, read):
    """The dict dropin.road_obstacles and Batch.read_road_hull return, from read(pts, cap, hull_mask, obstacles,
    info), a call of sv_road_obstacles / sv_batch_read_road_hull."""
    import numpy as np
    info = HullInfo()
    pts = np.empty((2 * H, 2), np.int32)
    mask = np.empty((H, W), np.uint8) if images else None
    obst = np.empty((H, W), np.uint8) if images else None
    read(pts, 2 * H, mask, obst, ctypes.byref(info))
    return {"hull": pts[: info.n].reshape(-1, 1, 2).copy(), "hull_mask": mask, "obstacles": obst,
            "centre": (int(info.cx), int(info.cy)) if info.valid & 1 else None,
            "tip": (int(info.tipx), int(info.tipy)) if info.valid & 2 else None, "valid": int(info.valid)}


def obstacle_result(cap, read):
    """(n, entries) as dropin.obstacle_list and Batch.read_obstacle_list return them, from read(out, cap, n), a call
    of sv_obstacle_list / sv_batch_read_obstacle_list: n = the frame's components of at least min_area pixels,
    entries = the first min(n, cap) of them as a structured array of OBSTACLE_FIELDS."""
    import numpy as np
    cap = int(cap)
    out = np.zeros(max(cap, 1), np.dtype(OBSTACLE_FIELDS))
    n = ctypes.c_int32(0)
    read(out, cap, ctypes.byref(n))
    return int(n.value), out[: min(int(n.value), cap)].copy()


def ground_result(grid, read):
    """{"obst", "road": (nz, nx) uint32, "nearest": (nx,) int32, "info": (4,) int32} as dropin.ground_grid and
    Batch.read_ground_grid return them, from read(obst, road, nearest, info), a call of sv_ground_grid /
    sv_batch_read_ground_grid."""
    import numpy as np
    # (a grid out of range is the library's to refuse, before it writes anything: its arrays are placeholders)
    nz, nx = (grid.nz, grid.nx) if grid.nx >= 1 and grid.nz >= 1 and grid.nx * grid.nz <= 8192 else (1, 1)
    out = {"obst": np.zeros((nz, nx), np.uint32), "road": np.zeros((nz, nx), np.uint32),
           "nearest": np.zeros(nx, np.int32), "info": np.zeros(4, np.int32)}
    read(out["obst"], out["road"], out["nearest"], out["info"])
    return out


class _PinnedPool:
    """Page-locked host blocks (sv_host_alloc) for drop-in outputs, reused by size class: an array handed out by
    pinned_empty() returns its block here when the array and every view of it are gone, so a frame loop that drops
    each frame's points recycles the same few blocks and every device-to-host copy is a direct DMA."""

    def __init__(self):
        import threading
        self._free = {}
        self._lock = threading.Lock()
        self._closed = False
        self.allocs = 0   # blocks allocated (sv_host_alloc) so far: a steady loop stops adding to it

    def take(self, nbytes):
        size = 1 << max(16, (int(nbytes) - 1).bit_length())   # power-of-two classes from 64 KiB
        with self._lock:
            blocks = self._free.get(size)
            if blocks:
                return blocks.pop(), size
        p = P()
        call("sv_host_alloc", size, ctypes.byref(p))
        self.allocs += 1
        return p.value, size

    def give(self, addr, size):
        if self._closed:
            return
        with self._lock:
            self._free.setdefault(size, []).append(addr)

    def close(self):   # interpreter exit: the HIP runtime may already be gone, so the blocks are left to it
        self._closed = True


_pool = _PinnedPool()


def pinned_empty(shape, dtype):
    """An uninitialised numpy array in pooled page-locked host memory (see _PinnedPool)."""
    import weakref

    import numpy as np
    dt = np.dtype(dtype)
    count = int(np.prod(shape))
    nbytes = max(count * dt.itemsize, 1)
    addr, size = _pool.take(nbytes)
    buf = (ctypes.c_char * nbytes).from_address(addr)
    weakref.finalize(buf, _pool.give, addr, size)
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


import atexit  # noqa: E402

atexit.register(_pool.close)
