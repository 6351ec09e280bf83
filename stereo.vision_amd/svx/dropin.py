"""Drop-in replacements for the reference's hot-path functions.

The reference (thien/stereo.vision) has no plugin/FFI API: stereovision.py
does ``import functions as f`` (stereovision.py:3) and resolves
``f.projectDisparityTo3d`` etc. at call time (stereovision.py:84-111). The
boundary is therefore the attributes of the ``functions`` module:

    import functions, svx.dropin
    svx.dropin.install(functions)      # loop.py / single_frame.py then run unchanged

Signatures, argument meaning, return conventions and error behaviour follow the
reference:

* ``projectDisparityTo3d(disparity, max_disparity, rgb=[])`` (functions.py:178-198):
  ``max_disparity`` is accepted and ignored (as in the reference); ``rgb`` is
  used iff ``len(rgb) > 0``. Returns a Sequence (``random.sample`` in RANSAC
  needs one, functions.py:252,286; svx/points.py: rows made when first read, a
  plain list after a mutation) of rows supporting ``row[0..5]``
  and ``row[:3]``; XYZ are ``np.float64`` bit-identical to the reference and
  R,G,B are numpy scalars (np.float64), which keeps ``BGRtoHSVHue`` keys
  identical (Python ints would not: SURVEY §0 trap 3).
* ``project3DPointsTo2DImagePoints(points)`` (functions.py:201-209): returns
  an (N, 2) float64 array that ``np.array(.., np.int32).reshape((-1,1,2))``
  (stereovision.py:112-113) accepts, (0, 2) for no points.
* ``generatePointsAsImage(points)`` (functions.py:339-344): grey road image;
  ``nonzero_points(img)`` gives sanitiseRoadImage's final pixel walk.
* ``RANSAC(points, trials)`` (functions.py:278-298): see svx/ransac.py — same
  draws from the global ``random`` stream, trials on the GPU, same plane bits.
* ``calculatePointErrors``, ``computePlanarThreshold``,
  ``calculateColourHistogram``, ``filterPointsByHistogram`` (functions.py:
  212-230, :300-323): see svx/stages.py — one device call each, same return
  types, dict order and errors as the reference.
* disparity stage (functions.py:61-128): ``gammaChange``, ``preProcessImages``,
  ``greyscale`` and ``disparity`` (StereoSGBM + filterSpeckles + scaling) —
  see svx/disparity.py.
* ``sanitiseRoadImage(img, size)`` (functions.py:346-366): the road image's clean-up
  (close, erode, mask, close; ParticleCleansing is the identity after them) and its pixel
  walk; returns ``(img, np.matrix(pts))``. Installed only with ``install(.., morphology=True)``.
* ``getCenterPoint(points)`` (functions.py:418-421): the centre of the exact minimum enclosing
  circle; installed only with ``install(.., hull=True)``. ``road_obstacles`` gives the whole
  obstacle stage (hull, hull mask, obstacles, centre, glyph tip) of a cleaned road image,
  ``result_image`` the picture drawn from it (stereovision.py:181-209; array form only).
  ``obstacle_list`` turns the obstacle image into a list of its components (box, area, range;
  ``obstacle_xyz`` for metres): the reference has no such function, so nothing is installed.
  ``ground_grid`` lays the obstacle and road images out on the ground plane (counts a cell, the
  nearest occupied range a column; ``ground_grid_axes`` for metres): nothing is installed either.
* ``batchImages(imgList, size)`` (functions.py:456-501): the five-picture tile of
  stereovision.py:216 on the GPU (``image_tile`` is its array form); other lists go to the
  function it replaced. Installed only with ``install(.., tiles=True)``.
* ``resizeImage(image, height, width)`` and ``batchImages`` for any list of one to five
  pictures (functions.py:452-501): cv2.resize's 8-bit bilinear path at any scale on the GPU
  (``resize_linear``, ``images_tile`` are the array forms). Installed only with
  ``install(.., resize=True)``.
* ``rectify_map``, ``remap`` and ``camera_from_projection``: the stereo rectification in front of
  everything else (cv2.initUndistortRectifyMap's fixed-point map pair on the host, cv2.remap's
  8-bit bilinear path on the GPU, the rectified pair's camera). The reference's dataset ships
  rectified and it has no such function, so nothing is installed.
* disparity pre-pass (functions.py:141-172): ``fillDisparity`` (new array, or
  the input itself when there is no previous frame), ``fillAltDisparity`` (in
  place, returns its argument), ``maskDisparity`` (new array; the mask is the
  installed module's ``carmask``, functions.py:35) and ``capDisparity`` (returns
  its argument: the reference discards the masked result, functions.py:164-167).

Failures raise ``RuntimeError`` (``SvxError``), which the reference's own
``try/except`` at stereovision.py:92-126 handles like any reference error.
"""
import ctypes

import numpy as np

from . import _abi

# functions.py:15,19,21,22
DEFAULT_CAMERA = (399.9745178222656, 0.2090607502, 474.5, 262.0)
REFERENCE_STEP = 2   # functions.py:185-186 hard-codes the grid step

_module = None       # the installed `functions` module (its constants are read per call)


def _camera():
    if _module is not None:
        m = _module
        return _abi.Camera(m.camera_focal_length_px, m.stereo_camera_baseline_m,
                           m.image_centre_w, m.image_centre_h)
    return _abi.Camera(*DEFAULT_CAMERA)


def _as_u8(a, ndim, what):
    arr = np.asarray(a)
    if arr.dtype != np.uint8:
        raise TypeError(f"{what} must be uint8 (as functions.disparity / cv2.imread produce), got {arr.dtype}")
    if arr.ndim != ndim:
        raise ValueError(f"{what} must have {ndim} dimensions, got shape {arr.shape}")
    if arr.strides[-1] != arr.itemsize or (ndim == 3 and arr.strides[1] != 3):
        arr = np.ascontiguousarray(arr)
    return arr


def project_frame(disparity, rgb=None, step=REFERENCE_STEP, camera=None):
    """Array form: (xyz (N,3) float64, rgb (N,3) uint8 or None) in reference order."""
    disp = _as_u8(disparity, 2, "disparity")
    h, w = disp.shape
    bgr = None
    if rgb is not None and len(rgb) > 0:
        bgr = _as_u8(rgb, 3, "rgb")
        if bgr.shape[0] < h or bgr.shape[1] < w or bgr.shape[2] < 3:
            raise IndexError(f"rgb shape {bgr.shape} smaller than disparity {disp.shape}")
        if bgr.shape[2] != 3:
            bgr = np.ascontiguousarray(bgr[:, :, :3])
    hg = (h - 1 + step - 1) // step if h > 1 else 0
    wg = (w - 1 + step - 1) // step if w > 1 else 0
    cap = max(hg * wg, 1)
    xyz = np.empty((cap, 3), np.float64)
    out_rgb = np.empty((cap, 3), np.uint8) if bgr is not None else None
    n = ctypes.c_int64(0)
    cam = camera if camera is not None else _camera()
    _abi.call("sv_project_frame", _abi.ptr(disp), h, w, disp.strides[0],
              _abi.ptr(bgr), bgr.strides[0] if bgr is not None else 0, step, ctypes.byref(cam),
              _abi.ptr(xyz), _abi.ptr(out_rgb), cap, ctypes.byref(n))
    k = n.value
    return xyz[:k], (out_rgb[:k] if out_rgb is not None else None)


from .points import PointList, as_points_array, gather_columns  # noqa: E402,F401  (re-exported)


def project_rows(disparity, rgb=None, step=REFERENCE_STEP, camera=None):
    """(N, 6) float64 rows X, Y, Z, R, G, B — or (N, 3) without colours — in reference order, laid out on the
    device and copied straight into pooled page-locked memory (sv_project_rows, one DMA, no host assembly)."""
    disp = _as_u8(disparity, 2, "disparity")
    h, w = disp.shape
    bgr = None
    if rgb is not None and len(rgb) > 0:
        bgr = _as_u8(rgb, 3, "rgb")
        if bgr.shape[0] < h or bgr.shape[1] < w or bgr.shape[2] < 3:
            raise IndexError(f"rgb shape {bgr.shape} smaller than disparity {disp.shape}")
        if bgr.shape[2] != 3:
            bgr = np.ascontiguousarray(bgr[:, :, :3])
    cols = 6 if bgr is not None else 3
    hg = (h - 1 + step - 1) // step if h > 1 else 0
    wg = (w - 1 + step - 1) // step if w > 1 else 0
    cap = max(hg * wg, 1)
    cam = camera if camera is not None else _camera()
    n = ctypes.c_int64(0)
    if hg * wg == 0:
        rows = np.empty((cap, cols), np.float64)
    else:
        rows = _abi.pinned_empty((cap, cols), np.float64)
    _abi.call("sv_project_rows", _abi.ptr(disp), h, w, disp.strides[0], _abi.ptr(bgr),
              bgr.strides[0] if bgr is not None else 0, step, ctypes.byref(cam), _abi.ptr(rows), cols, cap,
              ctypes.byref(n))
    return rows[: n.value]


def projectDisparityTo3d(disparity, max_disparity, rgb=[]):  # noqa: N802,B006 (reference signature)
    """functions.py:178-198 on the GPU. Returns a Sequence of rows (see module doc)."""
    return PointList(project_rows(disparity, rgb))


def project3DPointsTo2DImagePoints(points):  # noqa: N802
    """functions.py:201-209 on the GPU: (N,2) float64 [x, y]."""
    n = len(points)
    if n == 0:
        return np.zeros((0, 2), np.float64)
    arr = gather_columns(points, 0, 3, pinned=True)   # X, Y, Z only (a selection: one C pass, svx/points.py)
    if arr.ndim != 2 or arr.shape[1] < 3:
        raise ValueError(f"points must be rows of at least [X, Y, Z], got shape {arr.shape}")
    out = _abi.pinned_empty((n, 2), np.float64)   # page-locked: the device-to-host copy is a direct DMA
    cam = _camera()
    _abi.call("sv_backproject", _abi.ptr(arr), n, arr.shape[1], ctypes.byref(cam), _abi.ptr(out))
    return out


# ---------------------------------------------------------------------------
# disparity pre-pass (functions.py:141-172)
# ---------------------------------------------------------------------------
def fill_previous(disparity, previous):
    """Array form of fillDisparity: d > 2 ? d : min(255, d + prev)."""
    disp = _as_u8(disparity, 2, "disparity")
    prev = _as_u8(previous, 2, "previousDisparity")
    if prev.shape != disp.shape:
        raise ValueError(f"previousDisparity shape {prev.shape} != disparity shape {disp.shape}")
    out = np.empty_like(disp)
    _abi.call("sv_fill_previous", _abi.ptr(disp), _abi.ptr(prev), disp.shape[0], disp.shape[1], _abi.ptr(out))
    return out


def fillDisparity(disparity, previousDisparity):  # noqa: N802
    """functions.py:141-148 on the GPU."""
    if previousDisparity is None:
        return disparity
    return fill_previous(disparity, previousDisparity)


def fillAltDisparity(disparity):  # noqa: N802
    """functions.py:150-162 on the GPU: in place (like the reference), returns its argument."""
    if not isinstance(disparity, np.ndarray) or disparity.dtype != np.uint8 or disparity.ndim != 2:
        raise TypeError("fillAltDisparity expects a 2-D uint8 numpy array")
    work = np.ascontiguousarray(disparity).copy() if not disparity.flags.c_contiguous else disparity
    _abi.call("sv_fill_mean", _abi.ptr(work), work.shape[0], work.shape[1])
    if work is not disparity:
        disparity[...] = work
    return disparity


def mask_disparity(disparity, mask):
    """Array form of maskDisparity with an explicit grey mask: mask != 0 ? d : 0."""
    disp = _as_u8(disparity, 2, "disparity")
    m = _as_u8(mask, 2, "mask")
    if m.shape != disp.shape:
        raise ValueError(f"mask shape {m.shape} != disparity shape {disp.shape}")
    out = np.empty_like(disp)
    _abi.call("sv_mask_disparity", _abi.ptr(disp), _abi.ptr(m), disp.shape[0], disp.shape[1], _abi.ptr(out))
    return out


def maskDisparity(disparity):  # noqa: N802
    """functions.py:169-172 on the GPU, with the installed module's carmask."""
    if _module is None or getattr(_module, "carmask", None) is None:
        raise RuntimeError("maskDisparity needs the reference's carmask: install(functions) first "
                           "(or call mask_disparity(disparity, mask))")
    return mask_disparity(disparity, _module.carmask)


def capDisparity(disparity):  # noqa: N802
    """functions.py:164-167: the reference computes a masked copy and discards it,
    returning its argument; so does this (no device work)."""
    return disparity


# ---------------------------------------------------------------------------
# road raster (functions.py:339-344) and the non-zero walk (functions.py:359-365)
# ---------------------------------------------------------------------------
def road_raster(points, shape=(544, 1024)):
    """Array form of generatePointsAsImage: (H, W) uint8, 255 at each [x, y]."""
    p = np.ascontiguousarray(np.asarray(points).reshape(-1, 2), dtype=np.int32)
    H, W = shape
    img = np.empty((H, W), np.uint8)
    try:
        _abi.call("sv_road_raster", _abi.ptr(p), len(p), H, W, _abi.ptr(img))
    except _abi.SvxError as e:
        if "index out of range" in str(e):
            raise IndexError(str(e)) from None
        raise
    return img


def generatePointsAsImage(points):  # noqa: N802
    """functions.py:339-344 on the GPU: the installed module's blackImg shape (the
    reference copies that black image), 544 x 1024 otherwise."""
    black = getattr(_module, "blackImg", None) if _module is not None else None
    shape = black.shape[:2] if black is not None else (544, 1024)
    return road_raster(points, shape)


def nonzero_points(img):
    """The pixel walk that ends sanitiseRoadImage (functions.py:359-365):
    (K, 2) int32 [j, i] of the non-zero pixels in raster order."""
    im = _as_u8(img, 2, "image")
    H, W = im.shape
    out = np.empty((max(H * W, 1), 2), np.int32)
    n = ctypes.c_int64(0)
    _abi.call("sv_nonzero_points", _abi.ptr(im), H, W, _abi.ptr(out), H * W, ctypes.byref(n))
    return out[: n.value]


# ---------------------------------------------------------------------------
# the road image's clean-up (functions.py:346-366)
# ---------------------------------------------------------------------------
def sanitise_road(img, mask=None):
    """Array form of sanitiseRoadImage: (cleaned image (H, W) uint8 of 0 / 255, (K, 2) int32 [j, i] of its non-zero
    pixels in raster order). The image's non-zero pixels are closed by 9 x 9, eroded by 17 x 17, ANDed with
    mask != 0 (None: no mask) and closed by 9 x 9 again, OpenCV's default borders; ParticleCleansing changes
    nothing after that (include/svx.h, sv_sanitise_road)."""
    im = _as_u8(img, 2, "image")
    if not im.flags.c_contiguous:
        im = np.ascontiguousarray(im)
    H, W = im.shape
    m = None
    if mask is not None:
        m = np.ascontiguousarray(_as_u8(mask, 2, "mask"))
        if m.shape != im.shape:
            raise ValueError(f"mask shape {m.shape} != image shape {im.shape}")
    out = np.empty((H, W), np.uint8)
    n = ctypes.c_int64(0)
    pts = np.empty((max(H * W, 1), 2), np.int32)
    _abi.call("sv_sanitise_road", _abi.ptr(im), _abi.ptr(m), H, W, _abi.ptr(out), _abi.ptr(pts), H * W,
              ctypes.byref(n))
    return out, pts[: n.value].copy()


def sanitiseRoadImage(img, size):  # noqa: N802
    """functions.py:346-366 on the GPU, with the installed module's road_threshold_mask (functions.py:31): returns
    (img, np.matrix(pts)) like the reference — the walk restricted to [0:height, 0:width] of `size`, an int64
    (K, 2) matrix, or np.matrix([]) ((1, 0) float64) without points."""
    if _module is None or getattr(_module, "road_threshold_mask", None) is None:
        raise RuntimeError("sanitiseRoadImage needs the reference's road_threshold_mask: install(functions, "
                           "morphology=True) first (or call sanitise_road(img, mask))")
    (height, width) = size
    out, pts = sanitise_road(img, _module.road_threshold_mask)
    if height < out.shape[0] or width < out.shape[1]:
        pts = pts[(pts[:, 0] < width) & (pts[:, 1] < height)]
    if len(pts) == 0:
        return out, np.matrix([])
    return out, np.matrix(pts.astype(np.int64))


# ---------------------------------------------------------------------------
# the obstacle stage (stereovision.py:170-189, functions.py:396-421)
# ---------------------------------------------------------------------------
def road_obstacles(cleaned, disparity=None, abc=None, camera=None):
    """What stereovision.py:170-189 and :198-204 derive from the cleaned road image (non-zero = road), on the GPU:
    {"hull": (n, 1, 2) int32, the strict vertices of the convex hull of the road pixels (cv2.convexHull's shape; from
    the top-left vertex down the left side and back up the right side), "hull_mask": the closed hull filled, 0 / 255,
    "obstacles": hull_mask & ~cleaned, "centre": the centre of the hull's exact minimum enclosing circle truncated
    (None without road pixels), "tip": getNormalVectorLine(centre, abc, disparity) (None without disparity or abc,
    or where the reference raises), "valid": the flags} (include/svx.h, sv_road_obstacles)."""
    im = np.ascontiguousarray(_as_u8(cleaned, 2, "image"))
    H, W = im.shape
    dp = None
    if disparity is not None:
        dp = np.ascontiguousarray(_as_u8(disparity, 2, "disparity"))
        if dp.shape != im.shape:
            raise ValueError(f"disparity shape {dp.shape} != image shape {im.shape}")
    pl = None
    if abc is not None:
        a, b, c = (float(v) for v in np.asarray(abc, np.float64).reshape(-1)[:3])
        pl = ctypes.byref(_abi.Plane(a, b, c))
    cam = _abi.Camera(*camera) if camera is not None else _camera()
    return _abi.hull_result(H, W, True, lambda pts, cap, m, o, info: _abi.call(
        "sv_road_obstacles", _abi.ptr(im), _abi.ptr(dp), pl, H, W, ctypes.byref(cam), _abi.ptr(pts), cap,
        _abi.ptr(m), _abi.ptr(o), info))


def obstacle_list(obstacles, disparity=None, min_area=70, cap=16):
    """The obstacle image (non-zero = obstacle; what road_obstacles returns) as a list, on the GPU: (n, entries).
    n = the number of 8-connected components of at least min_area pixels (70 is ParticleCleansing's threshold);
    entries = the first min(n, cap) of them, largest area first, then by first pixel, as a structured array with
    x0, y0, x1, y1 (the inclusive box), area, first (y * W + x of the first pixel in raster order), nd, dmax, dmed
    (number, maximum and lower median of the component's disparities > 0; 0 without any), sx, sy (the sums of the
    pixels' x and y). 1 <= cap <= 32 (include/svx.h, sv_obstacle_list). obstacle_xyz gives an entry's metres."""
    im = np.ascontiguousarray(_as_u8(obstacles, 2, "obstacles"))
    H, W = im.shape
    dp = None
    if disparity is not None:
        dp = np.ascontiguousarray(_as_u8(disparity, 2, "disparity"))
        if dp.shape != im.shape:
            raise ValueError(f"disparity shape {dp.shape} != image shape {im.shape}")
    return _abi.obstacle_result(cap, lambda out, c, n: _abi.call(
        "sv_obstacle_list", _abi.ptr(im), _abi.ptr(dp), H, W, int(min_area), _abi.ptr(out), c, n))


def obstacle_xyz(entry, camera=None):
    """(X, Y, Z) in metres of an obstacle_list entry, in float64 on the host: Z = f B / dmed, and X, Y those of the
    box's centre at that Z (functions.py:191-193). None for dmed == 0 (no disparity under the component). camera:
    (f, B, cw, ch); default: the installed module's, else the reference's constants."""
    cam = _abi.Camera(*camera) if camera is not None else _camera()
    dmed = int(entry["dmed"])
    if dmed == 0:
        return None
    z = (cam.f * cam.B) / dmed
    cx = (int(entry["x0"]) + int(entry["x1"])) / 2.0
    cy = (int(entry["y0"]) + int(entry["y1"])) / 2.0
    return ((cx - cam.cw) * z) / cam.f, ((cy - cam.ch) * z) / cam.f, z


def ground_grid(obstacles, disp, road=None, camera=None, grid=None, min_count=1):
    """The obstacle image (non-zero = obstacle) and, if given, the road image laid out on the ground plane, on the
    GPU: {"obst", "road": (nz, nx) uint32, the pixels with d > 0 that fall in each cell (row 0 nearest; road all zero
    without a road image), "nearest": (nx,) int32, the smallest iz with obst[iz, ix] >= min_count or -1, "info":
    (4,) int32, obstacle pixels in the grid, with d > 0 outside it, with d == 0, road pixels in the grid}. A pixel
    (y, x) with d = disp[y, x] > 0 is at Z = f B / d, X = (x - cw) Z / f (functions.py:191-192, float64) and in cell
    iz = floor((Z - z0) / cell), ix = floor((X - x0) / cell). camera: (f, B, cw, ch), default: the installed
    module's, else the reference's constants; grid: (x0, z0, cell, nx, nz), nx nz <= 8192, default (-8, 0, 0.25,
    64, 128) (include/svx.h, sv_ground_grid). ground_grid_axes gives the cells' centres in metres."""
    im = np.ascontiguousarray(_as_u8(obstacles, 2, "obstacles"))
    H, W = im.shape
    dp = np.ascontiguousarray(_as_u8(disp, 2, "disparity"))
    if dp.shape != im.shape:
        raise ValueError(f"disparity shape {dp.shape} != image shape {im.shape}")
    rd = None
    if road is not None:
        rd = np.ascontiguousarray(_as_u8(road, 2, "road"))
        if rd.shape != im.shape:
            raise ValueError(f"road shape {rd.shape} != image shape {im.shape}")
    cam = _abi.Camera(*camera) if camera is not None else _camera()
    g = _abi.as_grid(grid)
    return _abi.ground_result(g, lambda o, r, n, i: _abi.call(
        "sv_ground_grid", _abi.ptr(im), _abi.ptr(rd), _abi.ptr(dp), H, W, ctypes.byref(cam), ctypes.byref(g),
        int(min_count), _abi.ptr(o), _abi.ptr(r), _abi.ptr(n), _abi.ptr(i)))


def ground_grid_axes(grid=None):
    """(X, Z): the cell centres of a ground grid in metres, X of nx and Z of nz float64 values (host only)."""
    g = _abi.as_grid(grid)
    return (g.x0 + (np.arange(g.nx, dtype=np.float64) + 0.5) * g.cell,
            g.z0 + (np.arange(g.nz, dtype=np.float64) + 0.5) * g.cell)


def result_image(imgL, obstacles, hull, centre=None, tip=None):  # noqa: N803
    """The "Result" image of stereovision.py:181-209 on the GPU: imgL (H, W, 3) uint8 BGR dimmed to 0.6 with the
    obstacles (H, W, non-zero = obstacle) tinted yellow (cv2.addWeighted), the hull outlined in red (drawRoadLine)
    and, with a centre and a tip, the road-normal glyph (drawNormalLine). It takes what road_obstacles returns:
    result_image(imgL, r["obstacles"], r["hull"], r["centre"], r["tip"]). hull: (n, 1, 2) or (n, 2) integers, a
    convex polygon in outline order; no vertex: imgL unchanged. The overlay is cv2's byte for byte; the strokes are
    the exact capsules and disc of include/svx.h (sv_result_image), unpinned against cv2's rasteriser."""
    im = np.ascontiguousarray(_as_u8(imgL, 3, "image"))
    if im.shape[2] != 3:
        raise ValueError(f"image shape {im.shape}: (H, W, 3) expected")
    H, W = im.shape[:2]
    ob = np.ascontiguousarray(_as_u8(obstacles, 2, "obstacles"))
    if ob.shape != (H, W):
        raise ValueError(f"obstacles shape {ob.shape} != image shape {(H, W)}")
    hp = np.asarray(hull)
    if hp.size and (hp.dtype.kind not in "iu" or hp.size % 2):
        raise TypeError("hull: an (n, 1, 2) or (n, 2) integer array")
    hp = hp.reshape(-1, 2).astype(np.int64)
    if hp.size and np.abs(hp).max() > 16383:
        raise ValueError("hull: coordinates beyond +-16383")
    hp = np.ascontiguousarray(hp, np.int32)
    info = _abi.HullInfo()
    if centre is not None:
        info.cx, info.cy, info.valid = int(centre[0]), int(centre[1]), 1
        if tip is not None:
            tx, ty = int(tip[0]), int(tip[1])
            if abs(tx) < 2 ** 63 and abs(ty) < 2 ** 63:   # beyond int64 the reference's int() result cannot be drawn
                info.tipx, info.tipy, info.valid = tx, ty, 3
    out = np.empty((H, W, 3), np.uint8)
    _abi.call("sv_result_image", _abi.ptr(im), _abi.ptr(ob), _abi.ptr(hp) if len(hp) else None, len(hp),
              ctypes.byref(info), H, W, _abi.ptr(out))
    return out


# ---------------------------------------------------------------------------
# the image tile (stereovision.py:216, functions.py:452-499)
# ---------------------------------------------------------------------------
def image_tile(disparity, imgL, road, cleaned, result):  # noqa: N803
    """The img_tile of stereovision.py:216 on the GPU, (H // 2, W, 3) uint8 BGR: batchImages of the disparity,
    imageRoadMap, the road image and the cleaned road image (a quarter each, left) and the result image (a half,
    right). disparity, road, cleaned: (H, W) uint8; imgL, result: (H, W, 3) uint8; H and W multiples of 4, 4..4096.
    imageRoadMap is imgL with (0, 255, 0) where road != 0 (stereovision.py:131-133), painted on the device
    (include/svx.h, sv_image_tile); unpinned against cv2.resize."""
    dp = np.ascontiguousarray(_as_u8(disparity, 2, "disparity"))
    H, W = dp.shape
    grey = [np.ascontiguousarray(_as_u8(a, 2, what)) for a, what in ((road, "road"), (cleaned, "cleaned"))]
    bgr = [np.ascontiguousarray(_as_u8(a, 3, what)) for a, what in ((imgL, "image"), (result, "result"))]
    for a, what in ((grey[0], "road"), (grey[1], "cleaned")):
        if a.shape != (H, W):
            raise ValueError(f"{what} shape {a.shape} != disparity shape {(H, W)}")
    for a, what in ((bgr[0], "image"), (bgr[1], "result")):
        if a.shape != (H, W, 3):
            raise ValueError(f"{what} shape {a.shape} != {(H, W, 3)}")
    out = np.empty((H // 2, W, 3), np.uint8)
    _abi.call("sv_image_tile", _abi.ptr(dp), _abi.ptr(bgr[0]), _abi.ptr(grey[0]), _abi.ptr(grey[1]), _abi.ptr(bgr[1]),
              H, W, _abi.ptr(out))
    return out


def jpeg_encode(img, quality=75):
    """The baseline JPEG stream (bytes) of a picture, encoded on the GPU: what the MJPG VideoWriter of
    loop.py:49-54,82-89 writes for one frame (include/svx.h, sv_jpeg_encode). img: (h, w, 3) uint8 BGR,
    or (h, w) uint8 grey, encoded as B = G = R; 1..4096 each way. The scan's bytes are libjpeg's at this quality with
    4:2:0 and one restart interval an MCU row; unpinned against cv2's own MJPG encoder."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError(f"picture must be uint8, got {a.dtype}")
    if a.ndim == 2:
        a = np.repeat(a[:, :, None], 3, axis=2)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"picture must be (h, w) or (h, w, 3), got {a.shape}")
    a = np.ascontiguousarray(a)
    h, w = a.shape[:2]
    cap = int(_abi.lib().sv_jpeg_bound(h, w))
    out = np.empty(max(cap, 1), np.uint8)
    size = ctypes.c_int64(0)
    _abi.call("sv_jpeg_encode", _abi.ptr(a), h, w, 3 * w, int(quality), _abi.ptr(out), cap, ctypes.byref(size))
    return out[: size.value].tobytes()


def jpeg_info(stream):
    """(h, w, restart interval in MCUs, header length) of a baseline JPEG stream, parsed on the host
    (include/svx.h, sv_jpeg_info); SvxError, naming what was met, for a stream outside the accepted kind."""
    s = np.frombuffer(bytes(stream), np.uint8)
    d = _abi.JpegDesc()
    _abi.call("sv_jpeg_info", _abi.ptr(s) if s.size else None, s.size, ctypes.byref(d))
    return int(d.h), int(d.w), int(d.restart_interval), int(d.header_len)


def jpeg_pack(streams):
    """A list of streams (bytes) as the packed run the decoder takes: (uint8 array, int64 offsets of len + 1)."""
    offs = np.zeros(len(streams) + 1, np.int64)
    np.cumsum([len(s) for s in streams], out=offs[1:])
    buf = np.frombuffer(b"".join(bytes(s) for s in streams), np.uint8)
    return (buf if buf.size else np.zeros(1, np.uint8)), offs


def jpeg_decode(stream, with_status=False):
    """The (h, w, 3) uint8 BGR picture of a baseline 4:2:0 JPEG stream (bytes), decoded on the GPU: libjpeg-turbo's
    default pixels byte for byte (include/svx.h, sv_jpeg_decode), the counterpart of jpeg_encode and
    what svx.video.VideoCapture.read() returns. A stream outside the accepted kind raises SvxError before anything
    is launched; so does malformed entropy-coded data (a non-zero status), unless with_status is set: then the
    result is (picture, status) and the picture of a frame with a status is unspecified."""
    s = np.frombuffer(bytes(stream), np.uint8)
    h, w, _, _ = jpeg_info(s)
    out = np.empty((h, w, 3), np.uint8)
    status = ctypes.c_int32(0)
    _abi.call("sv_jpeg_decode", _abi.ptr(s), s.size, _abi.ptr(out), h, w, 3 * w, ctypes.byref(status))
    if with_status:
        return out, int(status.value)
    if status.value:
        raise _abi.SvxError(f"malformed JPEG scan (status {status.value})")
    return out


def jpeg_decode_many(streams, device=0):
    """Streams of one size (a list of bytes) -> ((n, h, w, 3) uint8 BGR, (n,) int32 statuses): one upload, one
    read-back (sv_jpeg_decode_many)."""
    if not len(streams):
        raise ValueError("no streams")
    h, w, _, _ = jpeg_info(streams[0])
    buf, offs = jpeg_pack(streams)
    out = np.empty((len(streams), h, w, 3), np.uint8)
    status = np.zeros(len(streams), np.int32)
    _abi.call("sv_jpeg_decode_many", int(device), _abi.ptr(buf), _abi.ptr(offs), len(streams), h, w, _abi.ptr(out),
              _abi.ptr(status))
    return out, status


def jpeg_decode_stage_ms(device=0):
    """ms of the last jpeg_decode_many's four kernels: marker scan, entropy walk, chroma planes, picture."""
    ms = (ctypes.c_float * 4)()
    _abi.call("sv_jpeg_decode_stage_ms", int(device), ms)
    return [float(v) for v in ms]


def _tile_images(imgList, size):  # noqa: N803
    """The five arrays of a batchImages list that the device takes (grey, BGR, grey, grey, BGR uint8, all of shape
    `size`, H and W multiples of 4, the second one already green wherever the third is set: what stereovision.py:216
    passes), or None."""
    try:
        H, W = (int(v) for v in size)
        imgs = [np.asarray(i[1]) for i in imgList]
    except (TypeError, ValueError, IndexError):
        return None
    if len(imgs) != 5 or H % 4 or W % 4 or not (4 <= H <= 4096 and 4 <= W <= 4096):
        return None
    for a, colour in zip(imgs, (False, True, False, False, True)):
        if a.dtype != np.uint8 or a.shape != ((H, W, 3) if colour else (H, W)):
            return None
    # sv_image_tile paints imageRoadMap's quadrant from the road image: the same bytes only for a map that is painted
    if not (imgs[1][imgs[2] != 0] == (0, 255, 0)).all():
        return None
    return imgs


def batchImages(imgList, size):  # noqa: N802,N803
    """functions.py:456-501 for the list stereovision.py:216 passes: [(name, image)] of five images of shape `size`
    (grey, BGR, grey, grey, BGR; H and W multiples of 4; the second the imageRoadMap of the third) becomes the tile
    on the GPU (image_tile). Any other list goes to the function install() replaced, which needs cv2 as before;
    without one, SvxError. Installed only with install(.., tiles=True)."""
    imgs = _tile_images(imgList, size)
    if imgs is not None:
        return image_tile(*imgs)
    orig = _saved.get("batchImages", _ABSENT)
    if orig is _ABSENT or orig is None:
        raise _abi.SvxError("batchImages: only five images of shape `size` (grey, BGR, grey, grey, BGR, H and W "
                            "multiples of 4) are built on the device, and no function was replaced to take this list")
    return orig(imgList, size)


# ---------------------------------------------------------------------------
# general-scale bilinear resize (functions.py:452-454, :456-501)
# ---------------------------------------------------------------------------
RESIZE_MAX_SRC, RESIZE_MAX_DST = 8192, 4096   # include/svx.h, sv_resize_linear_u8


def resize_linear(img, size):
    """cv2.resize(img, (dw, dh)) of a uint8 image on the GPU, size = (dw, dh) as cv2 takes it: OpenCV's 8-bit
    INTER_LINEAR path at any scale (include/svx.h, sv_resize_linear_u8; unpinned against cv2 itself). img: (H, W)
    or (H, W, 3); or a stack (n, H, W, 3), or (n, H, W) whose W is not 3, resized in one launch. Source dimensions
    1..8192, destination dimensions 1..4096."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        raise TypeError(f"image must be uint8, got {a.dtype}")
    dw, dh = (int(v) for v in size)
    if a.ndim == 2:
        lead, (sh, sw), ch = (), a.shape, 1
    elif a.ndim == 3 and a.shape[2] == 3:
        lead, (sh, sw), ch = (), a.shape[:2], 3
    elif a.ndim == 3:
        lead, (sh, sw), ch = a.shape[:1], a.shape[1:], 1
    elif a.ndim == 4 and a.shape[3] == 3:
        lead, (sh, sw), ch = a.shape[:1], a.shape[1:3], 3
    else:
        raise ValueError(f"image must be (H, W), (H, W, 3), (n, H, W) or (n, H, W, 3), got shape {a.shape}")
    a = np.ascontiguousarray(a)
    out = np.empty(lead + (max(dh, 0), max(dw, 0)) + ((3,) if ch == 3 else ()), np.uint8)
    _abi.call("sv_resize_linear_u8", _abi.ptr(a), lead[0] if lead else 1, sh, sw, ch, _abi.ptr(out), dh, dw)
    return out


# ---------------------------------------------------------------------------
# stereo rectification: the fixed-point map pair and the remap (no reference function: nothing is installed)
# ---------------------------------------------------------------------------
REMAP_MAX_DIM = 8192   # include/svx.h, sv_remap_u8


def rectify_map(K, D, R, P, shape):
    """cv2.initUndistortRectifyMap(K, D, R, P, (dw, dh), cv2.CV_16SC2) for shape = (dh, dw), on the host in float64
    (include/svx.h, sv_rectify_map; no device): K the raw camera's 3 x 3 matrix, D up to 8 distortion coefficients
    k1, k2, p1, p2, k3, k4, k5, k6 (missing ones are 0), R the rectifying rotation, P the new camera matrix (3 x 3, or
    stereoRectify's 3 x 4, whose left 3 x 3 is taken). Returns (xy, frac): int16 (dh, dw, 2) holding (sx, sy) and
    uint16 (dh, dw) holding fy * 32 + fx. Unpinned against cv2 itself."""
    K = np.ascontiguousarray(np.asarray(K, np.float64))
    R = np.ascontiguousarray(np.asarray(R, np.float64))
    P = np.asarray(P, np.float64)
    if K.shape != (3, 3) or R.shape != (3, 3) or P.shape not in ((3, 3), (3, 4)):
        raise ValueError(f"K and R must be 3 x 3 and P 3 x 3 or 3 x 4, got {K.shape}, {R.shape}, {P.shape}")
    P = np.ascontiguousarray(P[:, :3])
    d = np.asarray([] if D is None else D, np.float64).reshape(-1)
    if d.size > 8:
        raise ValueError("at most the 8 coefficients k1, k2, p1, p2, k3, k4, k5, k6 (no thin-prism or tilt terms)")
    D8 = np.zeros(8, np.float64)
    D8[:d.size] = d
    dh, dw = (int(v) for v in shape)
    if not (1 <= dh <= REMAP_MAX_DIM and 1 <= dw <= REMAP_MAX_DIM):
        raise ValueError(f"shape (dh, dw) within 1 .. {REMAP_MAX_DIM}, got {(dh, dw)}")
    xy, frac = np.empty((dh, dw, 2), np.int16), np.empty((dh, dw), np.uint16)
    _abi.call("sv_rectify_map", _abi.ptr(K), _abi.ptr(D8), _abi.ptr(R), _abi.ptr(P), dh, dw, _abi.ptr(xy),
              _abi.ptr(frac))
    return xy, frac


def as_rectify_maps(xy, frac, shape=None):
    """The map pair as contiguous int16 (dh, dw, 2) and uint16 (dh, dw) arrays, checked on the host: dtypes, shapes
    (against `shape` = (dh, dw) when given) and every frac entry < 1024. cv2's CV_16SC2 pair passes as it is."""
    xy, frac = np.asarray(xy), np.asarray(frac)
    if xy.dtype != np.int16 or frac.dtype != np.uint16:
        raise TypeError(f"maps must be int16 (xy) and uint16 (frac) as cv2's CV_16SC2 pair, got {xy.dtype}, {frac.dtype}")
    if xy.ndim != 3 or xy.shape[2] != 2 or frac.shape != xy.shape[:2]:
        raise ValueError(f"maps must be (dh, dw, 2) and (dh, dw), got {xy.shape} and {frac.shape}")
    if shape is not None and xy.shape[:2] != tuple(shape):
        raise ValueError(f"maps of {xy.shape[:2]} for pictures of {tuple(shape)}")
    if not (1 <= xy.shape[0] <= REMAP_MAX_DIM and 1 <= xy.shape[1] <= REMAP_MAX_DIM):
        raise ValueError(f"map dimensions within 1 .. {REMAP_MAX_DIM}, got {xy.shape[:2]}")
    if int(frac.max()) >= 1024:
        raise ValueError("a frac entry >= 1024: entries are fy * 32 + fx with 5 bits each")
    return np.ascontiguousarray(xy), np.ascontiguousarray(frac)


def remap(src, xy, frac):
    """cv2.remap(src, xy, frac, cv2.INTER_LINEAR) (border constant 0) of a uint8 picture on the GPU through the
    fixed-point map pair (include/svx.h, sv_remap_u8; unpinned against cv2 itself). src: (H, W) or (H, W, 3); or a
    stack (n, H, W, 3), or (n, H, W) whose W is not 3, remapped through the one map in one launch. The result has the
    map's shape, which need not be the source's. Dimensions 1..8192."""
    a = np.asarray(src)
    if a.dtype != np.uint8:
        raise TypeError(f"image must be uint8, got {a.dtype}")
    if a.ndim == 2:
        lead, (sh, sw), ch = (), a.shape, 1
    elif a.ndim == 3 and a.shape[2] == 3:
        lead, (sh, sw), ch = (), a.shape[:2], 3
    elif a.ndim == 3:
        lead, (sh, sw), ch = a.shape[:1], a.shape[1:], 1
    elif a.ndim == 4 and a.shape[3] == 3:
        lead, (sh, sw), ch = a.shape[:1], a.shape[1:3], 3
    else:
        raise ValueError(f"image must be (H, W), (H, W, 3), (n, H, W) or (n, H, W, 3), got shape {a.shape}")
    if not (1 <= sh <= REMAP_MAX_DIM and 1 <= sw <= REMAP_MAX_DIM) or (lead and lead[0] < 1):
        raise ValueError(f"source dimensions within 1 .. {REMAP_MAX_DIM} and at least one picture, got shape {a.shape}")
    xy, frac = as_rectify_maps(xy, frac)
    dh, dw = frac.shape
    a = np.ascontiguousarray(a)
    out = np.empty(lead + (dh, dw) + ((3,) if ch == 3 else ()), np.uint8)
    _abi.call("sv_remap_u8", _abi.ptr(a), lead[0] if lead else 1, sh, sw, ch, _abi.ptr(xy), _abi.ptr(frac), dh, dw,
              _abi.ptr(out))
    return out


def camera_from_projection(P_left, P_right):  # noqa: N803
    """The sv_camera of a rectified pair from stereoRectify's projections, in float64 on the host: f = P1[0][0],
    B = -P2[0][3] / f, cw = P1[0][2], ch = P1[1][2]. P_left 3 x 3 or 3 x 4, P_right 3 x 4. This is the camera to hand
    to every stage behind Batch.rectify()."""
    P1, P2 = np.asarray(P_left, np.float64), np.asarray(P_right, np.float64)
    if P1.shape not in ((3, 3), (3, 4)) or P2.shape != (3, 4):
        raise ValueError(f"P_left must be 3 x 3 or 3 x 4 and P_right 3 x 4, got {P1.shape} and {P2.shape}")
    f = float(P1[0, 0])
    if not np.isfinite(f) or f == 0.0:
        raise ValueError("P_left[0][0], the focal length, must be finite and not 0")
    return _abi.Camera(f, float(-P2[0, 3] / P1[0, 0]), float(P1[0, 2]), float(P1[1, 2]))


def _list_images(imgList):  # noqa: N803
    """The arrays of a batchImages list: [(name, image)] pairs or plain arrays."""
    return [np.asarray(i[1] if isinstance(i, (tuple, list)) else i) for i in imgList]


def _images_tile_shape(imgs, size):
    """The (rows, columns) of batchImages(imgs, size) where the device builds it (include/svx.h, sv_images_tile), else
    None: a dtype other than uint8, other than 1..5 pictures, an odd H or W the final resize excludes, or a dimension
    beyond the limits. Host arithmetic only."""
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        return None
    n = len(imgs)
    if not (1 <= n <= 5 and 1 <= H <= RESIZE_MAX_DST and 1 <= W <= RESIZE_MAX_DST):
        return None
    if (n in (2, 5) and H % 2) or (n == 5 and W % 2):
        return None
    for a in imgs:
        if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
            return None
        if not (1 <= a.shape[0] <= RESIZE_MAX_DST and 1 <= a.shape[1] <= RESIZE_MAX_DST):
            return None
    return (H // 2 if n in (2, 5) else H), W


def images_tile(imgList, size):  # noqa: N803
    """batchImages(imgList, size) (functions.py:456-501) on the GPU for one to five pictures, size = (H, W): a list of
    (name, image) pairs or of arrays, each (h, w) or (h, w, 3) uint8 of any shape within 1..4096. Every picture is
    resized to `size`, grey becomes BGR, the stack is built and resized on the device as the reference composes it
    (include/svx.h, sv_images_tile). H even for two pictures, H and W even for five."""
    imgs = [np.ascontiguousarray(a) for a in _list_images(imgList)]
    for a in imgs:
        if a.dtype != np.uint8:
            raise TypeError(f"images must be uint8, got {a.dtype}")
        if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
            raise ValueError(f"images must be (h, w) or (h, w, 3), got shape {a.shape}")
    H, W = (int(v) for v in size)
    n = len(imgs)
    pics = (_abi.Picture * max(n, 1))()
    for k, a in enumerate(imgs[:len(pics)]):
        pics[k] = _abi.Picture(a.ctypes.data, a.shape[0], a.shape[1], 3 if a.ndim == 3 else 1)
    oh, ow = ctypes.c_int(0), ctypes.c_int(0)
    _abi.call("sv_images_tile_shape", n, H, W, ctypes.byref(oh), ctypes.byref(ow))
    out = np.empty((oh.value, ow.value, 3), np.uint8)
    _abi.call("sv_images_tile", pics, n, H, W, _abi.ptr(out))
    return out


def resizeImage(image, height, width):  # noqa: N802
    """functions.py:452-454, cv2.resize(image, (width, height)), on the GPU (resize_linear). An image the kernel does
    not take (not uint8, not (H, W) or (H, W, 3), a dimension beyond the limits) goes to the function install()
    replaced; without one, SvxError. Installed only with install(.., resize=True)."""
    a = np.asarray(image)
    ok = a.dtype == np.uint8 and (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) and \
        all(1 <= v <= RESIZE_MAX_SRC for v in a.shape[:2]) and \
        1 <= int(height) <= RESIZE_MAX_DST and 1 <= int(width) <= RESIZE_MAX_DST
    if ok:
        return resize_linear(a, (width, height))
    orig = _saved.get("resizeImage", _ABSENT)
    if orig is _ABSENT or orig is None:
        raise _abi.SvxError("resizeImage: only uint8 (H, W) or (H, W, 3) images within the limits are resized on the "
                            "device, and no function was replaced to take this one")
    return orig(image, height, width)


def batch_images(imgList, size):  # noqa: N803
    """functions.py:456-501 for any list the device takes (images_tile): one to five uint8 pictures of any shapes.
    A list it cannot take (a dtype other than uint8, no or more than five pictures, an odd H or W that the final
    resize excludes, a dimension beyond the limits) goes to the function install() replaced, which needs cv2 as
    before; without one, SvxError. This is what install(.., resize=True) puts in batchImages' place."""
    try:
        imgs = _list_images(imgList)
    except (TypeError, ValueError, IndexError):
        imgs = None
    if imgs is not None and _images_tile_shape(imgs, size) is not None:
        return images_tile(imgs, size)
    orig = _saved.get("batchImages", _ABSENT)
    if orig is _ABSENT or orig is None:
        raise _abi.SvxError("batchImages: one to five uint8 pictures within 1..4096 (H even for two, H and W even for "
                            "five) are built on the device, and no function was replaced to take this list")
    return orig(imgList, size)


def getCenterPoint(points):  # noqa: N802
    """functions.py:418-421 with the exact circle: (int(x), int(y)) of the centre of the minimum enclosing circle of
    any (n, 1, 2) or (n, 2) integer points (|coordinate| <= 16383, at most 8192 distinct ones), computed in integers on the GPU. The reference's
    cv2.minEnclosingCircle is a float32 approximation: installed only with install(.., hull=True)."""
    p = np.asarray(points)
    if p.dtype.kind not in "iu" or p.size == 0 or p.size % 2:
        raise TypeError("getCenterPoint takes a non-empty (n, 1, 2) or (n, 2) integer array")
    p = np.unique(p.reshape(-1, 2).astype(np.int64), axis=0)     # duplicates do not move the circle
    if len(p) > 8192:
        raise ValueError("getCenterPoint takes at most 8192 distinct points (a hull, not a cloud)")
    if np.abs(p).max() > 16383:
        raise ValueError("getCenterPoint: coordinates beyond +-16383")
    p = p.astype(np.int32)
    out = np.zeros(2, np.int32)
    _abi.call("sv_min_circle_centre", _abi.ptr(p), len(p), _abi.ptr(out))
    return (int(out[0]), int(out[1]))


# snake_case names used by BASELINE.json
project_disparity_to_3d = projectDisparityTo3d
project_3D_points_to_2D = project3DPointsTo2DImagePoints

from .ransac import RANSAC  # noqa: E402  (functions.py:278-298)
from .stages import (calculateColourHistogram, calculatePointErrors, computePlanarThreshold,  # noqa: E402,F401
                     filterPointsByHistogram)
from .disparity import disparity, gammaChange, greyscale, preProcessImages  # noqa: E402,F401 (functions.py:61-128)
from .io import getImagePaths, loadImages  # noqa: E402,F401 (functions.py:41-55, PNG ingest without cv2)

# Functions whose GPU results are pinned against the reference itself (fixtures made by running the reference's
# own code, tests/golden/): installed by default.
PINNED = ("projectDisparityTo3d", "project3DPointsTo2DImagePoints", "fillAltDisparity", "capDisparity",
          "generatePointsAsImage", "RANSAC", "calculatePointErrors", "computePlanarThreshold",
          "calculateColourHistogram", "filterPointsByHistogram", "gammaChange", "preProcessImages")
# Functions that restate OpenCV calls (cv2 is absent here, so nothing pins them to the reference's OpenCV 3.x):
# StereoSGBM + filterSpeckles (functions.py:104-128), cvtColor + equalizeHist (:88-96), cv2.threshold / bitwise /
# add (:140-147), bitwise_and with the carmask (:169-171) and cv2.imread's PNG decode behind getImagePaths /
# loadImages (:41-55; lossless, but OpenCV's channel handling is restated, svx/io.py). Installed only on request
# (install(.., unpinned=True)).
UNPINNED = ("disparity", "greyscale", "fillDisparity", "maskDisparity", "getImagePaths", "loadImages")
PATCHED = PINNED + UNPINNED
# sanitiseRoadImage (functions.py:346-366) restates cv2.morphologyEx / erode / bitwise_and and argues ParticleCleansing
# away: unpinned like the above, and installed only with install(.., morphology=True).
MORPHOLOGY = ("sanitiseRoadImage",)
# getCenterPoint (functions.py:418-421) returns the exact circle's centre where cv2.minEnclosingCircle approximates
# in float32 (which way depends on its version): unpinned too, installed only with install(.., hull=True).
HULL = ("getCenterPoint",)
# batchImages (functions.py:456-501) restates cv2.resize at the two scales stereovision.py:216 uses (exact quarter
# weights, include/svx.h): unpinned as well, installed only with install(.., tiles=True).
TILES = ("batchImages",)
# resizeImage and batchImages (functions.py:452-501) over cv2.resize's 8-bit bilinear path at any scale (include/svx.h,
# sv_resize_linear_u8, sv_images_tile): unpinned likewise, installed only with install(.., resize=True). With
# tiles=True as well, this group decides batchImages.
RESIZE = ("resizeImage", "batchImages")
_RESIZE_IMPL = {"resizeImage": "resizeImage", "batchImages": "batch_images"}
ALIASES = {"project_disparity_to_3d": "projectDisparityTo3d",
           "project_3D_points_to_2D": "project3DPointsTo2DImagePoints"}
_saved = {}
_ABSENT = object()


def install(functions_module, unpinned=False, morphology=False, hull=False, tiles=False, resize=False):
    """Patch the reference's `functions` module in place (stereovision.py resolves
    f.<name> at call time, so performStereoVision picks the GPU path up).

    By default only the PINNED functions are replaced: the ones whose outputs equal the
    reference's own on its fixtures. unpinned=True also replaces the UNPINNED ones, the
    restatements of OpenCV (SGBM, grey + equalizeHist, fillDisparity, maskDisparity, and
    getImagePaths / loadImages: cv2.imread of the PNG pairs, svx.io) whose equality with the
    reference's cv2 cannot be checked here. morphology=True also replaces
    sanitiseRoadImage (MORPHOLOGY: the road image's 9 x 9 close / erode / mask / close and its
    pixel walk, with the module's road_threshold_mask), a restatement of cv2 calls as well;
    hull=True also replaces getCenterPoint (HULL) by the exact circle's centre; tiles=True
    also replaces batchImages (TILES): the five-picture tile on the device, any other list
    handed on to the module's own function; resize=True replaces resizeImage and batchImages
    (RESIZE) by the general-scale resize: any list of one to five uint8 pictures is composed on
    the device, and it decides batchImages when tiles=True is given too."""
    global _module
    _abi.lib()  # fail loudly now if libsvx is missing
    _module = functions_module
    names = PINNED + (UNPINNED if unpinned else ()) + (MORPHOLOGY if morphology else ()) + \
        (HULL if hull else ()) + (TILES if tiles else ()) + (RESIZE if resize else ()) + tuple(ALIASES)
    for name in names:
        if name not in _saved:
            _saved[name] = getattr(functions_module, name, _ABSENT)
        impl = _RESIZE_IMPL[name] if resize and name in RESIZE else ALIASES.get(name, name)
        setattr(functions_module, name, globals()[impl])
    return functions_module


def uninstall():
    """Restore the attributes install() replaced."""
    global _module
    if _module is not None:
        for name, fn in _saved.items():
            if fn is _ABSENT:
                if hasattr(_module, name):
                    delattr(_module, name)
            else:
                setattr(_module, name, fn)
    _saved.clear()
    _module = None
