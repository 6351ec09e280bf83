"""Cameras, frames and planes of the non-default-camera tests (shared by make_camera_golden.py,
tests/test_camera_cpu.py and tests/test_gpu_camera.py, so only outputs are stored).

A camera is (f, B, cw, ch): focal length in pixels, baseline in metres, image centre (functions.py:15-22).
The reference's own centre (474.5, 262.0) is exact in fp32, so the low words of the kernels' split centre
(KParams::cw_lo / ch_lo, svx_device.h centred()) are zero there. These cameras make them matter:

* near_int      centre inside the small frames, a hair off the even grid point (36, 22): x - cw cancels to
                about 3e-4, so the low word is most of the value (a dropped low word is a 4.5e-3 relative
                error in X, against the suite's 1e-5)
* near_int_big  the same from the other side of the integer, at another f and B
* rig2          another plausible rig (the one test_delta_tables uses); centre not exact in fp32, inside
                544 x 1024 and outside the small frames
* off           principal point outside the frame on both axes, cw negative: x - cw never changes sign and
                the chunk-skipping bound ub0 is large
"""
import numpy as np

CAMERAS = {
    "near_int": (401.25, 0.21, 36.0003, 22.0002),
    "near_int_big": (1203.9, 0.075, 100.00004, 47.99997),
    "rig2": (401.25, 0.21, 500.3, 250.7),
    "off": (612.7, 0.12, -35.4, 700.9),
}
# the grid point (x, y) next to the centre of the two near-integer cameras
NEAR_GRID = {"near_int": (36, 22), "near_int_big": (100, 48)}

# 72 x 152: multiples of 4 and not of 32 (the last word of each delta-table row is partial);
# 69 x 149: ragged (the grid is range(0, H - 1, step), the pitch is padded)
SHAPES = ((72, 152), (69, 149))
FIXTURE_SHAPE = SHAPES[0]
SEED = 20250


def frame(H, W, k=0):
    """Frame k of a shape: a disparity ramp d = rint(0.6 (y - 8)) + {-2..2} with a quarter of the pixels
    zeroed, and uniformly random colours. The ramp puts a band of points on the keep1 boundary of PLANES."""
    rng = np.random.default_rng([SEED, H, W, k])
    y = np.arange(H, dtype=np.float64)[:, None]
    d = np.rint(0.6 * (y - 8)) + rng.integers(-2, 3, (H, W))
    d = np.clip(d, 0, 255).astype(np.uint8)
    d[rng.random((H, W)) < 0.25] = 0
    bgr = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    return d, bgr


def sparse_frame(H, W, n=300, k=0):
    """A frame whose step-2 grid holds exactly n (< 600) points: RANSAC finds no plane for it."""
    rng = np.random.default_rng([SEED, H, W, 1000 + k])
    hg, wg = (H - 1 + 1) // 2, (W - 1 + 1) // 2
    cells = rng.choice(hg * wg, n, replace=False)
    d = np.zeros((H, W), np.uint8)
    d[2 * (cells // wg), 2 * (cells % wg)] = rng.integers(1, 40, n)
    return d, rng.integers(0, 256, (H, W, 3)).astype(np.uint8)


# carmask()[:72, :152] is all zero (the mask starts at row 108): under it every frame has no maskpoints and
# takes the no-plane path. This 72 x 152 window crosses the mask's edge and keeps about two thirds of the grid.
MASK_WINDOW = (152, 392)


def mask_cuts(carmask):
    """{"corner": carmask[:72, :152] (all zero), "edge": the window at MASK_WINDOW} of the 544 x 1024 carmask."""
    H, W = FIXTURE_SHAPE
    y0, x0 = MASK_WINDOW
    return {"corner": np.ascontiguousarray(carmask[:H, :W]),
            "edge": np.ascontiguousarray(carmask[y0:y0 + H, x0:x0 + W])}


def plane(camera, horizon, a):
    """u = a X + b Y + c Z is about 0.6 (y - horizon) / d in image terms, whatever the camera."""
    f, B, _, ch = camera
    return (a, 0.6 / B, -0.6 * (horizon - ch) / (f * B))


# name -> (horizon, a, point_thr, hist_thr)
PLANES = {
    "some": (8, 0.003, 0.02, 1),
    "tight": (8, 0.02, 0.005, 1),
    "all_out": (-1000, 0.003, 0.05, 1),     # every chunk is ruled out
    "none_out": (8, 0.003, 1e9, 1),         # none is: every valid point is kept
}
FIXTURE_PLANES = ("some", "tight")


def plane_case(camera, name):
    """(abc, point_thr, hist_thr) of a named plane under a camera."""
    horizon, a, pthr, hthr = PLANES[name]
    return plane(camera, horizon, a), pthr, hthr
