"""The result image's oracle (stereovision.py:181-209, functions.py:390-394, :424-431), restated without the kernel's
shortcuts: include/svx.h (sv_result_image) states the semantics, tests/test_result_cpu.py pins this file.

  blend(bgr, obst)          layer 1: rint(0.6 i) on every channel, + 102 on G and R of obstacle pixels, in integers
  near_segment(shape, a, b, kn, kd)   every pixel against one segment: kn * D(p; a, b) <= kd, exact integers
  outline(shape, hull)      layer 2's pixels: every pixel against every edge of the closed polygon
  glyph_drawn(valid, tip)   whether layers 3 and 4 are drawn
  result(bgr, obstacles, hull, centre, tip, valid)   the whole image
"""
import numpy as np

OUTLINE_BGR = (0, 0, 255)
LINE_BGR = (204, 185, 22)
HEAD_BGR = (214, 195, 32)
INT32_MAX = 2 ** 31 - 1


def blend(bgr, obst):
    """cv2.addWeighted(obst_image, 0.4, img, 0.6, 0) with obst_image = (0, 255, 255) on obstacle pixels, else 0."""
    v = np.asarray(bgr).astype(np.int64)
    out = (6 * v + 5) // 10
    tint = np.where(np.asarray(obst) != 0, 102, 0)
    out[..., 1] += tint
    out[..., 2] += tint
    assert out.max(initial=0) <= 255
    return out.astype(np.uint8)


def near_segment(shape, a, b, kn, kd):
    """(H, W) bool: kn * D(p; a, b) <= kd, D the squared distance from the pixel p = (x, y) to the closed segment
    ab (a point when a == b). Exact: int64 while every term fits, Python ints beyond."""
    H, W = shape
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    big = max(abs(ax), abs(ay), abs(bx), abs(by)) > 30000
    dt = object if big else np.int64
    X, Y = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    X, Y = X.astype(dt), Y.astype(dt)
    dx, dy = bx - ax, by - ay
    wx, wy = X - ax, Y - ay
    ux, uy = X - bx, Y - by
    t = wx * dx + wy * dy
    L = dx * dx + dy * dy
    cr = dx * wy - dy * wx
    at_a = (kn * (wx * wx + wy * wy) <= kd).astype(bool)
    at_b = (kn * (ux * ux + uy * uy) <= kd).astype(bool)
    inner = (kn * cr * cr <= kd * L).astype(bool)
    return np.where((t <= 0).astype(bool), at_a, np.where((t >= L).astype(bool), at_b, inner))


def edges(hull):
    """The segments of the closed polygon in the stored order: n = 1 the point, n = 2 the one segment."""
    v = [(int(x), int(y)) for x, y in np.asarray(hull).reshape(-1, 2).tolist()]
    if len(v) <= 1:
        return [(p, p) for p in v]
    if len(v) == 2:
        return [(v[0], v[1])]
    return [(v[i], v[(i + 1) % len(v)]) for i in range(len(v))]


def outline(shape, hull):
    m = np.zeros(shape, bool)
    for a, b in edges(hull):
        m |= near_segment(shape, a, b, 4, 25)
    return m


def glyph_drawn(valid, tip):
    return bool(valid & 2) and tip is not None and abs(int(tip[0])) <= INT32_MAX and abs(int(tip[1])) <= INT32_MAX


def result(bgr, obstacles, hull, centre=None, tip=None, valid=None):
    """The result image of one frame: bgr (H, W, 3) uint8, obstacles (H, W) non-zero = obstacle, hull (n, 1, 2) or
    (n, 2), centre / tip as Batch.read_road_hull returns them (None where the valid bit is clear)."""
    bgr = np.asarray(bgr)
    shape = bgr.shape[:2]
    n = len(np.asarray(hull).reshape(-1, 2))
    if valid is None:
        valid = (1 if centre is not None else 0) | (2 if centre is not None and tip is not None else 0)
    if n == 0:
        return bgr.copy()
    out = blend(bgr, obstacles)
    out[outline(shape, hull)] = OUTLINE_BGR
    if glyph_drawn(valid, tip):
        out[near_segment(shape, centre, tip, 1, 1)] = LINE_BGR
        out[near_segment(shape, tip, tip, 1, 49)] = HEAD_BGR
    return out
