"""The obstacle stage's oracle (stereovision.py:170-189, functions.py:396-421), restated without the kernel's
shortcuts: include/svx.h (sv_road_obstacles) states the semantics, tests/test_hull_cpu.py pins this file.

  hull(img)            Andrew's monotone chain over ALL set pixels with Python ints (no row extremes), strict
                       vertices, in the ABI's order: from the smallest (y, x) down the left side, up the right side
  hull_mask(shape, v)  every pixel against every edge, int64 half-plane tests (n <= 2: the lattice points of the
                       point or segment)
  min_circle(pts)      brute force over all pairs and triples with fractions.Fraction
  centre(pts)          its centre truncated toward zero
  glyph(centre, abc, disparity, camera)   getNormalVectorLine statement for statement with numpy scalars
  obstacles(img, ...)  the whole stage as the dict Batch.read_road_hull returns
"""
import math
from fractions import Fraction

import numpy as np

CAMERA = (399.9745178222656, 0.2090607502, 474.5, 262.0)   # functions.py:15,19,21,22


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull_of_points(points, presorted=False):
    """Strict convex-hull vertices of integer (x, y) points, in the ABI's order (presorted: distinct tuples of
    Python ints, already sorted)."""
    pts = points if presorted else sorted({(int(x), int(y)) for x, y in points})
    if len(pts) <= 1:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    ring = lower[:-1] + upper[:-1]          # collinear points: [first, last]
    # start at the smallest (y, x) ...
    k = min(range(len(ring)), key=lambda i: (ring[i][1], ring[i][0]))
    ring = ring[k:] + ring[:k]
    if len(ring) > 2:
        # ... and go down the left side first: on the screen (x right, y down) that ring has a negative
        # shoelace sum ((0,0) -> (0,1) -> (1,1) -> (1,0) gives -2)
        area2 = sum(ring[i][0] * ring[(i + 1) % len(ring)][1] - ring[(i + 1) % len(ring)][0] * ring[i][1]
                    for i in range(len(ring)))
        assert area2 != 0
        if area2 > 0:
            ring = [ring[0]] + ring[:0:-1]
    return ring


def hull(img):
    """(n, 2) int32 [x, y] of the strict hull vertices of the non-zero pixels of img (all of them go through the
    chain)."""
    ys, xs = np.nonzero(np.asarray(img))
    order = np.lexsort((ys, xs))             # by x, then y; the pixels are distinct
    ring = hull_of_points(list(zip(xs[order].tolist(), ys[order].tolist())), presorted=True)
    return np.array(ring, np.int32).reshape(-1, 2)


def hull_mask(shape, verts):
    """(H, W) uint8 of 0 / 255: the pixels in the closed hull, each against every edge in int64."""
    H, W = shape
    v = np.asarray(verts, np.int64).reshape(-1, 2)
    out = np.zeros((H, W), bool)
    if len(v) == 0:
        return out.astype(np.uint8)
    X, Y = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    if len(v) == 1:
        out = (X == v[0, 0]) & (Y == v[0, 1])
    elif len(v) == 2:
        (ax, ay), (bx, by) = v
        cr = (bx - ax) * (Y - ay) - (by - ay) * (X - ax)
        out = (cr == 0) & (X >= min(ax, bx)) & (X <= max(ax, bx)) & (Y >= min(ay, by)) & (Y <= max(ay, by))
    else:
        out = np.ones((H, W), bool)
        sign = 0
        for i in range(len(v)):
            ax, ay = v[i]
            bx, by = v[(i + 1) % len(v)]
            cr = (bx - ax) * (Y - ay) - (by - ay) * (X - ax)
            if sign == 0:   # the ring's orientation, from a vertex that is not on this edge
                cx, cy = v[(i + 2) % len(v)]
                sign = 1 if (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) > 0 else -1
            out &= (cr * sign >= 0)
    return out.astype(np.uint8) * 255


def _circle2(a, b):
    c = (Fraction(a[0] + b[0], 2), Fraction(a[1] + b[1], 2))
    return c, (c[0] - a[0]) ** 2 + (c[1] - a[1]) ** 2


def _circle3(a, b, c):
    bx, by, cx, cy = b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1]
    d = 2 * (bx * cy - by * cx)
    if d == 0:
        return None
    ux = Fraction(cy * (bx * bx + by * by) - by * (cx * cx + cy * cy), d)
    uy = Fraction(bx * (cx * cx + cy * cy) - cx * (bx * bx + by * by), d)
    return (a[0] + ux, a[1] + uy), ux * ux + uy * uy


def min_circle(points):
    """((cx, cy), r^2) as Fractions: the smallest of the circles through two points (as a diameter) or three that
    holds every point. Brute force."""
    pts = sorted({(int(x), int(y)) for x, y in np.asarray(points).reshape(-1, 2).tolist()})
    if not pts:
        return None
    if len(pts) == 1:
        return (Fraction(pts[0][0]), Fraction(pts[0][1])), Fraction(0)
    best = None

    def offer(circ):
        nonlocal best
        if circ is None:
            return
        (cx, cy), r2 = circ
        if best is not None and r2 >= best[1]:
            return
        for x, y in pts:
            if (x - cx) ** 2 + (y - cy) ** 2 > r2:
                return
        best = circ

    n = len(pts)
    for i in range(n):
        for j in range(i + 1, n):
            offer(_circle2(pts[i], pts[j]))
    for i in range(n):
        for j in range(i + 1, n):
            for k in range(j + 1, n):
                offer(_circle3(pts[i], pts[j], pts[k]))
    return best


def centre(points):
    """(int(cx), int(cy)) of min_circle, truncated toward zero; None without points."""
    c = min_circle(points)
    if c is None:
        return None
    return (math.trunc(c[0][0]), math.trunc(c[0][1]))


def glyph(base, abc, disparity, camera=CAMERA):
    """functions.py:396-416 getNormalVectorLine(basePoint, abc, disparity): the same operations in the same order on
    the same numpy scalar types, one statement per statement of the reference; raises where it raises."""
    f, B, cw, ch = camera
    x, y = base
    with np.errstate(all="ignore"):
        depth = (f * B) / disparity[y, x]
        px = ((x - cw) * depth) / f
        py = ((y - ch) * depth) / f
        py = py - 0.7
        px = px + 0.0
        norm = math.sqrt(abc[0] * abc[0] + abc[1] * abc[1] + abc[2] * abc[2])
        depth = norm - ((abc[0] * px) + (abc[1] * py))
        px = ((px * f) / depth) + cw
        py = ((py * f) / depth) + ch
    return (int(px), int(py))


def tip(base, abc, disparity, camera=CAMERA):
    """glyph() or None where the reference raises (d == 0 included: numpy's division gives inf / nan there and
    int() raises) or a result does not fit an int64."""
    if base is None or abc is None or disparity is None:
        return None
    if disparity[base[1], base[0]] == 0:
        return None
    try:
        t = glyph(base, np.asarray(abc, np.float64), disparity, camera)
    except (ValueError, OverflowError, ZeroDivisionError):
        return None
    if abs(t[0]) >= 2 ** 63 or abs(t[1]) >= 2 ** 63:
        return None
    return t


def obstacles(cleaned, disparity=None, abc=None, camera=CAMERA):
    """The whole stage, as Batch.read_road_hull / dropin.road_obstacles return it."""
    img = np.asarray(cleaned)
    v = hull(img)
    m = hull_mask(img.shape, v)
    c = centre(v) if len(v) else None
    t = tip(c, abc, disparity, camera)
    return {"hull": v.reshape(-1, 1, 2), "hull_mask": m, "obstacles": m & np.where(img != 0, 0, 255).astype(np.uint8),
            "centre": c, "tip": t, "valid": (1 if c is not None else 0) | (2 if t is not None else 0)}


# ---- the test inputs shared by tests/test_hull_cpu.py and tests/test_gpu_hull.py -------------------------------
def fill_polygon(shape, verts):
    """The lattice points of the closed convex polygon `verts`, as an image of 0 / 255."""
    return hull_mask(shape, np.array(hull_of_points(verts)))


def polygon_steep_shallow(H, W):
    """An octagon-like ring with a steep and a shallow edge on each side, going down and going up (both signs of
    the spans' numerators on both chains); coordinates scale with the frame."""
    fr = [(0.45, 0.03), (0.12, 0.10), (0.03, 0.52), (0.10, 0.90), (0.50, 0.97), (0.88, 0.80), (0.97, 0.33),
          (0.70, 0.08)]
    return [(int(round(fx * (W - 1))), int(round(fy * (H - 1)))) for fx, fy in fr]


def cases(H, W, seed=0):
    """name -> (H, W) uint8 image of 0 / 255: the inputs tests/test_gpu_hull.py lists."""
    rng = np.random.default_rng(7000 + 31 * H + W + seed)
    z = lambda: np.zeros((H, W), np.uint8)   # noqa: E731
    out = {}
    out["empty"] = z()
    a = z(); a[H // 3, W - 2] = 255; out["one_pixel"] = a
    a = z(); a[H - 2, 3:W - 1:5] = 255; out["one_row"] = a
    a = z(); a[1:H - 2:3, 33 if W > 40 else 5] = 255; out["one_column"] = a
    a = z()
    k = min((W - 3) // 3, (H - 2) // 2)
    for i in range(k):
        a[1 + 2 * i, 2 + 3 * i] = 255        # slope 2 / 3: all collinear
    out["diagonal_2_3"] = a
    out["full"] = np.full((H, W), 255, np.uint8)
    a = z(); a[0, 0] = a[0, W - 1] = a[H - 1, 0] = a[H - 1, W - 1] = 255; out["corners"] = a
    # a right triangle whose hypotenuse (steps of (-3, 2)) and legs carry extra lattice points
    m = min((W - 8) // 3, (H - 8) // 2)
    out["triangle"] = fill_polygon((H, W), [(4, 3), (4 + 3 * m, 3), (4, 3 + 2 * m)])
    a = z()
    a[2:2 + H // 4, 3:3 + W // 5] = 255
    a[H - 1 - H // 3:H - 1, W - 2 - W // 4:W - 2] = 255
    out["two_blobs"] = a
    a = z()
    n = max(12, H * W // 3000)
    a[rng.integers(0, H, n), rng.integers(0, W, n)] = 255
    out["sparse"] = a
    a = z()
    for x, y in polygon_steep_shallow(H, W):
        a[y, x] = 255
    a[rng.integers(H // 3, 2 * H // 3, 20), rng.integers(W // 3, 2 * W // 3, 20)] = 255   # inside the ring
    out["steep_shallow"] = a
    a = z(); a[H // 4:H // 4 + H // 3, W // 5:W // 5 + W // 2] = 255; out["rectangle"] = a
    return out
