"""CPU: the result image's oracle tests/result_numpy.py (include/svx.h, sv_result_image) pinned: the overlay against
cv2.addWeighted's arithmetic under four fp32 evaluation orders, the strokes against closed forms, layer priority,
clipping, the glyph's conditions, and a Python restatement of the kernel's method (kernels/result.hip: per-row
intervals found by bisection, two runs for the outline) against the brute-force oracle."""
import numpy as np
import pytest

import hull_numpy as hn
import result_numpy as rn

ABC = (0.013, -0.62, 0.047)
RED = list(rn.OUTLINE_BGR)
LINE = list(rn.LINE_BGR)
HEAD = list(rn.HEAD_BGR)


def _bgr(shape, seed=0):
    """Random BGR with the values 0 and 255 in it."""
    rng = np.random.default_rng(4100 + seed + shape[0])
    a = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
    a[rng.random(shape) < 0.05] = 0
    a[rng.random(shape) < 0.05] = 255
    return a


# ---- layer 1 against cv2.addWeighted's arithmetic --------------------------------------------------------------
def test_blend_table_under_four_fp32_orders():
    """All 512 (obst, i) pairs: saturate_cast<uchar>(obst * 0.4 + i * 0.6 + 0) (cvRound: to nearest, ties to even)
    gives the integer form whichever way the fp32 (or fp64) expression is evaluated."""
    f32 = np.float32
    i = np.arange(256)
    for obst in (0, 255):
        want = (6 * i + 5) // 10 + (102 if obst else 0)
        assert want.max() <= 255
        o32, i32 = f32(obst), i.astype(f32)
        a, b, g = f32(0.4), f32(0.6), f32(0.0)
        orders = {
            "left to right": (o32 * a + i32 * b) + g,
            "image first": (i32 * b + g) + o32 * a,
            # fused: the products exact (fp64 holds a product of two fp32), one rounding at the end
            "fused": (np.float64(o32) * np.float64(a) + i32.astype(np.float64) * np.float64(b)).astype(f32),
            "fp64": np.float64(obst) * 0.4 + i.astype(np.float64) * 0.6 + 0.0,
        }
        for name, v in orders.items():
            assert v.dtype == (np.float64 if name == "fp64" else f32), name
            frac = np.abs(v.astype(np.float64) - np.rint(v.astype(np.float64)))
            assert (np.abs(frac - 0.5) > 0.05).all(), name            # never near a tie
            assert np.array_equal(np.rint(v).astype(np.int64), want), (obst, name)
    # the oracle's blend is that table: B never tinted, G and R tinted on obstacle pixels
    img = np.stack([i, i, i], -1).astype(np.uint8)[None]                # (1, 256, 3)
    for obst in (0, 255):
        got = rn.blend(img, np.full((1, 256), obst, np.uint8))
        t = 102 if obst else 0
        assert np.array_equal(got[0, :, 0], (6 * i + 5) // 10)
        assert np.array_equal(got[0, :, 1], (6 * i + 5) // 10 + t) and np.array_equal(got[0, :, 2], got[0, :, 1])


# ---- closed-form strokes ---------------------------------------------------------------------------------------
def test_dot_head_and_point_line_counts():
    shape = (40, 70)
    m = rn.outline(shape, [(30, 20)])
    assert m.sum() == 21                                                  # dx^2 + dy^2 <= 6
    ys, xs = np.nonzero(m)
    assert set(zip((xs - 30).tolist(), (ys - 20).tolist())) == {(dx, dy) for dx in range(-3, 4) for dy in range(-3, 4)
                                                               if dx * dx + dy * dy <= 6}
    assert rn.near_segment(shape, (30, 20), (30, 20), 1, 49).sum() == 149  # the head, radii 0-7
    assert rn.near_segment(shape, (30, 20), (30, 20), 1, 1).sum() == 5     # a line with centre == tip


def test_horizontal_and_vertical_outline_segments():
    shape = (40, 70)
    m = rn.outline(shape, [(10, 20), (50, 20)])
    want = np.zeros(shape, bool)
    want[18:23, 10:51] = True                                             # |dy| <= 2 along the segment
    for dy, r in ((0, 2), (1, 2), (-1, 2), (2, 1), (-2, 1)):              # caps: dx^2 + dy^2 <= 6.25
        want[20 + dy, 10 - r:10] = True
        want[20 + dy, 51:51 + r] = True
    assert np.array_equal(m, want)
    assert np.array_equal(rn.outline(shape, [(50, 20), (10, 20)]), want)  # either direction
    v = rn.outline((70, 40), [(20, 10), (20, 50)])
    assert np.array_equal(v, want.T)


def test_layer_priority_where_all_four_meet():
    shape = (40, 70)
    bgr = _bgr(shape)
    obst = np.full(shape, 255, np.uint8)
    hull = [(20, 10), (20, 30), (40, 30), (40, 10)]
    centre, tip = (30, 20), (20, 20)                                      # the tip on the left edge
    full = rn.result(bgr, obst, hull, centre, tip)
    assert full[20, 20].tolist() == HEAD                                  # obstacle, outline, line and head
    assert rn.result(bgr, obst, hull, centre, None)[20, 20].tolist() == RED
    assert full[20, 28].tolist() == LINE                                  # beyond the head (8 > 7), on the line
    assert full[20, 27].tolist() == HEAD
    no_hull_edge = rn.result(bgr, obst, [(60, 35)], centre, tip)
    assert no_hull_edge[20, 28].tolist() == LINE and no_hull_edge[20, 20].tolist() == HEAD
    b, g, r = (int(v) for v in bgr[5, 5])
    assert full[5, 5].tolist() == [(6 * b + 5) // 10, 102 + (6 * g + 5) // 10, 102 + (6 * r + 5) // 10]
    assert rn.result(bgr, np.zeros(shape, np.uint8), hull, centre, tip)[5, 5].tolist() == \
        [(6 * b + 5) // 10, (6 * g + 5) // 10, (6 * r + 5) // 10]


def test_clipping_at_all_four_borders():
    shape = (40, 70)
    bgr = _bgr(shape, 1)
    obst = np.zeros(shape, np.uint8)
    hull = [(0, 0), (0, 39), (69, 39), (69, 0)]                            # the frame itself
    got = rn.result(bgr, obst, hull, (35, 20), (69, 39))
    m = np.zeros(shape, bool)
    m[:3] = m[-3:] = True
    m[:, :3] = m[:, -3:] = True
    red = (got == np.array(RED, np.uint8)).all(-1)
    headm = (got == np.array(HEAD, np.uint8)).all(-1)
    assert np.array_equal(red | headm, m | headm)
    assert headm.sum() == sum(1 for dx in range(-7, 1) for dy in range(-7, 1) if dx * dx + dy * dy <= 49)
    for tip in ((-3, 20), (72, 20), (35, -3), (35, 42)):                   # heads over each border
        g = rn.result(bgr, obst, [(35, 20)], (35, 20), tip)
        h = (g == np.array(HEAD, np.uint8)).all(-1)
        want = sum(1 for dx in range(-7, 8) for dy in range(-7, 8) if dx * dx + dy * dy <= 49
                   and 0 <= tip[0] + dx < 70 and 0 <= tip[1] + dy < 40)
        assert h.sum() == want and want > 0, tip
    # vertices outside the image: only the visible part of the outline
    g = rn.result(bgr, obst, [(-20, -10), (-20, 60), (35, 20)], None, None)
    red = (g == np.array(RED, np.uint8)).all(-1)
    assert red[20, 35] and red[1, 0] and red.sum() > 40 and not red[10:30, :8].any()   # the left edge is outside


TIPS = {"far": (-10 ** 6, 10 ** 6), "int32 max": (2 ** 31 - 1, 2 ** 31 - 1), "2^31": (2 ** 31, 5),
        "-2^31 y": (5, -2 ** 31), "inside": (50, 9)}


@pytest.mark.parametrize("name", list(TIPS))
def test_glyph_drawn_or_not(name):
    shape = (40, 70)
    bgr = _bgr(shape, 2)
    obst = hn.cases(*shape)["two_blobs"]
    hull = [(5, 5), (5, 35), (60, 35), (60, 5)]
    centre, tip = (32, 20), TIPS[name]
    got = rn.result(bgr, obst, hull, centre, tip)
    outline_only = rn.result(bgr, obst, hull, centre, None)
    line = (got == np.array(LINE, np.uint8)).all(-1) & ~(outline_only == np.array(LINE, np.uint8)).all(-1)
    if name in ("2^31", "-2^31 y"):
        assert np.array_equal(got, outline_only)
        assert not rn.glyph_drawn(3, tip)
    else:
        assert rn.glyph_drawn(3, tip)
        assert line[20, 32] and line.sum() >= 20, name                    # from the centre to the border
        if name == "far":
            assert line[39, 13] or line[39, 12] or line[39, 14]            # slope -1 down to the last row
        if name == "int32 max":
            assert line[39, 51] and line[19, 32] and not line[:19].any()   # slope 1 down from the centre's cap
    assert np.array_equal(rn.result(bgr, obst, hull, centre, tip, valid=1), outline_only)   # valid = 1
    assert np.array_equal(rn.result(bgr, obst, np.zeros((0, 1, 2), np.int32), centre, tip), bgr)   # n = 0


# ---- the kernel's method, restated ---------------------------------------------------------------------------
def _near(ax, ay, bx, by, px, py, kn, kd):
    dx, dy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    t, L = wx * dx + wy * dy, dx * dx + dy * dy
    if t <= 0:
        return kn * (wx * wx + wy * wy) <= kd
    if t >= L:
        return kn * ((px - bx) ** 2 + (py - by) ** 2) <= kd
    cr = dx * wy - dy * wx
    return kn * cr * cr <= kd * L


def _row_interval(a, b, y, W, kn, kd, reach):
    """kernels/result.hip row_interval: a seed pixel that satisfies the predicate, a bisection on each side."""
    (ax, ay), (bx, by) = a, b
    ymin, ymax = min(ay, by), max(ay, by)
    if y < ymin - reach or y > ymax + reach:
        return None
    if y <= ymin:
        x0 = ax if ay <= by else bx
    elif y >= ymax:
        x0 = bx if ay <= by else ax
    else:
        num, den = (bx - ax) * (y - ay), by - ay
        if den < 0:
            num, den = -num, -den
        x0 = ax + (2 * num + den) // (2 * den)
    A, B = max(0, min(ax, bx) - reach - 1), min(W - 1, max(ax, bx) + reach + 1)
    if A > B:
        return None
    xs = min(max(x0, A), B)
    pred = lambda x: _near(ax, ay, bx, by, x, y, kn, kd)   # noqa: E731
    if xs == x0:
        assert pred(xs), (a, b, y)                         # the seed's guarantee
    elif not pred(xs):
        return None
    lo, h = A, xs
    while lo < h:
        m = (lo + h) >> 1
        if pred(m):
            h = m
        else:
            lo = m + 1
    l2, hi = xs, B
    while l2 < hi:
        m = (l2 + hi + 1) >> 1
        if pred(m):
            l2 = m
        else:
            hi = m - 1
    return lo, l2


def _touches(lo, hi, r):
    return r is not None and lo <= r[1] + 1 and hi >= r[0] - 1


def _plan_outline(verts, y, W):
    n = len(verts)
    r0 = r1 = None
    for e in range(n if n >= 3 else 1):
        iv = _row_interval(verts[e], verts[e + 1 if e + 1 < n else 0], y, W, 4, 25, 2)
        if iv is None:
            continue
        lo, hi = iv
        if r0 is None:
            r0 = (lo, hi)
        elif _touches(lo, hi, r0):
            r0 = (min(r0[0], lo), max(r0[1], hi))
        elif _touches(lo, hi, r1):
            r1 = (min(r1[0], lo), max(r1[1], hi))
        elif r1 is None:
            r1 = (lo, hi)
        else:
            raise AssertionError(("a third run", verts, y))
        if r1 is not None and _touches(r0[0], r0[1], r1):
            r0, r1 = (min(r0[0], r1[0]), max(r0[1], r1[1])), None
    return [r for r in (r0, r1) if r is not None]


def method_result(bgr, obst, hull, centre, tip, valid):
    verts = [(int(x), int(y)) for x, y in np.asarray(hull).reshape(-1, 2).tolist()]
    if not verts:
        return bgr.copy()
    H, W = bgr.shape[:2]
    out = rn.blend(bgr, obst)
    drawn = bool(valid & 2) and abs(tip[0]) <= 2 ** 31 - 1 and abs(tip[1]) <= 2 ** 31 - 1
    for y in range(H):
        for lo, hi in _plan_outline(verts, y, W):
            out[y, lo:hi + 1] = rn.OUTLINE_BGR
        if drawn:
            iv = _row_interval(centre, tip, y, W, 1, 1, 1)
            if iv:
                out[y, iv[0]:iv[1] + 1] = rn.LINE_BGR
            dy = y - tip[1]
            if abs(dy) <= 7:
                hw = 0
                while (hw + 1) ** 2 + dy * dy <= 49:
                    hw += 1
                a, b = max(tip[0] - hw, 0), min(tip[0] + hw, W - 1)
                if a <= b:
                    out[y, a:b + 1] = rn.HEAD_BGR
    return out


@pytest.mark.parametrize("shape", [(40, 70), (64, 96)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_method_on_the_hull_cases(shape):
    bgr = _bgr(shape, 3)
    rng = np.random.default_rng(shape[1])
    disp = rng.integers(1, 256, shape).astype(np.uint8)
    sizes = set()
    for name, img in hn.cases(*shape).items():
        r = hn.obstacles(img, disp, ABC)
        want = rn.result(bgr, r["obstacles"], r["hull"], r["centre"], r["tip"], r["valid"])
        got = method_result(bgr, r["obstacles"], r["hull"], r["centre"], r["tip"], r["valid"])
        assert np.array_equal(got, want), name
        sizes.add(len(r["hull"]))
        for tip in TIPS.values():
            if r["centre"] is not None:
                assert np.array_equal(method_result(bgr, r["obstacles"], r["hull"], r["centre"], tip, 3),
                                      rn.result(bgr, r["obstacles"], r["hull"], r["centre"], tip, 3)), (name, tip)
    assert {0, 1, 2, 3, 4, 8} <= sizes


def test_method_on_random_hulls():
    """Random convex rings, vertices outside the image included, started at any vertex in either orientation;
    random centres and tips, steep, shallow and far."""
    rng = np.random.default_rng(77)
    shape = (48, 80)
    bgr = _bgr(shape, 4)
    obst = (rng.random(shape) < 0.3).astype(np.uint8) * 255
    for it in range(60):
        n = int(rng.integers(1, 12))
        span = 30 if it % 3 else 8
        pts = np.stack([rng.integers(-span, shape[1] + span, n), rng.integers(-span, shape[0] + span, n)], 1)
        ring = hn.hull_of_points(pts.tolist())
        k = int(rng.integers(0, len(ring)))
        ring = ring[k:] + ring[:k]
        if it % 2:
            ring = ring[::-1]
        centre = (int(rng.integers(0, shape[1])), int(rng.integers(0, shape[0])))
        scale = (20, 300, 10 ** 5, 2 ** 31 - 1)[it % 4]
        tip = (int(rng.integers(-scale, scale + 1)), int(rng.integers(-scale, scale + 1)))
        want = rn.result(bgr, obst, ring, centre, tip, 3)
        got = method_result(bgr, obst, ring, centre, tip, 3)
        bad = np.argwhere((got != want).any(-1))
        assert len(bad) == 0, (it, ring, centre, tip, bad[:5].tolist())
