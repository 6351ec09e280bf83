"""CPU checks of tests/hull_numpy.py, the oracle of the obstacle stage (stereovision.py:170-189,
functions.py:396-421): closed-form cases, scipy.spatial.ConvexHull on points in general position, the properties
the kernel's method rests on (the hull of the row extremes is the hull of all pixels; per-row integer spans fill the
closed hull; the farthest-point basis exchange ends on the brute-force circle), the glyph against fixtures made by
the reference's own getNormalVectorLine. (The host code that sizes the buffers has a stand-alone sanitizer program
of its own, tools/hull_host_check.cpp, run by hand on the development machine; no test runs it.)"""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import hull_numpy as hn
from conftest import GOLDEN


def _img(H, W, pts):
    a = np.zeros((H, W), np.uint8)
    for x, y in pts:
        a[y, x] = 255
    return a


# ---- closed-form cases ------------------------------------------------------------------------------------------
def test_empty_one_pixel_and_collinear():
    assert hn.hull(np.zeros((9, 12), np.uint8)).shape == (0, 2)
    r = hn.obstacles(np.zeros((9, 12), np.uint8))
    assert r["centre"] is None and r["valid"] == 0 and not r["hull_mask"].any() and r["hull"].shape == (0, 1, 2)
    r = hn.obstacles(_img(9, 12, [(7, 3)]))
    assert r["hull"].tolist() == [[[7, 3]]] and r["centre"] == (7, 3) and r["valid"] == 1
    assert np.argwhere(r["hull_mask"]).tolist() == [[3, 7]] and not r["obstacles"].any()
    # a row, a column, a diagonal of slope 2 / 3: the two ends, start at the smallest (y, x)
    assert hn.hull(_img(9, 12, [(2, 4), (5, 4), (9, 4)])).tolist() == [[2, 4], [9, 4]]
    assert hn.hull(_img(9, 12, [(3, 1), (3, 2), (3, 8)])).tolist() == [[3, 1], [3, 8]]
    diag = _img(9, 12, [(1, 1), (4, 3), (10, 7)])
    r = hn.obstacles(diag)
    assert r["hull"].reshape(-1, 2).tolist() == [[1, 1], [10, 7]]
    # the segment's lattice points: every (3, 2) step, whether set or not
    assert np.argwhere(r["hull_mask"]).tolist() == [[1, 1], [3, 4], [5, 7], [7, 10]]
    assert np.argwhere(r["obstacles"]).tolist() == [[5, 7]]
    assert r["centre"] == (5, 4)          # (11 / 2, 4) truncated
    # an anti-diagonal: the start is still the smallest y
    assert hn.hull(_img(9, 12, [(10, 1), (1, 7)])).tolist() == [[10, 1], [1, 7]]


def test_order_and_strict_vertices():
    # a square with points on its sides: four vertices, from the top-left down the left side
    sq = _img(12, 12, [(2, 2), (5, 2), (9, 2), (2, 6), (9, 5), (2, 9), (6, 9), (9, 9), (5, 5)])
    assert hn.hull(sq).tolist() == [[2, 2], [2, 9], [9, 9], [9, 2]]
    # a top row of one pixel: the start is the apex, then the left side
    tri = _img(12, 12, [(6, 1), (1, 8), (10, 10)])
    assert hn.hull(tri).tolist() == [[6, 1], [1, 8], [10, 10]]
    # the filled right triangle of the GPU cases: legs and hypotenuse carry lattice points, three vertices
    t = hn.cases(40, 70)["triangle"]
    assert hn.hull(t).tolist() == [[4, 3], [4, 35], [52, 3]]
    assert np.array_equal(hn.hull_mask(t.shape, hn.hull(t)), t)


def test_hull_mask_closed_and_integer():
    # the triangle (0,0), (0,3), (4,0): row y holds x <= floor(4 - 4 y / 3)
    v = [(0, 0), (0, 3), (4, 0)]
    m = hn.hull_mask((5, 6), v)
    assert [int(r.sum()) // 255 for r in m] == [5, 3, 2, 1, 0]
    # negative slopes on the left: (4,0), (0,3), (4,3): row y starts at ceil(4 - 4 y / 3)
    m = hn.hull_mask((5, 6), [(4, 0), (0, 3), (4, 3)])
    assert [np.flatnonzero(r).tolist() for r in m] == [[4], [3, 4], [2, 3, 4], [0, 1, 2, 3, 4], []]
    # either orientation of the ring gives the same mask
    assert np.array_equal(m, hn.hull_mask((5, 6), [(4, 0), (4, 3), (0, 3)]))


def test_circle_closed_forms():
    assert hn.min_circle([(3, 4)]) == ((3, 4), 0)
    assert hn.min_circle([(0, 0), (3, 0)]) == ((Fraction(3, 2), 0), Fraction(9, 4))
    assert hn.centre([(0, 0), (3, 0)]) == (1, 0) and hn.centre([(0, 0), (-3, -5)]) == (-1, -2)   # toward zero
    # a rectangle: cocircular vertices, the centre is the crossing of the diagonals whatever the support
    assert hn.min_circle([(1, 1), (1, 6), (10, 6), (10, 1)]) == ((Fraction(11, 2), Fraction(7, 2)), Fraction(106, 4))
    # an obtuse triangle: the longest side is a diameter; an acute one: the circumcircle
    assert hn.min_circle([(0, 0), (10, 0), (5, 1)])[0] == (5, 0)
    c, r2 = hn.min_circle([(0, 0), (8, 0), (4, 7)])
    assert c == (4, Fraction(33, 14)) and r2 == 16 + Fraction(33, 14) ** 2
    # a point inside changes nothing; duplicates neither
    assert hn.min_circle([(0, 0), (8, 0), (4, 7), (4, 3), (4, 3)]) == (c, r2)
    with np.errstate(all="ignore"):
        assert hn.obstacles(hn.cases(40, 70)["rectangle"])["centre"] == (31, 16)   # (14 + 48) / 2, (10 + 22) / 2


# ---- scipy cross-check ------------------------------------------------------------------------------------------
def test_hull_vertex_set_against_scipy():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(5)
    done = 0
    for trial in range(60):
        n = int(rng.integers(5, 60))
        pts = np.unique(np.stack([rng.integers(0, 997, n), rng.integers(0, 541, n)], 1), axis=0)
        ours = hn.hull_of_points(pts.tolist())
        # general position: no point of the set on a hull edge's line besides its ends (else qhull's vertex set
        # depends on its tolerance); checked exactly
        ring = np.array(ours, np.int64)
        a, b = ring, np.roll(ring, -1, axis=0)
        cr = (b[:, None, 0] - a[:, None, 0]) * (pts[None, :, 1] - a[:, None, 1]) - \
             (b[:, None, 1] - a[:, None, 1]) * (pts[None, :, 0] - a[:, None, 0])
        if ((cr == 0).sum(axis=1) > 2).any():
            continue
        sp = spatial.ConvexHull(pts.astype(np.float64))
        assert {tuple(p) for p in pts[sp.vertices].tolist()} == set(ours), trial
        done += 1
    assert done >= 40, done


# ---- the kernel's method, restated: what kernels/hull.hip computes instead of the oracle's brute force ---------
def _floor_div(n, d):
    q = abs(n) // d            # C's truncating division, then the correction the kernel applies
    q = -q if n < 0 else q
    return q - 1 if n - q * d < 0 else q


def _rows_method(img):
    """Row extremes -> two monotone chains -> vertices in the ABI's order, and the per-row integer spans."""
    H, W = img.shape
    L, R = [-1] * H, [-1] * H
    for y in range(H):
        xs = np.flatnonzero(img[y])
        if len(xs):
            L[y], R[y] = int(xs[0]), int(xs[-1])
    rows = [y for y in range(H) if L[y] >= 0]
    if not rows:
        return [], np.zeros((H, W), np.uint8)

    def chain(X, left):
        S = []
        for y in rows:
            x = X[y]
            while len(S) >= 2:
                (ax, ay), (bx, by) = S[-2], S[-1]
                cr = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
                if (cr < 0) if left else (cr > 0):
                    break
                S.pop()
            S.append((x, y))
        return S
    SL, SR = chain(L, True), chain(R, False)
    rhi = len(SR) - 1 - (1 if SR[-1] == SL[-1] else 0)
    rlo = 1 if SR[0] == SL[0] else 0
    verts = SL + [SR[i] for i in range(rhi, rlo - 1, -1)]

    def cross(S, y, left):
        i = max(k for k in range(len(S)) if S[k][1] <= y)
        if i == len(S) - 1:
            if len(S) == 1:
                return S[0][0]
            i -= 1
        (ax, ay), (bx, by) = S[i], S[i + 1]
        num, den = (bx - ax) * (y - ay), by - ay
        return ax + (-_floor_div(-num, den) if left else _floor_div(num, den))
    mask = np.zeros((H, W), np.uint8)
    for y in range(rows[0], rows[-1] + 1):
        lo, hi = cross(SL, y, True), cross(SR, y, False)
        if lo <= hi:
            mask[y, lo:hi + 1] = 255
    return verts, mask


def _exchange_circle(pts):
    """The kernel's circle: basis exchange with the farthest outside point, candidates through the new point."""
    def c2(a, b):
        return hn._circle2(a, b)

    def c3(a, b, c):
        bx, by, cx, cy = b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1]
        if bx * cx + by * cy < 0 or bx * (bx - cx) + by * (by - cy) < 0 or cx * (cx - bx) + cy * (cy - by) < 0:
            return None
        return hn._circle3(a, b, c)

    def holds(circ, q):
        return (q[0] - circ[0][0]) ** 2 + (q[1] - circ[0][1]) ** 2 <= circ[1]
    basis = [pts[0]]
    circ = ((Fraction(pts[0][0]), Fraction(pts[0][1])), Fraction(0))
    for it in range(4 * len(pts) + 64):
        d = [(q[0] - circ[0][0]) ** 2 + (q[1] - circ[0][1]) ** 2 for q in pts]
        far = max(range(len(pts)), key=lambda i: (d[i], -i))
        if d[far] <= circ[1]:
            return circ, it
        p = pts[far]
        cands = [((b,), c2(p, b)) for b in basis]
        cands += [((basis[i], basis[j]), c3(p, basis[i], basis[j]))
                  for i in range(len(basis)) for j in range(i + 1, len(basis))]
        for keep, c in cands:
            if c is not None and all(holds(c, b) for b in basis):
                basis, circ = list(keep) + [p], c
                break
        else:
            raise AssertionError("no circle through the new point holds the basis")
    raise AssertionError("the exchange did not end")


SHAPES = [(40, 70), (64, 96)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_extremes_spans_and_exchange_give_the_oracle(shape):
    H, W = shape
    for name, img in hn.cases(H, W).items():
        ref = hn.obstacles(img)
        verts, mask = _rows_method(img)
        assert verts == [tuple(v) for v in ref["hull"].reshape(-1, 2).tolist()], name
        assert np.array_equal(mask, ref["hull_mask"]), name
        assert np.array_equal(ref["obstacles"], ref["hull_mask"] & ~img), name
        if verts:
            circ, _ = _exchange_circle(verts)
            assert circ == hn.min_circle(verts), name
        assert len(verts) <= 2 * H


def test_random_blobs_rows_method_and_exchange():
    rng = np.random.default_rng(11)
    most = 0
    for trial in range(25):
        H, W = int(rng.integers(8, 60)), int(rng.integers(8, 90))
        img = (rng.random((H, W)) < rng.choice([0.003, 0.02, 0.3])).astype(np.uint8) * 255
        if trial % 3 == 0:   # a disc: many vertices, many near-cocircular
            yy, xx = np.mgrid[0:H, 0:W]
            img = (((xx - W // 2) ** 2 + (yy - H // 2) ** 2) <= (min(H, W) // 2 - 1) ** 2).astype(np.uint8) * 255
        ref = hn.obstacles(img)
        verts, mask = _rows_method(img)
        assert verts == [tuple(v) for v in ref["hull"].reshape(-1, 2).tolist()], trial
        assert np.array_equal(mask, ref["hull_mask"]), trial
        if verts:
            circ, its = _exchange_circle(verts)
            assert circ == hn.min_circle(verts), trial
            most = max(most, its)
            assert abs(circ[0][0].denominator) < 2 ** 26 and abs(circ[0][1].denominator) < 2 ** 26
    assert most <= 12, most     # a handful of exchanges, far from the kernel's bound of 4 n + 64


def test_exchange_on_arbitrary_points():
    """getCenterPoint takes any points: collinear triples, duplicates, negative coordinates."""
    rng = np.random.default_rng(3)
    for trial in range(40):
        n = int(rng.integers(1, 14))
        pts = [(int(x), int(y)) for x, y in rng.integers(-9, 10, (n, 2))]
        circ, _ = _exchange_circle(pts)
        assert circ == hn.min_circle(pts), pts


# ---- the glyph tip against the reference's own function --------------------------------------------------------
@pytest.fixture(scope="module")
def glyph_golden():
    with open(os.path.join(GOLDEN, "hull_glyph.json")) as fh:
        return json.load(fh)


def test_glyph_against_reference_fixtures(glyph_golden):
    g = glyph_golden
    assert tuple(g["camera"]) == hn.CAMERA and len(g["cases"]) >= 36
    H, W = g["shape"]
    raised = 0
    for c in g["cases"]:
        disp = np.zeros((H, W), np.uint8)
        cx, cy = c["centre"]
        disp[cy, cx] = c["d"]
        if c["tip"] == "raises":
            raised += 1
            with pytest.raises((ValueError, OverflowError, ZeroDivisionError)):
                hn.glyph((cx, cy), np.array(c["abc"]), disp)
            assert hn.tip((cx, cy), c["abc"], disp) is None
        else:
            assert list(hn.glyph((cx, cy), np.array(c["abc"]), disp)) == c["tip"], c
            assert list(hn.tip((cx, cy), c["abc"], disp)) == c["tip"]
    assert raised >= 3 and any(c["d"] == 0 for c in g["cases"])
