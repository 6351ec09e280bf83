"""CPU checks of tests/morph_numpy.py, the oracle of the road clean-up (sanitiseRoadImage's morphology,
functions.py:346-358): closed-form cases worked out by hand, scipy.ndimage where it is installed, and the
property that makes ParticleCleansing (functions.py:378-384) the identity on the result."""
import numpy as np
import pytest

import morph_numpy as mn

H, W = 40, 64


def _img(*blocks):
    a = np.zeros((H, W), np.uint8)
    for y0, y1, x0, x1 in blocks:
        a[y0:y1, x0:x1] = 255
    return a


def _box(y0, y1, x0, x1):
    return _img((y0, y1, x0, x1))


def test_all_set_stays_all_set():
    assert np.array_equal(mn.sanitise(np.full((H, W), 255, np.uint8)), np.full((H, W), 255, np.uint8))
    assert np.array_equal(mn.sanitise(np.full((H, W), 1, np.uint8)), np.full((H, W), 255, np.uint8))


def test_empty_stays_empty():
    assert not mn.sanitise(np.zeros((H, W), np.uint8)).any()


def test_one_pixel_vanishes():
    assert not mn.sanitise(_box(20, 21, 30, 31)).any()


def test_17x17_block_leaves_its_centre():
    out = mn.sanitise(_box(10, 27, 20, 37))
    assert np.array_equal(out, _box(18, 19, 28, 29))
    assert np.array_equal(mn.walk(out), [[28, 18]])


def test_16x17_block_vanishes():
    assert not mn.sanitise(_box(10, 26, 20, 37)).any()
    assert not mn.sanitise(_box(10, 27, 20, 36)).any()


def test_corner_block_keeps_the_border_side():
    """The erosion's border counts as set: a 25 x 25 block in the corner (0, 0) loses 8 pixels on its two inner
    sides only."""
    out = mn.sanitise(_box(0, 25, 0, 25))
    assert np.array_equal(out, _box(0, 17, 0, 17)) and int((out != 0).sum()) == 289


def test_bars_8_apart_are_joined():
    """Two 30 x 17 bars 8 columns apart: the first close fills the gap, so the erosion sees one 30 x 42 block."""
    out = mn.sanitise(_img((5, 35, 10, 27), (5, 35, 35, 52)))
    assert np.array_equal(out, _box(13, 27, 18, 44)) and int((out != 0).sum()) == 364


def test_bars_9_apart_stay_apart():
    """9 columns apart the close leaves the gap open: each bar erodes to its own centre column."""
    out = mn.sanitise(_img((5, 35, 10, 27), (5, 35, 36, 53)))
    ys, xs = np.nonzero(out)
    assert len(ys) == 28 and sorted(set(xs.tolist())) == [18, 44]
    assert np.array_equal(out, _img((13, 27, 18, 19), (13, 27, 44, 45)))


def test_block_near_every_edge_fills_the_image():
    """[2:38, 4:60] is within 4 pixels of every edge: the dilation reaches the border, and the erosions' border
    never clears a pixel."""
    assert np.array_equal(mn.sanitise(_box(2, 38, 4, 60)), np.full((H, W), 255, np.uint8))


def test_mask_keeps_any_non_zero_value():
    img = np.full((H, W), 255, np.uint8)
    m = np.zeros((H, W), np.uint8)
    m[:, :20] = 128
    m[:, 40:] = 255
    out = mn.sanitise(img, m)
    assert np.array_equal(out != 0, m != 0)


def test_two_erosions_equal_one_radius_8():
    rng = np.random.default_rng(3)
    a = mn.close(mn.rectangles(rng, 61, 97, 12) != 0, 4)
    assert np.array_equal(mn.erode(mn.erode(a, 4), 4), mn.erode(a, 8))


def test_walk_is_raster_order_and_respects_size():
    a = np.zeros((5, 7), np.uint8)
    a[1, 5] = a[1, 2] = a[3, 0] = a[4, 6] = 9
    assert np.array_equal(mn.walk(a), [[2, 1], [5, 1], [0, 3], [6, 4]])
    assert np.array_equal(mn.walk(a, (4, 6)), [[2, 1], [5, 1], [0, 3]])
    assert mn.walk(np.zeros((3, 3), np.uint8)).shape == (0, 2)


SHAPES = [(96, 160), (61, 889)]


def _cases():
    for h, w in SHAPES:
        for seed in range(3):
            rng = np.random.default_rng(100 * seed + h)
            yield mn.rectangles(rng, h, w, max(6, h * w // 2500)), mn.random_mask(rng, h, w)


def test_against_scipy_ndimage():
    ndi = pytest.importorskip("scipy.ndimage")
    k9, k17 = np.ones((9, 9), bool), np.ones((17, 17), bool)

    def ref(img, mask):
        b = img != 0
        b = ndi.binary_erosion(ndi.binary_dilation(b, k9, border_value=0), k9, border_value=1)
        b = ndi.binary_erosion(ndi.binary_erosion(b, k9, border_value=1), k9, border_value=1)
        assert np.array_equal(b, ndi.binary_erosion(
            ndi.binary_erosion(ndi.binary_dilation(img != 0, k9, border_value=0), k9, border_value=1), k17,
            border_value=1))
        b &= mask != 0
        b = ndi.binary_erosion(ndi.binary_dilation(b, k9, border_value=0), k9, border_value=1)
        return np.where(b, 255, 0).astype(np.uint8)

    for img, mask in _cases():
        out = mn.sanitise(img, mask)
        assert 0 < (out != 0).mean() < 1
        assert np.array_equal(out, ref(img, mask))
        assert np.array_equal(mn.sanitise(img), ref(img, np.ones_like(mask)))


def _holes(out):
    """Sizes of the 4-connected background components of `out` that do not touch the frame (flood fill)."""
    bg = out == 0
    h, w = bg.shape
    seen = np.zeros_like(bg)
    sizes = []
    for y0, x0 in zip(*np.nonzero(bg)):
        if seen[y0, x0]:
            continue
        stack, n, edge = [(y0, x0)], 0, False
        seen[y0, x0] = True
        while stack:
            y, x = stack.pop()
            n += 1
            edge |= y == 0 or x == 0 or y == h - 1 or x == w - 1
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < h and 0 <= xx < w and bg[yy, xx] and not seen[yy, xx]:
                    seen[yy, xx] = True
                    stack.append((yy, xx))
        if not edge:
            sizes.append(n)
    return sizes


def test_particle_cleansing_has_nothing_to_fill():
    """ParticleCleansing fills external contours of area < 70; it can only change enclosed background (holes). A
    hole that survives the last 9 x 9 close holds a full 9 x 9 block of zeros, so every hole has >= 81 pixels (and
    its outer contour an area above 70). Images with holes are part of the cases: a ring wide enough to survive."""
    ring = np.zeros((96, 160), np.uint8)
    ring[10:90, 20:140] = 255
    ring[40:60, 60:100] = 0
    cases = [(ring, None)] + list(_cases())
    found = 0
    for img, mask in cases:
        out = mn.sanitise(img, mask)
        sizes = _holes(out)
        found += len(sizes)
        assert all(s >= 81 for s in sizes), sizes
    assert found >= 1
