"""CPU: the image tile's oracle (tests/tile_numpy.py). batchImages restated literally over OpenCV's 8-bit bilinear
resize equals the closed form the device computes (include/svx.h, sv_image_tile), plus hand-written cases and the
opt-in group of the drop-in."""
import types

import numpy as np
import pytest

import tile_numpy as tn

SHAPES = [(4, 4), (8, 12), (40, 76), (64, 96), (544, 1024)]


def pictures(shape, seed=0):
    """Five random pictures with the values 0 and 255 in them: disparity, BGR, road, cleaned (0 / 255), result."""
    H, W = shape
    rng = np.random.default_rng(7100 + seed + H)

    def rnd(*s):
        a = rng.integers(0, 256, s).astype(np.uint8)
        a[rng.random(s) < 0.05] = 0
        a[rng.random(s) < 0.05] = 255
        return a
    road = ((rng.random(shape) < 0.5) * 255).astype(np.uint8)
    cleaned = ((rng.random(shape) < 0.5) * 255).astype(np.uint8)
    return rnd(H, W), rnd(H, W, 3), road, cleaned, rnd(H, W, 3)


def five(shape, seed=0):
    disp, bgr, road, cleaned, result = pictures(shape, seed)
    return [disp, tn.road_map(bgr, road), road, cleaned, result]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_literal_equals_closed_form(shape):
    imgs = five(shape)
    got = tn.tile(*imgs)
    assert got.shape == (shape[0] // 2, shape[1], 3) and got.dtype == np.uint8
    assert np.array_equal(got, tn.tile_closed(*imgs))


def test_general_resize_at_scale_2_is_the_area_mean():
    """OpenCV turns INTER_LINEAR at scale 2 into the 2 x 2 area mean; its general path gives the same bytes."""
    rng = np.random.default_rng(3)
    for shape in ((2, 2), (10, 14), (6, 250, 3), (64, 96, 3)):
        a = rng.integers(0, 256, shape).astype(np.uint8)
        a[rng.random(shape) < 0.1] = 255
        want = tn.mean4(a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2])
        assert np.array_equal(tn.resize_linear_u8(a, shape[1] // 2, shape[0] // 2), want), shape
    # the same size is a copy, and a scale that is no power of two interpolates and clamps at the border
    assert np.array_equal(tn.resize_linear_u8(a, 96, 64), a)
    ramp = np.array([[0, 100, 200]], np.uint8)
    assert tn.resize_linear_u8(ramp, 6, 1).tolist() == [[0, 25, 75, 125, 175, 200]]


def test_five_values_of_a_binary_quadrant():
    """A 0 / 255 picture's quadrant pixel is one of {0, 64, 128, 191, 255}, by the count of its four samples."""
    want = {0: 0, 1: 64, 2: 128, 3: 191, 4: 255}
    z = np.zeros((4, 4), np.uint8)
    z3 = np.zeros((4, 4, 3), np.uint8)
    seen = set()
    for pattern in range(16):
        road = np.zeros((4, 4), np.uint8)
        road[0, :] = road[3, :] = road[:, 0] = road[:, 3] = 255 * (pattern & 1)     # unsampled pixels: ignored
        for k, (y, x) in enumerate(((1, 1), (1, 2), (2, 1), (2, 2))):
            road[y, x] = 255 if (pattern >> k) & 1 else 0
        for fn in (tn.tile, tn.tile_closed):
            t = fn(z, z3, road, road.T.copy(), z3)
            v = int(t[1, 0, 0])
            assert v == want[bin(pattern).count("1")] and (t[1, 0] == v).all(), (pattern, v)
            assert int(t[1, 1, 0]) == v                # the cleaned quadrant: the transposed pattern has the same count
            seen.add(v)
    assert seen == set(want.values())


def test_each_quadrant_depends_on_its_own_picture():
    shape = (40, 76)
    H, W = shape
    base = five(shape)
    ref = tn.tile_closed(*base)
    regions = [(slice(0, H // 4), slice(0, W // 4)), (slice(0, H // 4), slice(W // 4, W // 2)),
               (slice(H // 4, H // 2), slice(0, W // 4)), (slice(H // 4, H // 2), slice(W // 4, W // 2)),
               (slice(0, H // 2), slice(W // 2, W))]
    for k in range(5):
        imgs = [a.copy() for a in base]
        imgs[k] = (255 - imgs[k]).astype(np.uint8)
        for fn in (tn.tile, tn.tile_closed):
            got = fn(*imgs)
            changed = (got != ref).any(-1)
            inside = np.zeros_like(changed)
            inside[regions[k]] = True
            assert changed.any() and not (changed & ~inside).any(), k


def test_hand_written_4x4():
    disp = (np.arange(16, dtype=np.uint8) * 10).reshape(4, 4)      # rows 1, 2 x columns 1, 2: 50 60 90 100
    bgr = np.empty((4, 4, 3), np.uint8)
    bgr[:] = (10, 20, 30)
    road = np.zeros((4, 4), np.uint8)
    road[1, 1] = 255                                                # one of the four samples
    road[0, 0] = road[3, 3] = 255                                   # not sampled
    cleaned = np.zeros((4, 4), np.uint8)
    cleaned[1, 1] = cleaned[1, 2] = cleaned[2, 1] = 255             # three of them
    y, x, c = np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij")
    result = (16 * y + 4 * x + c).astype(np.uint8)
    want = np.array([[[75, 75, 75], [8, 79, 23], [10, 11, 12], [18, 19, 20]],
                     [[64, 64, 64], [191, 191, 191], [42, 43, 44], [50, 51, 52]]], np.uint8)
    rmap = tn.road_map(bgr, road)
    assert rmap[1, 1].tolist() == [0, 255, 0] and rmap[0, 0].tolist() == [0, 255, 0] and rmap[1, 2].tolist() == [10, 20, 30]
    for fn in (tn.tile, tn.tile_closed):
        assert np.array_equal(fn(disp, rmap, road, cleaned, result), want), fn.__name__


def test_hand_written_8x8_rounds_halves_up():
    """Sums whose remainder mod 4 is 2 round up (an implementation rounding ties to even would give 0, 2 and 254)."""
    disp = np.full((8, 8), 99, np.uint8)                            # 99: never sampled
    disp[1:3, 1:3] = [[1, 1], [0, 0]]                               # 2 / 4 -> 1
    disp[1:3, 5:7] = [[1, 2], [3, 4]]                               # 10 / 4 -> 3
    disp[5:7, 1:3] = [[255, 255], [255, 254]]                       # 1019 / 4 -> 255
    disp[5:7, 5:7] = [[0, 0], [0, 1]]                               # 1 / 4 -> 0
    bgr = np.zeros((8, 8, 3), np.uint8)
    bgr[1:3, 1:3] = [[[4, 5, 6], [0, 0, 0]], [[0, 0, 0], [6, 5, 4]]]   # (10, 10, 10) / 4 -> 3
    road = np.zeros((8, 8), np.uint8)
    road[5, 5:7] = 255                                              # map: two samples green -> (0, 128, 0); road: 128
    cleaned = np.full((8, 8), 255, np.uint8)
    cleaned[2, 6] = 0                                               # 191 at (0, 1) of its quadrant
    result = np.zeros((8, 8, 3), np.uint8)
    result[0:2, 0:2, 0] = [[253, 255], [255, 255]]                  # 1018 / 4 -> 255 (254.5 rounds up)
    result[6:8, 6:8, 2] = [[1, 0], [0, 1]]                          # 2 / 4 -> 1
    want = np.zeros((4, 8, 3), np.uint8)
    want[0, 0], want[0, 1], want[1, 0], want[1, 1] = 1, 3, 255, 0   # the disparity's quadrant
    want[0, 2] = 3                                                  # the map's
    want[1, 3] = (0, 128, 0)
    want[3, 1] = 128                                                # the road's
    want[2:4, 2:4] = 255                                            # the cleaned one's
    want[2, 3] = 191
    want[0, 4, 0] = 255                                             # the result's
    want[3, 7, 2] = 1
    rmap = tn.road_map(bgr, road)
    for fn in (tn.tile, tn.tile_closed):
        assert np.array_equal(fn(disp, rmap, road, cleaned, result), want), fn.__name__


def test_default_install_leaves_batch_images_alone():
    """batchImages is an opt-in group of its own (TILES, install(.., tiles=True)); a list the device does not take
    reaches the function install() replaced, and without one the drop-in raises SvxError (no device is touched)."""
    from svx import SvxError, dropin
    calls = []

    def original(img_list, size):
        calls.append((len(img_list), tuple(size)))
        return "original"
    m = types.SimpleNamespace(camera_focal_length_px=1.0, stereo_camera_baseline_m=2.0, image_centre_w=3.0,
                              image_centre_h=4.0, batchImages=original)
    assert dropin.TILES == ("batchImages",) and "batchImages" not in dropin.PATCHED
    dropin.install(m)
    try:
        assert m.batchImages is original
    finally:
        dropin.uninstall()
    dropin.install(m, tiles=True)
    try:
        assert m.batchImages is dropin.batchImages
        z, z3 = np.zeros((8, 8), np.uint8), np.zeros((8, 8, 3), np.uint8)
        four = [("a", z), ("b", z3), ("c", z), ("d", z)]
        assert m.batchImages(four, (8, 8)) == "original"
        odd = np.zeros((6, 8), np.uint8), np.zeros((6, 8, 3), np.uint8)       # H no multiple of 4
        assert m.batchImages([("", odd[0]), ("", odd[1]), ("", odd[0]), ("", odd[0]), ("", odd[1])], (6, 8)) == "original"
        assert m.batchImages([("", z), ("", z3), ("", z), ("", z), ("", z3)], (4, 4)) == "original"   # not of `size`
        unpainted = np.full((8, 8), 255, np.uint8)                              # the second image is no map of the third
        assert m.batchImages([("", z), ("", z3), ("", unpainted), ("", z), ("", z3)], (8, 8)) == "original"
        assert calls == [(4, (8, 8)), (5, (6, 8)), (5, (4, 4)), (5, (8, 8))]
    finally:
        dropin.uninstall()
    assert m.batchImages is original
    with pytest.raises(SvxError):
        dropin.batchImages(four, (8, 8))
