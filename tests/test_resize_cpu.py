"""CPU: the general-scale resize's host side. sv_resize_coefficients (csrc/svx_resize_host.h) against
tile_numpy._coefficients on every field; the oracle of batchImages for any list (tests/resize_numpy.py) against
tile_numpy's literal tile and its closed form; the oracle's resize at the identity and on constant pictures; the
drop-in's RESIZE group. No device is touched."""
import types

import numpy as np
import pytest

import resize_numpy as rn
import tile_numpy as tn

E_ARG = -1
PAIRS = [(1024, 889), (544, 390), (889, 1024), (390, 544), (4095, 4096), (4096, 8192), (8192, 1)]


def _coefficients(dn, sn):
    from svx import _abi
    s0, s1 = np.full(dn, -7, np.int32), np.full(dn, -7, np.int32)
    c0, c1 = np.full(dn, -7, np.int16), np.full(dn, -7, np.int16)
    rc = _abi.lib().sv_resize_coefficients(dn, sn, _abi.ptr(s0), _abi.ptr(s1), _abi.ptr(c0), _abi.ptr(c1))
    return rc, s0, s1, c0, c1


def test_coefficients_equal_the_oracle():
    """Every pair of dn, sn in 1..40 and the shapes of the cropped mode, the limits and an 8192-fold stretch: the
    source index, the clamped next one and both int16 coefficients (c0 computed, not 2048 - c1)."""
    pairs = [(dn, sn) for dn in range(1, 41) for sn in range(1, 41)] + PAIRS
    for dn, sn in pairs:
        rc, s0, s1, c0, c1 = _coefficients(dn, sn)
        assert rc == 0, (dn, sn)
        w0, w1, k0, k1 = tn._coefficients(dn, sn)
        for name, got, want in (("s0", s0, w0), ("s1", s1, w1), ("c0", c0, k0), ("c1", c1, k1)):
            bad = np.flatnonzero(got.astype(np.int64) != want)
            assert len(bad) == 0, (dn, sn, name, bad[:5].tolist(), got[bad[:5]].tolist(), want[bad[:5]].tolist())
        assert s0.min() >= 0 and s1.max() <= sn - 1 and c0.min() >= 0 and c1.min() >= 0


def test_coefficients_argument_errors():
    from svx import _abi
    for dn, sn in ((0, 5), (5, 0), (-1, 5), (8193, 5), (5, 8193)):
        n = max(1, min(dn, 8))
        a, b = np.zeros(n, np.int32), np.zeros(n, np.int32)
        c, d = np.zeros(n, np.int16), np.zeros(n, np.int16)
        assert _abi.lib().sv_resize_coefficients(dn, sn, _abi.ptr(a), _abi.ptr(b), _abi.ptr(c), _abi.ptr(d)) == E_ARG
    a = np.zeros(4, np.int32)
    c = np.zeros(4, np.int16)
    assert _abi.lib().sv_resize_coefficients(4, 4, None, _abi.ptr(a), _abi.ptr(c), _abi.ptr(c)) == E_ARG
    assert _abi.lib().sv_resize_coefficients(4, 4, _abi.ptr(a), _abi.ptr(a), _abi.ptr(c), None) == E_ARG


def test_images_tile_shape_is_host_arithmetic():
    """The output shapes and the excluded odd sizes (no device: the plan is host code)."""
    import ctypes

    from svx import _abi

    def shape(count, H, W):
        oh, ow = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = _abi.lib().sv_images_tile_shape(count, H, W, ctypes.byref(oh), ctypes.byref(ow))
        return rc, oh.value, ow.value
    assert shape(1, 7, 9) == (0, 7, 9) and shape(2, 8, 9) == (0, 4, 9)
    assert shape(3, 7, 9) == (0, 7, 9) and shape(4, 7, 9) == (0, 7, 9) and shape(5, 6, 10) == (0, 3, 10)
    for count, H, W in ((2, 7, 8), (5, 8, 9), (5, 7, 8), (0, 8, 8), (6, 8, 8), (1, 0, 8), (1, 8, 4097)):
        assert shape(count, H, W)[0] == E_ARG, (count, H, W)


def _pictures(shape, seed=0):
    H, W = shape
    rng = np.random.default_rng(8200 + seed + H)

    def rnd(*s):
        a = rng.integers(0, 256, s).astype(np.uint8)
        a[rng.random(s) < 0.05] = 0
        a[rng.random(s) < 0.05] = 255
        return a
    road = ((rng.random(shape) < 0.5) * 255).astype(np.uint8)
    cleaned = ((rng.random(shape) < 0.5) * 255).astype(np.uint8)
    return [rnd(H, W), tn.road_map(rnd(H, W, 3), road), road, cleaned, rnd(H, W, 3)]


@pytest.mark.parametrize("shape", [(8, 12), (40, 76)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_equals_the_tile(shape):
    imgs = _pictures(shape)
    got = rn.batch_images(imgs, shape)
    assert got.dtype == np.uint8 and got.shape == (shape[0] // 2, shape[1], 3)
    assert np.array_equal(got, tn.tile(*imgs))
    assert np.array_equal(got, tn.tile_closed(*imgs))


def test_oracle_count_1_is_the_picture_as_bgr():
    imgs = _pictures((7, 9))
    assert np.array_equal(rn.batch_images([imgs[0]], (7, 9)), np.repeat(imgs[0][:, :, None], 3, axis=2))
    assert np.array_equal(rn.batch_images([imgs[4]], (7, 9)), imgs[4])


def test_oracle_counts_2_to_4_are_the_half_size_stack():
    """Counts 2, 3, 4 at a size the stack's halves divide: the 2 x 2 means of the stack that functions.py builds."""
    imgs = _pictures((8, 12), seed=1)
    b = [tn._bgr(i) for i in imgs]

    def half(s):
        return tn.mean4(s[0::2, 0::2], s[0::2, 1::2], s[1::2, 0::2], s[1::2, 1::2])
    assert np.array_equal(rn.batch_images(imgs[:2], (8, 12)), half(np.hstack((b[0], b[1]))))
    top = np.hstack((b[0], b[1]))
    assert np.array_equal(rn.batch_images(imgs[:3], (8, 12)), half(np.vstack((top, np.hstack((b[2], b[2]))))))
    assert np.array_equal(rn.batch_images(imgs[:4], (8, 12)), half(np.vstack((top, np.hstack((b[2], b[3]))))))


def test_oracle_resize_identity_and_constant():
    rng = np.random.default_rng(5)
    for shape in ((7, 9), (7, 9, 3), (1, 1), (390, 889)):
        a = rng.integers(0, 256, shape).astype(np.uint8)
        assert np.array_equal(tn.resize_linear_u8(a, shape[1], shape[0]), a), shape
    for (sh, sw), (dh, dw) in (((390, 889), (544, 1024)), ((13, 17), (5, 4)), ((2, 3), (7, 5))):
        assert (tn.resize_linear_u8(np.full((sh, sw), 255, np.uint8), dw, dh) == 255).all(), (sh, sw, dh, dw)
        assert (rn.resize_image(np.full((sh, sw, 3), 255, np.uint8), dh, dw) == 255).all()


def test_resize_group_is_opt_in():
    """RESIZE is a group of its own: install(m) and install(m, tiles=True) leave resizeImage alone; with resize=True a
    list the device cannot take reaches the function that was replaced, and without one the drop-in raises."""
    from svx import SvxError, dropin
    calls = []

    def original_batch(img_list, size):
        calls.append(("batch", len(img_list)))
        return "original"

    def original_resize(image, height, width):
        calls.append(("resize", height, width))
        return "resized"
    m = types.SimpleNamespace(camera_focal_length_px=1.0, stereo_camera_baseline_m=2.0, image_centre_w=3.0,
                              image_centre_h=4.0, batchImages=original_batch, resizeImage=original_resize)
    assert dropin.RESIZE == ("resizeImage", "batchImages")
    assert "resizeImage" not in dropin.PATCHED + dropin.TILES + dropin.MORPHOLOGY + dropin.HULL
    for kw in ({}, {"tiles": True}):
        dropin.install(m, **kw)
        try:
            assert m.resizeImage is original_resize
            assert m.batchImages is (dropin.batchImages if kw else original_batch)
        finally:
            dropin.uninstall()
    z = np.zeros((8, 8), np.uint8)
    for kw in ({"resize": True}, {"resize": True, "tiles": True}):
        dropin.install(m, **kw)
        try:
            assert m.resizeImage is dropin.resizeImage and m.batchImages is dropin.batch_images
            calls.clear()
            assert m.batchImages([("a", z.astype(np.float32)), ("b", z.astype(np.float32))], (8, 8)) == "original"
            assert m.batchImages([("", z)] * 6, (8, 8)) == "original"
            assert m.batchImages([("", z)] * 2, (7, 8)) == "original"            # H odd for two pictures
            assert m.batchImages([("", z)] * 5, (8, 9)) == "original"            # W odd for five
            assert m.batchImages([("", z)], (8, 5000)) == "original"             # beyond the limits
            assert m.resizeImage(z.astype(np.float32), 4, 6) == "resized"
            assert calls == [("batch", 2), ("batch", 6), ("batch", 2), ("batch", 5), ("batch", 1), ("resize", 4, 6)]
        finally:
            dropin.uninstall()
        assert m.batchImages is original_batch and m.resizeImage is original_resize
    with pytest.raises(SvxError):
        dropin.batch_images([("", z)] * 6, (8, 8))
    with pytest.raises(SvxError):
        dropin.batch_images([("", z.astype(np.float32))], (8, 8))
    with pytest.raises(SvxError):
        dropin.resizeImage(z.astype(np.float32), 4, 6)
