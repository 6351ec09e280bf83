"""GPU: the general-scale bilinear resize — kernels/resize.hip behind sv_resize_linear_u8, sv_images_tile
(batchImages of one to five pictures, composed on the device), the batch's resized disparity (Batch.resize_disp) and
the drop-in's RESIZE group — bit for bit against the oracles tests/tile_numpy.py (resize_linear_u8) and
tests/resize_numpy.py (batch_images), which tests/test_tile_cpu.py and tests/test_resize_cpu.py pin."""
import ctypes
import types

import numpy as np
import pytest

import resize_numpy as rn
import tile_numpy as tn

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import _abi, batch, dropin
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, abi=_abi, batch=batch, dropin=dropin)


def same(got, ref, what):
    """Equality with the first differing pixels reported."""
    assert got.dtype == np.uint8 and got.shape == ref.shape, (what, got.shape, ref.shape)
    diff = got != ref
    bad = np.argwhere(diff.any(-1) if got.ndim == 3 else diff)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())


def rnd(rng, *s):
    """Random bytes with 0 and 255 in them."""
    a = rng.integers(0, 256, s).astype(np.uint8)
    a[rng.random(s) < 0.05] = 0
    a[rng.random(s) < 0.05] = 255
    if a.size >= 2:
        a.flat[0], a.flat[-1] = 0, 255
    return a


# ---- sv_resize_linear_u8 ---------------------------------------------------------------------------------------
# (3, 4096) -> (2, 4095): the widest row of a pixel per lane; (2, 8192) -> (2, 4096): the widest source, four pixels a
# lane; 124 / 128 / 132 wide: either side of the width from which a lane takes four pixels, and a width that is no
# multiple of 4 above it. A grey source whose width is a multiple of 4 is read through 16-byte windows up to a scale
# of 3: 100 -> 128, 300 -> 132 and 8192 -> 4096 are, 384 -> 128 is the last scale that is, 388 -> 128 the first that
# is not, 102 -> 128 a source that is not aligned; the last row of each ends in lanes that gather by bytes
CASES = [((1, 1), (1, 1)), ((1, 1), (5, 7)), ((2, 3), (7, 5)), ((13, 17), (5, 4)), ((5, 7), (1, 1)), ((7, 9), (7, 9)),
         ((31, 33), (64, 64)), ((64, 64), (31, 33)), ((3, 4096), (2, 4095)), ((2, 8192), (2, 4096)),
         ((390, 889), (544, 1024)), ((544, 1024), (390, 889)), ((9, 100), (21, 124)), ((9, 100), (21, 128)),
         ((9, 100), (21, 130)), ((21, 300), (9, 132)), ((5, 384), (6, 128)), ((7, 388), (3, 128)),
         ((9, 102), (21, 128)), ((1, 4), (1, 128)), ((40, 1024), (40, 1024))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}")
def test_resize_against_the_oracle(sv, case):
    (sh, sw), (dh, dw) = case
    rng = np.random.default_rng(1000 * sh + sw + dh)
    for ch in (1, 3):
        src = rnd(rng, sh, sw) if ch == 1 else rnd(rng, sh, sw, 3)
        got = sv.dropin.resize_linear(src, (dw, dh))
        same(got, tn.resize_linear_u8(src, dw, dh), (case, ch))
        if (sh, sw) == (dh, dw):
            same(got, src, ("identity", case, ch))


def test_three_images_in_one_call(sv):
    """n = 3 different images of (13, 17) -> (20, 11), each against its own oracle (the frame strides); and at a
    width where a lane takes four pixels, from bytes (50 wide) and from windows (52 wide)."""
    rng = np.random.default_rng(77)
    for (sh, sw), (dh, dw) in (((13, 17), (20, 11)), ((6, 50), (5, 136)), ((6, 52), (9, 136))):
        for tail in ((), (3,)):
            stack = rnd(rng, 3, sh, sw, *tail)
            got = sv.dropin.resize_linear(stack, (dw, dh))
            assert got.shape == (3, dh, dw) + tail
            for k in range(3):
                same(got[k], tn.resize_linear_u8(stack[k], dw, dh), (k, tail, dw))
            assert not np.array_equal(got[0], got[1])


def test_resize_argument_errors(sv):
    abi = sv.abi
    f = abi.lib().sv_resize_linear_u8
    src = np.zeros((3, 8, 8, 3), np.uint8)
    dst = np.zeros((3, 16, 16, 3), np.uint8)
    s, d = abi.ptr(src), abi.ptr(dst)
    assert f(s, 1, 8, 8, 1, d, 5, 7) == 0 and f(s, 3, 8, 8, 3, d, 16, 16) == 0
    assert f(None, 1, 8, 8, 1, d, 5, 7) == E_ARG and f(s, 1, 8, 8, 1, None, 5, 7) == E_ARG
    assert f(s, 1, 8, 8, 1, s, 4, 4) == E_ARG                                  # dst is src
    assert f(s, 1, 8, 8, 1, ctypes.c_void_p(src.ctypes.data + 63), 4, 4) == E_ARG   # ... or its last byte
    assert f(s, 1, 8, 8, 1, ctypes.c_void_p(src.ctypes.data + 64), 4, 4) == 0
    for dh, dw in ((0, 4), (4, 0), (4097, 4), (4, 4097), (-1, 4)):
        assert f(s, 1, 8, 8, 1, d, dh, dw) == E_ARG, (dh, dw)
    for sh, sw in ((0, 8), (8, 0), (8193, 1), (1, 8193)):
        assert f(s, 1, sh, sw, 1, d, 4, 4) == E_ARG, (sh, sw)
    for ch in (0, 2, 4):
        assert f(s, 1, 8, 8, ch, d, 4, 4) == E_ARG, ch
    assert f(s, 0, 8, 8, 1, d, 4, 4) == E_ARG and f(s, -1, 8, 8, 1, d, 4, 4) == E_ARG
    with pytest.raises(TypeError):
        sv.dropin.resize_linear(np.zeros((4, 4), np.float32), (4, 4))
    with pytest.raises(sv.svx.SvxError):
        sv.dropin.resize_linear(np.zeros((4, 4), np.uint8), (4097, 4))


# ---- sv_images_tile --------------------------------------------------------------------------------------------
def _mixed(rng, count, size):
    """`count` pictures of mixed shapes, grey and BGR, one of them already of `size`."""
    H, W = size
    shapes = [(H, W), (H + 3, 2 * W + 1, 3), (max(H // 2, 1), W + 5), (2 * H + 1, max(W - 3, 1), 3), (H, W, 3)]
    return [rnd(rng, *shapes[k]) for k in range(count)]


IMAGE_LISTS = [(1, (6, 10)), (2, (6, 10)), (3, (6, 10)), (4, (6, 10)), (5, (6, 10)), (5, (40, 76)), (2, (8, 9)),
               (3, (7, 9)), (4, (7, 9)), (1, (7, 9)), (4, (36, 132))]


@pytest.mark.parametrize("case", IMAGE_LISTS, ids=lambda c: f"{c[0]}at{c[1][0]}x{c[1][1]}")
def test_images_tile_against_the_oracle(sv, case):
    """At 6 x 10 an output pixel of the left part mixes two pictures; 8 x 9: W odd for two pictures; 7 x 9: H and W odd
    for one, three and four; 36 x 132: quadrants and an output four pixels a lane."""
    count, size = case
    imgs = _mixed(np.random.default_rng(31 * count + size[0]), count, size)
    got = sv.dropin.images_tile([("", i) for i in imgs], size)
    same(got, rn.batch_images(imgs, size), case)
    if count == 1:
        same(sv.dropin.images_tile(imgs, size), got, "a list of arrays")


def test_images_tile_of_the_cropped_mode(sv):
    """The five-picture list at (544, 1024) with a 390 x 889 disparity: what crop_disparity=True passes."""
    rng = np.random.default_rng(544)
    H, W = 544, 1024
    imgs = [rnd(rng, 390, 889), rnd(rng, H, W, 3), rnd(rng, H, W), rnd(rng, H, W), rnd(rng, H, W, 3)]
    got = sv.dropin.images_tile(imgs, (H, W))
    assert got.shape == (H // 2, W, 3)
    same(got, rn.batch_images(imgs, (H, W)), "cropped mode")


def test_images_tile_argument_errors(sv):
    abi = sv.abi
    f = abi.lib().sv_images_tile
    z = np.zeros((8, 8), np.uint8)
    out = np.zeros((16, 16, 3), np.uint8)

    def pics(n, channels=1, data=z):
        arr = (abi.Picture * max(n, 1))()
        for k in range(max(n, 1)):
            arr[k] = abi.Picture(data.ctypes.data, 8, 8, channels)
        return arr
    assert f(pics(2), 2, 8, 8, abi.ptr(out)) == 0
    assert f(pics(2), 2, 7, 8, abi.ptr(out)) == E_ARG          # H odd for two pictures
    assert f(pics(5), 5, 8, 9, abi.ptr(out)) == E_ARG          # W odd for five
    assert f(pics(5), 5, 7, 8, abi.ptr(out)) == E_ARG
    assert f(pics(1), 0, 8, 8, abi.ptr(out)) == E_ARG and f(pics(6), 6, 8, 8, abi.ptr(out)) == E_ARG
    assert f(pics(1, channels=2), 1, 8, 8, abi.ptr(out)) == E_ARG
    assert f(None, 1, 8, 8, abi.ptr(out)) == E_ARG and f(pics(1), 1, 8, 8, None) == E_ARG
    assert f(pics(1), 1, 0, 8, abi.ptr(out)) == E_ARG and f(pics(1), 1, 8, 4097, abi.ptr(out)) == E_ARG
    null = (abi.Picture * 1)()
    null[0] = abi.Picture(None, 8, 8, 1)
    assert f(null, 1, 8, 8, abi.ptr(out)) == E_ARG
    big = np.zeros((8, 8, 3), np.uint8)
    assert f(pics(1, data=big), 1, 8, 8, abi.ptr(big)) == E_ARG                # out overlaps the picture
    with pytest.raises(sv.svx.SvxError):
        sv.dropin.images_tile([z] * 6, (8, 8))
    with pytest.raises(TypeError):
        sv.dropin.images_tile([z.astype(np.float32)], (8, 8))


@pytest.mark.parametrize("shape", [(12, 48), (40, 76)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_cross_check_with_the_tile_stage(sv, shape):
    """For the list sv_image_tile takes, composing the stack for real gives the closed form's bytes."""
    H, W = shape
    rng = np.random.default_rng(12 + H)
    disp, bgr, road, cleaned, result = rnd(rng, H, W), rnd(rng, H, W, 3), rnd(rng, H, W), rnd(rng, H, W), rnd(rng, H, W, 3)
    got = sv.dropin.images_tile([disp, tn.road_map(bgr, road), road, cleaned, result], (H, W))
    same(got, sv.dropin.image_tile(disp, bgr, road, cleaned, result), shape)


# ---- the batch -------------------------------------------------------------------------------------------------
def test_batch_resize_disp(sv):
    H, W = 40, 76
    rng = np.random.default_rng(4076)
    frames = [rnd(rng, H, W) for _ in range(3)]
    lib = sv.abi.lib()
    t = ctypes.c_float(0)
    with sv.batch.Batch(3, H, W, with_bgr=False) as b:
        for f, d in enumerate(frames):
            b.upload(f, d)
        out = np.empty((54, 102), np.uint8)
        assert lib.sv_batch_read_resized_disp(b._h, 0, sv.abi.ptr(out)) == E_STATE      # before the first call
        assert lib.sv_batch_resize_disp_ms(b._h, ctypes.byref(t)) == E_STATE
        for dh, dw in ((54, 102), (30, 50)):
            b.resize_disp((dh, dw))
            assert b.resize_disp_ms() > 0
            for f in range(3):
                same(b.read_resized_disp(f), tn.resize_linear_u8(b.read_disp(f), dw, dh), (dh, dw, f))
        b.resize_disp((H, W))
        for f in range(3):
            same(b.read_resized_disp(f), b.read_disp(f), ("identity", f))
            same(b.read_disp(f), frames[f], ("the frames are not touched", f))
        for dh, dw in ((0, 5), (4097, 8), (5, 0), (8, 4097)):
            assert lib.sv_batch_resize_disp(b._h, dh, dw, 1) == E_ARG, (dh, dw)
        b.resize_disp((54, 102))
        b.upload(1, frames[0])                                                          # new frames: stale
        assert lib.sv_batch_read_resized_disp(b._h, 0, sv.abi.ptr(out)) == E_STATE
        assert lib.sv_batch_resize_disp_ms(b._h, ctypes.byref(t)) == E_STATE
        with pytest.raises(sv.svx.SvxError):
            b.read_resized_disp(0)
        b.resize_disp((54, 102))
        same(b.read_resized_disp(1), tn.resize_linear_u8(frames[0], 102, 54), "after the new upload")
        b.prepass("mean")                                                               # a new pre-pass: stale too
        assert lib.sv_batch_read_resized_disp(b._h, 0, sv.abi.ptr(out)) == E_STATE
        b.resize_disp((54, 102))                                                        # ... and of the cleaned frames
        same(b.read_resized_disp(2), tn.resize_linear_u8(b.read_disp(2), 102, 54), "after the pre-pass")


def test_batch_72x1024_stride_equal_to_width(sv):
    H, W = 72, 1024
    rng = np.random.default_rng(72)
    frames = [rnd(rng, H, W) for _ in range(2)]
    with sv.batch.Batch(2, H, W, with_bgr=False) as b:
        for f, d in enumerate(frames):
            b.upload(f, d)
        b.resize_disp((100, 1000))
        for f in range(2):
            same(b.read_resized_disp(f), tn.resize_linear_u8(frames[f], 1000, 100), f)


def test_batch_cropped_frame_to_the_display_size(sv):
    """One 390 x 889 frame (rows at a stride of 896) to (544, 1024): the Disparity picture of the cropped mode's tile."""
    rng = np.random.default_rng(390)
    d = rnd(rng, 390, 889)
    with sv.batch.Batch(1, 390, 889, with_bgr=False) as b:
        b.upload(0, d)
        b.resize_disp((544, 1024))
        same(b.read_resized_disp(0), tn.resize_linear_u8(d, 1024, 544), "390 x 889")


# ---- the drop-in -----------------------------------------------------------------------------------------------
def test_dropin_resize_group(sv):
    calls = []

    def original_batch(img_list, size):
        calls.append("batch")
        return "original"

    def original_resize(image, height, width):
        calls.append("resize")
        return "original"
    m = types.SimpleNamespace(camera_focal_length_px=1.0, stereo_camera_baseline_m=2.0, image_centre_w=3.0,
                              image_centre_h=4.0, batchImages=original_batch, resizeImage=original_resize)
    rng = np.random.default_rng(5)
    img = rnd(rng, 40, 76)
    four = [("a", rnd(rng, 6, 10)), ("b", rnd(rng, 9, 21, 3)), ("c", rnd(rng, 3, 15)), ("d", rnd(rng, 13, 7, 3))]
    sv.dropin.install(m, resize=True)
    try:
        same(m.resizeImage(img, 54, 102), tn.resize_linear_u8(img, 102, 54), "resizeImage")
        same(m.batchImages(four, (6, 10)), rn.batch_images([i for _, i in four], (6, 10)), "batchImages")
        assert calls == []
    finally:
        sv.dropin.uninstall()
    assert m.batchImages is original_batch and m.resizeImage is original_resize
