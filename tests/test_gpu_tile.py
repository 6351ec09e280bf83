"""GPU: the image tile (stereovision.py:216, functions.py:452-499 batchImages) — kernels/tile.hip behind
sv_image_tile, the batch path (Batch.tile), the frame loop (road="tile") and dropin.batchImages — bit for bit over
whole tiles against the oracle tests/tile_numpy.py (pinned by tests/test_tile_cpu.py)."""
import ctypes
import types

import numpy as np
import pytest

import hull_numpy as hn
import tile_numpy as tn

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import _abi, batch, dropin, loop
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, abi=_abi, batch=batch, dropin=dropin, loop=loop)


def same(got, ref, what):
    assert got.dtype == np.uint8 and got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.argwhere((got != ref).any(-1))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())


def _pictures(shape, kind):
    """disparity, BGR, road, cleaned, result. "random": every picture random bytes with 0 and 255 in them (the two
    road pictures too: the host entry averages whatever bytes it gets); "binary": road pictures of 0 / 255 with
    isolated pixels, isolated holes and full rows."""
    H, W = shape
    rng = np.random.default_rng(6100 + H + (kind == "binary"))

    def rnd(*s):
        a = rng.integers(0, 256, s).astype(np.uint8)
        a[rng.random(s) < 0.05] = 0
        a[rng.random(s) < 0.05] = 255
        return a
    if kind == "random":
        road, cleaned = rnd(H, W), rnd(H, W)
    else:
        road = ((rng.random(shape) < 0.03) * 255).astype(np.uint8)          # isolated pixels
        road[1::5, :] = 255                                                 # full rows, sampled and not
        cleaned = ((rng.random(shape) < 0.97) * 255).astype(np.uint8)       # isolated holes
        cleaned[2::7, :] = 0
    return rnd(H, W), rnd(H, W, 3), road, cleaned, rnd(H, W, 3)


_REF = {}


def _ref(shape, kind):
    """One case's pictures and its oracle tile, computed once and shared (left unchanged)."""
    if (shape, kind) not in _REF:
        disp, bgr, road, cleaned, result = _pictures(shape, kind)
        _REF[(shape, kind)] = ((disp, bgr, road, cleaned, result),
                               tn.tile_closed(disp, tn.road_map(bgr, road), road, cleaned, result))
    return _REF[(shape, kind)]


# ---- the host entry --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 4), (12, 48), (40, 76), (64, 96), (544, 1024)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry(sv, shape):
    """4 x 4: one output pixel per quadrant; 40 x 76: W no multiple of 8 or 32 (the padded BGR stride, partial bitmap
    words, 3 W no multiple of 16: a pixel per lane); 12 x 48 and 64 x 96: the 16-byte path, W / 16 odd and even;
    544 x 1024: one frame."""
    for kind in ("random", "binary"):
        pics, want = _ref(shape, kind)
        got = sv.dropin.image_tile(*pics)
        assert got.shape == (shape[0] // 2, shape[1], 3)
        same(got, want, (shape, kind))
    if shape == (4, 4):
        assert np.array_equal(_ref(shape, "random")[1], tn.tile(*_with_map(_ref(shape, "random")[0])))


def _with_map(pics):
    disp, bgr, road, cleaned, result = pics
    return disp, tn.road_map(bgr, road), road, cleaned, result


def test_argument_errors(sv):
    abi = sv.abi
    f = abi.lib().sv_image_tile

    def call(H, W, null=None, alloc=None):
        h, w = alloc or (max(H, 4), max(W, 4))
        a = [np.zeros((h, w), np.uint8), np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8),
             np.zeros((h, w), np.uint8), np.zeros((h, w, 3), np.uint8), np.zeros((h // 2 + 1, w, 3), np.uint8)]
        p = [abi.ptr(x) for x in a]
        if null is not None:
            p[null] = None
        return f(p[0], p[1], p[2], p[3], p[4], H, W, p[5])
    assert call(8, 8) == 0
    for H, W in ((6, 8), (8, 6), (390, 889), (390, 888), (392, 889), (0, 8), (8, 0), (4100, 8), (8, 4100), (-4, 8)):
        assert call(H, W, alloc=(8, 8) if max(H, W) > 4096 or min(H, W) <= 0 else None) == E_ARG, (H, W)
    for k in range(6):
        assert call(8, 8, null=k) == E_ARG, k
    d = np.zeros((8, 8), np.uint8)
    c = np.zeros((8, 8, 3), np.uint8)
    assert f(abi.ptr(d), abi.ptr(c), abi.ptr(d), abi.ptr(d), abi.ptr(c), 8, 8, abi.ptr(c)) == E_ARG    # out overlaps
    with pytest.raises(sv.svx.SvxError):
        sv.dropin.image_tile(np.zeros((390, 889), np.uint8), np.zeros((390, 889, 3), np.uint8),
                             np.zeros((390, 889), np.uint8), np.zeros((390, 889), np.uint8),
                             np.zeros((390, 889, 3), np.uint8))
    with pytest.raises(ValueError):
        sv.dropin.image_tile(d, c, np.zeros((8, 12), np.uint8), d, c)
    with pytest.raises(TypeError):
        sv.dropin.image_tile(d.astype(np.float32), c, d, d, c)


# ---- the batch path --------------------------------------------------------------------------------------------
def _blocks(H, W, *blocks):
    a = np.zeros((H, W), np.uint8)
    for y0, y1, x0, x1 in blocks:
        a[y0:y1, x0:x1] = 200
    return a


def _five_frames(H, W):
    """tests/test_gpu_result.py's recipe: disparities whose road images differ: full, empty, full (an empty frame
    between two full ones), two blobs, a filled ring with steep and shallow sides."""
    ring = (hn.fill_polygon((H, W), hn.polygon_steep_shallow(H, W)) != 0).astype(np.uint8) * 200
    return [np.full((H, W), 200, np.uint8), np.zeros((H, W), np.uint8), np.full((H, W), 200, np.uint8),
            _blocks(H, W, (2, 2 + H // 3, 5, 5 + W // 4), (H - 4 - H // 3, H - 4, W - 9 - W // 3, W - 9)), ring]


def _oracle(b, f, rmap=None):
    """The tile of the batch's own five pictures, each pinned by its own test."""
    road = b.read_road(f)
    return tn.tile_closed(b.read_disp(f), rmap if rmap is not None else b.read_road_map(f), road,
                          b.read_road_clean(f), b.read_result(f))


def _run_batch(sv, H, W, mode, bits, want_map):
    frames_disp = _five_frames(H, W)
    n = len(frames_disp)
    rng = np.random.default_rng(H + n)
    bgrs = []
    for f in range(n):      # one hue (the histogram filter keeps every point), the brightness random, 0 and 255 in it
        g = rng.integers(0, 256, (H, W, 1)).astype(np.uint8)
        g[rng.random((H, W)) < 0.05] = 0
        g[rng.random((H, W)) < 0.05] = 255
        bgrs.append(np.repeat(g, 3, axis=2))
    plane = (0.0, 0.0, 0.01)
    with sv.batch.Batch(n, H, W, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode(mode)
        b.road_bits(bits)
        b.road_map(want_map)
        for f, d in enumerate(frames_disp):
            b.upload(f, d, bgrs[f])
        b.pipeline(plane=plane, point_thr=1e9, hist_thr=2)
        b.road_raster()
        b.road_clean()
        b.road_hull()
        with pytest.raises(sv.svx.SvxError):        # SV_E_STATE: no result image yet
            b.tile()
        assert sv.abi.lib().sv_batch_tile(b._h, 1) == E_STATE
        b.result()
        with pytest.raises(sv.svx.SvxError):        # ... and no tile yet
            b.read_tile(0)
        maps = [b.read_road_map(f) if want_map else tn.road_map(bgrs[f], b.read_road(f)) for f in range(n)]
        results = [b.read_result(f) for f in range(n)]
        b.tile()
        assert b.tile_ms() > 0
        got, road_px = [], []
        for f in range(n):
            t = b.read_tile(f)
            assert t.shape == (H // 2, W, 3)
            same(t, _oracle(b, f, None if want_map else maps[f]), (H, W, f))
            same(sv.dropin.image_tile(b.read_disp(f), bgrs[f], b.read_road(f), b.read_road_clean(f), results[f]), t,
                 ("host entry", H, W, f))
            got.append(t)
            road_px.append(int((b.read_road(f) != 0).sum()))
        # the empty frame between two full ones: its road quadrants are black, its map quadrant is the BGR's
        assert road_px[0] > 0 and road_px[1] == 0 and road_px[2] > 0, road_px
        assert not got[1][H // 4:, : W // 2].any() and got[0][H // 4:, : W // 4].any()
        z = np.zeros((H, W), np.uint8)
        same(got[1][: H // 4, W // 4: W // 2], tn.tile_closed(z, bgrs[1], z, z, bgrs[1])[: H // 4, W // 4: W // 2],
             "empty frame's map")
        b.tile()                                      # nothing it reads is touched: the same bytes again
        for f in range(n):
            assert np.array_equal(b.read_tile(f), got[f]), f
            assert np.array_equal(b.read_result(f), results[f]), f
            if want_map:
                assert np.array_equal(b.read_road_map(f), maps[f]), f
        b.road_clean()                                # a new clean-up: hull, result and tile are not current
        for call in (b.tile, b.tile_ms, lambda: b.read_tile(0)):
            with pytest.raises(sv.svx.SvxError):
                call()
        b.road_hull()
        b.result()
        with pytest.raises(sv.svx.SvxError):        # a new result: the old tile is not its picture
            b.read_tile(0)
        b.tile()
        assert np.array_equal(b.read_tile(n - 1), got[n - 1])
        b.road_hull()                                 # a new obstacle stage drops result and tile
        assert sv.abi.lib().sv_batch_tile(b._h, 1) == E_STATE
        b.result()
        b.tile()
        b.pipeline(plane=plane, point_thr=1e9, hist_thr=2)   # new points: SV_E_STATE again
        assert sv.abi.lib().sv_batch_tile(b._h, 1) == E_STATE
        out = np.empty((H // 2, W, 3), np.uint8)
        assert sv.abi.lib().sv_batch_read_tile(b._h, 0, sv.abi.ptr(out)) == E_STATE


def test_batch_72x1024_from_the_bitmaps(sv):
    """The resident pipeline's road bitmap and the clean-up's, 16-byte loads; imageRoadMap on."""
    _run_batch(sv, 72, 1024, "resident", True, True)


def test_batch_72x1024_without_the_map(sv):
    """sv_batch_road_map off: the map quadrant is painted from the road picture all the same."""
    _run_batch(sv, 72, 1024, "resident", True, False)


def test_batch_40x76_from_the_u8_road_image(sv):
    """No pipeline bitmap: the road picture is read as u8 (the cleaned one from its partial bitmap words), a pixel
    per lane at a row stride of 80."""
    _run_batch(sv, 40, 76, "auto", False, True)


def test_batch_without_bgr_and_odd_shape(sv):
    with sv.batch.Batch(1, 72, 1024, step=1, with_bgr=False) as b:
        with pytest.raises(sv.svx.SvxError):
            b.tile()
        assert sv.abi.lib().sv_batch_tile(b._h, 1) == E_STATE
        out = np.empty((36, 1024, 3), np.uint8)
        assert sv.abi.lib().sv_batch_read_tile(b._h, 0, sv.abi.ptr(out)) == E_STATE
        t = ctypes.c_float(0)
        assert sv.abi.lib().sv_batch_tile_ms(b._h, ctypes.byref(t)) == E_STATE
    with sv.batch.Batch(1, 42, 72, step=1, with_bgr=True) as b:       # H no multiple of 4
        assert sv.abi.lib().sv_batch_tile(b._h, 1) == E_ARG
    with sv.batch.Batch(1, 40, 70, step=1, with_bgr=True) as b:       # W no multiple of 4
        assert sv.abi.lib().sv_batch_tile(b._h, 1) == E_ARG


# ---- the frame loop --------------------------------------------------------------------------------------------
def test_frame_loop_tile(sv):
    """road="tile" on two 2-frame synthetic batches in flight: every frame's tile against the oracle on that batch's
    five read-backs (the loop leaves sv_batch_road_map off: the map is made from the BGR here)."""
    import oracle
    from svx.loop import STAGES, FrameLoop
    frames = 2
    seen = 0
    with FrameLoop(frames, slots=2, source="synth", road="tile") as loop:
        def verify(seq):
            nonlocal seen
            b, first = loop.batch(seq)
            for f in range(frames):
                _, bgr = oracle.synth_frame(first + f)
                same(b.read_tile(f), _oracle(b, f, tn.road_map(bgr, b.read_road(f))), (seq, f))
                seen += int((b.read_road(f) != 0).any())
        s0 = loop.submit(0)
        s1 = loop.submit(frames)
        verify(s0)
        verify(s1)
        tl = loop.timeline(s1)
        assert tuple(tl) == STAGES and tl["road"][0] <= tl["road"][1]
    assert seen >= 1
    with FrameLoop(frames, slots=2, source="synth", road="result") as loop:   # road = 5 makes no tile
        b, _ = loop.batch(loop.submit(0))
        assert b.read_result(0).shape == (544, 1024, 3)
        with pytest.raises(sv.svx.SvxError):
            b.read_tile(0)
    with pytest.raises(sv.svx.SvxError):                                       # the shape is checked at creation
        FrameLoop(frames, H=42, W=64, slots=2, source="synth", road="tile")


# ---- the drop-in -----------------------------------------------------------------------------------------------
def test_dropin_batch_images(sv):
    """batchImages through install(m, tiles=True) on a stub module equals read_tile; a four-image list reaches the
    stub's own function."""
    H, W = 72, 1024
    calls = []

    def original(img_list, size):
        calls.append(len(img_list))
        return "original"
    m = types.SimpleNamespace(camera_focal_length_px=1.0, stereo_camera_baseline_m=2.0, image_centre_w=3.0,
                              image_centre_h=4.0, batchImages=original)
    disp = _five_frames(H, W)[4]
    g = np.random.default_rng(9).integers(0, 256, (H, W, 1)).astype(np.uint8)
    bgr = np.repeat(g, 3, axis=2)
    with sv.batch.Batch(1, H, W, step=1, with_bgr=True, with_points=True) as b:
        b.road_map(True)
        b.upload(0, disp, bgr)
        b.pipeline(plane=(0.0, 0.0, 0.01), point_thr=1e9, hist_thr=2)
        b.road_raster()
        b.road_clean()
        b.road_hull()
        b.result()
        b.tile()
        want = b.read_tile(0)
        imgs = [("Disparity", b.read_disp(0)), ("ImageRoadMap", b.read_road_map(0)), ("RoadImage", b.read_road(0)),
                ("FilteredRoadImage", b.read_road_clean(0)), ("Result", b.read_result(0))]
    assert (imgs[2][1] != 0).any() and (imgs[3][1] != 0).any()
    sv.dropin.install(m, tiles=True)
    try:
        same(m.batchImages(imgs, (H, W)), want, "batchImages")
        assert calls == []
        assert m.batchImages(imgs[:4], (H, W)) == "original" and calls == [4]
    finally:
        sv.dropin.uninstall()
    assert m.batchImages is original
