"""GPU: the result image (stereovision.py:181-209, functions.py:390-394, :424-431) — kernels/result.hip behind
sv_result_image, the batch path (Batch.result), the frame loop (road="result") and dropin.result_image — bit for bit
over whole images against the oracle tests/result_numpy.py (pinned by tests/test_result_cpu.py)."""
import ctypes
import types

import numpy as np
import pytest

import hull_numpy as hn
import morph_numpy as mn
import result_numpy as rn

pytestmark = pytest.mark.gpu

ABC = (0.013, -0.62, 0.047)
TIPS = {"far": (-10 ** 6, 10 ** 6), "int32 max": (2 ** 31 - 1, 2 ** 31 - 1), "2^31": (2 ** 31, 5),
        "-2^31 y": (5, -2 ** 31)}


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import _abi, batch, dropin, loop
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, abi=_abi, batch=batch, dropin=dropin, loop=loop)


def same(got, ref, what):
    assert got.dtype == np.uint8 and got.shape == ref.shape, what
    bad = np.argwhere((got != ref).any(-1))
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())


def _bgr(shape, seed=0):
    """Random BGR with the values 0 and 255 in it."""
    rng = np.random.default_rng(5200 + seed + shape[0])
    a = rng.integers(0, 256, tuple(shape) + (3,)).astype(np.uint8)
    a[rng.random(shape) < 0.05] = 0
    a[rng.random(shape) < 0.05] = 255
    return a


def _disp(shape):
    return np.random.default_rng(900 + shape[0]).integers(1, 256, shape).astype(np.uint8)


_REF = {}


def _ref(shape, name):
    """The obstacle stage's oracle for one case, and the result's, computed once and shared (left unchanged)."""
    if (shape, name) not in _REF:
        bgr = _bgr(shape)
        r = hn.obstacles(hn.cases(*shape)[name], _disp(shape), ABC)
        _REF[(shape, name)] = (bgr, r, rn.result(bgr, r["obstacles"], r["hull"], r["centre"], r["tip"], r["valid"]))
    return _REF[(shape, name)]


def _host(sv, bgr, r, tip="own"):
    return sv.dropin.result_image(bgr, r["obstacles"], r["hull"], r["centre"], r["tip"] if tip == "own" else tip)


CASES = tuple(hn.cases(40, 70))
SMALL = [(40, 70), (64, 96), (390, 889)]


# ---- the host entry --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_cases(sv, shape):
    """40 x 70: W % 32 != 0 and 3 W no multiple of 16 (a row stride of 72 pixels: the 8-pixel path); 64 x 96: the
    16-pixel path, one band; 390 x 889: seven bands, the last one short, a row stride of 896."""
    sizes = set()
    for name in CASES:
        bgr, r, want = _ref(shape, name)
        same(_host(sv, bgr, r), want, (shape, name))
        sizes.add(len(r["hull"]))
    assert {0, 1, 2, 3, 4, 8} <= sizes
    assert np.array_equal(_ref(shape, "empty")[2], _ref(shape, "empty")[0])          # n = 0: the identity


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_tip_variants(sv, shape):
    bgr, r, outline_only = _ref(shape, "steep_shallow")
    centre = r["centre"]
    outline_only = rn.result(bgr, r["obstacles"], r["hull"], centre, None)
    for name, tip in TIPS.items():
        want = rn.result(bgr, r["obstacles"], r["hull"], centre, tip, 3)
        assert np.array_equal(want, outline_only) == (name in ("2^31", "-2^31 y")), name
        same(_host(sv, bgr, r, tip), want, (shape, name))
    same(_host(sv, bgr, r, None), outline_only, "valid = 1")
    same(sv.dropin.result_image(bgr, r["obstacles"], r["hull"], None, (3, 3)), outline_only, "no centre")
    same(sv.dropin.result_image(bgr, r["obstacles"], np.zeros((0, 1, 2), np.int32), centre, (3, 3)), bgr, "n = 0")
    # a ring started elsewhere and turned round paints the same outline
    ring = r["hull"].reshape(-1, 2)
    ring = np.roll(ring, 3, axis=0)[::-1].copy()
    same(sv.dropin.result_image(bgr, r["obstacles"], ring, centre, r["tip"]), _ref(shape, "steep_shallow")[2], "ring")
    # heads and lines over every border, every layer on one pixel
    H, W = shape
    for c, tip in (((W // 2, H // 2), (-3, H // 2)), ((W // 2, H // 2), (W + 2, 3)), ((2, 2), (W // 3, -5)),
                   ((W - 1, H - 1), (W // 2, H + 4)), ((W // 2, H // 2), (W // 2, H // 2))):
        same(sv.dropin.result_image(bgr, r["obstacles"], r["hull"], c, tip),
             rn.result(bgr, r["obstacles"], r["hull"], c, tip, 3), (shape, c, tip))


def test_host_entry_544x1024(sv):
    """The reference's shape, three cases: one wave a row, 16 pixels a lane."""
    for name in ("sparse", "steep_shallow", "two_blobs"):
        bgr, r, want = _ref((544, 1024), name)
        same(_host(sv, bgr, r), want, name)


def test_argument_errors(sv):
    abi, dropin = sv.abi, sv.dropin
    bgr, ob = np.zeros((4, 8, 3), np.uint8), np.zeros((4, 8), np.uint8)
    hull = np.array([[1, 1], [1, 3], [6, 3]], np.int32)
    assert dropin.result_image(bgr, ob, hull).shape == (4, 8, 3)
    with pytest.raises(sv.svx.SvxError):
        dropin.result_image(np.zeros((4, 1, 3), np.uint8), np.zeros((4, 1), np.uint8), hull)       # W < 2
    with pytest.raises(sv.svx.SvxError):
        dropin.result_image(np.zeros((2, 4097, 3), np.uint8), np.zeros((2, 4097), np.uint8), hull)   # W > 4096
    with pytest.raises(sv.svx.SvxError):
        dropin.result_image(np.zeros((4097, 2, 3), np.uint8), np.zeros((4097, 2), np.uint8), hull)   # H > 4096
    with pytest.raises(sv.svx.SvxError):                                                            # not convex
        dropin.result_image(bgr, ob, np.array([[0, 0], [6, 0], [3, 1], [6, 3], [0, 3]], np.int32))
    with pytest.raises(sv.svx.SvxError):                                                            # twice around
        dropin.result_image(bgr, ob, np.array([[3, 0], [5, 3], [0, 1], [6, 1], [1, 3]], np.int32))
    with pytest.raises(sv.svx.SvxError):                                                            # the centre's range
        dropin.result_image(bgr, ob, hull, (20000, 1), (2, 2))
    with pytest.raises(ValueError):
        dropin.result_image(bgr, ob, np.array([[0, 0], [20000, 1]], np.int32))
    with pytest.raises(ValueError):
        dropin.result_image(bgr, np.zeros((4, 9), np.uint8), hull)
    with pytest.raises(TypeError):
        dropin.result_image(bgr.astype(np.float32), ob, hull)
    # SV_E_ARG (-1) from the C entry: null pointers, n out of range, a vertex out of range
    out = np.empty_like(bgr)
    f = abi.lib().sv_result_image
    assert f(abi.ptr(bgr), abi.ptr(ob), abi.ptr(hull), 3, None, 4, 8, abi.ptr(out)) == 0
    assert f(None, abi.ptr(ob), abi.ptr(hull), 3, None, 4, 8, abi.ptr(out)) == -1
    assert f(abi.ptr(bgr), None, abi.ptr(hull), 3, None, 4, 8, abi.ptr(out)) == -1
    assert f(abi.ptr(bgr), abi.ptr(ob), abi.ptr(hull), 3, None, 4, 8, None) == -1
    assert f(abi.ptr(bgr), abi.ptr(ob), None, 3, None, 4, 8, abi.ptr(out)) == -1
    assert f(abi.ptr(bgr), abi.ptr(ob), abi.ptr(hull), -1, None, 4, 8, abi.ptr(out)) == -1
    assert f(abi.ptr(bgr), abi.ptr(ob), abi.ptr(hull), 8193, None, 4, 8, abi.ptr(out)) == -1
    far = np.array([[1, 1], [1, 3], [16384, 3]], np.int32)
    assert f(abi.ptr(bgr), abi.ptr(ob), abi.ptr(far), 3, None, 4, 8, abi.ptr(out)) == -1
    assert f(abi.ptr(bgr), abi.ptr(ob), None, 0, None, 4, 8, abi.ptr(out)) == 0 and np.array_equal(out, bgr)


# ---- the batch path --------------------------------------------------------------------------------------------
def _blocks(H, W, *blocks):
    a = np.zeros((H, W), np.uint8)
    for y0, y1, x0, x1 in blocks:
        a[y0:y1, x0:x1] = 200
    return a


def _five_frames(H, W):
    """Disparities whose road images differ: full, empty, full (an empty frame between two full ones), two blobs,
    a filled ring with steep and shallow sides."""
    ring = (hn.fill_polygon((H, W), hn.polygon_steep_shallow(H, W)) != 0).astype(np.uint8) * 200
    return [np.full((H, W), 200, np.uint8), np.zeros((H, W), np.uint8), np.full((H, W), 200, np.uint8),
            _blocks(H, W, (2, 2 + H // 3, 5, 5 + W // 4), (H - 4 - H // 3, H - 4, W - 9 - W // 3, W - 9)), ring]


def _run_batch(sv, H, W, mode, bits, frames_disp):
    """Every frame's own BGR: one hue (the pipeline's histogram filter keeps every point), the brightness random,
    0 and 255 in it."""
    n = len(frames_disp)
    rng = np.random.default_rng(H + n)
    bgrs = []
    for f in range(n):
        g = rng.integers(0, 256, (H, W, 1)).astype(np.uint8)
        g[rng.random((H, W)) < 0.05] = 0
        g[rng.random((H, W)) < 0.05] = 255
        bgrs.append(np.repeat(g, 3, axis=2))
    plane = (0.0, 0.0, 0.01)
    with sv.batch.Batch(n, H, W, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode(mode)
        b.road_bits(bits)
        b.road_map(True)
        for f, d in enumerate(frames_disp):
            b.upload(f, d, bgrs[f])
        b.pipeline(plane=plane, point_thr=1e9, hist_thr=2)
        b.road_raster()
        b.road_clean()
        with pytest.raises(sv.svx.SvxError):        # SV_E_STATE: no obstacle stage yet
            b.result()
        b.road_hull()
        with pytest.raises(sv.svx.SvxError):        # ... and no result yet
            b.read_result(0)
        maps = [b.read_road_map(f) for f in range(n)]
        b.result()
        assert b.result_ms() > 0
        counts, got = [], []
        for f in range(n):
            r = b.read_road_hull(f)
            img = b.read_result(f)
            same(img, rn.result(bgrs[f], r["obstacles"], r["hull"], r["centre"], r["tip"], r["valid"]), (H, W, f))
            same(sv.dropin.result_image(bgrs[f], r["obstacles"], r["hull"], r["centre"], r["tip"]), img,
                 ("host entry", H, W, f))
            assert np.array_equal(b.read_road_map(f), maps[f]), f          # the map is untouched
            counts.append(len(r["hull"]))
            got.append(img)
        b.result()                                    # the BGR is untouched: the same picture again
        for f in range(n):
            assert np.array_equal(b.read_result(f), got[f]), f
        b.road_clean()                                # a new clean-up: neither hull nor result is current
        with pytest.raises(sv.svx.SvxError):
            b.result()
        with pytest.raises(sv.svx.SvxError):
            b.read_result(0)
        with pytest.raises(sv.svx.SvxError):
            b.result_ms()
        b.road_hull()
        with pytest.raises(sv.svx.SvxError):        # a new obstacle stage: the old result is not its picture
            b.read_result(0)
        b.result()
        assert np.array_equal(b.read_result(n - 1), got[n - 1])
        b.pipeline(plane=plane, point_thr=1e9, hist_thr=2)   # new points: SV_E_STATE again
        with pytest.raises(sv.svx.SvxError):
            b.result()
        with pytest.raises(sv.svx.SvxError):
            b.read_result(0)
        b.road_raster()                               # ... and the map made from the BGR anew is the same
        for f in range(n):
            assert np.array_equal(b.read_road_map(f), maps[f]), f
    return counts


def test_batch_five_frames_do_not_leak(sv):
    """72 x 1024 from the pipeline's bitmap: an empty frame (the identity) between two full ones."""
    counts = _run_batch(sv, 72, 1024, "resident", True, _five_frames(72, 1024))
    assert counts[0] == 4 and counts[1] == 0 and counts[2] == 4 and counts[3] >= 5 and counts[4] >= 3, counts


def test_batch_390x889(sv):
    """W % 32 != 0 at a row stride of 896 pixels."""
    counts = _run_batch(sv, 390, 889, "auto", False, _five_frames(390, 889)[1:])
    assert counts[0] == 0 and counts[1] == 4, counts


def test_batch_without_bgr(sv):
    with sv.batch.Batch(1, 72, 1024, step=1, with_bgr=False) as b:
        with pytest.raises(sv.svx.SvxError):
            b.result()
        assert sv.abi.lib().sv_batch_result(b._h, 1) == -4        # SV_E_STATE
        out = np.empty((72, 1024, 3), np.uint8)
        assert sv.abi.lib().sv_batch_read_result(b._h, 0, sv.abi.ptr(out)) == -4
        t = ctypes.c_float(0)
        assert sv.abi.lib().sv_batch_result_ms(b._h, ctypes.byref(t)) == -4


# ---- the frame loop --------------------------------------------------------------------------------------------
def test_frame_loop_result(sv):
    """road="result" on two 2-frame synthetic batches in flight: every frame against the chain morph_numpy ->
    hull_numpy -> result_numpy on the synthetic frame's BGR."""
    import oracle
    from svx.loop import STAGES, FrameLoop
    frames = 2
    seen = []
    with FrameLoop(frames, slots=2, source="synth", road="result") as loop:
        def verify(seq):
            b, first = loop.batch(seq)
            for f in range(frames):
                ref_clean = mn.sanitise(b.read_road(f))
                pl = b.read_frame_plane(f)
                abc = tuple(pl[:3]) if pl[3] >= 0 else None
                r = hn.obstacles(ref_clean, b.read_disp(f), abc)
                _, bgr = oracle.synth_frame(first + f)
                same(b.read_result(f), rn.result(bgr, r["obstacles"], r["hull"], r["centre"], r["tip"], r["valid"]),
                     (seq, f))
                seen.append((len(r["hull"]), r["valid"]))
        s0 = loop.submit(0)
        s1 = loop.submit(frames)
        verify(s0)
        verify(s1)
        tl = loop.timeline(s1)
        assert tuple(tl) == STAGES and tl["road"][0] <= tl["road"][1]
    assert len(seen) == 2 * frames and any(n >= 3 and v == 3 for n, v in seen), seen
    with FrameLoop(frames, slots=2, source="synth", road="obstacles") as loop:   # road = 4 makes no picture
        b, _ = loop.batch(loop.submit(0))
        assert b.read_road_hull(0, images=False)["valid"] in (0, 1, 3)
        with pytest.raises(sv.svx.SvxError):
            b.read_result(0)
