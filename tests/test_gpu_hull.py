"""GPU: the obstacle stage (stereovision.py:170-189, functions.py:396-421) — kernels/hull.hip behind
sv_road_obstacles, the batch path (Batch.road_hull), the frame loop (road="obstacles") and the drop-ins — bit for
bit against the oracle tests/hull_numpy.py (pinned by tests/test_hull_cpu.py): hull vertices and their order, hull
mask, obstacles, circle centre, glyph tip and the valid flags."""
import json
import os
import types

import numpy as np
import pytest

import hull_numpy as hn
import morph_numpy as mn
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ABC = (0.013, -0.62, 0.047)


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import _abi, batch, dropin, loop
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, abi=_abi, batch=batch, dropin=dropin, loop=loop)


def same(got, ref, what):
    """One frame's result dict against the oracle's, field by field."""
    assert got["hull"].dtype == np.int32 and got["hull"].ndim == 3 and got["hull"].shape[1:] == (1, 2), what
    assert got["hull"].tolist() == ref["hull"].tolist(), (what, got["hull"].reshape(-1, 2).tolist()[:8],
                                                          ref["hull"].reshape(-1, 2).tolist()[:8])
    for k in ("hull_mask", "obstacles"):
        if got[k] is not None:
            assert got[k].dtype == np.uint8 and got[k].shape == ref[k].shape, (what, k)
            bad = np.argwhere(got[k] != ref[k])
            assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist())
    assert got["centre"] == ref["centre"], (what, got["centre"], ref["centre"])
    assert got["tip"] == ref["tip"], (what, got["tip"], ref["tip"])
    assert got["valid"] == ref["valid"], (what, got["valid"], ref["valid"])


def _disp(shape, seed=0):
    """A disparity with zeros in it (a centre that lands on one has no tip)."""
    rng = np.random.default_rng(900 + seed + shape[0])
    d = rng.integers(1, 256, shape).astype(np.uint8)
    d[rng.random(shape) < 0.1] = 0
    return d


# ---- the host entry: every case at the small shapes --------------------------------------------------------------
_REF = {}


def _ref(shape, name):
    """The oracle's answer for one case, computed once and shared (left unchanged by its users)."""
    if (shape, name) not in _REF:
        img, disp = hn.cases(*shape)[name], _disp(shape)
        _REF[(shape, name)] = (img, disp, hn.obstacles(img, disp, ABC))
    return _REF[(shape, name)]


CASES = tuple(hn.cases(40, 70))
SMALL = [(40, 70), (64, 96), (390, 889)]


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_cases(sv, shape):
    """40 x 70: W % 32 != 0, three words a row; 64 x 96; 390 x 889: the odd shape of the clean-up's tests (28 words,
    the 16-byte path; its last word partly filled)."""
    for name in CASES:
        img, disp, ref = _ref(shape, name)
        got = sv.dropin.road_obstacles(img, disp, ABC)
        same(got, ref, (shape, name))
        assert len(ref["hull"]) == {"empty": 0, "one_pixel": 1, "one_row": 2, "one_column": 2, "diagonal_2_3": 2,
                                    "full": 4, "corners": 4, "triangle": 3, "rectangle": 4}.get(name, len(ref["hull"]))
    assert _ref(shape, "corners")[2]["hull"].reshape(-1, 2).tolist()[2] == [shape[1] - 1, shape[0] - 1]
    assert len(_ref(shape, "steep_shallow")[2]["hull"]) == 8 and len(_ref(shape, "sparse")[2]["hull"]) >= 5


def test_host_entry_544x1024(sv):
    """The reference's shape, three frames: 32 words a row."""
    for name in ("sparse", "steep_shallow", "two_blobs"):
        img, disp, ref = _ref((544, 1024), name)
        same(sv.dropin.road_obstacles(img, disp, ABC), ref, name)


def test_non_zero_is_road_and_no_disparity_no_tip(sv):
    img, disp, ref = _ref((40, 70), "steep_shallow")
    got = sv.dropin.road_obstacles((img != 0).astype(np.uint8) * 7)          # any non-zero value is road
    assert got["tip"] is None and got["valid"] == 1 and got["centre"] == ref["centre"]
    assert np.array_equal(got["obstacles"], ref["obstacles"]) and got["hull"].tolist() == ref["hull"].tolist()
    assert sv.dropin.road_obstacles(img, disp)["tip"] is None               # no plane
    assert sv.dropin.road_obstacles(img, None, ABC)["tip"] is None          # no disparity
    zero = disp.copy()
    zero[ref["centre"][1], ref["centre"][0]] = 0                            # d == 0 under the centre
    assert sv.dropin.road_obstacles(img, zero, ABC)["valid"] == 1
    one = disp.copy()
    one[ref["centre"][1], ref["centre"][0]] = 9
    got = sv.dropin.road_obstacles(img, one, ABC)
    assert got["valid"] == 3 and got["tip"] == hn.tip(ref["centre"], ABC, one)
    assert sv.dropin.road_obstacles(img, one, (0.0, 0.0, 0.0))["valid"] == 1   # a zero plane: int(inf) raises


def test_glyph_tip_against_the_reference_fixtures(sv):
    """A one-pixel road at the fixture's centre: the centre is that pixel, the tip what the reference's own
    getNormalVectorLine returned (tests/golden/hull_glyph.json)."""
    with open(os.path.join(GOLDEN, "hull_glyph.json")) as fh:
        g = json.load(fh)
    H, W = g["shape"]
    for c in g["cases"]:
        cx, cy = c["centre"]
        img = np.zeros((H, W), np.uint8)
        img[cy, cx] = 255
        disp = np.zeros((H, W), np.uint8)
        disp[cy, cx] = c["d"]
        got = sv.dropin.road_obstacles(img, disp, c["abc"], camera=g["camera"])
        assert got["centre"] == (cx, cy) and got["hull"].tolist() == [[[cx, cy]]]
        if c["tip"] == "raises":
            assert got["tip"] is None and got["valid"] == 1, c
        else:
            assert got["tip"] == tuple(c["tip"]) and got["valid"] == 3, (c, got["tip"])


def test_arguments_and_capacity(sv):
    abi, dropin = sv.abi, sv.dropin
    with pytest.raises(sv.svx.SvxError):
        dropin.road_obstacles(np.zeros((4, 1), np.uint8))          # W < 2
    with pytest.raises(sv.svx.SvxError):
        dropin.road_obstacles(np.zeros((2, 4097), np.uint8))       # W > 4096
    with pytest.raises(sv.svx.SvxError):
        dropin.road_obstacles(np.zeros((4097, 2), np.uint8))       # H > 4096
    with pytest.raises(ValueError):
        dropin.road_obstacles(np.zeros((4, 8), np.uint8), np.zeros((4, 9), np.uint8))
    with pytest.raises(TypeError):
        dropin.road_obstacles(np.zeros((4, 8), np.float32))
    # SV_E_CAP (-3) when the vertices do not fit; info->n says how many there are
    import ctypes
    img = hn.cases(40, 70)["steep_shallow"]
    cam = abi.Camera(*hn.CAMERA)
    info = abi.HullInfo()
    pts = np.full((8, 2), -7, np.int32)
    rc = abi.lib().sv_road_obstacles(abi.ptr(img), None, None, 40, 70, ctypes.byref(cam), abi.ptr(pts), 7, None, None,
                                     ctypes.byref(info))
    assert rc == -3 and info.n == 8 and (pts == -7).all()
    rc = abi.lib().sv_road_obstacles(abi.ptr(img), None, None, 40, 70, ctypes.byref(cam), abi.ptr(pts), 8, None, None,
                                     ctypes.byref(info))
    assert rc == 0 and pts.tolist() == hn.hull(img).tolist()
    rc = abi.lib().sv_road_obstacles(abi.ptr(img), None, None, 40, 70, ctypes.byref(cam), None, 0, None, None,
                                     ctypes.byref(info))
    assert rc == 0 and info.n == 8                                  # no vertices asked for: no capacity needed


# ---- the batch path --------------------------------------------------------------------------------------------
def _blocks(H, W, *blocks):
    a = np.zeros((H, W), np.uint8)
    for y0, y1, x0, x1 in blocks:
        a[y0:y1, x0:x1] = 200
    return a


def _five_frames(H, W):
    """Disparities whose road images differ: full, empty, full (an empty frame between two full ones), two blobs,
    a filled ring with steep and shallow sides. The pipeline below keeps every grid point with d > 0."""
    ring = (hn.fill_polygon((H, W), hn.polygon_steep_shallow(H, W)) != 0).astype(np.uint8) * 200
    return [np.full((H, W), 200, np.uint8), np.zeros((H, W), np.uint8), np.full((H, W), 200, np.uint8),
            _blocks(H, W, (2, 2 + H // 3, 5, 5 + W // 4), (H - 4 - H // 3, H - 4, W - 9 - W // 3, W - 9)), ring]


def _run_batch(sv, H, W, mode, bits, frames_disp):
    bgr = np.full((H, W, 3), 90, np.uint8)
    n = len(frames_disp)
    with sv.batch.Batch(n, H, W, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode(mode)
        b.road_bits(bits)
        for f, d in enumerate(frames_disp):
            b.upload(f, d, bgr)
        plane = (0.0, 0.0, 0.01)
        b.pipeline(plane=plane, point_thr=1e9, hist_thr=2)
        b.road_raster()
        with pytest.raises(sv.svx.SvxError):       # SV_E_STATE: no clean-up yet
            b.road_hull()
        b.road_clean()
        with pytest.raises(sv.svx.SvxError):       # ... and no hull yet
            b.read_road_hull(0)
        b.road_hull()
        assert b.road_hull_ms() > 0
        counts = []
        for f in range(n):
            raw = b.read_road(f)
            cleaned = b.read_road_clean(f)
            assert np.array_equal(cleaned, mn.sanitise(raw)), f
            disp = b.read_disp(f)
            assert np.array_equal(disp, frames_disp[f])
            ref = hn.obstacles(cleaned, disp, plane)
            got = b.read_road_hull(f)
            same(got, ref, (H, W, mode, f))
            same(sv.dropin.road_obstacles(cleaned, disp, plane), got, ("host entry", H, W, f))   # the two entries agree
            lean = b.read_road_hull(f, images=False)
            assert lean["hull_mask"] is None and lean["hull"].tolist() == got["hull"].tolist()
            counts.append(len(got["hull"]))
        b.road_clean()                              # a new clean-up: the hull is no longer current
        with pytest.raises(sv.svx.SvxError):
            b.read_road_hull(0)
        b.road_hull()
        same(b.read_road_hull(n - 1, images=False), hn.obstacles(b.read_road_clean(n - 1), b.read_disp(n - 1), plane),
             "again")
        b.pipeline(plane=plane, point_thr=1e9, hist_thr=2)   # new points: SV_E_STATE again
        with pytest.raises(sv.svx.SvxError):
            b.road_hull()
        with pytest.raises(sv.svx.SvxError):
            b.read_road_hull(0)
        with pytest.raises(sv.svx.SvxError):
            b.road_hull_ms()
    return counts


def test_batch_five_frames_do_not_leak(sv):
    """72 x 1024 from the pipeline's bitmap, frame by frame: an empty frame between two full ones."""
    counts = _run_batch(sv, 72, 1024, "resident", True, _five_frames(72, 1024))
    assert counts[0] == 4 and counts[1] == 0 and counts[2] == 4 and counts[3] >= 5 and counts[4] >= 3, counts


def test_batch_390x889(sv):
    """W % 32 != 0 at a row stride of 896: packed road images, 28 words a row."""
    counts = _run_batch(sv, 390, 889, "auto", False, _five_frames(390, 889)[1:])
    assert counts[0] == 0 and counts[1] == 4, counts


def test_batch_544x1024_three_frames(sv):
    fr = _five_frames(544, 1024)
    counts = _run_batch(sv, 544, 1024, "resident", True, [fr[4], fr[1], fr[3]])
    assert counts[0] >= 3 and counts[1] == 0 and counts[2] >= 5, counts


def test_batch_read_capacity(sv):
    import ctypes
    H, W = 72, 1024
    with sv.batch.Batch(1, H, W, step=1, with_bgr=True, with_points=True) as b:
        b.upload(0, np.full((H, W), 200, np.uint8), np.full((H, W, 3), 90, np.uint8))
        b.pipeline(plane=(0.0, 0.0, 0.01), point_thr=1e9, hist_thr=2)
        b.road_raster()
        b.road_clean()
        b.road_hull()
        info = sv.abi.HullInfo()
        pts = np.full((4, 2), -7, np.int32)
        rc = sv.abi.lib().sv_batch_read_road_hull(b._h, 0, sv.abi.ptr(pts), 3, None, None, ctypes.byref(info))
        assert rc == -3 and info.n == 4 and (pts == -7).all()
        rc = sv.abi.lib().sv_batch_read_road_hull(b._h, 0, sv.abi.ptr(pts), 4, None, None, None)
        assert rc == 0 and pts.tolist() == hn.hull(b.read_road_clean(0)).tolist()


# ---- the frame loop --------------------------------------------------------------------------------------------
def test_frame_loop_obstacles(sv):
    """road="obstacles" on two small batches in flight, against the oracle chain morph_numpy -> hull_numpy; the
    glyph tip takes each frame's own RANSAC plane and the batch's cleaned disparity."""
    from svx.loop import STAGES, FrameLoop
    frames = 2
    seen = []
    with FrameLoop(frames, slots=2, source="synth", road="obstacles") as loop:
        def verify(seq):
            b, first = loop.batch(seq)
            for f in range(frames):
                ref_clean = mn.sanitise(b.read_road(f))
                assert np.array_equal(b.read_road_clean(f), ref_clean), (seq, f)
                pl = b.read_frame_plane(f)
                abc = tuple(pl[:3]) if pl[3] >= 0 else None
                ref = hn.obstacles(ref_clean, b.read_disp(f), abc)
                got = b.read_road_hull(f)
                same(got, ref, (seq, f))
                seen.append((len(got["hull"]), got["valid"]))
        s0 = loop.submit(0)
        s1 = loop.submit(frames)
        verify(s0)
        verify(s1)
        tl = loop.timeline(s1)
        assert tuple(tl) == STAGES and tl["road"][0] <= tl["road"][1]
    assert len(seen) == 2 * frames and max(n for n, _ in seen) >= 3 and any(v == 3 for _, v in seen), seen
    with FrameLoop(frames, slots=2, source="synth", road="clean") as loop:   # road = 3 runs no obstacle stage
        b, _ = loop.batch(loop.submit(0))
        assert b.read_road_clean(0).shape == (544, 1024)
        with pytest.raises(sv.svx.SvxError):
            b.read_road_hull(0)


# ---- the drop-ins ----------------------------------------------------------------------------------------------
def test_dropin_get_centre_point(sv):
    dropin = sv.dropin

    def orig(points):
        return "original"
    m = types.SimpleNamespace(getCenterPoint=orig)
    assert dropin.HULL == ("getCenterPoint",) and "getCenterPoint" not in dropin.PATCHED
    dropin.install(m)
    try:
        assert m.getCenterPoint is orig             # not without the flag
    finally:
        dropin.uninstall()
    dropin.install(m, hull=True)
    try:
        assert m.getCenterPoint is dropin.getCenterPoint
        for shape in ((40, 70), (390, 889)):
            for name in ("steep_shallow", "sparse", "rectangle", "one_pixel", "diagonal_2_3"):
                _, _, ref = _ref(shape, name)
                c = m.getCenterPoint(ref["hull"])                       # cv2.convexHull's (n, 1, 2)
                assert c == ref["centre"] and all(type(v) is int for v in c), (shape, name)
        # any integer points: inner ones, duplicates, collinear triples, negative coordinates
        rng = np.random.default_rng(8)
        for n in (1, 2, 3, 9, 25):
            pts = rng.integers(-40, 41, (n, 2))
            assert m.getCenterPoint(pts) == hn.centre(pts), pts.tolist()
        assert m.getCenterPoint(np.array([[0, 0], [-3, -5]])) == (-1, -2)   # truncated toward zero
        with pytest.raises(ValueError):
            m.getCenterPoint(np.array([[0, 0], [20000, 1]]))
        with pytest.raises(TypeError):
            m.getCenterPoint(np.zeros((0, 2), np.int32))
        with pytest.raises(ValueError):             # a hull, not a cloud: one lane computes the circle
            m.getCenterPoint(np.stack([np.arange(8193), np.arange(8193) % 7], 1))
        many = np.repeat(np.array([[3, 4], [9, 4], [6, 9]]), 5000, axis=0)   # duplicates do not count
        assert m.getCenterPoint(many) == hn.centre(many[::5000])
    finally:
        dropin.uninstall()
    assert m.getCenterPoint is orig
