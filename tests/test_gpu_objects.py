"""GPU: the obstacle list (include/svx.h, sv_obstacle_list) — kernels/objects.hip behind sv_obstacle_list, the batch
path (Batch.obstacle_list) and svx.dropin.obstacle_list — exact against the oracle tests/objects_numpy.py (pinned by
tests/test_objects_cpu.py): the count, the list's order and every field of every entry."""
import ctypes
import types

import numpy as np
import pytest

import objects_numpy as on

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import _abi, batch, dropin
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, abi=_abi, batch=batch, dropin=dropin)


def same(got, ref, what):
    """(n, entries) from the device against the oracle's."""
    assert got[0] == ref[0], (what, got[0], ref[0])
    g = on.as_dicts(got[1])
    assert len(g) == len(ref[1]), (what, len(g), len(ref[1]))
    for i, (a, b) in enumerate(zip(g, ref[1])):
        assert a == b, (what, i, a, b)


def _disp(shape):
    """A disparity with zeros, odd and even values."""
    rng = np.random.default_rng(700 + shape[0] + shape[1])
    d = rng.integers(1, 256, shape).astype(np.uint8)
    d[rng.random(shape) < 0.2] = 0
    return d


# ---- the host entry on patterns ---------------------------------------------------------------------------------
SHAPES = [(1, 2), (1, 70), (40, 33), (40, 70), (45, 64), (9, 4096)]
_REF = {}


def _ref(shape):
    """The oracle's answers for one shape's patterns, computed once and shared (left unchanged by their users)."""
    if shape not in _REF:
        disp = _disp(shape)
        _REF[shape] = (disp, {name: (img, on.obstacle_list(img, disp, 1, 32)) for name, img in
                              on.cases(*shape).items()})
    return _REF[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_patterns(sv, shape):
    disp, cases = _ref(shape)
    H, W = shape
    for name, (img, ref) in cases.items():
        got = sv.dropin.obstacle_list(img, disp, min_area=1, cap=32)
        same(got, ref, (shape, name))
    assert cases["empty"][1][0] == 0
    n, e = cases["full"][1]
    assert n == 1 and e[0]["area"] == H * W and e[0]["first"] == 0
    # one component under 8-connectivity, with the most runs a row can hold (a single row: every run on its own)
    assert cases["checkerboard"][1][0] == (1 if H > 1 else (W + 1) // 2)
    n, e = cases["stripes"][1]
    assert n == (W + 1) // 2 and all(c["area"] == H for c in e)  # ties in area: ordered by first pixel
    assert [c["first"] for c in e] == list(range(0, 2 * len(e), 2))
    assert cases["comb"][1][0] == 1 and cases["comb_mirror"][1][0] == 1 and cases["serpentine"][1][0] == 1
    if "rings" in cases:
        n, e = cases["rings"][1]
        assert n == 2 and e[0]["x0"] < e[1]["x0"] and e[0]["y0"] < e[1]["y0"] and e[0]["x1"] > e[1]["x1"]


def test_host_entry_any_nonzero_value_and_no_disparity(sv):
    disp, cases = _ref((40, 70))
    img, _ = cases["rings"]
    ref = on.obstacle_list(img, None, 1, 32)
    same(sv.dropin.obstacle_list((img != 0).astype(np.uint8) * 3, None, min_area=1, cap=32), ref, "disp=None")
    assert all(c["nd"] == c["dmax"] == c["dmed"] == 0 for c in ref[1])
    got = sv.dropin.obstacle_list(img, disp)                     # the defaults: min_area 70, cap 16
    same(got, on.obstacle_list(img, disp, 70, 16), "defaults")
    assert got[1].dtype == np.dtype(sv.abi.OBSTACLE_FIELDS) and got[1].dtype.itemsize == 56


def test_host_entry_limits(sv):
    img = on.limit_rectangles()
    full = on.obstacle_list(img, None, 1, 32)
    assert [c["area"] for c in full[1]] == [12, 12, 11, 6, 6, 6, 2, 1]
    for min_area, want in ((1, 8), (6, 6), (7, 3), (12, 2), (13, 0)):   # at the threshold kept, below it dropped
        got = sv.dropin.obstacle_list(img, None, min_area=min_area, cap=32)
        same(got, on.obstacle_list(img, None, min_area, 32), ("min_area", min_area))
        assert got[0] == want
    for cap in (1, 3, 32):                                              # n in full, the list its head
        got = sv.dropin.obstacle_list(img, None, min_area=1, cap=cap)
        same(got, (8, full[1][:cap]), ("cap", cap))
    # entries past the list stay as the caller filled them
    for min_area, cap, n_want in ((1, 3, 8), (12, 32, 2), (13, 32, 0)):
        out = np.full(32 * 56, 0xA5, np.uint8)
        n = ctypes.c_int32(-1)
        sv.abi.call("sv_obstacle_list", sv.abi.ptr(img), None, 40, 70, min_area, sv.abi.ptr(out), cap, ctypes.byref(n))
        length = min(n_want, cap)
        assert n.value == n_want and (out[56 * length:] == 0xA5).all()
        head = out[:56 * length].view(np.dtype(sv.abi.OBSTACLE_FIELDS))
        assert on.as_dicts(head) == full[1][:length] and (head["reserved"] == 0).all()


def test_host_entry_disparity(sv):
    img = np.zeros((40, 70), np.uint8)
    img[3:6, 4:10] = 255          # wholly over d = 0
    img[10:14, 20:50] = 255       # over a ramp with odd and even values
    img[20, 30:34] = 255          # [2, 4, 4, 250]
    img[30:33, 62:66] = 255       # one value under it
    disp = np.zeros((40, 70), np.uint8)
    disp[10:14, 20:50] = (np.arange(30) * 7 + np.arange(4)[:, None] * 3 + 1) % 256
    disp[20, 30:34] = [2, 4, 4, 250]
    disp[31, 63] = 77
    disp[25:28, :] = 201          # under no component
    ref = on.obstacle_list(img, disp, 1, 8)
    same(sv.dropin.obstacle_list(img, disp, min_area=1, cap=8), ref, "disparity")
    by_first = {c["first"]: c for c in ref[1]}
    assert [by_first[3 * 70 + 4][k] for k in ("nd", "dmax", "dmed")] == [0, 0, 0]
    assert [by_first[20 * 70 + 30][k] for k in ("nd", "dmax", "dmed")] == [4, 250, 4]
    assert [by_first[30 * 70 + 62][k] for k in ("nd", "dmax", "dmed")] == [1, 77, 77]
    ramp = by_first[10 * 70 + 20]
    assert ramp["nd"] == 120 and ramp["dmax"] == 213
    cam = (399.9745178222656, 0.2090607502, 474.5, 262.0)
    got = sv.dropin.obstacle_list(img, disp, min_area=1, cap=8)[1]
    for e, r in zip(got, ref[1]):
        assert sv.dropin.obstacle_xyz(e, cam) == on.obstacle_xyz(r, cam)
    assert sum(sv.dropin.obstacle_xyz(e, cam) is None for e in got) == 1


def test_argument_errors(sv):
    """Each is SV_E_ARG, raised before anything is launched."""
    img = np.zeros((40, 70), np.uint8)
    out = np.zeros(32, np.dtype(sv.abi.OBSTACLE_FIELDS))
    n = ctypes.c_int32(0)

    def call(obst, o, cnt):
        return sv.abi.call("sv_obstacle_list", sv.abi.ptr(obst), None, 40, 70, 1, sv.abi.ptr(o), 32, cnt)
    assert call(img, out, ctypes.byref(n)) == 0
    for args in ((None, out, ctypes.byref(n)), (img, None, ctypes.byref(n)), (img, out, None)):   # null pointers
        with pytest.raises(sv.svx.SvxError, match=r"\(-1\)"):
            call(*args)
    for kw in ({"min_area": 0}, {"cap": 0}, {"cap": 33}):
        with pytest.raises(sv.svx.SvxError, match=r"\(-1\)"):
            sv.dropin.obstacle_list(img, None, **kw)
    with pytest.raises(sv.svx.SvxError, match=r"\(-1\)"):
        sv.dropin.obstacle_list(np.zeros((4, 1), np.uint8))           # W = 1
    with pytest.raises(sv.svx.SvxError, match=r"\(-1\)"):
        sv.dropin.obstacle_list(np.zeros((4097, 2), np.uint8))        # H = 4097
    with pytest.raises(sv.svx.SvxError, match=r"\(-1\)"):
        sv.dropin.obstacle_list(np.zeros((2, 4097), np.uint8))
    with pytest.raises(ValueError):
        sv.dropin.obstacle_list(img, np.zeros((40, 71), np.uint8))


# ---- the batch, through the real chain --------------------------------------------------------------------------
PLANE = (0.0, 0.0, 0.01)


def _chain(b):
    b.pipeline(plane=PLANE, point_thr=1e9, hist_thr=2)   # the road image is every pixel with d > 0
    b.road_raster()
    b.road_clean()


def _run_batch(sv, H, W, mode, bits, frames_disp, want):
    bgr = np.full((H, W, 3), 90, np.uint8)
    n = len(frames_disp)
    E_STATE, E_ARG = r"\(-4\)", r"\(-1\)"
    with sv.batch.Batch(n, H, W, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode(mode)
        b.road_bits(bits)
        for f, d in enumerate(frames_disp):
            b.upload(f, d, bgr)
        _chain(b)
        with pytest.raises(sv.svx.SvxError, match=E_STATE):      # no obstacle stage yet
            b.obstacle_list()
        b.road_hull()
        with pytest.raises(sv.svx.SvxError, match=E_STATE):      # ... and no list yet
            b.read_obstacle_list(0)
        with pytest.raises(sv.svx.SvxError, match=E_STATE):
            b.obstacle_list_ms()
        with pytest.raises(sv.svx.SvxError, match=E_ARG):
            b.obstacle_list(min_area=0)
        with pytest.raises(sv.svx.SvxError, match=E_ARG):
            b.obstacle_list(cap=33)
        b.obstacle_list()
        assert b.obstacle_list_ms() > 0
        counts = []
        for f in range(n):
            obst = b.read_road_hull(f)["obstacles"]
            disp = b.read_disp(f)
            assert np.array_equal(disp, frames_disp[f])
            ref = on.obstacle_list(obst, disp, 70, 16)
            got = b.read_obstacle_list(f)
            same(got, ref, (H, W, f))
            same(sv.dropin.obstacle_list(obst, disp), ref, ("host entry", H, W, f))   # the two entries agree
            same(b.read_obstacle_list(f, cap=1), (ref[0], ref[1][:1]), ("head", H, W, f))
            counts.append(got[0])
        assert all(c >= w for c, w in zip(counts, want)) and all(c == 0 for c, w in zip(counts, want) if w == 0), counts
        with pytest.raises(sv.svx.SvxError, match=E_ARG):        # a read above the call's cap
            b.read_obstacle_list(0, cap=17)
        b.obstacle_list(min_area=1, cap=3, sync=False)            # other limits, read without an explicit sync
        f = n - 1
        ref = on.obstacle_list(b.read_road_hull(f)["obstacles"], b.read_disp(f), 1, 3)
        same(b.read_obstacle_list(f), ref, "min_area 1, cap 3")
        with pytest.raises(sv.svx.SvxError, match=E_ARG):
            b.read_obstacle_list(0, cap=4)
        b.result()                                                # later stages leave the list alone
        same(b.read_obstacle_list(f), ref, "after result")
        b.road_clean()                                            # a new clean-up: no hull, no list
        for call in (lambda: b.read_obstacle_list(0), b.obstacle_list_ms, b.obstacle_list):
            with pytest.raises(sv.svx.SvxError, match=E_STATE):
                call()
        b.road_hull()                                             # a new hull: the old list is not its list
        for call in (lambda: b.read_obstacle_list(0), b.obstacle_list_ms):
            with pytest.raises(sv.svx.SvxError, match=E_STATE):
                call()
        b.obstacle_list()
        same(b.read_obstacle_list(0), on.obstacle_list(b.read_road_hull(0)["obstacles"], b.read_disp(0), 70, 16),
             "again")
        b.pipeline(plane=PLANE, point_thr=1e9, hist_thr=2)        # new points
        for call in (lambda: b.read_obstacle_list(0), b.obstacle_list_ms, b.obstacle_list):
            with pytest.raises(sv.svx.SvxError, match=E_STATE):
                call()
        b.road_raster()
        b.road_clean()
        b.road_hull()
        with pytest.raises(sv.svx.SvxError, match=E_STATE):
            b.read_obstacle_list(0)
        b.obstacle_list()
        assert b.read_obstacle_list(0)[0] == counts[0] and b.obstacle_list_ms() > 0
    return counts


def test_batch_72x1024(sv):
    """From the pipeline's bitmap: the holed road, an empty frame, the holed road again, two blobs."""
    counts = _run_batch(sv, 72, 1024, "resident", True, on.batch_frames(72, 1024), (3, 0, 3, 1))
    assert counts[0] == counts[2]


def test_batch_390x889(sv):
    """W % 32 != 0 at a row stride of 896: 28 words a row."""
    counts = _run_batch(sv, 390, 889, "auto", False, on.batch_frames(390, 889), (3, 0, 3, 1))
    assert counts[0] == counts[2]


def test_batch_544x1024_three_frames(sv):
    fr = on.batch_frames(544, 1024)
    _run_batch(sv, 544, 1024, "resident", True, [fr[0], fr[1], fr[3]], (3, 0, 1))
