"""GPU: the ground grid (include/svx.h, sv_ground_grid) — kernels/ground.hip behind sv_ground_grid, the batch path
(Batch.ground_grid) and svx.dropin.ground_grid — exact against the oracle tests/ground_numpy.py (pinned by
tests/test_ground_cpu.py): both planes, the nearest profile and the four totals."""
import ctypes
import types

import numpy as np
import pytest

import ground_numpy as gn
import objects_numpy as on
from test_gpu_objects import _chain

pytestmark = pytest.mark.gpu

CAMS = gn.cameras()
KEYS = ("obst", "road", "nearest", "info")


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import _abi, batch, dropin
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, abi=_abi, batch=batch, dropin=dropin)


def same(got, ref, what):
    """The four arrays from the device against the oracle's: values, shapes and types."""
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        if not np.array_equal(got[k], ref[k]):
            bad = np.flatnonzero(got[k].ravel() != ref[k].ravel())
            raise AssertionError((what, k, len(bad), bad[:8], got[k].ravel()[bad[:8]], ref[k].ravel()[bad[:8]]))


def _disp(shape):
    """A disparity with zeros, odd and even values."""
    rng = np.random.default_rng(900 + shape[0] + shape[1])
    d = rng.integers(1, 256, shape).astype(np.uint8)
    d[rng.random(shape) < 0.2] = 0
    return d


def _runs_disp(shape):
    """Piecewise constant along the rows, in runs of 1 to 40 pixels that ignore the word boundaries, with zero runs:
    what the run aggregation is made for."""
    rng = np.random.default_rng(77 + shape[1])
    flat = np.zeros(shape[0] * shape[1], np.uint8)
    i = 0
    while i < len(flat):
        n = int(rng.integers(1, 41))
        flat[i:i + n] = 0 if rng.random() < 0.15 else rng.integers(1, 256)
        i += n
    return flat.reshape(shape)


# ---- the host entry on patterns ---------------------------------------------------------------------------------
SHAPES = [(1, 2), (1, 70), (40, 33), (40, 70), (45, 64), (9, 4096)]


def _road_for(cases, name):
    """Another pattern with the obstacle pixels removed (any non-zero value counts)."""
    names = sorted(cases)
    other = cases[names[(names.index(name) + 3) % len(names)]]
    return ((other != 0) & (cases[name] == 0)).astype(np.uint8) * 7


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_patterns(sv, shape):
    cases = on.cases(*shape)
    disp = _disp(shape)
    runs = _runs_disp(shape)
    # a camera whose centre lies in the frame, so that the small shapes spread over the default grid's columns too
    mid = (399.9745178222656, 0.2090607502, shape[1] / 2 - 0.25, 262.0)
    for name, img in cases.items():
        road = _road_for(cases, name)
        for cam in (gn.DEFAULT_CAMERA, mid):
            for d in (disp, runs):
                got = sv.dropin.ground_grid(img, d, road=road, camera=cam)
                same(got, gn.ground_grid(img, d, road, cam), (shape, name, cam[2]))
    full, checker = cases["full"], cases["checkerboard"]
    r = sv.dropin.ground_grid(full, runs, road=None, camera=mid)
    same(r, gn.ground_grid(full, runs, None, mid), (shape, "road=None"))
    assert int(r["info"][:3].sum()) == shape[0] * shape[1] and not r["road"].any() and r["info"][3] == 0
    r = sv.dropin.ground_grid(cases["empty"], disp, road=full, camera=mid)
    assert not r["obst"].any() and (r["nearest"] == -1).all() and list(r["info"][:3]) == [0, 0, 0]
    assert r["info"][3] == r["road"].sum() > 0
    # every grid at every camera
    road = _road_for(cases, "checkerboard")
    for gname, grid in gn.GRIDS.items():
        for cname, cam in CAMS.items():
            got = sv.dropin.ground_grid(checker, disp, road=road, camera=cam, grid=grid)
            same(got, gn.ground_grid(checker, disp, road, cam, grid), (shape, gname, cname))
        # a constant disparity: every pixel of a row segment in one cell, the heaviest collisions; and no depth at all
        const = np.full(shape, 100, np.uint8)
        same(sv.dropin.ground_grid(full, const, road=None, grid=grid, camera=mid),
             gn.ground_grid(full, const, None, mid, grid), (shape, gname, "d = 100"))
        zero = np.zeros(shape, np.uint8)
        r = sv.dropin.ground_grid(full, zero, road=full, grid=grid)
        same(r, gn.ground_grid(full, zero, full, gn.DEFAULT_CAMERA, grid), (shape, gname, "d = 0"))
        assert list(r["info"]) == [0, 0, shape[0] * shape[1], 0] and (r["nearest"] == -1).all()


def test_wide_grid_is_populated(sv):
    """8192 x 1 and 1 x 8192 cells with pixels in them (the cell cap: 64 KB of planes in LDS)."""
    full = np.full((45, 1024), 255, np.uint8)
    const = np.full((45, 1024), 100, np.uint8)
    r = sv.dropin.ground_grid(full, const, road=full, grid=gn.GRIDS["wide"])
    same(r, gn.ground_grid(full, const, full, gn.DEFAULT_CAMERA, gn.GRIDS["wide"]), "wide")
    assert r["info"][0] == 45 * 1024 and (r["obst"] > 0).sum() > 200 and np.array_equal(r["obst"], r["road"])
    ramp = np.broadcast_to((np.arange(1024) % 255 + 1).astype(np.uint8), (45, 1024))
    r = sv.dropin.ground_grid(full, ramp, grid=gn.GRIDS["tall"])
    same(r, gn.ground_grid(full, ramp, None, gn.DEFAULT_CAMERA, gn.GRIDS["tall"]), "tall")
    assert r["info"][0] > 0 and r["nearest"][0] >= 0


def test_count_above_16_bits(sv):
    full = np.full((65, 1024), 255, np.uint8)
    disp = np.full((65, 1024), 100, np.uint8)
    grid = (-500.0, -500.0, 1000.0, 1, 1)
    r = sv.dropin.ground_grid(full, disp, road=full, grid=grid)
    assert r["obst"][0, 0] == 66560 and r["road"][0, 0] == 66560 and list(r["info"]) == [66560, 0, 0, 66560]
    assert list(r["nearest"]) == [0]
    same(r, gn.ground_grid(full, disp, full, gn.DEFAULT_CAMERA, grid), "66560")


def test_nearest_min_count(sv):
    shape = (40, 70)
    cases = on.cases(*shape)
    cam = (399.9745178222656, 0.2090607502, 34.75, 262.0)
    disp = _runs_disp(shape)
    img = cases["checkerboard"]
    profiles = []
    for min_count in (1, 2, 5, 40, 10 ** 6):
        got = sv.dropin.ground_grid(img, disp, camera=cam, min_count=min_count)
        same(got, gn.ground_grid(img, disp, None, cam, gn.DEFAULT_GRID, min_count), ("min_count", min_count))
        profiles.append(got["nearest"])
    assert (profiles[0] >= 0).sum() > (profiles[2] >= 0).sum() > 0      # some columns go, some stay
    assert (profiles[-1] == -1).all()
    keep = profiles[2] >= 0
    assert (profiles[2][keep] >= profiles[0][keep]).all()
    # exactly the count, and one above it
    one = np.zeros(shape, np.uint8)
    one[0:3, 35] = 255
    d = np.full(shape, 100, np.uint8)
    at = sv.dropin.ground_grid(one, d, camera=cam, min_count=3)
    above = sv.dropin.ground_grid(one, d, camera=cam, min_count=4)
    assert at["obst"].max() == 3 and (at["nearest"] >= 0).sum() == 1 and (above["nearest"] == -1).all()


def test_outputs_are_written_whole_and_road_out_is_optional(sv):
    shape = (40, 70)
    cases = on.cases(*shape)
    img, road, disp = cases["rings"], _road_for(cases, "rings"), _disp(shape)
    cam = sv.abi.Camera(*CAMS["near_int"])
    for gname in ("default", "one", "tall", "out"):
        grid = gn.GRIDS[gname]
        g = sv.abi.as_grid(grid)
        ref = gn.ground_grid(img, disp, road, CAMS["near_int"], grid)
        for with_road_out in (True, False):
            obst = np.full((g.nz, g.nx), 0xA5A5A5A5, np.uint32)
            rout = np.full((g.nz, g.nx), 0xA5A5A5A5, np.uint32)
            nearest = np.full(g.nx, 0xA5A5A5A5, np.uint32).view(np.int32)
            info = np.full(4, 0xA5A5A5A5, np.uint32).view(np.int32)
            sv.abi.call("sv_ground_grid", sv.abi.ptr(img), sv.abi.ptr(road), sv.abi.ptr(disp), 40, 70,
                        ctypes.byref(cam), ctypes.byref(g), 1, sv.abi.ptr(obst),
                        sv.abi.ptr(rout) if with_road_out else None, sv.abi.ptr(nearest), sv.abi.ptr(info))
            want_road = ref["road"] if with_road_out else np.full((g.nz, g.nx), 0xA5A5A5A5, np.uint32)
            same({"obst": obst, "road": rout, "nearest": nearest, "info": info}, dict(ref, road=want_road),
                 (gname, with_road_out))
    # a null grid is the default
    obst = np.full((128, 64), 0xA5A5A5A5, np.uint32)
    nearest = np.zeros(64, np.int32)
    info = np.zeros(4, np.int32)
    sv.abi.call("sv_ground_grid", sv.abi.ptr(img), None, sv.abi.ptr(disp), 40, 70, ctypes.byref(cam), None, 1,
                sv.abi.ptr(obst), None, sv.abi.ptr(nearest), sv.abi.ptr(info))
    ref = gn.ground_grid(img, disp, None, CAMS["near_int"])
    assert np.array_equal(obst, ref["obst"]) and np.array_equal(nearest, ref["nearest"])
    assert np.array_equal(info, ref["info"])


def test_argument_errors(sv):
    """Each is SV_E_ARG, raised before anything is launched."""
    img = np.zeros((40, 70), np.uint8)
    obst = np.zeros((128, 64), np.uint32)
    nearest = np.zeros(64, np.int32)
    info = np.zeros(4, np.int32)
    cam = sv.abi.Camera(*gn.DEFAULT_CAMERA)

    def call(ob=img, dp=img, c=cam, grid=None, min_count=1, o=obst, n=nearest, i=info, H=40, W=70):
        return sv.abi.call("sv_ground_grid", sv.abi.ptr(ob), None, sv.abi.ptr(dp), H, W,
                           ctypes.byref(c) if c is not None else None,
                           ctypes.byref(grid) if grid is not None else None, min_count, sv.abi.ptr(o), None,
                           sv.abi.ptr(n), sv.abi.ptr(i))
    assert call() == 0
    for kw in ({"ob": None}, {"dp": None}, {"c": None}, {"o": None}, {"n": None}, {"i": None},          # null pointers
               {"min_count": 0}, {"min_count": -3}, {"H": 0}, {"H": 4097}, {"W": 1}, {"W": 4097}):
        with pytest.raises(sv.svx.SvxError, match=r"\(-1\)"):
            call(**kw)
    nan, inf = float("nan"), float("inf")
    for grid in ((-8, 0, 0.25, 8193, 1), (-8, 0, 0.25, 1, 8193), (-8, 0, 0.25, 128, 65), (-8, 0, 0.25, 0, 1),
                 (-8, 0, 0.25, 1, 0), (-8, 0, 0.25, -1, -1), (-8, 0, 0.0, 64, 128), (-8, 0, -0.25, 64, 128),
                 (-8, 0, nan, 64, 128), (-8, 0, inf, 64, 128), (nan, 0, 0.25, 64, 128), (-8, inf, 0.25, 64, 128)):
        with pytest.raises(sv.svx.SvxError, match=r"\(-1\)"):
            sv.dropin.ground_grid(img, img, grid=grid)
    for camera in ((0.0, 0.2, 474.5, 262.0), (-400.0, 0.2, 474.5, 262.0), (nan, 0.2, 474.5, 262.0),
                   (inf, 0.2, 474.5, 262.0), (400.0, 0.0, 474.5, 262.0), (400.0, -0.2, 474.5, 262.0),
                   (400.0, nan, 474.5, 262.0), (400.0, inf, 474.5, 262.0)):
        with pytest.raises(sv.svx.SvxError, match=r"\(-1\)"):
            sv.dropin.ground_grid(img, img, camera=camera)
    with pytest.raises(sv.svx.SvxError, match=r"\(-1\)"):
        sv.dropin.ground_grid(np.zeros((4, 1), np.uint8), np.zeros((4, 1), np.uint8))           # W = 1
    with pytest.raises(sv.svx.SvxError, match=r"\(-1\)"):
        sv.dropin.ground_grid(np.zeros((4097, 2), np.uint8), np.zeros((4097, 2), np.uint8))     # H = 4097
    with pytest.raises(ValueError):
        sv.dropin.ground_grid(img, np.zeros((40, 71), np.uint8))
    with pytest.raises(ValueError):
        sv.dropin.ground_grid(img, img, road=np.zeros((41, 70), np.uint8))


# ---- the batch, through the real chain --------------------------------------------------------------------------
def _run_batch(sv, H, W, mode, bits, frames_disp, cam_name):
    bgr = np.full((H, W, 3), 90, np.uint8)
    n = len(frames_disp)
    cam_t = CAMS[cam_name]
    cam = sv.abi.Camera(*cam_t)
    E_STATE, E_ARG = r"\(-4\)", r"\(-1\)"
    fine = gn.GRIDS["fine"]
    with sv.batch.Batch(n, H, W, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode(mode)
        b.road_bits(bits)
        for f, d in enumerate(frames_disp):
            b.upload(f, d, bgr)
        _chain(b)
        with pytest.raises(sv.svx.SvxError, match=E_STATE):      # no obstacle stage yet
            b.ground_grid()
        b.road_hull()
        for call in (lambda: b.read_ground_grid(0), b.read_ground_nearest, b.ground_grid_ms):   # ... and no grid yet
            with pytest.raises(sv.svx.SvxError, match=E_STATE):
                call()
        for kw in ({"min_count": 0}, {"grid": (-8, 0, 0.25, 8193, 1)}, {"grid": (-8, 0, 0.0, 64, 128)},
                   {"camera": sv.abi.Camera(0.0, 0.2, 474.5, 262.0)}):
            with pytest.raises(sv.svx.SvxError, match=E_ARG):
                b.ground_grid(**kw)
        b.ground_grid(camera=cam)
        assert b.ground_grid_ms() > 0
        got_all = []
        for f in range(n):
            obst = b.read_road_hull(f)["obstacles"]
            road = b.read_road_clean(f)
            disp = b.read_disp(f)
            assert np.array_equal(disp, frames_disp[f])
            ref = gn.ground_grid(obst, disp, road, cam_t)
            got = b.read_ground_grid(f)
            same(got, ref, (H, W, f))
            same(sv.dropin.ground_grid(obst, disp, road=road, camera=cam_t), ref, ("host entry", H, W, f))
            assert int(ref["info"][:3].sum()) == int((obst != 0).sum())
            if not frames_disp[f].any():                          # the empty frame
                assert not got["obst"].any() and not got["road"].any() and (got["nearest"] == -1).all()
                assert not got["info"].any()
            else:
                assert got["info"][3] > 0 and got["info"][:3].sum() > 0
            got_all.append(got)
        profile = b.read_ground_nearest()
        assert profile.shape == (n, 64) and profile.dtype == np.int32
        assert np.array_equal(profile, np.stack([g["nearest"] for g in got_all]))
        b.obstacle_list()                                         # the list and the grid leave each other alone
        lst = b.read_obstacle_list(0)
        same(b.read_ground_grid(0), got_all[0], "after obstacle_list")
        b.ground_grid(grid=fine, min_count=3, camera=cam, sync=False)   # another grid, read without an explicit sync
        f = n - 1
        obst, road, disp = b.read_road_hull(f)["obstacles"], b.read_road_clean(f), b.read_disp(f)
        ref = gn.ground_grid(obst, disp, road, cam_t, fine, 3)
        same(b.read_ground_grid(f), ref, "fine, min_count 3")
        assert np.array_equal(b.read_ground_nearest()[f], ref["nearest"]) and b.ground_grid_ms() > 0
        again = b.read_obstacle_list(0)
        assert again[0] == lst[0] and np.array_equal(again[1], lst[1])
        b.result()                                                # later stages leave the grid alone
        same(b.read_ground_grid(f), ref, "after result")
        b.road_clean()                                            # a new clean-up: no hull, no grid
        for call in (lambda: b.read_ground_grid(0), b.read_ground_nearest, b.ground_grid_ms, b.ground_grid):
            with pytest.raises(sv.svx.SvxError, match=E_STATE):
                call()
        b.road_hull()                                             # a new hull: the old grid is not its grid
        for call in (lambda: b.read_ground_grid(0), b.read_ground_nearest, b.ground_grid_ms):
            with pytest.raises(sv.svx.SvxError, match=E_STATE):
                call()
        b.ground_grid(camera=cam)
        same(b.read_ground_grid(0), got_all[0], "again")
        b.pipeline(plane=(0.0, 0.0, 0.01), point_thr=1e9, hist_thr=2)   # new points
        for call in (lambda: b.read_ground_grid(0), b.read_ground_nearest, b.ground_grid_ms, b.ground_grid):
            with pytest.raises(sv.svx.SvxError, match=E_STATE):
                call()
        b.road_raster()
        b.road_clean()
        b.road_hull()
        with pytest.raises(sv.svx.SvxError, match=E_STATE):
            b.read_ground_grid(0)
        b.ground_grid(camera=cam)
        same(b.read_ground_grid(n - 1), got_all[n - 1], "after a new pipeline")
        assert b.ground_grid_ms() > 0
    return got_all


def test_batch_72x1024(sv):
    """From the pipeline's bitmap: the holed road, an empty frame, the holed road again, two blobs."""
    got = _run_batch(sv, 72, 1024, "resident", True, on.batch_frames(72, 1024), "default")
    same(got[0], got[2], "equal frames")


def test_batch_390x889(sv):
    """W % 32 != 0 at a row stride of 896: 28 words a row; a camera other than the default."""
    got = _run_batch(sv, 390, 889, "auto", False, on.batch_frames(390, 889), "rig2")
    same(got[0], got[2], "equal frames")


def test_batch_544x1024_three_frames(sv):
    fr = on.batch_frames(544, 1024)
    _run_batch(sv, 544, 1024, "resident", True, [fr[0], fr[1], fr[3]], "default")
