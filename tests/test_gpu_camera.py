"""Every camera-dependent kernel at cameras other than the reference's own.

The reference's image centre (474.5, 262.0) is exact in fp32, so at the default camera the low words of the
kernels' split centre (KParams::cw_lo / ch_lo, svx_device.h centred()) are zero, the per-device delta-table
cache (runtime.hip ensure_tables / same_cam) is never asked for a second camera, and the chunk-skipping bound
(rows_keepable) only sees the principal point inside the frame. These tests run K1, both drop-in projection
paths, the delta tables, every pipeline kernel family, the table cache, the batched RANSAC with per-frame
planes, the digest kernel and the frame loop at the four cameras of tests/golden/camera_inputs.py, against the
oracle called with the same camera; tests/test_camera_cpu.py pins that oracle to the reference's own run at
these cameras (tests/golden/camera.npz), and near_int is compared with that fixture directly as well.

Tolerances are the suite's: integers, indices, bytes and all fp64 bit-exact; fp32 X, Y, Z within 1e-5
relative, atol = 0. A dropped or mis-signed low word is a 4.5e-3 relative error in X on the grid column next
to a near-integer centre (camera_inputs.py), so those columns and rows are asserted by themselves."""
import functools
import os
import random
import sys
import types

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, sparse_frame
from oracle import ransac as oransac

sys.path.insert(0, GOLDEN)
import camera_inputs as ci  # noqa: E402
from test_gpu_parity import KINDS, RTOL, _check_pipe, _pipe  # noqa: E402
from test_prepass_cpu import carmask  # noqa: E402

pytestmark = pytest.mark.gpu

CAMS = list(ci.CAMERAS)
FIX = np.load(os.path.join(GOLDEN, "camera.npz"))


@pytest.fixture(scope="module")
def svx_mod():
    import svx
    from svx import _abi, batch, dropin
    assert svx.device_count() >= 1
    return types.SimpleNamespace(svx=svx, batch=batch, dropin=dropin, cam=lambda c: _abi.Camera(*c))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _frame(H, W, k=0):
    return ci.frame(H, W, k)


@functools.lru_cache(maxsize=None)
def _ref_pipe(cname, shape, step, pname, k=0):
    """The oracle's chain of frame k of a shape under a named plane (computed once, shared, never written)."""
    cam = ci.CAMERAS[cname] if cname else None
    disp, bgr = _frame(*shape, k)
    abc, pthr, hthr = ci.plane_case(cam or oracle.DEFAULT_CAMERA, pname)
    return oracle.pipeline_frame(disp, bgr, step, camera=cam, abc=np.array(abc), point_thr=pthr, hist_thr=hthr)


def _plane_kw(svx_mod, cname, pname):
    cam = ci.CAMERAS[cname] if cname else oracle.DEFAULT_CAMERA
    abc, pthr, hthr = ci.plane_case(cam, pname)
    return dict(plane=abc, point_thr=pthr, hist_thr=hthr, camera=svx_mod.cam(cam))


def _assert_close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rel = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
    bad = np.flatnonzero(~(rel <= RTOL))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} beyond {RTOL} relative, worst {rel.max():.3g}"


# ---------------------------------------------------------------------------
# a. K1
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tune", [(1, 0), (4, 1)])
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("shape", ci.SHAPES)
@pytest.mark.parametrize("cname", CAMS)
def test_k1_dense(svx_mod, cname, shape, step, tune):
    """K1's dense planes of three uploaded frames: the zero pattern of the oracle's, X, Y and Z within 1e-5; for
    the near-integer cameras the grid column (X) and grid row (Y) next to the centre on their own."""
    cam = ci.CAMERAS[cname]
    H, W = shape
    with svx_mod.batch.Batch(3, H, W, step, with_bgr=False) as b:
        b.tune(*tune)
        for f in range(3):
            b.upload(f, _frame(H, W, f)[0])
        b.project(camera=svx_mod.cam(cam))
        for f in range(3):
            X, Y, Z = b.read_dense(f)
            RX, RY, RZ = oracle.project_dense(_frame(H, W, f)[0], step, camera=cam, pitch=b.pitch)
            wg = b.Wg
            assert X.shape == RX.shape
            assert np.array_equal(Z[:, :wg] == 0, RZ[:, :wg] == 0), (cname, f)
            assert not Z[:, wg:].any()
            valid = RZ[:, :wg] != 0
            if cname in ci.NEAR_GRID:
                gx, gy = (v // step for v in ci.NEAR_GRID[cname])
                assert valid[:, gx].sum() >= 10 and valid[gy].sum() >= 10
                _assert_close(X[:, gx][valid[:, gx]], RX[:, gx][valid[:, gx]], f"{cname} frame {f}: X on the centre column")
                _assert_close(Y[gy, :wg][valid[gy]], RY[gy, :wg][valid[gy]], f"{cname} frame {f}: Y on the centre row")
            for name, a, r in (("X", X, RX), ("Y", Y, RY), ("Z", Z, RZ)):
                _assert_close(a[:, :wg][valid], r[:, :wg][valid], f"{cname} frame {f}: {name}")
                np.testing.assert_allclose(a[:, :wg], r[:, :wg], rtol=RTOL, atol=0)


def test_k1_dense_full_size_rig2(svx_mod):
    """544 x 1024, step 1, two synthetic frames at rig2 (its centre lies inside this frame) through the oracle's
    own checker."""
    cam = ci.CAMERAS["rig2"]
    with svx_mod.batch.Batch(2, step=1, with_bgr=False) as b:
        b.synth(0)
        b.project(camera=svx_mod.cam(cam))
        for f in range(2):
            bad, worst = oracle.check_dense_f32(f, *b.read_dense(f), 1, RTOL, camera=cam)
            assert bad == 0 and worst <= RTOL, (f, bad, worst)


# ---------------------------------------------------------------------------
# b. drop-in projection, both paths
# ---------------------------------------------------------------------------
def _fixture_points(cname, pname):
    """(the fp64 rows whose back-projection the fixture holds, the fixture's int32 plane_points)."""
    r = _ref_pipe(cname, ci.FIXTURE_SHAPE, 2, pname)
    rows = FIX["near_int_xyz"][FIX[f"near_int_{pname}_keep2_idx"]] if cname == "near_int" else r["xyz2"]
    return rows, FIX[f"{cname}_{pname}_plane_points"]


@pytest.mark.parametrize("shape", ci.SHAPES)
@pytest.mark.parametrize("cname", CAMS)
def test_dropin_array_paths(svx_mod, cname, shape):
    """project_frame and project_rows with camera=: X, Y, Z bits and colours of oracle.project (and of the
    reference's own run for near_int)."""
    cam = ci.CAMERAS[cname]
    C = svx_mod.cam(cam)
    disp, bgr = _frame(*shape)
    rxyz, rrgb = oracle.project(disp, bgr, 2, camera=cam)
    if cname == "near_int" and shape == ci.FIXTURE_SHAPE:
        assert np.array_equal(_bits(rxyz), _bits(FIX["near_int_xyz"])) and np.array_equal(rrgb, FIX["near_int_rgb"])
    xyz, rgb = svx_mod.dropin.project_frame(disp, bgr, camera=C)
    assert xyz.shape == rxyz.shape and np.array_equal(_bits(xyz), _bits(rxyz)) and np.array_equal(rgb, rrgb)
    xyz, none = svx_mod.dropin.project_frame(disp, None, camera=C)
    assert none is None and np.array_equal(_bits(xyz), _bits(rxyz))
    rows = svx_mod.dropin.project_rows(disp, bgr, camera=C)
    assert rows.shape == (len(rxyz), 6)
    assert np.array_equal(_bits(rows[:, :3]), _bits(rxyz)) and np.array_equal(rows[:, 3:], rrgb.astype(np.float64))
    rows = svx_mod.dropin.project_rows(disp, None, camera=C)
    assert rows.shape == (len(rxyz), 3) and np.array_equal(_bits(rows), _bits(rxyz))
    for step in (1, 3):
        sxyz, srgb = svx_mod.dropin.project_frame(disp, bgr, step=step, camera=C)
        oxyz, orgb = oracle.project(disp, bgr, step, camera=cam)
        assert np.array_equal(_bits(sxyz), _bits(oxyz)) and np.array_equal(srgb, orgb)


@pytest.mark.parametrize("cname", CAMS)
def test_dropin_installed_module(svx_mod, cname):
    """projectDisparityTo3d / project3DPointsTo2DImagePoints after dropin.install of a module object carrying the
    camera: the rows' bits and colours, the back-projected fp64 bits of oracle.backproject, and the int32 points
    of the reference's own run (camera.npz)."""
    cam = ci.CAMERAS[cname]
    disp, bgr = _frame(*ci.FIXTURE_SHAPE)
    mod = types.SimpleNamespace(camera_focal_length_px=cam[0], stereo_camera_baseline_m=cam[1],
                                image_centre_w=cam[2], image_centre_h=cam[3])
    svx_mod.dropin.install(mod)
    try:
        rxyz, rrgb = oracle.project(disp, bgr, 2, camera=cam)
        pts = mod.projectDisparityTo3d(disp, 128, bgr)
        got = np.array([[v for v in row] for row in pts], np.float64).reshape(-1, 6)
        assert np.array_equal(_bits(got[:, :3]), _bits(rxyz)) and np.array_equal(got[:, 3:], rrgb.astype(np.float64))
        assert type(pts[0][0]) is np.float64 and isinstance(pts[0][3], np.generic)
        mpts = mod.projectDisparityTo3d(disp, 128)
        got = np.array([[v for v in row] for row in mpts], np.float64).reshape(-1, 3)
        assert np.array_equal(_bits(got), _bits(rxyz))
        for pname in ci.FIXTURE_PLANES:
            rows, want = _fixture_points(cname, pname)
            assert len(rows) > 0
            xy = mod.project3DPointsTo2DImagePoints(list(rows))
            assert np.array_equal(_bits(xy), _bits(oracle.backproject(rows, camera=cam)))
            assert np.array_equal(np.array(xy, np.int32).reshape((-1, 1, 2)), want)
        # the device's own rows of the points the reference kept, back again
        src = oracle.project(disp, bgr, 2, camera=cam, with_src=True)[2]
        pos = {tuple(s): i for i, s in enumerate(src.tolist())}
        idx = [pos[tuple(s)] for s in _ref_pipe(cname, ci.FIXTURE_SHAPE, 2, "some")["src2"].tolist()]
        if cname == "near_int":
            assert idx == FIX["near_int_some_keep2_idx"].tolist()
        xy = mod.project3DPointsTo2DImagePoints([pts[i] for i in idx])
        assert np.array_equal(np.array(xy, np.int32).reshape((-1, 1, 2)), FIX[f"{cname}_some_plane_points"])
    finally:
        svx_mod.dropin.uninstall()


# ---------------------------------------------------------------------------
# c. the rows path against reference data at the default camera
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_rows_path_sparse_frames_against_reference(svx_mod, golden, k):
    """projectDisparityTo3d (sv_project_rows) on the reference-run sparse frames: every row's X, Y, Z bits and
    R, G, B equal the reference's, with and without colours, and every element is a numpy scalar."""
    disp, bgr = sparse_frame(golden, k)
    s = golden.sparse
    pts = svx_mod.dropin.projectDisparityTo3d(disp, 128, bgr)
    want_xyz, want_rgb = s[f"f{k}_xyz"], s[f"f{k}_rgb"]
    assert len(pts) == len(want_xyz)
    for i, row in enumerate(pts):
        assert len(row) == 6 and all(isinstance(v, np.generic) for v in row), i
        assert all(type(v) is np.float64 for v in row[:3]), i
        assert np.array_equal(_bits(np.array(row[:3])), _bits(want_xyz[i])), i
        assert [int(v) for v in row[3:6]] == [int(v) for v in want_rgb[i]] and all(v == int(v) for v in row[3:6]), i
    mpts = svx_mod.dropin.projectDisparityTo3d(disp, 128)
    want = s[f"f{k}_mask_xyz"]
    assert len(mpts) == len(want)
    for i, row in enumerate(mpts):
        assert len(row) == 3 and all(type(v) is np.float64 for v in row), i
        assert np.array_equal(_bits(np.array(row[:3])), _bits(want[i])), i


@pytest.mark.parametrize("fid", ["0", "1", "4095"])
def test_rows_path_full_frames_against_reference(svx_mod, golden, fid):
    """The rows path on full synthetic frames: the reference run's digests of XYZ, colours and maskpoints."""
    m = golden.meta["full_frames_step2"][fid]
    disp, bgr = oracle.synth_frame(int(fid))
    rows = svx_mod.dropin.as_points_array(svx_mod.dropin.projectDisparityTo3d(disp, 128, bgr))
    assert rows.shape == (m["n"], 6)
    assert oracle.digest(np.ascontiguousarray(rows[:, :3])) == m["xyz"]
    assert np.array_equal(rows[:, 3:], np.rint(rows[:, 3:])) and rows[:, 3:].min() >= 0 and rows[:, 3:].max() <= 255
    assert oracle.digest(rows[:, 3:].astype(np.uint8)) == m["rgb"]
    mrows = svx_mod.dropin.as_points_array(svx_mod.dropin.projectDisparityTo3d(disp, 128))
    assert mrows.shape == (m["n"], 3) and oracle.digest(mrows) == m["mask_xyz"]


# ---------------------------------------------------------------------------
# d. delta tables
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", CAMS)
def test_delta_tables(svx_mod, cname):
    cam = ci.CAMERAS[cname]
    for H, W in ci.SHAPES:
        dx, dy = svx_mod.batch.delta_tables(H, W, camera=svx_mod.cam(cam))
        rdx, rdy = oracle.delta_tables(H, W, camera=cam)
        assert np.array_equal(dx, rdx) and np.array_equal(dy, rdy), (H, W)
    H, W = ci.FIXTURE_SHAPE   # the deltas measured through the reference's projection and back-projection
    dx, dy = svx_mod.batch.delta_tables(H, W, camera=svx_mod.cam(cam))
    assert np.array_equal(dx.T[0:W - 1:2, 1:], FIX[cname + "_dx_even"][0:W - 1:2, 1:])
    assert np.array_equal(dy.T[0:H - 1:2, 1:], FIX[cname + "_dy_even"][0:H - 1:2, 1:])


# ---------------------------------------------------------------------------
# e. fused pipeline, every kernel family
# ---------------------------------------------------------------------------
def _check_centre_kept(cname, step, got, ref):
    """Under "none_out" every valid point passes keep1: the outputs hold points of the grid column and row next
    to a near-integer centre, checked on their own (X on the column, Y on the row)."""
    if cname not in ci.NEAR_GRID:
        return
    gx, gy = ci.NEAR_GRID[cname]
    col, row = np.flatnonzero(ref["src2"][:, 1] == gx), np.flatnonzero(ref["src2"][:, 0] == gy)
    assert col.size >= 5 and row.size >= 5, (cname, col.size, row.size)
    assert len(got["xyz2"]) == len(ref["xyz2"])
    _assert_close(got["xyz2"][col, 0], ref["xyz2"][col, 0], f"{cname} step {step}: X of the kept centre column")
    _assert_close(got["xyz2"][row, 1], ref["xyz2"][row, 1], f"{cname} step {step}: Y of the kept centre row")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cname", CAMS)
def test_pipeline_one_frame(svx_mod, cname, kind):
    """sv_pipeline_frame and the three resident variants: both steps, both shapes, the four planes."""
    for shape in ci.SHAPES:
        disp, bgr = _frame(*shape)
        for step in (1, 2):
            for pname in ci.PLANES:
                ref = _ref_pipe(cname, shape, step, pname)
                got = _pipe(svx_mod, kind, disp, bgr, step, **_plane_kw(svx_mod, cname, pname))
                try:
                    _check_pipe(got, ref)
                except AssertionError as e:
                    raise AssertionError(f"{cname} {kind} {shape} step {step} plane {pname}: {e}") from None
                if pname == "none_out":
                    assert got["counts"][1] == got["counts"][0] > got["counts"][2] > 0
                    _check_centre_kept(cname, step, got, ref)
                if pname == "all_out":
                    assert got["counts"][0] > 0 and got["counts"][1:] == (0, 0)


@pytest.mark.parametrize("chunk", [1, 3])
@pytest.mark.parametrize("cname", CAMS)
def test_pipeline_tiled_batch(svx_mod, cname, chunk):
    """Batch in "tiled" mode over five frames, chunks of 1 and 3 frames (a chunk boundary is crossed), and the
    digest kernel's summary of the same outputs against oracle.digest_frame, column by column (72 x 152: the
    digests take H * W a multiple of 4)."""
    cam = ci.CAMERAS[cname]
    for shape in ci.SHAPES:
        H, W = shape
        for step in (1, 2):
            with svx_mod.batch.Batch(5, H, W, step, with_bgr=True, with_points=True) as b:
                b.pipeline_mode("tiled")
                for f in range(5):
                    b.upload(f, *_frame(H, W, f))
                for pname in ci.PLANES:
                    kw = _plane_kw(svx_mod, cname, pname)
                    b.pipeline(chunk=chunk, **kw)
                    counts = b.read_counts()
                    for f in range(5):
                        ref = _ref_pipe(cname, shape, step, pname, f)
                        xyz, pts = b.read_points(f)
                        got = dict(counts=tuple(int(v) for v in counts[f]), hist=b.read_hist(f), pts=pts, xyz2=xyz)
                        try:
                            _check_pipe(got, ref)
                        except AssertionError as e:
                            raise AssertionError(f"{cname} {shape} step {step} plane {pname} frame {f}: {e}") from None
                        if pname == "none_out":
                            _check_centre_kept(cname, step, got, ref)
                    if (H * W) % 4 == 0:
                        dg = b.digest("pipeline", camera=kw["camera"])
                        for f in range(5):
                            want = oracle.digest_frame(*_frame(H, W, f), step, camera=cam, abc=np.array(kw["plane"]),
                                                       point_thr=kw["point_thr"], hist_thr=kw["hist_thr"])
                            assert tuple(int(v) for v in dg[f, :6]) == want, (cname, step, pname, f)
                        assert not dg[:, 6].any(), (cname, step, pname, dg[:, 6])


# ---------------------------------------------------------------------------
# f. the per-device table cache
# ---------------------------------------------------------------------------
def _run_and_check(svx_mod, cam, shape, what, step=2, pname="some"):
    disp, bgr = _frame(*shape)
    abc, pthr, hthr = ci.plane_case(cam or oracle.DEFAULT_CAMERA, pname)
    ref = oracle.pipeline_frame(disp, bgr, step, camera=cam, abc=np.array(abc), point_thr=pthr, hist_thr=hthr)
    assert ref["counts"][2] > 100, (what, ref["counts"])
    got = svx_mod.batch.pipeline_frame(disp, bgr, step, plane=abc, point_thr=pthr, hist_thr=hthr,
                                       camera=svx_mod.cam(cam) if cam else None)
    try:
        _check_pipe(got, ref)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
    return ref


def test_table_cache_camera_switches(svx_mod):
    """One process, one device: sv_pipeline_frame at default, near_int, default, near_int on the ragged shape,
    off, near_int again. Each result must be its own camera's: a table kept from the previous camera moves the
    int32 points (the oracle's tables of these cameras differ at these shapes). Then near_int against cameras
    that differ from it in ONE constant each, so a cache key that ignores any one of f, B, cw, ch is caught."""
    A, B = ci.SHAPES
    near, off = ci.CAMERAS["near_int"], ci.CAMERAS["off"]
    t0, t1 = oracle.delta_tables(*A), oracle.delta_tables(*A, camera=near)
    assert (t0[0][1:48] != t1[0][1:48]).any() and (t0[1][1:48] != t1[1][1:48]).any()
    for i, (cam, shape) in enumerate([(None, A), (near, A), (None, A), (near, B), (off, B), (near, A)]):
        _run_and_check(svx_mod, cam, shape, f"step {i + 1} of the switch sequence")
    for i, dv in enumerate((7.5, 0.03, 40.25, -9.5)):
        other = list(near)
        other[i] += dv
        other = tuple(other)
        to = oracle.delta_tables(*A, camera=other)
        assert (to[0][1:48] != t1[0][1:48]).any() or (to[1][1:48] != t1[1][1:48]).any(), i
        for rep in range(2):
            _run_and_check(svx_mod, near, A, f"near_int before the camera with constant {i} changed, round {rep}")
            _run_and_check(svx_mod, other, A, f"the camera with constant {i} changed, round {rep}", pname="none_out")


def test_table_cache_two_batches_alive(svx_mod):
    """Two Batch objects alive at once on different cameras (and a third on another shape), pipeline() called
    alternately: each batch's results stay its own camera's."""
    specs = [(None, ci.SHAPES[0]), ("near_int", ci.SHAPES[0]), ("off", ci.SHAPES[1])]
    batches = []
    try:
        for cname, (H, W) in specs:
            b = svx_mod.batch.Batch(2, H, W, 2, with_bgr=True, with_points=True)
            batches.append(b)
            for f in range(2):
                b.upload(f, *_frame(H, W, f))
        for rnd in range(3):
            for mode in ("tiled", "resident"):
                for b, (cname, shape) in zip(batches, specs):
                    b.pipeline_mode(mode)
                    b.pipeline(**_plane_kw(svx_mod, cname, "some"))
                    counts = b.read_counts()
                    for f in range(2):
                        ref = _ref_pipe(cname, shape, 2, "some", f)
                        xyz, pts = b.read_points(f)
                        got = dict(counts=tuple(int(v) for v in counts[f]), hist=b.read_hist(f), pts=pts, xyz2=xyz)
                        try:
                            _check_pipe(got, ref)
                        except AssertionError as e:
                            raise AssertionError(f"round {rnd} {mode} camera {cname} frame {f}: {e}") from None
    finally:
        for b in batches:
            b.close()


# ---------------------------------------------------------------------------
# g. batched RANSAC and per-frame planes
# ---------------------------------------------------------------------------
def _winner(recs):
    win, best = -1, float("inf")
    for i, r in enumerate(recs):   # the first strict minimum (functions.py:289-292)
        e = r.get("err")
        if e is not None and e < best:
            win, best = i, e
    return win, best


@pytest.mark.parametrize("mask_name", ["none", "edge", "corner"])
@pytest.mark.parametrize("step", [2, 1])
@pytest.mark.parametrize("cname", CAMS)
def test_ransac_and_frame_planes(svx_mod, cname, step, mask_name):
    """sv_batch_ransac's fp64 X / Y / Z tables and the per-frame-plane pipeline under a camera: the maskpoints'
    bits, the winning trial, its error and plane bit for bit, then each frame through both pipeline families
    with the oracle's plane. Frame 3 holds 300 points (fewer than k = 600): no plane, nothing kept. Masks: none;
    "edge", a 72 x 152 window across the carmask's edge; "corner", carmask()[:72, :152], which is all zero, so
    every frame takes the no-plane path."""
    cam = ci.CAMERAS[cname]
    C = svx_mod.cam(cam)
    H, W = ci.FIXTURE_SHAPE
    frames = [_frame(H, W, f) for f in range(3)] + [ci.sparse_frame(H, W)]
    m = None if mask_name == "none" else ci.mask_cuts(carmask())[mask_name]
    pthr, hthr, trials = 0.05, 1, 40
    with svx_mod.batch.Batch(4, H, W, step, with_bgr=True, with_points=True) as b:
        for f, (d, c) in enumerate(frames):
            b.upload(f, d, c)
        b.set_mask(m)
        b.ransac(seed_base=5, trials=trials, camera=C)
        planes = []
        for f, (d, c) in enumerate(frames):
            mpts = oracle.project(d if m is None else oracle.mask_disparity(d, m), None, 2, camera=cam)[0]
            got = b.read_maskpoints(f)
            assert got.shape == mpts.shape and np.array_equal(_bits(got), _bits(mpts)), (f, got.shape, mpts.shape)
            abc, recs = oransac.ransac(mpts, trials, rng=random.Random(5 + f))
            res = b.read_ransac(f)
            if abc is None:
                assert len(mpts) < 600 and res["trial"] == -1, (f, res)
                planes.append(None)
                continue
            win, err = _winner(recs)
            assert res["trial"] == win and res["err"] == err, (f, res, win, err)
            assert np.array_equal(_bits(res["abc"]), _bits(abc.reshape(3))), (f, res["abc"], abc.reshape(3))
            planes.append(abc.reshape(3))
        assert planes[3] is None and (mask_name == "corner") == all(p is None for p in planes)
        for mode in ("tiled", "resident"):
            b.pipeline_mode(mode)
            b.pipeline_planes(point_thr=pthr, hist_thr=hthr, camera=C)
            counts = b.read_counts()
            for f, (d, c) in enumerate(frames):
                fp = b.read_frame_plane(f)
                if planes[f] is None:
                    assert fp[3] == -1.0 and tuple(counts[f][1:3]) == (0, 0), (mode, f)
                    assert int(counts[f][0]) == len(oracle.project(d, None, step, camera=cam)[0])
                    continue
                assert np.array_equal(_bits(fp[:3]), _bits(planes[f]))
                ref = oracle.pipeline_frame(d, c, step, camera=cam, abc=planes[f], point_thr=pthr, hist_thr=hthr)
                assert ref["counts"][2] > 100, ref["counts"]
                xyz, pts = b.read_points(f)
                got = dict(counts=tuple(int(v) for v in counts[f]), hist=b.read_hist(f), pts=pts, xyz2=xyz)
                try:
                    _check_pipe(got, ref)
                except AssertionError as e:
                    raise AssertionError(f"{cname} step {step} {mode} frame {f}: {e}") from None


# ---------------------------------------------------------------------------
# h. the digest kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("cname", CAMS)
def test_digest_dense(svx_mod, cname, step):
    """sv_batch_digest("dense") of K1's planes with the batch's camera: the valid count and disparity hash are
    the oracle's and no point is out of tolerance. With the WRONG camera (the default one) on a near-integer
    batch it must notice: the bench's parity verdict rests on that."""
    cam = ci.CAMERAS[cname]
    H, W = ci.FIXTURE_SHAPE
    zeros = np.zeros((H, W, 3), np.uint8)
    with svx_mod.batch.Batch(3, H, W, step, with_bgr=False) as b:
        for f in range(3):
            b.upload(f, _frame(H, W, f)[0])
        b.project(camera=svx_mod.cam(cam))
        dg = b.digest("dense", camera=svx_mod.cam(cam))
        for f in range(3):
            want = oracle.digest_frame(_frame(H, W, f)[0], zeros, step, camera=cam)
            assert (int(dg[f, 0]), int(dg[f, 3])) == (want[0], want[3]), (cname, f)
        assert not dg[:, 6].any(), dg[:, 6]
        wrong = b.digest("dense")
        assert (wrong[:, 6] != 0).all(), wrong[:, 6]


@pytest.mark.parametrize("cname", CAMS)
def test_digest_pipeline_notices_wrong_camera(svx_mod, cname):
    """sv_batch_digest("pipeline") with the default camera on another camera's outputs: the mismatch column or
    a hash differs from the right camera's digest for every frame. (The right camera's digests are compared
    with the oracle's in test_pipeline_tiled_batch.)"""
    H, W = ci.FIXTURE_SHAPE
    with svx_mod.batch.Batch(2, H, W, 2, with_bgr=True, with_points=True) as b:
        for f in range(2):
            b.upload(f, *_frame(H, W, f))
        kw = _plane_kw(svx_mod, cname, "some")
        b.pipeline(**kw)
        right = b.digest("pipeline", camera=kw["camera"])
        wrong = b.digest("pipeline")
        assert not right[:, 6].any() and (right[:, 2] > 100).all()
        for f in range(2):
            assert wrong[f, 6] != 0 or not np.array_equal(wrong[f, 3:6], right[f, 3:6]), (cname, f)


# ---------------------------------------------------------------------------
# i. the frame loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("cname", ["near_int", "off"])
def test_frame_loop_camera(svx_mod, cname, step):
    """FrameLoop(camera=) at 72 x 152 (the loop takes that shape), source="caller": three batches of 4 frames
    give, frame for frame, what one 12-frame Batch gives with the same camera, pre-pass, RANSAC and pipeline
    (the construction of test_gpu_loop.test_caller_filled_batches_equal_one_batch), and frames 0 and 5 (the
    second lies behind a batch boundary and a carried pre-pass frame) equal the oracle's chain."""
    from svx.loop import FrameLoop
    cam = ci.CAMERAS[cname]
    C = svx_mod.cam(cam)
    H, W = ci.FIXTURE_SHAPE
    ids = list(range(300, 312))
    frames = [_frame(H, W, k) for k in range(12)]
    mask = ci.mask_cuts(carmask())["edge"]
    pthr, hthr = 0.05, 1
    with svx_mod.batch.Batch(12, H=H, W=W, step=step, with_bgr=True, with_points=True) as one:
        for f, (d, c) in enumerate(frames):
            one.upload(f, d, c)
        one.set_mask(mask)
        one.prepass("previous")
        one.ransac(seed_base=7, trials=600, first_frame=ids[0], camera=C)
        one.pipeline_planes(point_thr=pthr, hist_thr=hthr, camera=C)
        one.road_map()
        one.road_raster()
        want = one.digest("pipeline", camera=C)
        want_r = [one.read_ransac(f) for f in range(12)]
        want_road = [one.read_road(f, walk=True) for f in range(12)]
        want_map = one.read_road_map(11)
    assert not want[:, 6].any() and (want[:, 2] > 100).all(), want[:, [2, 6]]
    # the oracle's chain for frames 0 and 5 (stereovision.py:53-113)
    cleaned = oracle.fill_previous_chain([d for d, _ in frames[:6]])
    oref = {}
    for f in (0, 5):
        mpts = oracle.project(oracle.mask_disparity(cleaned[f], mask), None, 2, camera=cam)[0]
        abc, recs = oransac.ransac(mpts, 600, rng=random.Random(7 + ids[f]))
        win, err = _winner(recs)
        r = want_r[f]
        assert r["trial"] == win and r["err"] == err and np.array_equal(_bits(r["abc"]), _bits(abc.reshape(3))), f
        oref[f] = oracle.pipeline_frame(cleaned[f], frames[f][1], step, camera=cam, abc=abc.reshape(3),
                                        point_thr=pthr, hist_thr=hthr)
        assert tuple(int(v) for v in want[f, :3]) == oref[f]["counts"], f

    def check_oracle(b, local, f):
        xyz, pts = b.read_points(local)
        got = dict(counts=tuple(int(v) for v in b.read_counts()[local]), hist=b.read_hist(local), pts=pts, xyz2=xyz)
        _check_pipe(got, oref[f])

    with FrameLoop(4, H=H, W=W, step=step, slots=2, source="caller", seed_base=7, road="map", carmask=mask,
                   camera=C, point_thr=pthr, hist_thr=hthr) as loop:
        def check(seq):
            loop.wait(seq)
            pb, first = loop.batch(seq)
            base = first - ids[0]
            assert np.array_equal(pb.digest("pipeline", camera=C), want[base:base + 4]), seq
            for f in range(4):
                r, w = pb.read_ransac(f), want_r[base + f]
                assert r["trial"] == w["trial"] and r["err"] == w["err"] and np.array_equal(r["abc"], w["abc"]), (seq, f)
                img, walk = pb.read_road(f, walk=True)
                assert np.array_equal(img, want_road[base + f][0]) and np.array_equal(walk, want_road[base + f][1])
                if base + f in oref:
                    check_oracle(pb, f, base + f)
            return pb
        for i in range(3):
            b = loop.acquire()
            for f in range(4):
                b.upload(f, *frames[4 * i + f])
            seq = loop.submit(ids[4 * i])
            if i >= 1:
                check(seq - 1)
        pb = check(seq)
        assert np.array_equal(pb.read_road_map(3), want_map)
