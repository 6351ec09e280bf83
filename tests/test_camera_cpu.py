"""The oracle at cameras other than the reference's own, pinned to the reference itself (CPU only).

tests/golden/camera.npz was written by running the reference's unmodified chain with its four camera
constants set to each camera of tests/golden/camera_inputs.py (make_camera_golden.py). The oracle called with
camera= must reproduce every array of it bit for bit: oracle.project, pipeline_frame, backproject and
delta_tables. This is the CPU half of the chain reference -> oracle -> GPU (tests/test_gpu_camera.py is the
other half), as tests/test_oracle_golden.py is for the default camera.

The input conditions the GPU tests rely on are asserted here too, for every camera, shape and step, so those
tests cannot pass vacuously: each plane of camera_inputs.PLANES keeps what its name says, the frames have
valid points on the grid column and row next to a near-integer centre, RANSAC's frames hold at least 600
maskpoints (and the sparse one fewer), and the delta tables of the cameras differ from one another."""
import json
import os
import sys

import numpy as np
import pytest

import oracle
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import camera_inputs as ci  # noqa: E402
from test_prepass_cpu import carmask  # noqa: E402

FIX = np.load(os.path.join(GOLDEN, "camera.npz"))
with open(os.path.join(GOLDEN, "camera.json")) as _fh:
    META = json.load(_fh)
CAMS = list(ci.CAMERAS)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_fixture_describes_these_inputs():
    assert {k: tuple(v) for k, v in META["cameras"].items()} == ci.CAMERAS
    assert tuple(META["shape"]) == ci.FIXTURE_SHAPE and META["seed"] == ci.SEED and META["step"] == 2
    disp, bgr = ci.frame(*ci.FIXTURE_SHAPE, 0)
    assert oracle.digest(disp) == META["frame"]["disp"] and oracle.digest(bgr) == META["frame"]["bgr"]
    for cname, cam in ci.CAMERAS.items():
        for pname in ci.FIXTURE_PLANES:
            abc, pthr, hthr = ci.plane_case(cam, pname)
            m = META["planes"][cname][pname]
            assert tuple(m["abc"]) == abc and m["point_thr"] == pthr and m["hist_thr"] == hthr
    assert os.path.getsize(os.path.join(GOLDEN, "camera.npz")) <= os.path.getsize(os.path.join(GOLDEN, "crops.npz"))


@pytest.mark.parametrize("cname", CAMS)
def test_projection_equals_reference(cname):
    """oracle.project(camera=): X, Y, Z bits and colours, with and without colours."""
    cam = ci.CAMERAS[cname]
    disp, bgr = ci.frame(*ci.FIXTURE_SHAPE, 0)
    xyz, rgb = oracle.project(disp, bgr, 2, camera=cam)
    mxyz, none = oracle.project(disp, None, 2, camera=cam)
    d = META["digests"][cname]
    assert none is None
    assert oracle.digest(xyz) == d["xyz"] and oracle.digest(rgb) == d["rgb"] and oracle.digest(mxyz) == d["mask_xyz"]
    if cname == "near_int":
        assert xyz.shape == FIX["near_int_xyz"].shape
        assert np.array_equal(_bits(xyz), _bits(FIX["near_int_xyz"]))
        assert np.array_equal(_bits(mxyz), _bits(FIX["near_int_mask_xyz"]))
        assert np.array_equal(rgb, FIX["near_int_rgb"])


@pytest.mark.parametrize("pname", ci.FIXTURE_PLANES)
@pytest.mark.parametrize("cname", CAMS)
def test_chain_equals_reference(cname, pname):
    """oracle.pipeline_frame(camera=) and oracle.backproject(camera=): counts, histogram, int32 points; for
    near_int also which points survive each filter and the survivors' X, Y, Z bits."""
    cam = ci.CAMERAS[cname]
    disp, bgr = ci.frame(*ci.FIXTURE_SHAPE, 0)
    abc, pthr, hthr = ci.plane_case(cam, pname)
    r = oracle.pipeline_frame(disp, bgr, 2, camera=cam, abc=np.array(abc), point_thr=pthr, hist_thr=hthr)
    pre = f"{cname}_{pname}_"
    assert r["counts"] == tuple(int(v) for v in FIX[pre + "counts"]) == tuple(META["planes"][cname][pname]["counts"])
    assert np.array_equal(r["hist"], FIX[pre + "hist"])
    assert np.array_equal(r["pts"].reshape(-1, 1, 2), FIX[pre + "plane_points"])
    back = oracle.backproject(r["xyz2"], camera=cam)
    assert np.array_equal(np.array(back, np.int32).reshape(-1, 1, 2), FIX[pre + "plane_points"])
    if cname == "near_int":
        xyz = FIX["near_int_xyz"]
        keep = np.flatnonzero(oracle.point_errors(xyz, abc) < pthr)
        assert np.array_equal(keep, FIX[pre + "keep_idx"])
        assert np.array_equal(_bits(r["xyz2"]), _bits(xyz[FIX[pre + "keep2_idx"]]))
        _, _, src = oracle.project(disp, bgr, 2, camera=cam, with_src=True)
        assert np.array_equal(r["src2"], src[FIX[pre + "keep2_idx"]])


@pytest.mark.parametrize("cname", CAMS)
def test_delta_tables_equal_reference_roundtrip(cname):
    """oracle.delta_tables(camera=) against the deltas measured through the reference's projection and
    back-projection, over the frame's even x and y and every d in 1..255."""
    H, W = ci.FIXTURE_SHAPE
    dx, dy = oracle.delta_tables(H, W, camera=ci.CAMERAS[cname])
    ref_dx, ref_dy = FIX[cname + "_dx_even"], FIX[cname + "_dy_even"]
    assert np.array_equal(dx.T[0:W - 1:2, 1:], ref_dx[0:W - 1:2, 1:])
    assert np.array_equal(dy.T[0:H - 1:2, 1:], ref_dy[0:H - 1:2, 1:])
    assert set(np.unique(dx)) <= {-1, 0} and set(np.unique(dy)) <= {-1, 0}
    d = META["digests"][cname]
    assert oracle.digest(ref_dx) == d["dx"] and oracle.digest(ref_dy) == d["dy"]


def test_delta_tables_differ_between_cameras():
    """A stale table after a camera switch must change the points: the tables of the cameras the cache test
    alternates (default, near_int, off) differ at both shapes, on grid points the frames use."""
    for H, W in ci.SHAPES:
        tabs = {n: oracle.delta_tables(H, W, camera=c) for n, c in
                (("default", None), ("near_int", ci.CAMERAS["near_int"]), ("off", ci.CAMERAS["off"]))}
        for a, b in (("default", "near_int"), ("near_int", "off"), ("default", "off")):
            ddx = tabs[a][0][1:48, 0:W - 1] != tabs[b][0][1:48, 0:W - 1]    # the ramp's disparities are below 48
            ddy = tabs[a][1][1:48, 0:H - 1] != tabs[b][1][1:48, 0:H - 1]
            assert ddx.sum() > 100 and ddy.sum() > 50, (H, W, a, b, int(ddx.sum()), int(ddy.sum()))


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("shape", ci.SHAPES)
@pytest.mark.parametrize("cname", CAMS)
def test_plane_conditions(cname, shape, step):
    """Every frame the GPU tests use (k = 0..4) under every named plane keeps what the plane's name says."""
    cam = ci.CAMERAS[cname]
    for k in range(5):
        disp, bgr = ci.frame(*shape, k)
        for pname in ci.PLANES:
            abc, pthr, hthr = ci.plane_case(cam, pname)
            n, n1, n2 = oracle.pipeline_frame(disp, bgr, step, camera=cam, abc=np.array(abc), point_thr=pthr,
                                              hist_thr=hthr)["counts"]
            what = (cname, shape, step, k, pname, (n, n1, n2))
            if pname in ("some", "tight"):
                assert 0 < n2 < n1 < n, what
            elif pname == "all_out":
                assert n > 0 and (n1, n2) == (0, 0), what
            else:
                assert n1 == n and 0 < n2 < n1, what


@pytest.mark.parametrize("cname", sorted(ci.NEAR_GRID))
def test_frames_have_points_next_to_the_centre(cname):
    """The grid column and row next to a near-integer centre lie inside both shapes, on the step-1 and step-2
    grids, hold valid points in every frame, and x - cw (y - ch) there is tiny: the low word of the fp32 split
    is most of the value."""
    gx, gy = ci.NEAR_GRID[cname]
    _, _, cw, ch = ci.CAMERAS[cname]
    assert 0 < abs(gx - cw) < 1e-3 and 0 < abs(gy - ch) < 1e-3 and gx % 2 == 0 and gy % 2 == 0
    assert float(np.float32(cw)) != cw and float(np.float32(ch)) != ch    # the low words are not zero
    for H, W in ci.SHAPES:
        assert gx < W - 1 and gy < H - 1
        for k in range(5):
            disp, _ = ci.frame(H, W, k)
            assert (disp[0:H - 1:2, gx] != 0).sum() >= 10 and (disp[gy, 0:W - 1:2] != 0).sum() >= 10, (H, W, k)


def test_ransac_frames():
    """Batched RANSAC's frames at 72 x 152: at least 600 step-2 maskpoints without a mask and under the mask
    window that crosses the carmask's edge; none under carmask()[:72, :152], which is all zero; the sparse
    frame has fewer than 600 either way."""
    H, W = ci.FIXTURE_SHAPE
    cuts = ci.mask_cuts(carmask())
    assert not cuts["corner"].any() and 0.5 < (cuts["edge"] != 0).mean() < 0.8
    for k in range(3):
        d, _ = ci.frame(H, W, k)
        assert len(oracle.project(d, None, 2)[0]) >= 1500
        assert 600 <= len(oracle.project(oracle.mask_disparity(d, cuts["edge"]), None, 2)[0]) < 1500
    d, _ = ci.sparse_frame(H, W)
    assert len(oracle.project(d, None, 2)[0]) == 300
