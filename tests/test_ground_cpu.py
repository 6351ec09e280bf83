"""CPU: the ground grid's oracle (tests/ground_numpy.py) pinned against the reference's projection as
oracle/cpu_loop.py restates it and against closed forms, and the host-made mapping (csrc/svx_ground_host.h, through
tools/ground_host_check.cpp built with the host compiler) against that oracle for every (d, x). No GPU.
(The sanitizer run of the same program is by hand on the development machine; no test runs it.)"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ground_numpy as gn
from conftest import REPO

CAMS = gn.cameras()
EXACT = (400.0, 0.25, 474.5, 262.0)   # f B = 100 exactly


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("cam", sorted(CAMS))
def test_oracle_xz_is_the_reference_projection(cam):
    """X and Z have the bits of functions.py:191-192 as oracle/cpu_loop.py restates them (step 1; its grid leaves
    the last row and column out)."""
    from oracle import cpu_loop
    f, B, cw, ch = CAMS[cam]
    rng = np.random.default_rng(11)
    disp = rng.integers(0, 256, (9, 41)).astype(np.uint8)
    disp[rng.random(disp.shape) < 0.2] = 0
    rows = np.array(cpu_loop.project(disp, None, step=1, f=f, B=B, cw=cw, ch=ch), np.float64)
    X, Z = gn.xz(disp, CAMS[cam])
    sel = np.zeros(disp.shape, bool)
    sel[:-1, :-1] = disp[:-1, :-1] > 0
    assert len(rows) == sel.sum() > 100
    assert np.array_equal(_bits(rows[:, 0]), _bits(X[sel])) and np.array_equal(_bits(rows[:, 2]), _bits(Z[sel]))
    assert np.isnan(X[disp == 0]).all() and np.isnan(Z[disp == 0]).all()


def test_closed_forms():
    disp = np.zeros((2, 1024), np.uint8)
    disp[0, 394] = 200          # Z = 0.5: on a cell edge at cell 0.25; X = (394 - 474.5) * 0.5 / 400 = -0.100625
    X, Z = gn.xz(disp, EXACT)
    assert Z[0, 394] == 0.5 and X[0, 394] == -0.100625
    ix, iz, inside = gn.cells(disp, EXACT, gn.DEFAULT_GRID)
    assert (ix[0, 394], iz[0, 394], inside[0, 394]) == (31, 2, True)          # floor((8 - 0.1) / 0.25) = 31
    ob = (disp > 0).astype(np.uint8) * 255
    r = gn.ground_grid(ob, disp, None, EXACT, gn.DEFAULT_GRID)
    assert r["obst"][2, 31] == 1 and r["obst"].sum() == 1 and list(r["info"]) == [1, 0, 0, 0]
    assert r["nearest"][31] == 2 and (np.delete(r["nearest"], 31) == -1).all()
    # x0 = 0: the quotient is -0.4; floor puts it outside, truncation would put it in column 0
    ix, iz, inside = gn.cells(disp, EXACT, gn.GRIDS["x0zero"])
    assert ix[0, 394] == -1 and not inside[0, 394]
    r = gn.ground_grid(ob, disp, None, EXACT, gn.GRIDS["x0zero"])
    assert r["obst"].sum() == 0 and list(r["info"]) == [0, 1, 0, 0] and (r["nearest"] == -1).all()
    # d = 2 at the reference's camera is 41.8 m ahead: beyond the default 32 m
    disp2 = np.full((1, 1024), 2, np.uint8)
    X, Z = gn.xz(disp2)
    assert 41.7 < Z[0, 0] < 41.9
    assert not gn.cells(disp2)[2].any()
    r = gn.ground_grid(np.full((1, 1024), 255, np.uint8), disp2)
    assert list(r["info"]) == [0, 1024, 0, 0]
    # d == 0 has no depth: counted apart, never binned; the road image counts only inside the grid
    ob3 = np.full((2, 1024), 255, np.uint8)
    r = gn.ground_grid(ob3, disp, ob3, EXACT, gn.DEFAULT_GRID)
    assert list(r["info"]) == [1, 0, 2047, 1] and r["road"][2, 31] == 1 and r["road"].sum() == 1


def _random_case(seed, shape=(40, 70)):
    rng = np.random.default_rng(seed)
    disp = rng.integers(1, 256, shape).astype(np.uint8)
    disp[rng.random(shape) < 0.2] = 0
    ob = (rng.random(shape) < 0.5).astype(np.uint8) * 255
    rd = ((rng.random(shape) < 0.6) & (ob == 0)).astype(np.uint8) * 200
    return ob, rd, disp


@pytest.mark.parametrize("cam", sorted(CAMS))
@pytest.mark.parametrize("grid", sorted(gn.GRIDS))
def test_conservation(cam, grid):
    ob, rd, disp = _random_case(5)
    r = gn.ground_grid(ob, disp, rd, CAMS[cam], gn.GRIDS[grid])
    nx, nz = gn.GRIDS[grid][3:]
    assert r["obst"].shape == r["road"].shape == (nz, nx) and r["obst"].dtype == r["road"].dtype == np.uint32
    assert r["nearest"].shape == (nx,) and r["nearest"].dtype == np.int32 and r["info"].dtype == np.int32
    info = [int(v) for v in r["info"]]
    assert int(r["obst"].sum()) == info[0] and int(r["road"].sum()) == info[3]
    assert info[0] + info[1] + info[2] == int((ob != 0).sum())
    assert info[2] == int(((ob != 0) & (disp == 0)).sum())
    if grid == "out":
        assert info[0] == info[3] == 0 and (r["nearest"] == -1).all()
    if grid == "one" and cam == "default":
        assert info[0] > 0 and info[3] > 0


def test_nearest_thresholds():
    """A column with 3 pixels in row 4 and 5 in row 10: min_count 1 and 3 (exactly the count) give row 4, 4 and 5
    give row 10, 6 gives -1."""
    disp = np.zeros((8, 1024), np.uint8)
    disp[0:3, 475] = 100        # Z = 1: row 4;   X = 0.5 / 400: column 32
    disp[3:8, 475] = 40         # Z = 2.5: row 10
    ix, iz, inside = gn.cells(disp, EXACT)
    assert inside[:, 475].all() and set(ix[:, 475]) == {32} and list(iz[:, 475]) == [4] * 3 + [10] * 5
    ob = (disp > 0).astype(np.uint8)
    for min_count, want in ((1, 4), (3, 4), (4, 10), (5, 10), (6, -1)):
        r = gn.ground_grid(ob, disp, None, EXACT, gn.DEFAULT_GRID, min_count)
        assert r["nearest"][32] == want and (np.delete(r["nearest"], 32) == -1).all(), (min_count, r["nearest"][32])
        assert r["obst"][4, 32] == 3 and r["obst"][10, 32] == 5


@pytest.mark.parametrize("cam", sorted(CAMS))
def test_ix_is_monotone_in_x(cam):
    """For a fixed d the in-grid ix never decreases with x, and the in-grid columns are one interval (what a
    threshold form of the mapping would rest on; the full table does not)."""
    for grid in ("default", "fine", "wide", "x0zero"):
        ix, iz = gn.mapping(CAMS[cam], gn.GRIDS[grid], 4096)
        assert (ix[0] == -1).all() and iz[0] == -1
        for d in range(1, 256):
            cols = np.flatnonzero(ix[d] >= 0)
            if len(cols):
                assert (np.diff(ix[d, cols].astype(np.int64)) >= 0).all(), (grid, d)
                assert cols[-1] - cols[0] + 1 == len(cols), (grid, d)


# ---- the host mapping, through the stand-alone program ----------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("ground") / "ground_host_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off",
                           os.path.join(REPO, "tools", "ground_host_check.cpp"), "-o", str(exe)])
    return str(exe)


def _run(exe, cam, grid, W):
    f, B, cw, _ = cam
    args = [repr(float(v)) for v in (f, B, cw, grid[0], grid[1], grid[2])] + [str(grid[3]), str(grid[4]), str(W)]
    return subprocess.run([exe] + args, capture_output=True)


def test_host_check_self_check(host_check):
    p = subprocess.run([host_check], capture_output=True, text=True)
    assert p.returncode == 0 and "ground host check ok" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("cam", sorted(CAMS))
def test_host_mapping_equals_the_oracle(host_check, cam):
    """Every (d, x) of the table the kernel looks up, for the widths, cameras and grids of the GPU tests."""
    for gname in ("default", "one", "wide", "tall", "out", "x0zero"):
        grid = gn.GRIDS[gname]
        for W in (2, 70, 889, 1024, 4096):
            p = _run(host_check, CAMS[cam], grid, W)
            assert p.returncode == 0, p.stderr
            got = np.frombuffer(p.stdout, "<i2")
            assert got.size == 512 * W + 256
            ix, iz = gn.mapping(CAMS[cam], grid, W)
            assert np.array_equal(got[:256 * W].reshape(256, W), ix), (cam, gname, W)
            assert np.array_equal(got[256 * W:256 * W + 256], iz), (cam, gname, W)
            # the folded table the device holds: iz nx + ix, or -1 where either is outside
            cell = np.where((ix >= 0) & (iz[:, None] >= 0), iz[:, None].astype(np.int64) * grid[3] + ix, -1)
            assert np.array_equal(got[256 * W + 256:].reshape(256, W), cell), (cam, gname, W)
            if gname == "out":
                assert (got == -1).all()
            if gname == "one" and cam == "default" and W == 1024:
                assert (ix[50:] == 0).all() and (iz[50:] == 0).all()     # the whole scene ahead is the one cell


def test_host_check_refuses_bad_grids(host_check):
    cam = CAMS["default"]
    for grid in ((-8.0, 0.0, 0.25, 8193, 1), (-8.0, 0.0, 0.25, 1, 8193), (-8.0, 0.0, 0.25, 4097, 2),
                 (-8.0, 0.0, 0.0, 64, 128), (-8.0, 0.0, -1.0, 64, 128), (float("nan"), 0.0, 0.25, 64, 128),
                 (-8.0, float("inf"), 0.25, 64, 128), (-8.0, 0.0, 0.25, 0, 128)):
        p = _run(host_check, cam, grid, 1024)
        assert p.returncode == 2 and p.stdout == b"" and b"refused" in p.stderr, grid
    assert _run(host_check, (0.0,) + cam[1:], gn.DEFAULT_GRID, 1024).returncode == 2
    assert _run(host_check, (cam[0], float("nan")) + cam[2:], gn.DEFAULT_GRID, 1024).returncode == 2
    assert _run(host_check, cam, gn.DEFAULT_GRID, 1).returncode == 2
    assert _run(host_check, cam, gn.DEFAULT_GRID, 4097).returncode == 2
    assert _run(host_check, cam, (-8.0, 0.0, 0.25, 8192, 1), 2).returncode == 0


def test_python_grid_structure_matches_header(tmp_path):
    """svx._abi.Grid has the size and field offsets of include/svx.h's sv_grid; ground_grid_axes gives the oracle's
    cell centres."""
    import ctypes

    from svx import _abi, dropin
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    fields = [f for f, _ in _abi.Grid._fields_]
    src = tmp_path / "g.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svx.h"\nint main(void){printf("%zu'
                   + "".join(" %zu" for _ in fields) + '\\n", sizeof(sv_grid)'
                   + "".join(f", offsetof(sv_grid, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "g"
    subprocess.check_call([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [ctypes.sizeof(_abi.Grid)] + [getattr(_abi.Grid, f).offset for f in fields] and got[0] == 32
    assert _abi.DEFAULT_GRID == gn.DEFAULT_GRID
    for grid in (None, gn.GRIDS["fine"], gn.GRIDS["wide"]):
        X, Z = dropin.ground_grid_axes(grid)
        rX, rZ = gn.axes(gn.DEFAULT_GRID if grid is None else grid)
        assert np.array_equal(X, rX) and np.array_equal(Z, rZ)
    X, Z = dropin.ground_grid_axes()
    assert X[0] == -7.875 and X[-1] == 7.875 and Z[0] == 0.125 and Z[-1] == 31.875
