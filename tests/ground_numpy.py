"""The ground grid in plain numpy float64, as the oracle of kernels/ground.hip and of the host-made mapping
(csrc/svx_ground_host.h). Direct and per pixel on purpose: no tables, no monotonicity shortcut. include/svx.h
(sv_ground_grid) states the semantics, tests/test_ground_cpu.py pins this file.

  DEFAULT_GRID, DEFAULT_CAMERA        (x0, z0, cell, nx, nz); (f, B, cw, ch)
  xz(disp, camera)                    X, Z of every pixel (float64, NaN where d == 0), functions.py:191-192's order
  cells(disp, camera, grid)           (ix, iz, inside) of every pixel: int64 indices (-1 outside) and the in-grid mask
  mapping(camera, grid, W)            (ix (256, W) int16, iz (256,) int16): cells() of every (d, x), -1 outside
  ground_grid(obstacles, disp, road, camera, grid, min_count)   what dropin.ground_grid / Batch.read_ground_grid return
  axes(grid)                          the cell centres (X of nx, Z of nz)
  cameras(), GRIDS                    the tests' cameras (the default and tests/golden/camera.json's) and grids
"""
import json
import os

import numpy as np

DEFAULT_GRID = (-8.0, 0.0, 0.25, 64, 128)
DEFAULT_CAMERA = (399.9745178222656, 0.2090607502, 474.5, 262.0)


def xz(disp, camera=DEFAULT_CAMERA):
    f, B, cw, _ = (np.float64(v) for v in camera)
    d = np.asarray(disp).astype(np.float64)
    x = np.arange(d.shape[-1], dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        Z = (f * B) / d                     # inf where d == 0: replaced below, never binned
        X = ((x - cw) * Z) / f
    zero = d == 0
    return np.where(zero, np.nan, X), np.where(zero, np.nan, Z)


def _index(v, origin, cell, n):
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((v - np.float64(origin)) / np.float64(cell))
        inside = (q >= 0) & (q < n)         # compared as doubles; NaN is outside
    return np.where(inside, q, -1).astype(np.int64), inside


def cells(disp, camera=DEFAULT_CAMERA, grid=DEFAULT_GRID):
    x0, z0, cell, nx, nz = grid
    X, Z = xz(disp, camera)
    ix, in_x = _index(X, x0, cell, nx)
    iz, in_z = _index(Z, z0, cell, nz)
    return ix, iz, in_x & in_z


def mapping(camera, grid, W):
    d = np.repeat(np.arange(256, dtype=np.uint8)[:, None], W, axis=1)   # a "disparity image" of every (d, x)
    ix, iz, _ = cells(d, camera, grid)
    return ix.astype(np.int16), iz[:, 0].astype(np.int16)


def ground_grid(obstacles, disp, road=None, camera=DEFAULT_CAMERA, grid=DEFAULT_GRID, min_count=1):
    x0, z0, cell, nx, nz = grid
    disp = np.asarray(disp)
    ob = np.asarray(obstacles) != 0
    rd = np.asarray(road) != 0 if road is not None else np.zeros(ob.shape, bool)
    ix, iz, inside = cells(disp, camera, grid)
    cell_of = iz * nx + ix
    obst = np.zeros(nz * nx, np.int64)
    rgrid = np.zeros(nz * nx, np.int64)
    np.add.at(obst, cell_of[ob & inside], 1)
    np.add.at(rgrid, cell_of[rd & inside], 1)
    obst = obst.reshape(nz, nx)
    nearest = np.full(nx, -1, np.int32)
    for c in range(nx):
        hit = np.flatnonzero(obst[:, c] >= min_count)
        if len(hit):
            nearest[c] = hit[0]
    info = np.array([(ob & inside).sum(), (ob & (disp > 0) & ~inside).sum(), (ob & (disp == 0)).sum(),
                     (rd & inside).sum()], np.int32)
    return {"obst": obst.astype(np.uint32), "road": rgrid.reshape(nz, nx).astype(np.uint32), "nearest": nearest,
            "info": info}


def axes(grid=DEFAULT_GRID):
    x0, z0, cell, nx, nz = grid
    return x0 + (np.arange(nx, dtype=np.float64) + 0.5) * cell, z0 + (np.arange(nz, dtype=np.float64) + 0.5) * cell


def cameras():
    """name -> (f, B, cw, ch): the reference's camera and the four of tests/golden/camera.json."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "camera.json")) as fh:
        cams = {k: tuple(float(x) for x in v) for k, v in json.load(fh)["cameras"].items()}
    return {"default": DEFAULT_CAMERA, **cams}


# The tests' grids. one: a single cell that holds the whole scene ahead; wide and tall: the cell cap as one row and as
# one column of 1 cm cells (wide's row is placed where d = 100 lies at the default camera); out: wholly out of range;
# x0zero: the left half of the scene is a negative quotient (truncation would put it in column 0); fine: 1 cm cells.
GRIDS = {
    "default": DEFAULT_GRID,
    "one": (-8.0, 0.0, 16.0, 1, 1),
    "wide": (-40.96, (399.9745178222656 * 0.2090607502) / 100 - 0.005, 0.01, 8192, 1),
    "tall": (-0.005, 0.0, 0.01, 1, 8192),
    "out": (1.0e6, 1.0e6, 0.25, 64, 128),
    "x0zero": (0.0, 0.0, 0.25, 64, 128),
    "fine": (-8.0, 0.0, 0.01, 64, 128),
}
