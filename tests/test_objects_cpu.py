"""CPU: tests/objects_numpy.py, the oracle of the obstacle list (include/svx.h, sv_obstacle_list), pinned: its
partition against scipy.ndimage.label with a 3 x 3 structure of ones, closed forms, the list's order and limits, the
bar the batch frames of tests/test_gpu_objects.py have to meet, and the ctypes layout of sv_obstacle."""
import os

import numpy as np
import pytest

import hull_numpy as hn
import morph_numpy as mn
import objects_numpy as on
from conftest import REPO

SHAPES = [(1, 2), (1, 70), (40, 33), (40, 70), (45, 64), (9, 4096)]


def _same_partition(img):
    ndi = pytest.importorskip("scipy.ndimage")
    lab, k = on.label(img)
    ref, kr = ndi.label(np.asarray(img) != 0, np.ones((3, 3)))
    assert k == kr
    assert ((lab != 0) == (ref != 0)).all()
    # a bijection between the two numberings
    pairs = np.unique(np.stack([lab[lab != 0], ref[ref != 0]], 1), axis=0)
    assert len(pairs) == k and len(set(pairs[:, 0])) == k and len(set(pairs[:, 1])) == k


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_partition_matches_scipy_on_patterns(shape):
    for name, img in on.cases(*shape).items():
        _same_partition(img)


def test_partition_matches_scipy_on_random_images():
    rng = np.random.default_rng(20)
    for i in range(20):
        for dens in (0.1, 0.4, 0.6):
            _same_partition((rng.random((40, 70)) < dens).astype(np.uint8) * 255)


def test_labels_follow_first_pixels():
    img = on.cases(40, 70)["stripes"]
    comps = on.components(img)
    assert [c["first"] for c in comps] == list(range(0, 70, 2))
    assert all(c["area"] == 40 for c in comps)


def test_rectangle_closed_form():
    for (y, x, b, a) in ((3, 5, 4, 7), (0, 0, 1, 1), (36, 60, 4, 10), (10, 31, 2, 2)):   # b rows of a pixels at (x, y)
        img = np.zeros((40, 70), np.uint8)
        img[y:y + b, x:x + a] = 9
        n, e = on.obstacle_list(img, None, 1, 4)
        assert n == 1 and e == [{"x0": x, "y0": y, "x1": x + a - 1, "y1": y + b - 1, "area": a * b,
                                 "first": y * 70 + x, "nd": 0, "dmax": 0, "dmed": 0, "reserved": 0,
                                 "sx": b * (a * x + a * (a - 1) // 2), "sy": a * (b * y + b * (b - 1) // 2)}]


def test_corner_contact_joins_and_a_pixel_more_separates():
    img = np.zeros((40, 70), np.uint8)
    img[2:5, 3:8] = 1
    img[5:9, 8:12] = 1            # touches the first at its corner only
    n, e = on.obstacle_list(img, None, 1, 4)
    assert n == 1 and e[0]["area"] == 15 + 16 and (e[0]["x0"], e[0]["y0"], e[0]["x1"], e[0]["y1"]) == (3, 2, 11, 8)
    img[:] = 0
    img[2:5, 3:8] = 1
    img[5:9, 9:13] = 1            # a pixel further
    n, e = on.obstacle_list(img, None, 1, 4)
    assert n == 2 and [c["area"] for c in e] == [16, 15]
    img[:] = 0
    img[2:5, 3:8] = 1
    img[6:9, 8:12] = 1            # ... or a row further
    assert on.obstacle_list(img, None, 1, 4)[0] == 2


def test_lower_median():
    assert on.lower_median([2, 4, 4, 250]) == 4
    assert on.lower_median([250, 4, 2, 4]) == 4
    assert on.lower_median([7]) == 7
    assert on.lower_median([1, 2]) == 1
    assert on.lower_median([3, 1, 2]) == 2
    img = np.zeros((4, 8), np.uint8)
    img[1, 2:6] = 1
    disp = np.zeros((4, 8), np.uint8)
    disp[1, 2:6] = [2, 4, 4, 250]
    disp[0, :] = 99                # not under the component
    n, e = on.obstacle_list(img, disp, 1, 1)
    assert (e[0]["nd"], e[0]["dmax"], e[0]["dmed"]) == (4, 250, 4)
    disp[1, 2:6] = [0, 0, 5, 0]    # zeros do not count
    assert [on.obstacle_list(img, disp, 1, 1)[1][0][k] for k in ("nd", "dmax", "dmed")] == [1, 5, 5]
    disp[1, 2:6] = 0
    assert [on.obstacle_list(img, disp, 1, 1)[1][0][k] for k in ("nd", "dmax", "dmed")] == [0, 0, 0]


def test_order_and_limits():
    img = on.limit_rectangles()
    n, e = on.obstacle_list(img, None, 1, 32)
    assert n == 8 and [c["area"] for c in e] == [12, 12, 11, 6, 6, 6, 2, 1]
    assert [c["first"] for c in e[:2]] == [72, 110]                 # equal areas: by first pixel
    assert [c["first"] for c in e[3:6]] == sorted(c["first"] for c in e[3:6])
    for min_area, want in ((1, 8), (6, 6), (7, 3), (12, 2), (13, 0)):
        assert on.obstacle_list(img, None, min_area, 32)[0] == want
    for cap in (1, 3, 32):
        n, head = on.obstacle_list(img, None, 1, cap)
        assert n == 8 and head == e[:cap]


def test_xyz():
    cam = (399.9745178222656, 0.2090607502, 474.5, 262.0)
    e = {"x0": 100, "y0": 50, "x1": 103, "y1": 59, "dmed": 8}
    X, Y, Z = on.obstacle_xyz(e, cam)
    assert Z == cam[0] * cam[1] / 8 and X == ((101.5 - cam[2]) * Z) / cam[0] and Y == ((54.5 - cam[3]) * Z) / cam[0]
    assert on.obstacle_xyz(dict(e, dmed=0), cam) is None


@pytest.mark.parametrize("shape", [(72, 1024), (390, 889), (544, 1024)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_frames_meet_their_bar(shape):
    """The frames tests/test_gpu_objects.py sends through the real chain, through the oracles of that chain: the
    holed road lists at least three obstacles (two of equal area), the empty frame none, the two blobs at least one."""
    fr = on.batch_frames(*shape)
    counts = []
    for d in fr:
        cleaned = mn.sanitise((d > 0).astype(np.uint8) * 255)
        obst = hn.obstacles(cleaned, d, (0.0, 0.0, 0.01))["obstacles"]
        counts.append(on.obstacle_list(obst, d, 70, 16))
    assert counts[0][0] >= 3 and counts[1][0] == 0 and counts[2] == counts[0] and counts[3][0] >= 1, \
        [c[0] for c in counts]
    areas = [c["area"] for c in counts[0][1]]
    assert len(areas) != len(set(areas)), areas      # a tie in area: the order falls to the first pixel


def test_obstacle_layout_matches_header(tmp_path):
    """svx._abi.Obstacle (ctypes) and OBSTACLE_FIELDS (numpy) have the size and field offsets of include/svx.h's
    sv_obstacle, 56 bytes (checked by compiling the header with the host C compiler)."""
    import ctypes
    import shutil
    import subprocess

    from svx import _abi
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    fields = [f for f, _ in _abi.Obstacle._fields_]
    assert tuple(fields) == on.FIELDS
    src = tmp_path / "ob.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "svx.h"\nint main(void){printf("%zu'
                   + "".join(" %zu" for _ in fields) + '\\n", sizeof(sv_obstacle)'
                   + "".join(f", offsetof(sv_obstacle, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "ob"
    subprocess.check_call([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == 56
    assert got == [ctypes.sizeof(_abi.Obstacle)] + [getattr(_abi.Obstacle, f).offset for f in fields]
    dt = np.dtype(_abi.OBSTACLE_FIELDS)
    assert got == [dt.itemsize] + [dt.fields[f][1] for f in fields]


def test_entry_points_exist():
    """The feature's surface: the C symbols are bound and the Python entries are there."""
    from svx import _abi, batch, dropin
    for name in ("sv_obstacle_list", "sv_batch_obstacle_list", "sv_batch_read_obstacle_list",
                 "sv_batch_obstacle_list_ms"):
        assert name in _abi.SIGNATURES and getattr(_abi.lib(), name) is not None
    for name in ("obstacle_list", "read_obstacle_list", "obstacle_list_ms"):
        assert callable(getattr(batch.Batch, name))
    assert callable(dropin.obstacle_list) and callable(dropin.obstacle_xyz)
    assert "obstacle_list" not in dropin.PATCHED
