"""CPU: the rectification's oracle (tests/rectify_numpy.py) pinned against closed forms, and the host-made map pair
(csrc/svx_rectify_host.h, through tools/rectify_host_check.cpp built with the host compiler, and through
sv_rectify_map of the library) against that oracle, every entry. No GPU. Parity with cv2 (remap and
initUndistortRectifyMap) is unpinned: cv2 is absent here.
(The sanitizer run of the same program is by hand on the development machine; no test runs it.)"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rectify_numpy as rn
from conftest import REPO


def _identity_maps(dh, dw, shift=(0, 0), frac=0):
    x, y = np.meshgrid(np.arange(dw), np.arange(dh))
    xy = np.stack([x + shift[0], y + shift[1]], -1).astype(np.int16)
    return xy, np.full((dh, dw), frac, np.uint16)


def _rnd(rng, *s):
    a = rng.integers(0, 256, s).astype(np.uint8)
    a.flat[0], a.flat[-1] = 0, 255
    return a


# ---- the remap's closed forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [(), (3,)], ids=["grey", "bgr"])
def test_identity_and_integer_shift(tail):
    rng = np.random.default_rng(1)
    src = _rnd(rng, 13, 17, *tail)
    assert np.array_equal(rn.remap(src, *_identity_maps(13, 17)), src)
    got = rn.remap(src, *_identity_maps(13, 17, (3, -2)))       # dst[y, x] = src[y - 2, x + 3]
    want = np.zeros_like(src)
    want[2:, :14] = src[:11, 3:]
    assert np.array_equal(got, want)
    assert not got[:2].any() and not got[:, 14:].any() and got.any()
    # a destination of another shape than the source
    big = rn.remap(src, *_identity_maps(20, 30))
    assert big.shape == (20, 30) + tail and np.array_equal(big[:13, :17], src) and not big[13:].any()
    assert not big[:, 17:].any()


def test_half_pixel_forms():
    rng = np.random.default_rng(2)
    src = _rnd(rng, 9, 11).astype(np.int32)
    s8 = src.astype(np.uint8)
    # fx = 16, fy = 0: (a + b + 1) >> 1 with the column to the right, 0 beyond the last one
    right = np.pad(src, ((0, 0), (0, 1)))[:, 1:]
    assert np.array_equal(rn.remap(s8, *_identity_maps(9, 11, frac=16)), (src + right + 1) >> 1)
    # fx = fy = 16: (a + b + c + d + 2) >> 2 of the 2 x 2 block
    p = np.pad(src, ((0, 1), (0, 1)))
    quad = p[:-1, :-1] + p[:-1, 1:] + p[1:, :-1] + p[1:, 1:]
    assert np.array_equal(rn.remap(s8, *_identity_maps(9, 11, frac=16 * 32 + 16)), (quad + 2) >> 2)
    blk = np.array([[10, 21], [33, 47]], np.uint8)
    one = rn.remap(blk, np.zeros((1, 1, 2), np.int16), np.full((1, 1), 16 * 32 + 16, np.uint16))
    assert one[0, 0] == (10 + 21 + 33 + 47 + 2) >> 2


def test_weights_sum_to_32768_and_nothing_saturates():
    fy, fx = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    w = rn.weights(fx, fy)
    assert all(x.dtype == np.int32 and (x >= 0).all() for x in w)
    assert (sum(w) == 32768).all() and sum(w).shape == (32, 32)
    # a constant picture stays constant for every fraction; 255 stays 255
    for v in (1, 128, 255):
        src = np.full((2, 2), v, np.uint8)
        frac = (fy * 32 + fx).astype(np.uint16)
        out = rn.remap(src, np.zeros((32, 32, 2), np.int16), frac)
        assert (out == v).all()


def test_remap_refuses_bad_maps():
    src = np.zeros((4, 4), np.uint8)
    xy, frac = _identity_maps(4, 4)
    with pytest.raises(ValueError):
        rn.remap(src, xy, np.full((4, 4), 1024, np.uint16))
    with pytest.raises(ValueError):
        rn.remap(src, xy, frac[:3])
    with pytest.raises(ValueError):
        rn.remap(src, xy.astype(np.int32), frac)
    with pytest.raises(ValueError):
        rn.remap(np.zeros((4, 4, 2), np.uint8), xy, frac)


# ---- the map maker's closed forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 70), (13, 17), (390, 889)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_model_is_the_identity_map(shape):
    K, D, R, P = rn.models(shape)["identity"]
    xy, frac = rn.rectify_map(K, D, R, P, shape)
    want, zero = _identity_maps(*shape)
    assert xy.dtype == np.int16 and frac.dtype == np.uint16
    assert np.array_equal(xy, want) and np.array_equal(frac, zero)


def test_principal_point_moved_by_two_and_a_half():
    """P = K with u0 + 2.5: destination x looks at source column x - 2.5, so sx = x - 3 with fx = 16 (the floor of
    a negative half goes down); moved by - 2.5 it is sx = x + 2 with fx = 16."""
    K = rn.camera_matrix(400.0, 35.0, 6.0)
    for du, off in ((2.5, -3), (-2.5, 2)):
        P = K.copy()
        P[0, 2] += du
        xy, frac = rn.rectify_map(K, np.zeros(8), np.eye(3), P, (13, 70))
        want, _ = _identity_maps(13, 70, (off, 0))
        assert np.array_equal(xy, want) and (frac == 16).all(), du


def test_singular_or_non_finite_is_refused():
    K = rn.camera_matrix(400.0, 35.0, 6.0)
    P0 = K.copy()
    P0[0, 0] = 0.0
    for R, P in ((np.eye(3), P0), (np.zeros((3, 3)), K), (np.eye(3), np.full((3, 3), np.nan)),
                 (np.eye(3), np.full((3, 3), np.inf))):
        with pytest.raises(ValueError):
            rn.rectify_map(K, np.zeros(8), R, P, (4, 4))
    for shape in ((0, 4), (4, 0), (8193, 1), (1, 8193)):
        with pytest.raises(ValueError):
            rn.rectify_map(K, np.zeros(8), np.eye(3), K, shape)
    assert rn.inverse_3x3(np.diag([2.0, 4.0, 0.5])).tolist() == [[0.5, 0, 0], [0, 0.25, 0], [0, 0, 2.0]]


def test_camera_from_projection():
    P1 = np.array([[700.0, 0, 320.5, 0], [0, 700.0, 240.25, 0], [0, 0, 1, 0]])
    P2 = P1.copy()
    P2[0, 3] = -84.0                     # -f B with B = 0.12
    assert rn.camera_from_projection(P1, P2) == (700.0, 0.12, 320.5, 240.25)
    assert rn.camera_from_projection(P1[:, :3], P2) == (700.0, 0.12, 320.5, 240.25)
    from svx import dropin
    cam = dropin.camera_from_projection(P1, P2)
    assert (cam.f, cam.B, cam.cw, cam.ch) == (700.0, 0.12, 320.5, 240.25)
    cam = dropin.camera_from_projection(P1[:, :3], P2)
    assert (cam.f, cam.B, cam.cw, cam.ch) == (700.0, 0.12, 320.5, 240.25)
    for bad in ((P1[:2], P2), (P1, P2[:, :3]), (P1 * 0.0, P2)):
        with pytest.raises(ValueError):
            dropin.camera_from_projection(*bad)


# ---- the C map maker against the oracle, every entry -------------------------------------------------------------
MODELS = ("identity", "barrel", "rational", "rot_x", "rot_y", "rot_z", "corners")
SHAPES = ((1, 1), (2, 70), (13, 17), (390, 889), (544, 1024))


@pytest.fixture(scope="module")
def oracle_maps():
    return {(m, s): rn.rectify_map(*rn.models(s)[m], s) for m in MODELS for s in SHAPES}


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("rectify") / "rectify_host_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off",
                           os.path.join(REPO, "tools", "rectify_host_check.cpp"), "-o", str(exe)])
    return str(exe)


def _run(exe, model, shape):
    K, D, R, P = model
    args = [repr(float(v)) for m in (K, D, R, P) for v in np.asarray(m, np.float64).reshape(-1)]
    return subprocess.run([exe] + args + [str(shape[0]), str(shape[1])], capture_output=True)


def test_host_check_self_check(host_check):
    p = subprocess.run([host_check], capture_output=True, text=True)
    assert p.returncode == 0 and "rectify host check ok" in p.stdout, p.stdout + p.stderr


def test_corner_model_has_every_kind_of_entry(oracle_maps):
    """So that the comparisons below and on the GPU are not vacuous: at 544 x 1024 the corner-leaving model has
    entries fully inside the source, entries with one to three taps outside and entries fully outside."""
    xy, frac = oracle_maps[("corners", (544, 1024))]
    n = rn.taps_inside(xy, 544, 1024)
    assert (n == 4).sum() > 1000 and ((n >= 1) & (n <= 3)).sum() > 100 and (n == 0).sum() > 1000
    assert len(np.unique(frac)) == 1024
    # and the barrel model pulls the corners inwards: every entry inside, the fractions all in use
    xy, frac = oracle_maps[("barrel", (544, 1024))]
    assert (rn.taps_inside(xy, 544, 1024) == 4).all() and len(np.unique(frac)) == 1024


@pytest.mark.parametrize("model", MODELS)
def test_host_map_equals_the_oracle(host_check, oracle_maps, model):
    for shape in SHAPES:
        p = _run(host_check, rn.models(shape)[model], shape)
        assert p.returncode == 0, p.stderr
        n = shape[0] * shape[1]
        assert len(p.stdout) == 6 * n
        xy = np.frombuffer(p.stdout, "<i2", 2 * n).reshape(shape + (2,))
        frac = np.frombuffer(p.stdout, "<u2", n, 4 * n).reshape(shape)
        rxy, rfrac = oracle_maps[(model, shape)]
        assert np.array_equal(xy, rxy), (model, shape, int((xy != rxy).any(-1).sum()))
        assert np.array_equal(frac, rfrac), (model, shape, int((frac != rfrac).sum()))
        assert int(frac.max()) < 1024


def test_host_check_refuses(host_check):
    K, D, R, P = rn.models((4, 4))["barrel"]
    P0 = P.copy()
    P0[1, 1] = 0.0
    for model, shape in (((K, D, R, P0), (4, 4)), ((K, D, np.zeros((3, 3)), P), (4, 4)),
                         ((K, D, R, P * np.nan), (4, 4)), ((K, D, R, P), (0, 4)), ((K, D, R, P), (4, 8193))):
        p = _run(host_check, model, shape)
        assert p.returncode == 2 and p.stdout == b"" and b"refused" in p.stderr, shape
    assert _run(host_check, (K, D, R, P), (1, 8192)).returncode == 0


@pytest.mark.parametrize("model", ["rational", "corners"])
def test_library_map_equals_the_oracle(oracle_maps, model):
    """sv_rectify_map of the built library (the same header, compiled by the device compiler's host pass) through
    dropin.rectify_map; needs no device."""
    from svx import dropin
    for shape in SHAPES:
        K, D, R, P = rn.models(shape)[model]
        xy, frac = dropin.rectify_map(K, D, R, P, shape)
        rxy, rfrac = oracle_maps[(model, shape)]
        assert np.array_equal(xy, rxy) and np.array_equal(frac, rfrac), (model, shape)
    K, D, R, P = rn.models((4, 4))[model]
    # a 3 x 4 projection's left 3 x 3 is taken; fewer coefficients are padded with zeros
    P4 = np.hstack([P, [[-50.0], [0.0], [0.0]]])
    a = dropin.rectify_map(K, D[:1], R, P4, (4, 4))
    b = rn.rectify_map(K, np.r_[D[:1], np.zeros(7)], R, P, (4, 4))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_python_argument_checks_need_no_device():
    from svx import SvxError, dropin
    K, D, R, P = rn.models((4, 4))["barrel"]
    with pytest.raises(SvxError, match=r"\(-1\)"):
        dropin.rectify_map(K, D, np.zeros((3, 3)), P, (4, 4))          # SV_E_ARG: singular
    for shape in ((0, 4), (4, 8193)):
        with pytest.raises(ValueError):
            dropin.rectify_map(K, D, R, P, shape)
    with pytest.raises(ValueError):
        dropin.rectify_map(K, np.zeros(9), R, P, (4, 4))
    with pytest.raises(ValueError):
        dropin.rectify_map(K[:2], D, R, P, (4, 4))
    xy, frac = _identity_maps(4, 4)
    src = np.zeros((4, 4), np.uint8)
    with pytest.raises(TypeError):
        dropin.remap(src.astype(np.float32), xy, frac)
    with pytest.raises(TypeError):
        dropin.remap(src, xy.astype(np.int32), frac)
    with pytest.raises(TypeError):
        dropin.remap(src, xy, frac.astype(np.int16))
    for bad in ((xy[:3], frac), (xy, frac[:, :3]), (xy[..., :1], frac), (xy, np.full((4, 4), 1024, np.uint16))):
        with pytest.raises(ValueError):
            dropin.remap(src, *bad)
    with pytest.raises(ValueError):
        dropin.remap(np.zeros((1, 8193), np.uint8), xy, frac)
    with pytest.raises(ValueError):
        dropin.remap(np.zeros((2, 4, 4, 2), np.uint8), xy, frac)           # two channels


def test_c_argument_checks_come_before_the_device():
    """sv_remap_u8 and sv_rectify_map refuse with SV_E_ARG before they look for a device: so also here."""
    from svx import _abi
    f = _abi.lib().sv_remap_u8
    src, dst = np.zeros((2, 4, 4, 3), np.uint8), np.zeros((2, 4, 4, 3), np.uint8)
    xy, frac = _identity_maps(4, 4)
    xy, frac = np.ascontiguousarray(xy), np.ascontiguousarray(frac)
    s, d, m, r = (_abi.ptr(a) for a in (src, dst, xy, frac))
    for args in ((None, 1, 4, 4, 1, m, r, 4, 4, d), (s, 1, 4, 4, 1, None, r, 4, 4, d), (s, 1, 4, 4, 1, m, None, 4, 4, d),
                 (s, 1, 4, 4, 1, m, r, 4, 4, None), (s, 0, 4, 4, 1, m, r, 4, 4, d), (s, 1, 4, 4, 2, m, r, 4, 4, d),
                 (s, 1, 4, 4, 4, m, r, 4, 4, d), (s, 1, 8193, 4, 1, m, r, 4, 4, d), (s, 1, 4, 8193, 1, m, r, 4, 4, d),
                 (s, 1, 4, 4, 1, m, r, 8193, 4, d), (s, 1, 4, 4, 1, m, r, 4, 8193, d), (s, 1, 4, 4, 1, m, r, 0, 4, d),
                 (s, 1, 4, 4, 1, m, r, 4, 4, s)):
        assert f(*args) == -1, args
    frac[3, 3] = 1024
    assert f(s, 1, 4, 4, 1, m, r, 4, 4, d) == -1
    g = _abi.lib().sv_rectify_map
    K, D, R, P = (np.ascontiguousarray(a, np.float64) for a in rn.models((4, 4))["barrel"])
    k, dd, rr, p = (_abi.ptr(a) for a in (K, D, R, P))
    assert g(k, dd, rr, p, 4, 4, m, r) == 0 and frac[3, 3] < 1024
    for args in ((None, dd, rr, p, 4, 4, m, r), (k, dd, rr, p, 4, 4, None, r), (k, dd, rr, p, 0, 4, m, r),
                 (k, dd, rr, p, 4, 8193, m, r), (k, dd, _abi.ptr(np.zeros((3, 3))), p, 4, 4, m, r)):
        assert g(*args) == -1, args
