"""GPU: the stereo rectification — kernels/remap.hip behind sv_remap_u8 (dropin.remap) and behind the
batch stage sv_batch_rectify (Batch.rectify_maps / rectify) — byte for byte against the oracle tests/rectify_numpy.py,
which tests/test_rectify_cpu.py pins. Every comparison is exact."""
import ctypes
import types

import numpy as np
import pytest

import rectify_numpy as rn

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import _abi, batch, dropin
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, abi=_abi, batch=batch, dropin=dropin)


def same(got, ref, what):
    """Equality with the first differing pixels reported."""
    assert got.dtype == np.uint8 and got.shape == ref.shape, (what, got.shape, ref.shape)
    diff = got != ref
    bad = np.argwhere(diff.any(-1) if got.ndim == 3 else diff)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])].tolist(), ref[tuple(bad[0])].tolist())


def rnd(rng, *s):
    """Random bytes with 0 and 255 in them."""
    a = rng.integers(0, 256, s).astype(np.uint8)
    a[rng.random(s) < 0.05] = 0
    a[rng.random(s) < 0.05] = 255
    if a.size >= 2:
        a.flat[0], a.flat[-1] = 0, 255
    return a


def random_maps(rng, sh, sw, dh, dw):
    """A map of (dh, dw) into an sh x sw source: positions from two before the source to one past it, so that every
    combination of taps inside and outside occurs; sprinkled over it the columns -1 and sw - 1, the rows -1 and
    sh - 1, entries far outside and the extreme coordinates; every frac value where the map has room for them."""
    n = dh * dw
    sx = rng.integers(-2, sw + 1, n)
    sy = rng.integers(-2, sh + 1, n)
    special = [(-1, 0), (sw - 1, 0), (0, -1), (0, sh - 1), (-1, -1), (sw - 1, sh - 1), (-1, sh - 1), (sw - 1, -1),
               (0, 0), (sw - 2, sh - 2), (-32768, -32768), (32767, 32767), (32767, -32768), (-32768, 32767),
               (32767, 0), (0, 32767), (-32768, 0), (0, -32768), (sw, sh), (-2, -2), (sw + 40, 1), (1, sh + 40)]
    at = rng.permutation(n)[:min(n, 3 * len(special))]
    for k, i in enumerate(at):
        sx[i], sy[i] = special[k % len(special)]
    frac = rng.integers(0, 1024, n)
    if n >= 1024:
        frac[rng.permutation(n)[:1024]] = np.arange(1024)
    xy = np.stack([sx, sy], -1).reshape(dh, dw, 2).astype(np.int16)
    return xy, frac.reshape(dh, dw).astype(np.uint16)


# (21, 124 / 128 / 130): either side of the width from which a lane takes four pixels, and a width above it that is
# no multiple of 4; (3, 4096) -> (2, 4095): the widest row of a pixel per lane; (2, 8192) -> (2, 4096): the widest
# source, four pixels a lane; (1, 1) -> (5, 7) and (2, 3) -> (7, 5): sources where most taps are outside
CASES = [((1, 1), (1, 1)), ((1, 1), (5, 7)), ((2, 3), (7, 5)), ((13, 17), (5, 4)), ((31, 33), (64, 64)),
         ((9, 100), (21, 124)), ((9, 100), (21, 128)), ((9, 100), (21, 130)), ((3, 4096), (2, 4095)),
         ((2, 8192), (2, 4096))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{c[1][0]}x{c[1][1]}")
def test_remap_against_the_oracle(sv, case):
    (sh, sw), (dh, dw) = case
    rng = np.random.default_rng(1000 * sh + sw + dh)
    xy, frac = random_maps(rng, sh, sw, dh, dw)
    taps = rn.taps_inside(xy, sh, sw)
    if dh * dw >= 1024:
        assert len(np.unique(frac)) == 1024 and {0, 1, 2, 4}.issubset(set(np.unique(taps)))
    for ch in (1, 3):
        src = rnd(rng, sh, sw) if ch == 1 else rnd(rng, sh, sw, 3)
        same(sv.dropin.remap(src, xy, frac), rn.remap(src, xy, frac), (case, ch))


def test_remap_through_the_barrel_map(sv):
    """(40, 1024) -> (40, 1024) through the barrel model's map: neighbouring lanes reading neighbouring pixels, the
    plain form of the four-pixel lanes nearly everywhere (the last row's middle rounds up to sy = 39, whose lower taps
    are outside with weight 0)."""
    shape = (40, 1024)
    xy, frac = rn.rectify_map(*rn.models(shape)["barrel"], shape)
    assert (rn.taps_inside(xy, *shape) == 4).mean() > 0.99
    rng = np.random.default_rng(40)
    for tail in ((), (3,)):
        src = rnd(rng, *shape, *tail)
        same(sv.dropin.remap(src, xy, frac), rn.remap(src, xy, frac), ("barrel", tail))
    # and the corner-leaving model: lanes of both forms in one wave
    xy, frac = rn.rectify_map(*rn.models(shape)["corners"], shape)
    taps = rn.taps_inside(xy, *shape)
    assert (taps == 4).any() and (taps == 0).any() and ((taps > 0) & (taps < 4)).any()
    src = rnd(rng, *shape, 3)
    same(sv.dropin.remap(src, xy, frac), rn.remap(src, xy, frac), "corners")


def test_three_pictures_through_one_map(sv):
    """n = 3 different pictures, each against its own oracle (the frame strides), a pixel and four pixels a lane."""
    rng = np.random.default_rng(77)
    for (sh, sw), (dh, dw) in (((13, 17), (20, 11)), ((6, 50), (5, 136))):
        xy, frac = random_maps(rng, sh, sw, dh, dw)
        for tail in ((), (3,)):
            stack = rnd(rng, 3, sh, sw, *tail)
            got = sv.dropin.remap(stack, xy, frac)
            assert got.shape == (3, dh, dw) + tail
            for k in range(3):
                same(got[k], rn.remap(stack[k], xy, frac), (k, tail, dw))
            assert not np.array_equal(got[0], got[1])


def test_identity_and_all_outside(sv):
    rng = np.random.default_rng(5)
    for shape in ((13, 17), (6, 136)):
        x, y = np.meshgrid(np.arange(shape[1]), np.arange(shape[0]))
        xy = np.stack([x, y], -1).astype(np.int16)
        zero = np.zeros(shape, np.uint16)
        for tail in ((), (3,)):
            src = rnd(rng, *shape, *tail)
            same(sv.dropin.remap(src, xy, zero), src, ("identity", shape, tail))
            # every entry outside: below the last row, right of the last column, far away; any fraction
            out = np.empty_like(xy)
            out[..., 0] = np.where(x % 3 == 0, shape[1], np.where(x % 3 == 1, -2, 32767))
            out[..., 1] = np.where(y % 2 == 0, shape[0], -32768)
            out[..., 1][x % 3 == 0] = y[x % 3 == 0]
            assert (rn.taps_inside(out, *shape) == 0).all()
            frac = rng.integers(0, 1024, shape).astype(np.uint16)
            got = sv.dropin.remap(src, out, frac)
            assert got.shape == src.shape and not got.any(), (shape, tail)


# ---- the batch ---------------------------------------------------------------------------------------------------
def _maps_for(shape, seed):
    """The two eyes' maps: the left a model's (smooth, the corners leaving the source), the right random."""
    left = rn.rectify_map(*rn.models(shape)["corners"], shape)
    right = random_maps(np.random.default_rng(seed), shape[0], shape[1], shape[0], shape[1])
    return left, right


@pytest.mark.parametrize("shapes", [((16, 24), None), ((40, 72), None), ((20, 25), (20, 160))],
                         ids=["16x24", "40x72", "pair20x160"])
def test_batch_rectify_equals_the_oracle(sv, shapes):
    """upload_bgr_pair -> rectify_maps -> rectify -> read_bgr_pair, both eyes of every frame; the third case is a
    batch whose pairs have another shape than its frames (pair_shape)."""
    (H, W), pair = shapes
    ph, pw = pair or (H, W)
    n = 3
    rng = np.random.default_rng(H + W)
    pairs = [(rnd(rng, ph, pw, 3), rnd(rng, ph, pw, 3)) for _ in range(n)]
    left, right = _maps_for((ph, pw), 9)
    with sv.batch.Batch(n, H, W, step=1, with_bgr=False) as b:
        if pair:
            b.pair_shape(ph, pw)
        for f, (L, R) in enumerate(pairs):
            b.upload_bgr_pair(f, L, R)
        b.rectify_maps(left, right)
        b.rectify()
        assert b.rectify_ms() > 0
        for f, (L, R) in enumerate(pairs):
            gl, gr = b.read_bgr_pair(f)
            same(gl, rn.remap(L, *left), ("L", f))
            same(gr, rn.remap(R, *right), ("R", f))
        # one frame written anew: the next rectify takes every frame from its raw picture, once
        newL, newR = rnd(rng, ph, pw, 3), rnd(rng, ph, pw, 3)
        b.upload_bgr_pair(1, newL, newR)
        b.rectify()
        for f, (L, R) in enumerate([pairs[0], (newL, newR), pairs[2]]):
            gl, gr = b.read_bgr_pair(f)
            same(gl, rn.remap(L, *left), ("L again", f))
            same(gr, rn.remap(R, *right), ("R again", f))
        # new maps replace the old ones
        b.upload_bgr_pair(0, *pairs[0])
        b.rectify_maps(right, left)
        b.rectify()
        gl, gr = b.read_bgr_pair(2)
        same(gl, rn.remap(pairs[2][0], *right), "swapped maps L")
        same(gr, rn.remap(pairs[2][1], *left), "swapped maps R")


def test_batch_preprocess_consumes_the_rectified_pairs(sv):
    """preprocess() behind rectify() equals preprocess() of a second batch uploaded with the oracle's rectified pairs,
    in what the existing tests read back of it: the disparity sgbm() makes of the grey pairs, and the counts, the
    hue histogram and the points of the pipeline, whose colours are the corrected left picture's. (SGBM takes no pair
    narrower than 128 + blockSize / 2 columns, so this runs at 40 x 152, as tests/test_gpu_jpeg_decode.py's does.)"""
    n, H, W = 3, 40, 152
    rng = np.random.default_rng(152)
    pairs = []
    for f in range(n):                          # blocks of 4 x 4 plus noise, the right picture the left moved by 6 + f
        L = np.kron(rng.integers(0, 256, (H // 4, W // 4, 3), dtype=np.uint8), np.ones((4, 4, 1), np.uint8))
        L = (L.astype(np.int32) + rng.integers(-20, 21, L.shape)).clip(0, 255).astype(np.uint8)
        pairs.append((L, np.roll(L, -(6 + f), axis=1)))
    shape = (H, W)
    left = rn.rectify_map(*rn.models(shape)["barrel"], shape)
    right = rn.rectify_map(*rn.models(shape)["barrel_rot1"], shape)
    assert not np.array_equal(left[0], right[0])
    plane = (0.0, 0.0, 0.01)

    def chain(b):
        b.preprocess(1.4)
        b.sgbm()
        b.pipeline(plane=plane, point_thr=1e9, hist_thr=2)
        return ([b.read_disp(f) for f in range(n)], b.read_counts(), [b.read_hist(f) for f in range(n)],
                [b.read_points(f)[1] for f in range(n)])
    with sv.batch.Batch(n, H, W, step=1, with_bgr=True, with_points=True) as b:
        for f, (L, R) in enumerate(pairs):
            b.upload_bgr_pair(f, L, R)
        b.rectify_maps(left, right)
        b.rectify()
        got = chain(b)
    with sv.batch.Batch(n, H, W, step=1, with_bgr=True, with_points=True) as b:
        for f, (L, R) in enumerate(pairs):
            b.upload_bgr_pair(f, rn.remap(L, *left), rn.remap(R, *right))
        ref = chain(b)
    for f in range(n):
        same(got[0][f], ref[0][f], ("disp", f))
        assert np.array_equal(got[2][f], ref[2][f]) and np.array_equal(got[3][f], ref[3][f]), f
    assert np.array_equal(got[1], ref[1])
    assert any(d.any() for d in got[0])


def test_batch_rectify_behind_the_jpeg_decoder(sv):
    """decode_bgr_pair -> rectify: the oracle's remap of the decoded pictures, read back before the rectify."""
    H, W = 40, 72
    rng = np.random.default_rng(72)
    smooth = np.kron(rng.integers(0, 256, (H // 4, W // 4 + 3, 3)).astype(np.uint8), np.ones((4, 4, 1), np.uint8))
    L, R = np.ascontiguousarray(smooth[:, :W]), np.ascontiguousarray(smooth[:, 6:6 + W])
    ls, rs = [sv.dropin.jpeg_encode(L, 90)], [sv.dropin.jpeg_encode(R, 90)]
    left, right = _maps_for((H, W), 3)
    with sv.batch.Batch(1, H, W, step=1, with_bgr=False) as b:
        assert not b.decode_bgr_pair(0, ls, rs).any()
        dl, dr = b.read_bgr_pair(0)
        assert dl.any() and dr.any()
        b.rectify_maps(left, right)
        b.rectify()
        gl, gr = b.read_bgr_pair(0)
        same(gl, rn.remap(dl, *left), "L")
        same(gr, rn.remap(dr, *right), "R")
        with pytest.raises(sv.svx.SvxError, match=r"\(-4\)"):
            b.rectify()
        assert not b.decode_bgr_pair(0, ls, rs).any()          # a fresh decode: fine again
        b.rectify()
        same(b.read_bgr_pair(0)[0], rn.remap(dl, *left), "L after the second decode")


def test_batch_state_and_arguments(sv):
    H, W = 16, 24
    lib = sv.abi.lib()
    t = ctypes.c_float(0)
    rng = np.random.default_rng(3)
    L, R = rnd(rng, H, W, 3), rnd(rng, H, W, 3)
    left, right = _maps_for((H, W), 4)
    with sv.batch.Batch(2, H, W, step=1, with_bgr=False) as b:
        assert lib.sv_batch_rectify_ms(b._h, ctypes.byref(t)) == E_STATE          # before any call
        assert lib.sv_batch_rectify(b._h, 1) == E_STATE                           # no maps
        b.rectify_maps(left, right)
        assert lib.sv_batch_rectify(b._h, 1) == E_STATE                           # maps, but no pair store
        assert lib.sv_batch_rectify_ms(b._h, ctypes.byref(t)) == E_STATE
        for f in range(2):
            b.upload_bgr_pair(f, L, R)
        assert lib.sv_batch_rectify(b._h, 1) == 0
        assert lib.sv_batch_rectify_ms(b._h, ctypes.byref(t)) == 0 and t.value > 0
        assert lib.sv_batch_rectify(b._h, 1) == E_STATE                           # twice
        same(b.read_bgr_pair(1)[0], rn.remap(L, *left), "the refused call changed nothing")
        b.upload_bgr_pair(0, L, R)
        assert lib.sv_batch_rectify(b._h, 0) == 0                                 # after a fresh upload
        b.sync()
        b.synth_bgr_pair(3)
        raw = b.read_bgr_pair(0)
        b.rectify()                                                               # ... and after a synth
        same(b.read_bgr_pair(0)[1], rn.remap(raw[1], *right), "synth")
        # maps: wrong shapes and dtypes raise before anything is uploaded, a frac entry >= 1024 is SV_E_ARG
        for bad in (((left[0][:8], left[1][:8]), right), (left, (right[0][:, :8], right[1][:, :8])),
                    ((left[0], left[1][:8]), right), ((left[0][..., :1], left[1]), right)):
            with pytest.raises(ValueError):
                b.rectify_maps(*bad)
        with pytest.raises(TypeError):
            b.rectify_maps((left[0].astype(np.int32), left[1]), right)
        big = right[1].copy()
        big[H - 1, W - 1] = 1024
        with pytest.raises(ValueError):
            b.rectify_maps(left, (right[0], big))
        args = [b._h] + [sv.abi.ptr(np.ascontiguousarray(a)) for a in (left[0], left[1], right[0], big)]
        assert lib.sv_batch_rectify_maps(*args) == E_ARG
        for i in range(5):
            a = list(args)
            a[i] = None
            assert lib.sv_batch_rectify_maps(*a) == E_ARG, i
        assert lib.sv_batch_rectify(None, 1) == E_ARG and lib.sv_batch_rectify_ms(b._h, None) == E_ARG
        # the refused maps replaced nothing
        b.upload_bgr_pair(1, L, R)
        b.rectify()
        same(b.read_bgr_pair(1)[1], rn.remap(R, *right), "the maps kept")
    # a new pair shape drops the maps with the stores
    with sv.batch.Batch(1, 20, 25, step=1, with_bgr=False) as b:
        b.pair_shape(20, 160)
        m = _maps_for((20, 160), 6)
        b.rectify_maps(*m)
        b.pair_shape(20, 25)
        assert lib.sv_batch_rectify(b._h, 1) == E_STATE
        with pytest.raises(ValueError):
            b.rectify_maps(*m)


def test_remap_argument_errors(sv):
    abi = sv.abi
    f = abi.lib().sv_remap_u8
    src, dst = np.zeros((3, 8, 8, 3), np.uint8), np.zeros((3, 16, 16, 3), np.uint8)
    x, y = np.meshgrid(np.arange(16), np.arange(16))
    xy = np.ascontiguousarray(np.stack([x, y], -1).astype(np.int16))
    frac = np.zeros((16, 16), np.uint16)
    s, d, m, r = abi.ptr(src), abi.ptr(dst), abi.ptr(xy), abi.ptr(frac)
    assert f(s, 1, 8, 8, 1, m, r, 16, 16, d) == 0 and f(s, 3, 8, 8, 3, m, r, 16, 16, d) == 0
    assert f(s, 3, 8, 8, 3, m, r, 5, 7, d) == 0                                    # a smaller map in the same memory
    assert f(None, 1, 8, 8, 1, m, r, 16, 16, d) == E_ARG and f(s, 1, 8, 8, 1, m, r, 16, 16, None) == E_ARG
    assert f(s, 1, 8, 8, 1, None, r, 16, 16, d) == E_ARG and f(s, 1, 8, 8, 1, m, None, 16, 16, d) == E_ARG
    assert f(s, 1, 8, 8, 1, m, r, 4, 4, s) == E_ARG                                # dst is src
    for dh, dw in ((0, 4), (4, 0), (8193, 4), (4, 8193), (-1, 4)):
        assert f(s, 1, 8, 8, 1, m, r, dh, dw, d) == E_ARG, (dh, dw)
    for sh, sw in ((0, 8), (8, 0), (8193, 1), (1, 8193)):
        assert f(s, 1, sh, sw, 1, m, r, 4, 4, d) == E_ARG, (sh, sw)
    for ch in (0, 2, 4):
        assert f(s, 1, 8, 8, ch, m, r, 4, 4, d) == E_ARG, ch
    assert f(s, 0, 8, 8, 1, m, r, 4, 4, d) == E_ARG and f(s, -1, 8, 8, 1, m, r, 4, 4, d) == E_ARG
    frac[15, 15] = 1024
    before = dst.copy()
    assert f(s, 1, 8, 8, 1, m, r, 16, 16, d) == E_ARG and np.array_equal(dst, before)
    with pytest.raises(ValueError):
        sv.dropin.remap(src[0], xy, frac)
    with pytest.raises(TypeError):
        sv.dropin.remap(src[0].astype(np.float32), xy, np.zeros((16, 16), np.uint16))
