"""GPU: the JPEG stream of the MJPG recording (loop.py:49-54,82-89) — kernels/jpeg.hip behind
sv_jpeg_encode, the batch stage (Batch.jpeg, the pack), the frame loop (road="video") and svx.video.VideoWriter —
byte for byte against the oracle tests/jpeg_numpy.py (pinned to libjpeg by tests/test_jpeg_cpu.py) and against
tests/golden/jpeg.npz."""
import ctypes
import io
import os
import types

import numpy as np
import pytest

import hull_numpy as hn
import jpeg_numpy as jn
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

E_ARG, E_CAP, E_STATE = -1, -3, -4


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import _abi, batch, dropin, loop, video
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, abi=_abi, batch=batch, dropin=dropin, loop=loop, video=video)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "jpeg.npz"))


_REF = {}


def _ref(case):
    """One case's picture and oracle stream, computed once and shared (left unchanged)."""
    name, h, w, content, q = case
    if name not in _REF:
        img = jn.case_image(h, w, content)
        _REF[name] = (img, jn.encode(img, q))
    return _REF[name]


def _same_stream(got, want, what):
    if got != want:
        n = min(len(got), len(want))
        first = next((i for i in range(n) if got[i] != want[i]), n)
        raise AssertionError((what, len(got), len(want), first, got[first:first + 8].hex(), want[first:first + 8].hex()))


# ---- the host entry --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", jn.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry(sv, gold, shape):
    """Every content and quality of the case list at this shape: the whole stream equals the oracle's, its scan the
    bytes libjpeg wrote into the fixture, and Pillow (where installed) decodes it."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for case in (c for c in jn.cases() if (c[1], c[2]) == shape):
        img, want = _ref(case)
        got = sv.dropin.jpeg_encode(img, case[4])
        _same_stream(got, want, case[0])
        scan = jn.scan_of(got)
        assert len(scan) == int(gold[case[0] + "/len"]) and jn.digest(scan) == str(gold[case[0] + "/sha"]), case[0]
        if case[0] + "/scan" in gold.files:
            assert scan == gold[case[0] + "/scan"].tobytes(), case[0]
        assert len(got) <= sv.abi.lib().sv_jpeg_bound(shape[0], shape[1]), case[0]
        if Image is not None:
            pic = Image.open(io.BytesIO(got))
            pic.load()
            assert pic.size == (shape[1], shape[0])


@pytest.mark.parametrize("shape", [(17, 1040), (8, 2100)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_wide_pictures(sv, shape):
    """More than 64 MCUs an interval: a lane of the interval's wave codes two (65 MCUs: 33 lanes busy, the transform's
    third workgroup holds one MCU) or three MCUs in a row (132 MCUs, byte loads, a partial last MCU)."""
    h, w = shape
    for content, q in (("noise", 75), ("impulse", 100), ("flat", 30)):
        img = jn.case_image(h, w, content)
        _same_stream(sv.dropin.jpeg_encode(img, q), jn.encode(img, q), (shape, content, q))


def test_grey_and_row_stride(sv):
    """A grey picture is encoded as B = G = R; rows further apart than 3 w bytes give the same stream."""
    g = jn.case_image(24, 40, "noise")[:, :, 0].copy()
    _same_stream(sv.dropin.jpeg_encode(g, 75), jn.encode(g, 75), "grey")
    img = jn.case_image(24, 40, "noise")
    wide = np.zeros((24, 64, 3), np.uint8)
    wide[:, :40] = img
    cap = int(sv.abi.lib().sv_jpeg_bound(24, 40))
    out = np.empty(cap, np.uint8)
    size = ctypes.c_int64(0)
    sv.abi.call("sv_jpeg_encode", sv.abi.ptr(wide), 24, 40, 3 * 64, 75, sv.abi.ptr(out), cap, ctypes.byref(size))
    _same_stream(out[: size.value].tobytes(), jn.encode(img, 75), "ld")


def test_argument_errors(sv):
    f = sv.abi.lib().sv_jpeg_encode
    img = np.zeros((16, 16, 3), np.uint8)
    out = np.empty(8192, np.uint8)
    size = ctypes.c_int64(0)

    def call(h=16, w=16, ld=48, q=75, null=None, cap=8192):
        p = [sv.abi.ptr(img), sv.abi.ptr(out), ctypes.byref(size)]
        if null is not None:
            p[null] = None
        return f(p[0], h, w, ld, q, p[1], cap, p[2])
    assert call() == 0 and size.value > 0
    for kw in (dict(h=0), dict(w=0), dict(h=-1), dict(h=4097), dict(w=4097), dict(q=0), dict(q=101), dict(q=-5),
               dict(ld=47), dict(cap=-1), dict(null=0), dict(null=1), dict(null=2)):
        assert call(**kw) == E_ARG, kw
    assert sv.abi.lib().sv_jpeg_bound(0, 16) == 0 and sv.abi.lib().sv_jpeg_bound(16, 4097) == 0
    with pytest.raises(TypeError):
        sv.dropin.jpeg_encode(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        sv.dropin.jpeg_encode(np.zeros((8, 8, 4), np.uint8))
    with pytest.raises(sv.svx.SvxError):
        sv.dropin.jpeg_encode(np.zeros((8, 8, 3), np.uint8), quality=0)
    with pytest.raises(sv.svx.SvxError):
        sv.video.VideoWriter("/dev/null", sv.video.VideoWriter_fourcc(*"XVID"), 8, (16, 16))


def test_overflow(sv):
    """Noise at quality 100 into half the bytes it needs: the overflow status, the needed size, and nothing written
    (a guard region behind out + cap, and out itself, keep their bytes)."""
    case = next(c for c in jn.cases() if c[0] == "40x76-noise-q100")
    img, want = _ref(case)
    cap = len(want) // 2
    buf = np.full(cap + 4096, 0xA5, np.uint8)
    size = ctypes.c_int64(0)
    rc = sv.abi.lib().sv_jpeg_encode(sv.abi.ptr(img), 40, 76, 3 * 76, 100, sv.abi.ptr(buf), cap, ctypes.byref(size))
    assert rc == E_CAP and size.value == len(want)
    assert (buf[cap:] == 0xA5).all() and (buf == 0xA5).all()
    rc = sv.abi.lib().sv_jpeg_encode(sv.abi.ptr(img), 40, 76, 3 * 76, 100, sv.abi.ptr(buf), len(want),
                                     ctypes.byref(size))                     # exactly enough
    assert rc == 0 and buf[: len(want)].tobytes() == want and (buf[len(want):] == 0xA5).all()


def test_bound_covers_every_case(sv):
    bound = sv.abi.lib().sv_jpeg_bound
    for case in jn.cases():
        assert len(_ref(case)[1]) <= bound(case[1], case[2]), case[0]
    assert bound(1, 1) == 640 + 2 * 1244 + 2 and bound(272, 1024) == 640 + 17 * (2 * 1244 * 64 + 2)


# ---- the batch path --------------------------------------------------------------------------------------------
def _blocks(H, W, *blocks):
    a = np.zeros((H, W), np.uint8)
    for y0, y1, x0, x1 in blocks:
        a[y0:y1, x0:x1] = 200
    return a


def _five_frames(H, W):
    """tests/test_gpu_tile.py's recipe: full, empty, full, two blobs, a filled ring."""
    ring = (hn.fill_polygon((H, W), hn.polygon_steep_shallow(H, W)) != 0).astype(np.uint8) * 200
    return [np.full((H, W), 200, np.uint8), np.zeros((H, W), np.uint8), np.full((H, W), 200, np.uint8),
            _blocks(H, W, (2, 2 + H // 3, 5, 5 + W // 4), (H - 4 - H // 3, H - 4, W - 9 - W // 3, W - 9)), ring]


def _to_tile(b):
    b.road_raster()
    b.road_clean()
    b.road_hull()
    b.result()
    b.tile()


def _run_batch(sv, H, W, mode, bits):
    frames_disp = _five_frames(H, W)
    n = len(frames_disp)
    rng = np.random.default_rng(H + n)
    plane = (0.0, 0.0, 0.01)
    lib = sv.abi.lib()
    with sv.batch.Batch(n, H, W, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode(mode)
        b.road_bits(bits)
        for f, d in enumerate(frames_disp):
            g = rng.integers(0, 256, (H, W, 1)).astype(np.uint8)
            b.upload(f, d, np.repeat(g, 3, axis=2))
        b.pipeline(plane=plane, point_thr=1e9, hist_thr=2)
        b.road_raster()
        b.road_clean()
        b.road_hull()
        b.result()
        assert lib.sv_batch_jpeg(b._h, 75, 0, 1) == E_STATE          # no tile yet
        b.tile()
        with pytest.raises(sv.svx.SvxError):                          # ... and no streams yet
            b.read_jpeg(0)
        with pytest.raises(sv.svx.SvxError):
            b.jpeg_sizes()
        assert lib.sv_batch_jpeg(b._h, 0, 0, 1) == E_ARG and lib.sv_batch_jpeg(b._h, 101, 0, 1) == E_ARG
        assert lib.sv_batch_jpeg(b._h, 75, -1, 1) == E_ARG
        tiles = [b.read_tile(f) for f in range(n)]
        want = [jn.encode(t, 75) for t in tiles]
        cap = int(lib.sv_jpeg_bound(H // 2, W))
        b.jpeg(75, cap)
        assert b.jpeg_ms() > 0
        got = [b.read_jpeg(f) for f in range(n)]
        for f in range(n):
            _same_stream(got[f], want[f], (H, W, f))
            _same_stream(sv.dropin.jpeg_encode(tiles[f], 75), want[f], ("host entry", H, W, f))
        assert b.jpeg_sizes().tolist() == [len(s) for s in want]
        out = np.empty(8, np.uint8)                                   # too small a buffer: the needed size
        size = ctypes.c_int64(0)
        assert lib.sv_batch_read_jpeg(b._h, 0, sv.abi.ptr(out), 8, ctypes.byref(size)) == E_CAP
        assert size.value == len(want[0])
        offs = np.empty(n, np.int64)
        total = ctypes.c_int64(0)
        big = np.empty(sum(map(len, want)) + 64, np.uint8)
        assert lib.sv_batch_read_jpeg_packed(b._h, sv.abi.ptr(big), big.size, sv.abi.ptr(offs),
                                             ctypes.byref(total)) == E_STATE     # not packed yet
        buf, offsets, total = b.read_jpegs_packed()
        assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(s) for s in want])[:-1]]).tolist()
        assert total == sum(map(len, want)) and buf[:total].tobytes() == b"".join(want)
        assert b.read_jpegs() == want
        b.jpeg(75, cap)                                              # nothing it reads is touched: the same again
        for f in range(n):
            assert b.read_jpeg(f) == want[f], f
            assert np.array_equal(b.read_tile(f), tiles[f]), f
        assert lib.sv_batch_read_jpeg_packed(b._h, sv.abi.ptr(big), big.size, sv.abi.ptr(offs),
                                             ctypes.byref(ctypes.c_int64(0))) == E_STATE   # new streams: pack again
        # a higher quality and the default slot (half the raw tile)
        b.jpeg(100)
        sizes100 = b.jpeg_sizes()
        for f in range(n):
            w100 = jn.encode(tiles[f], 100)
            assert abs(int(sizes100[f])) == len(w100), f
            if sizes100[f] > 0:
                _same_stream(b.read_jpeg(f), w100, ("q100", f))
        # one slot too small for the largest stream: that frame is flagged, its neighbours are intact
        lens = [len(s) for s in want]
        small = max(lens) - 1
        b.jpeg(75, small)
        sizes = b.jpeg_sizes()
        over = [f for f in range(n) if lens[f] > small]
        assert 1 <= len(over) < n
        assert sizes.tolist() == [-lens[f] if f in over else lens[f] for f in range(n)]
        for f in range(n):
            if f in over:
                with pytest.raises(sv.svx.SvxError):
                    b.read_jpeg(f)
            else:
                assert b.read_jpeg(f) == want[f], f
        packed = b.read_jpegs()
        assert packed == [b"" if f in over else want[f] for f in range(n)]
        w = sv.video.VideoWriter(os.devnull, "MJPG", 8, (W, H // 2))
        with pytest.raises(sv.svx.SvxError):                          # the writer refuses a batch with a gap
            w.write_batch(b)
        w.release()
        # whatever makes the tile stale makes the streams stale
        b.jpeg(75, cap)
        for stage in (b.tile, b.result, b.road_hull, lambda: b.pipeline(plane=plane, point_thr=1e9, hist_thr=2)):
            stage()
            for call in (b.jpeg_sizes, b.jpeg_ms, lambda: b.read_jpeg(0), b.read_jpegs):
                with pytest.raises(sv.svx.SvxError):
                    call()
            assert lib.sv_batch_jpeg_pack(b._h, 1) == E_STATE
            if stage != b.tile:
                assert lib.sv_batch_jpeg(b._h, 75, 0, 1) == E_STATE
            if stage == b.road_hull:
                b.result()
                b.tile()
            elif stage == b.result:
                b.tile()
            elif stage != b.tile:
                _to_tile(b)
            b.jpeg(75, cap)
            assert b.read_jpeg(n - 1) == want[n - 1]


def test_batch_72x1024(sv):
    """Tiles of 36 x 1024: 64 lanes an interval, a dummy luma block row, 16-byte loads."""
    _run_batch(sv, 72, 1024, "resident", True)


def test_batch_40x76(sv):
    """Tiles of 20 x 76: five MCUs an interval, dummy blocks both ways, byte loads (rows of 228 bytes)."""
    _run_batch(sv, 40, 76, "auto", False)


# ---- the frame loop --------------------------------------------------------------------------------------------
def test_frame_loop_video(sv):
    """road="video" on two 2-frame synthetic batches in flight: every frame's stream equals the oracle on that
    batch's read_tile; road="tile" afterwards makes no stream."""
    from svx.loop import FrameLoop
    frames = 2
    with FrameLoop(frames, slots=2, source="synth", road="video", jpeg_quality=75) as loop:
        s0 = loop.submit(0)
        s1 = loop.submit(frames)
        for seq in (s0, s1):
            b, _ = loop.batch(seq)
            streams = b.read_jpegs()
            for f in range(frames):
                want = jn.encode(b.read_tile(f), 75)
                _same_stream(b.read_jpeg(f), want, (seq, f))
                _same_stream(streams[f], want, ("packed", seq, f))
        with pytest.raises(sv.svx.SvxError):                          # after the first submit
            sv.abi.call("sv_loop_jpeg", loop._h, 50, 0)
    with FrameLoop(frames, slots=2, source="synth", road="tile") as loop:
        b, _ = loop.batch(loop.submit(0))
        assert b.read_tile(0).shape == (272, 1024, 3)
        with pytest.raises(sv.svx.SvxError):
            b.read_jpeg(0)
    with pytest.raises(sv.svx.SvxError):
        FrameLoop(frames, H=42, W=64, slots=2, source="synth", road="video")
    with pytest.raises(sv.svx.SvxError):
        FrameLoop(frames, slots=2, source="synth", road="video", jpeg_quality=0)


# ---- the writer ------------------------------------------------------------------------------------------------
def test_video_writer(sv, tmp_path):
    """write() of three host pictures (and one of another size, ignored) and write_batch() of one batch: the file
    holds the streams of jpeg_encode and read_jpeg, in order."""
    H, W = 72, 1024
    pics = [jn.case_image(H // 2, W, c) for c in ("noise", "ramp", "impulse")]
    path = tmp_path / "rec.avi"
    vw = sv.video.VideoWriter(str(path), sv.video.VideoWriter_fourcc(*"MJPG"), 8, (W, H // 2))
    assert vw.isOpened()
    for p in pics:
        vw.write(p)
    vw.write(np.zeros((H, W, 3), np.uint8))                          # another size: ignored, as cv2's writer does
    with sv.batch.Batch(2, H, W, step=1, with_bgr=True, with_points=True) as b:
        for f, d in enumerate(_five_frames(H, W)[3:]):
            b.upload(f, d, np.repeat(jn.case_image(H, W, "noise", seed=f)[:, :, :1], 3, axis=2))
        b.pipeline(plane=(0.0, 0.0, 0.01), point_thr=1e9, hist_thr=2)
        _to_tile(b)
        b.jpeg(75)
        from_batch = [b.read_jpeg(f) for f in range(2)]
        vw.write_batch(b)
    vw.release()
    frames = jn.avi_frames(path.read_bytes())
    assert frames == [sv.dropin.jpeg_encode(p, 75) for p in pics] + from_batch
    assert frames[:3] == [jn.encode(p, 75) for p in pics]
