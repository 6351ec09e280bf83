"""GPU: the JPEG decoder of the MJPG playback — kernels/jpeg_dec.hip behind sv_jpeg_decode,
sv_jpeg_decode_many, Batch.decode_bgr_pair and svx.video.VideoCapture — byte for byte against the oracle
tests/jpeg_decode_numpy.py (pinned to libjpeg-turbo by tests/test_jpeg_decode_cpu.py) and against
tests/golden/jpeg_decode.npz, Pillow's own pixels."""
import ctypes
import hashlib
import os
import types

import numpy as np
import pytest

import hull_numpy as hn
import jpeg_decode_numpy as jd
import jpeg_numpy as jn
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -4
VARIANTS = [f"{h}x{w}-{v}" for h, w in ((40, 76), (17, 33))
            for v in ("optimize", "blocks3", "blocks1", "plain", "optimize-rows1")]


@pytest.fixture(scope="module")
def sv():
    import svx
    from svx import _abi, batch, dropin, loop, video
    if svx.device_count() < 1:
        pytest.skip("no GPU")
    return types.SimpleNamespace(svx=svx, abi=_abi, batch=batch, dropin=dropin, loop=loop, video=video)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "jpeg_decode.npz"))


def _sha(bgr):
    return hashlib.sha256(np.ascontiguousarray(bgr).tobytes()).hexdigest()[:16]


def _same(got, want, what):
    if got.shape != want.shape or not np.array_equal(got, want):
        bad = np.argwhere(got != want) if got.shape == want.shape else []
        raise AssertionError((what, got.shape, want.shape, len(bad), bad[:4].tolist() if len(bad) else None))


_BASE = {}


def _base():
    """A valid stream of three restart intervals with the Annex K tables, and its picture (made once)."""
    if not _BASE:
        s = jn.encode(jn.case_image(40, 76, "noise"), 75)
        _BASE["s"], _BASE["pic"] = s, jd.decode(s)[0]
    return _BASE["s"], _BASE["pic"]


# ---- the host entry --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", jn.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry(sv, gold, shape):
    """Every content and quality of the case list at this shape, the stream made by the device's encoder (the
    oracle's bytes, tests/test_gpu_jpeg.py): the picture equals the oracle's pixel stage on the encoder's
    coefficients, what Pillow decoded (the fixture) and, at the small shapes, the oracle's whole decode of the
    stream. 1 x 1, 17 x 33, 18 x 72: the repeated edges and the ceil(w / 2) crop; 36 x 1024, 272 x 1024: a lane with
    64 MCUs."""
    for case in (c for c in jn.cases() if (c[1], c[2]) == shape):
        name, h, w, content, q = case
        img = jn.case_image(h, w, content)
        stream = sv.dropin.jpeg_encode(img, q)
        got = sv.dropin.jpeg_decode(stream)
        _same(got, jd.pixels_of_picture(img, q), name)
        assert list(got.shape) == gold[name + "/shape"].tolist() and _sha(got) == str(gold[name + "/sha"]), name
        if name + "/bgr" in gold.files:
            _same(got, gold[name + "/bgr"], name)
        if h * w <= 40 * 1024:
            want, status = jd.decode(stream)
            assert status == 0
            _same(got, want, name)
        assert sv.dropin.jpeg_info(stream)[:3] == (h, w, -(-w // 16)), name


@pytest.mark.parametrize("variant", VARIANTS)
def test_pillow_written_streams(sv, gold, variant):
    """Streams Pillow wrote: custom Huffman tables, intervals of three MCUs and of one (RSTn wraps), no restart
    markers at all (the whole scan one lane's)."""
    stream = gold[f"pil/{variant}/stream"].tobytes()
    _same(sv.dropin.jpeg_decode(stream), gold[f"pil/{variant}/bgr"], variant)


def test_stream_without_dht(sv, gold):
    s, pic = _base()
    bare = jd.strip_dht(s)
    _same(sv.dropin.jpeg_decode(bare), pic, "no DHT")
    _same(pic, gold["40x76-noise-q75/bgr"], "fixture")


def test_row_stride_and_wide(sv):
    """Rows further apart than 3 w bytes keep what lies between them; more than 32 MCUs a row (a second picture
    workgroup) at a width that is no multiple of 16; a tall picture of one MCU column."""
    s, pic = _base()
    out = np.full((40, 256), 0xA5, np.uint8)
    status = ctypes.c_int32(-1)
    buf = np.frombuffer(s, np.uint8)
    sv.abi.call("sv_jpeg_decode", sv.abi.ptr(buf), buf.size, sv.abi.ptr(out), 40, 76, 256, ctypes.byref(status))
    assert status.value == 0 and (out[:, 228:] == 0xA5).all()
    _same(out[:, :228].reshape(40, 76, 3), pic, "ld")
    for h, w in ((17, 1040), (24, 531), (300, 9)):
        img = jn.case_image(h, w, "noise")
        stream = sv.dropin.jpeg_encode(img, 75)
        _same(sv.dropin.jpeg_decode(stream), jd.pixels_of_picture(img, 75), (h, w))


# ---- many streams ----------------------------------------------------------------------------------------------
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


def _tile_streams(sv, H, W):
    """Five tiles of H / 2 x W encoded by Batch.jpeg and read packed: (bytes, offsets of 6 entries)."""
    frames = _five_frames(H, W)
    rng = np.random.default_rng(H)
    with sv.batch.Batch(len(frames), H, W, step=1, with_bgr=True, with_points=True) as b:
        for f, d in enumerate(frames):
            b.upload(f, d, np.repeat(rng.integers(0, 256, (H, W, 1)).astype(np.uint8), 3, axis=2))
        b.pipeline(plane=(0.0, 0.0, 0.01), point_thr=1e9, hist_thr=2)
        b.road_raster()
        b.road_clean()
        b.road_hull()
        b.result()
        b.tile()
        b.jpeg(75)
        buf, offsets, total = b.read_jpegs_packed()
    return buf, np.concatenate([offsets, [total]]).astype(np.int64)


@pytest.mark.parametrize("shape", [(40, 76), (72, 1024)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_many(sv, shape):
    """A batch's tiles, encoded on the device and read packed, decoded in one call: every frame equals the oracle's
    decode of its stream."""
    H, W = shape
    buf, offs = _tile_streams(sv, H, W)
    n = len(offs) - 1
    out = np.full((n, H // 2, W, 3), 0x5A, np.uint8)
    status = np.full(n, -1, np.int32)
    sv.abi.call("sv_jpeg_decode_many", 0, sv.abi.ptr(buf), sv.abi.ptr(offs), n, H // 2, W, sv.abi.ptr(out),
                sv.abi.ptr(status))
    assert status.tolist() == [0] * n
    for f in range(n):
        want, st = jd.decode(buf[offs[f]:offs[f + 1]].tobytes())
        assert st == 0
        _same(out[f], want, (shape, f))
    ms = sv.dropin.jpeg_decode_stage_ms()
    assert len(ms) == 4 and all(v >= 0 for v in ms)
    # a run that does not start at offset 0, through the Python entry
    got, st = sv.dropin.jpeg_decode_many([buf[offs[f]:offs[f + 1]].tobytes() for f in (3, 1)])
    assert st.tolist() == [0, 0]
    _same(got[0], out[3], "3")
    _same(got[1], out[1], "1")


def test_decode_many_mixed_tables(sv, gold):
    """Streams of one size whose tables and restart intervals differ from one to the next, in one call: a wave's
    lanes span frames, and the lanes of a frame with other tables than the wave's first read theirs from memory."""
    img = jn.case_image(40, 76, "ramp")
    names = ["optimize", "blocks1", "plain", "blocks3", "optimize-rows1"]
    streams = [_base()[0]] + [gold[f"pil/40x76-{v}/stream"].tobytes() for v in names]
    streams += [sv.dropin.jpeg_encode(img, 30), jd.strip_dht(_base()[0]), sv.dropin.jpeg_encode(img, 100)]
    streams = streams + streams[::-1]
    got, status = sv.dropin.jpeg_decode_many(streams)
    assert not status.any()
    for f, s in enumerate(streams):
        want, st = jd.decode(s)
        assert st == 0
        _same(got[f], want, f)


def test_malformed_scans(sv):
    """The malformed scans of tests/test_jpeg_decode_cpu.py (the inputs tools/jpeg_decode_host_check.cpp ran under
    the host sanitizers), each in a batch of four between valid frames: its status, intact neighbours, and the next
    valid call succeeds."""
    s, pic = _base()
    for name, (bad, want_status) in jd.malformed(s).items():
        streams = [s, bad, s, s]
        got, status = sv.dropin.jpeg_decode_many(streams)
        assert status[1] != 0 and [status[0], status[2], status[3]] == [0, 0, 0], (name, status)
        assert int(status[1]) == jd.decode(bad)[1], name
        if want_status is not None:
            assert status[1] == want_status, name
        for f in (0, 2, 3):
            _same(got[f], pic, (name, f))
        one, st = sv.dropin.jpeg_decode(bad, with_status=True)
        assert st == status[1] and one.shape == pic.shape
        with pytest.raises(sv.svx.SvxError):
            sv.dropin.jpeg_decode(bad)
        _same(sv.dropin.jpeg_decode(s), pic, (name, "after"))


# ---- the batch's input stage -----------------------------------------------------------------------------------
def _pairs(n, H, W, seed):
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n):
        L = np.kron(rng.integers(0, 256, (-(-H // 4), -(-W // 4), 3), dtype=np.uint8),
                    np.ones((4, 4, 1), np.uint8))[:H, :W]
        L = (L.astype(np.int32) + rng.integers(-20, 21, L.shape)).clip(0, 255).astype(np.uint8)
        out.append((L, np.roll(L, -(6 + f), axis=1)))
    return out


def test_batch_decode_bgr_pair_40x80(sv):
    """8 pairs of 40 x 80 decoded into frames 1 .. 8 of a batch of 10: the stored pairs read back are the oracle's
    pictures; a malformed right stream is flagged alone."""
    n, H, W = 8, 40, 80
    pairs = _pairs(n, H, W, 5)
    ls = [sv.dropin.jpeg_encode(p[0], 90) for p in pairs]
    rs = [sv.dropin.jpeg_encode(p[1], 90) for p in pairs]
    with sv.batch.Batch(n + 2, H, W, step=1, with_bgr=False) as b:
        with pytest.raises(sv.svx.SvxError):
            b.decode_ms()
        status = b.decode_bgr_pair(1, ls, rs)
        assert status.shape == (2, n) and not status.any()
        assert b.decode_ms() > 0
        for f in range(n):
            L, R = b.read_bgr_pair(1 + f)
            _same(L, jd.decode(ls[f])[0], ("L", f))
            _same(R, jd.decode(rs[f])[0], ("R", f))
        bad = jd.malformed(rs[2])["swapped-rst"][0]
        status = b.decode_bgr_pair(1, ls, rs[:2] + [bad] + rs[3:])
        assert status[1, 2] == jd.RST_ORDER and status.sum() == jd.RST_ORDER
        L, R = b.read_bgr_pair(4)
        _same(R, jd.decode(rs[3])[0], "neighbour")
        # argument errors
        lib = sv.abi.lib()
        bl, ol = sv.dropin.jpeg_pack(ls)
        st = np.zeros(2 * n, np.int32)
        args = [b._h, 1, n, sv.abi.ptr(bl), sv.abi.ptr(ol), sv.abi.ptr(bl), sv.abi.ptr(ol), sv.abi.ptr(st)]
        assert lib.sv_batch_decode_bgr_pair(*args) == 0
        for i, v in ((0, None), (1, -1), (1, 3), (2, 0), (3, None), (4, None), (5, None), (6, None), (7, None)):
            a = list(args)
            a[i] = v
            assert lib.sv_batch_decode_bgr_pair(*a) == E_ARG, (i, v)
        with pytest.raises(sv.svx.SvxError, match="40 x 76"):       # another size than the pair shape
            b.decode_bgr_pair(0, [_base()[0]], [_base()[0]])
        assert lib.sv_batch_read_bgr_pair(b._h, n + 2, sv.abi.ptr(st), sv.abi.ptr(st)) == E_ARG
        assert lib.sv_batch_decode_ms(None, None) == E_ARG


def test_batch_decode_then_sgbm(sv):
    """preprocess() + sgbm() behind decode_bgr_pair give the disparity that upload_bgr_pair of the same decoded
    pictures gives. (SGBM takes no pair narrower than 128 + blockSize / 2 columns, so this half of the check runs at
    40 x 152: also a width that is no multiple of 16, the decoder's byte stores.)"""
    n, H, W = 8, 40, 152
    pairs = _pairs(n, H, W, 6)
    ls = [sv.dropin.jpeg_encode(p[0], 90) for p in pairs]
    rs = [sv.dropin.jpeg_encode(p[1], 90) for p in pairs]
    with sv.batch.Batch(n, H, W, step=1, with_bgr=False) as b:
        assert not b.decode_bgr_pair(0, ls, rs).any()
        decoded = [b.read_bgr_pair(f) for f in range(n)]
        b.preprocess(1.4)
        b.sgbm()
        got = [b.read_disp(f) for f in range(n)]
    with sv.batch.Batch(n, H, W, step=1, with_bgr=False) as b:
        for f, (L, R) in enumerate(decoded):
            _same(L, jd.decode(ls[f])[0], ("L", f))
            b.upload_bgr_pair(f, L, R)
        b.preprocess(1.4)
        b.sgbm()
        for f in range(n):
            _same(got[f], b.read_disp(f), ("disp", f))
    assert any(g.any() for g in got)


# ---- the capture -----------------------------------------------------------------------------------------------
def test_video_capture(sv, tmp_path):
    """A file made by FrameLoop(road="video") + write_batch at the loop's tile shape, two frames a batch: count, size
    and rate are the writer's, every frame equals the oracle's decode of its stream, a seek works, read() past the
    end gives (False, None); a frame with a malformed scan gives (False, None) and the next one reads."""
    from svx.loop import FrameLoop
    path = tmp_path / "lap.avi"
    vw = sv.video.VideoWriter(str(path), "MJPG", 8, (1024, 272))
    with FrameLoop(2, slots=2, source="synth", road="video", jpeg_quality=75) as loop:
        b, _ = loop.batch(loop.submit(0))
        streams = b.read_jpegs()
        vw.write_batch(b)
    s, pic = _base()
    vw.write_encoded(jd.malformed(jn.encode(jn.case_image(272, 1024, "flat"), 75))["missing-rst"][0])
    vw.write_encoded(streams[0])
    vw.release()
    want = [jd.decode(x)[0] for x in streams]
    with sv.video.VideoCapture(str(path)) as cap:
        assert cap.isOpened() and cap.get(sv.video.CAP_PROP_FRAME_COUNT) == 4
        assert (cap.get(sv.video.CAP_PROP_FRAME_WIDTH), cap.get(sv.video.CAP_PROP_FRAME_HEIGHT)) == (1024, 272)
        assert cap.get(sv.video.CAP_PROP_FPS) == 8
        for f in range(2):
            ok, frame = cap.read()
            assert ok
            _same(frame, want[f], f)
        assert cap.read() == (False, None)                       # the malformed frame
        ok, frame = cap.read()
        assert ok and np.array_equal(frame, want[0])
        assert cap.read() == (False, None) and cap.get(sv.video.CAP_PROP_POS_FRAMES) == 4
        assert cap.set(sv.video.CAP_PROP_POS_FRAMES, 1)
        ok, frame = cap.read()
        assert ok and np.array_equal(frame, want[1])
        cap.set(sv.video.CAP_PROP_POS_FRAMES, 0)
        both = cap.read_batch(2)
        assert both.shape == (2, 272, 1024, 3) and np.array_equal(both[0], want[0]) and np.array_equal(both[1], want[1])
        with pytest.raises(sv.svx.SvxError):
            cap.read_batch(5)                                    # the malformed frame among them
        cap.set(sv.video.CAP_PROP_POS_FRAMES, 2)
        frames, status = cap.read_batch(5, with_status=True)
        assert frames.shape[0] == 2 and status.tolist() == [jd.RST_COUNT, 0] and np.array_equal(frames[1], want[0])
        assert cap.read_batch(3).shape == (0, 272, 1024, 3)


# ---- argument errors -------------------------------------------------------------------------------------------
def test_argument_errors(sv):
    lib = sv.abi.lib()
    s, pic = _base()
    buf = np.frombuffer(s, np.uint8)
    out = np.empty((40, 76, 3), np.uint8)
    st = ctypes.c_int32(0)
    d = sv.abi.JpegDesc()

    def dec(stream=buf, n=None, o=out, h=40, w=76, ld=228, status=ctypes.byref(st)):
        return lib.sv_jpeg_decode(sv.abi.ptr(stream), stream.size if n is None else n, sv.abi.ptr(o), h, w, ld, status)
    assert dec() == 0 and st.value == 0
    for kw in (dict(stream=None, n=10), dict(o=None), dict(status=None), dict(h=41), dict(w=80), dict(h=0), dict(w=0),
               dict(h=4097), dict(ld=227), dict(n=-1), dict(n=3), dict(n=100)):
        assert dec(**kw) == E_ARG, kw
    assert lib.sv_jpeg_info(None, 10, ctypes.byref(d)) == E_ARG and lib.sv_jpeg_info(sv.abi.ptr(buf), buf.size, None) == E_ARG
    assert lib.sv_jpeg_info(sv.abi.ptr(buf), buf.size, ctypes.byref(d)) == 0 and (d.h, d.w, d.restart_interval) == (40, 76, 5)
    for name, (bad, word) in jd.refused(s).items():              # refused by the parser, with what was met
        with pytest.raises(sv.svx.SvxError, match=word):
            sv.dropin.jpeg_decode(bad)
    offs = np.array([0, buf.size], np.int64)
    sts = np.zeros(2, np.int32)

    def many(device=0, p=buf, o=offs, count=1, h=40, w=76, out_=out, status=sts):
        return lib.sv_jpeg_decode_many(device, sv.abi.ptr(p), sv.abi.ptr(o), count, h, w, sv.abi.ptr(out_),
                                       sv.abi.ptr(status))
    assert many() == 0
    for kw in (dict(p=None), dict(o=None), dict(out_=None), dict(status=None), dict(count=0), dict(h=0), dict(w=4097),
               dict(h=24), dict(o=np.array([0, -5], np.int64)), dict(o=np.array([4, buf.size], np.int64))):
        assert many(**kw) == E_ARG, kw
    assert many(device=99) != 0
    other = np.frombuffer(sv.dropin.jpeg_encode(jn.case_image(24, 40, "ramp"), 75), np.uint8)   # two sizes in one run
    two = np.concatenate([buf, other])
    assert many(p=two, o=np.array([0, buf.size, two.size], np.int64), count=2,
                out_=np.empty((2, 40, 76, 3), np.uint8)) == E_ARG
    assert lib.sv_jpeg_decode_stage_ms(0, None) == E_ARG
    with pytest.raises(ValueError):
        sv.dropin.jpeg_decode_many([])
    _same(sv.dropin.jpeg_decode(s), pic, "after the errors")
