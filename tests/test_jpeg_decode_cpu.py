"""CPU: the JPEG decoder's contract — the oracle tests/jpeg_decode_numpy.py against what Pillow /
libjpeg-turbo decodes (tests/golden/jpeg_decode.npz, and Pillow itself where it is installed), the parser's
refusals in the oracle and in the library's host parser (sv_jpeg_info runs on the host), the statuses of malformed
scans, and svx.video.VideoCapture's RIFF reader."""
import ctypes
import hashlib
import io
import os
import struct

import numpy as np
import pytest

import jpeg_decode_numpy as jd
import jpeg_numpy as jn
from conftest import GOLDEN

VARIANTS = [f"{h}x{w}-{v}" for h, w in ((40, 76), (17, 33))
            for v in ("optimize", "blocks3", "blocks1", "plain", "optimize-rows1")]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "jpeg_decode.npz"))


_STREAM = {}


def _stream(case):
    """One case's oracle-encoded stream, made once and shared (left unchanged)."""
    name, h, w, content, q = case
    if name not in _STREAM:
        _STREAM[name] = jn.encode(jn.case_image(h, w, content), q)
    return _STREAM[name]


def _sha(bgr):
    return hashlib.sha256(np.ascontiguousarray(bgr).tobytes()).hexdigest()[:16]


def _check_fixture(gold, name, got):
    assert got.dtype == np.uint8 and list(got.shape) == gold[name + "/shape"].tolist(), name
    assert _sha(got) == str(gold[name + "/sha"]), name
    if name + "/bgr" in gold.files:
        assert np.array_equal(got, gold[name + "/bgr"]), name


def _base():
    """A valid stream of three restart intervals with the Annex K tables."""
    return _stream(next(c for c in jn.cases() if c[0] == "40x76-noise-q75"))


# ---- the oracle against libjpeg-turbo's pixels -----------------------------------------------------------------
@pytest.mark.parametrize("shape", jn.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_oracle_equals_fixture(gold, shape):
    """Every content and quality at this shape: the oracle's decode of the stream (entropy walk included) and its
    pixel stage on the encoder's coefficients both equal what Pillow decoded."""
    for case in (c for c in jn.cases() if (c[1], c[2]) == shape):
        got, status = jd.decode(_stream(case))
        assert status == 0, case[0]
        _check_fixture(gold, case[0], got)
        assert np.array_equal(jd.pixels_of_picture(jn.case_image(case[1], case[2], case[3]), case[4]), got), case[0]


def test_fixture_covers_the_list(gold):
    assert len(jn.cases()) == 117
    assert all(c[0] + "/sha" in gold.files for c in jn.cases())
    assert sum(c[0] + "/bgr" in gold.files for c in jn.cases()) >= 60
    assert all(f"pil/{v}/stream" in gold.files for v in VARIANTS)


@pytest.mark.parametrize("variant", VARIANTS)
def test_pillow_written_streams(gold, variant):
    """Streams Pillow wrote: custom Huffman tables, intervals that are no MCU rows (15 of them at 40 x 76 with one
    MCU each, so RSTn wraps), none at all."""
    stream = gold[f"pil/{variant}/stream"].tobytes()
    hdr = jd.parse(stream)
    got, status = jd.decode(stream)
    assert status == 0 and np.array_equal(got, gold[f"pil/{variant}/bgr"])
    if variant.endswith("blocks1"):
        assert hdr.ri == 1 and hdr.intervals == hdr.mcus and (hdr.intervals > 8 or variant.startswith("17x33"))
    if variant.endswith("blocks3"):
        assert hdr.ri == 3
    if variant.endswith("plain") or variant.endswith("-optimize"):
        assert hdr.ri == 0 and hdr.intervals == 1
    if "optimize" in variant:
        assert (hdr.ac[0][0], hdr.ac[0][1]) != (jn.AC_L[0], jn.AC_L[1])      # tables of its own


def test_stream_without_dht(gold):
    name = "40x76-noise-q75"
    bare = jd.strip_dht(_base())
    assert b"\xff\xc4" not in bare[:jd.parse(bare).scan_at] and len(bare) < len(_base())
    got, status = jd.decode(bare)
    assert status == 0
    _check_fixture(gold, name, got)


def test_oracle_equals_pillow_directly():
    """Where Pillow is installed: its decode of every oracle-encoded stream, of the streams it writes itself and
    of a stream without DHT."""
    Image = pytest.importorskip("PIL.Image")

    def pil(stream):
        pic = Image.open(io.BytesIO(stream))
        pic.load()
        return np.asarray(pic.convert("RGB"))[:, :, ::-1]
    for case in jn.cases():
        got, status = jd.decode(_stream(case))
        assert status == 0 and np.array_equal(got, pil(_stream(case))), case[0]
    assert np.array_equal(jd.decode(jd.strip_dht(_base()))[0], pil(jd.strip_dht(_base())))
    img = jn.case_image(40, 76, "noise", seed=9)
    for kw in (dict(optimize=True), dict(restart_marker_blocks=3), dict(restart_marker_blocks=1), dict(),
               dict(optimize=True, restart_marker_rows=1), dict(quality=97), dict(quality=12)):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(buf, "JPEG", subsampling="4:2:0",
                                                                    **{"quality": 80, **kw})
        got, status = jd.decode(buf.getvalue())
        assert status == 0 and np.array_equal(got, pil(buf.getvalue())), kw


# ---- the parser ------------------------------------------------------------------------------------------------
def _lib_info(stream):
    """(rc, descriptor, message) of the library's host parser."""
    from svx import _abi
    s = np.frombuffer(bytes(stream), np.uint8)
    d = _abi.JpegDesc()
    rc = _abi.lib().sv_jpeg_info(_abi.ptr(s) if s.size else None, s.size, ctypes.byref(d))
    return rc, d, _abi.last_error() if rc else ""


def test_parser_accepts(gold):
    for stream in [_base(), jd.strip_dht(_base())] + [gold[f"pil/{v}/stream"].tobytes() for v in VARIANTS]:
        hdr = jd.parse(stream)
        rc, d, _ = _lib_info(stream)
        assert rc == 0 and (d.h, d.w, d.restart_interval, d.header_len) == (hdr.h, hdr.w, hdr.ri, hdr.scan_at)
    # APPn and COM segments are skipped; fill bytes in front of a marker too
    s = _base()
    extra = s[:2] + b"\xff\xfe\x00\x05abc" + b"\xff\xe5\x00\x04xy" + b"\xff" + s[2:]
    assert jd.parse(extra).scan_at == jd.parse(s).scan_at + 14 and _lib_info(extra)[0] == 0
    assert np.array_equal(jd.decode(extra)[0], jd.decode(s)[0])


def test_parser_refuses_every_unsupported_kind():
    from svx import dropin
    import svx
    for name, (stream, word) in jd.refused(_base()).items():
        with pytest.raises(jd.JpegError):
            jd.parse(stream)
        rc, _, msg = _lib_info(stream)
        assert rc == -1 and word in msg, (name, msg)
        with pytest.raises(svx.SvxError, match=word):
            dropin.jpeg_info(stream)
        with pytest.raises(svx.SvxError, match=word):       # refused before anything is launched: no device needed
            dropin.jpeg_decode(stream)


def test_parser_refuses_every_truncated_header():
    s = _base()
    scan_at = jd.parse(s).scan_at
    for n in range(scan_at):
        with pytest.raises(jd.JpegError):
            jd.parse(s[:n])
        assert _lib_info(s[:n])[0] == -1, n
    assert _lib_info(s[:scan_at])[0] == 0              # the header alone parses; its scan has no EOI
    assert jd.decode(s[:scan_at])[1] != 0


def test_undefined_tables_are_refused():
    s = _base()
    no_dqt = jd._patch_segment(s, 0xC0, jd._set(8, 3))           # Y on a table no DQT defines
    one_dht = s[:s.index(b"\xff\xc4")] + s[s.index(b"\xff\xc4", s.index(b"\xff\xc4") + 2):]   # DC table 0 gone
    bad_dht = jd._patch_segment(s, 0xC4, jd._set(1, 3))          # three codes of one bit
    for stream in (no_dqt, one_dht, bad_dht):
        with pytest.raises(jd.JpegError):
            jd.parse(stream)
        assert _lib_info(stream)[0] == -1


# ---- malformed scans -------------------------------------------------------------------------------------------
def test_malformed_scans_give_a_status():
    want = jd.decode(_base())[0]
    for name, (stream, status) in jd.malformed(_base()).items():
        got, st = jd.decode(stream)                    # no exception
        assert st != 0 and (status is None or st == status), (name, st)
        assert got.shape == want.shape
        assert _lib_info(stream)[0] == 0               # the header is fine: the scan is not the parser's
    assert jd.decode(jd.malformed(_base())["cut"][0])[1] == jd.NO_EOI
    # sizes and runs out of range, from codes the Annex K tables hold
    s = bytearray(_base())
    at = jd.parse(bytes(s)).scan_at
    # DC size 0 ("00"), then ZRL ("11111111001") four times: the fourth run passes coefficient 63
    bits = "00" + "11111111001" * 4
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big").replace(b"\xff", b"\xff\x00")
    s[at:at + len(raw)] = raw
    assert jd.decode(bytes(s))[1] == jd.BAD_RUN


# ---- the AVI reader --------------------------------------------------------------------------------------------
def _write_avi(path, streams, fps=8, size=(76, 40)):
    from svx import video
    w = video.VideoWriter(str(path), "MJPG", fps, size)
    for s in streams:
        w.write_encoded(s)
    w.release()


def test_avi_reader_round_trip(tmp_path):
    from svx import video
    import svx
    streams = [jn.encode(jn.case_image(40, 76, c, seed=i), 75) for i, c in enumerate(("noise", "ramp", "flat"))]
    streams[1] += b"\x00" * (1 - len(streams[1]) % 2)     # an odd length: the chunk is padded
    assert len(streams[1]) % 2 == 1
    path = tmp_path / "a.avi"
    _write_avi(path, streams, fps=29.97)
    buf = path.read_bytes()
    # the same file without its index, and with JUNK in front of the movi list and 'rec ' lists inside it
    i = buf.index(b"idx1")
    no_idx = bytearray(buf[:i])
    no_idx[4:8] = struct.pack("<I", len(no_idx) - 8)
    (tmp_path / "b.avi").write_bytes(bytes(no_idx))
    m = buf.index(b"LIST", buf.index(b"strf"))
    junk = struct.pack("<4sI", b"JUNK", 6) + b"junk!\0"
    (tmp_path / "c.avi").write_bytes(buf[:m] + junk + buf[m:i])
    for name in ("a.avi", "b.avi", "c.avi"):
        with video.VideoCapture(str(tmp_path / name)) as cap:
            assert cap.isOpened()
            assert cap.get(video.CAP_PROP_FRAME_COUNT) == 3 and cap.get(video.CAP_PROP_FRAME_WIDTH) == 76
            assert cap.get(video.CAP_PROP_FRAME_HEIGHT) == 40 and abs(cap.get(video.CAP_PROP_FPS) - 29.97) < 1e-9
            assert [cap.read_encoded() for _ in range(3)] == streams, name
            assert cap.read_encoded() is None and cap.read() == (False, None)
            assert cap.get(video.CAP_PROP_POS_FRAMES) == 3
            assert cap.set(video.CAP_PROP_POS_FRAMES, 1) and cap.read_encoded() == streams[1]
            assert not cap.set(video.CAP_PROP_POS_FRAMES, 4) and not cap.set(video.CAP_PROP_FPS, 3)
        assert not cap.isOpened() and cap.read() == (False, None) and cap.get(video.CAP_PROP_FRAME_COUNT) == 0
    frames, w, h, rate, scale = jd.avi_index(buf)
    assert frames == streams and (w, h, rate, scale) == (76, 40, 2997, 100)
    # absolute offsets in the index (other writers)
    movi = buf.index(b"movi")
    ab = bytearray(buf)
    for k in range(3):
        at = i + 8 + 16 * k + 8
        ab[at:at + 4] = struct.pack("<I", struct.unpack_from("<I", buf, at)[0] + movi)
    (tmp_path / "d.avi").write_bytes(bytes(ab))
    with video.VideoCapture(str(tmp_path / "d.avi")) as cap:
        assert [cap.read_encoded() for _ in range(3)] == streams
    # what the reader refuses
    assert not video.VideoCapture(str(tmp_path / "missing.avi")).isOpened()
    (tmp_path / "e.avi").write_bytes(buf.replace(b"MJPG", b"XVID"))
    (tmp_path / "f.avi").write_bytes(buf + struct.pack("<4sI4s", b"RIFF", 4, b"AVIX"))
    (tmp_path / "g.avi").write_bytes(b"RIFF\x04\0\0\0WAVE")
    for name in ("e.avi", "f.avi", "g.avi"):
        with pytest.raises(svx.SvxError):
            video.VideoCapture(str(tmp_path / name))
