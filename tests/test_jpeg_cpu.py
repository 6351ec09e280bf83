"""CPU: the JPEG stream of the MJPG recording (loop.py:49-54,82-89). The oracle tests/jpeg_numpy.py
against Pillow / libjpeg-turbo where Pillow imports (scan bytes, tables, decode) and against tests/golden/jpeg.npz
everywhere; the quantiser's multiply-and-shift, exhaustively; the AVI container of svx.video.VideoWriter."""
import io
import os
import struct

import numpy as np
import pytest

import jpeg_numpy as jn
from conftest import GOLDEN

_ENC = {}


def _encoded(case):
    """One case's picture, oracle stream and coder statistics, computed once and shared."""
    name, h, w, content, q = case
    if name not in _ENC:
        img = jn.case_image(h, w, content)
        st = jn.Stats()
        _ENC[name] = (img, jn.encode(img, q, st), st)
    return _ENC[name]


def _pillow(bgr, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=quality, subsampling="4:2:0",
                                                                restart_marker_rows=1, optimize=False)
    return buf.getvalue()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "jpeg.npz"))


def test_case_list_reaches_every_path():
    """The oracle's own output over the case list: stuffed bytes, ZRL, intervals that end on a byte boundary and
    intervals that do not."""
    assert len(jn.cases()) == 9 * (4 * 3 + 1)
    tot = jn.Stats()
    for case in jn.cases():
        st = _encoded(case)[2]
        for k in vars(tot):
            setattr(tot, k, getattr(tot, k) + getattr(st, k))
    assert tot.stuffed >= 1 and tot.zrl >= 1 and tot.aligned_ends >= 1 and tot.unaligned_ends >= 1, vars(tot)


def test_scan_bytes_equal_golden(gold):
    """The oracle's scan of every case equals the bytes Pillow wrote when the fixture was made (or their length and
    digest, for the long ones)."""
    for case in jn.cases():
        scan = jn.scan_of(_encoded(case)[1])
        assert len(scan) == int(gold[case[0] + "/len"]), case[0]
        assert jn.digest(scan) == str(gold[case[0] + "/sha"]), case[0]
        if case[0] + "/scan" in gold.files:
            assert scan == gold[case[0] + "/scan"].tobytes(), case[0]


def test_tables_equal_golden(gold):
    for q in jn.QUALITIES:
        assert b"".join(jn.dqt_payloads(q)) == gold[f"dqt/q{q}"].tobytes(), q
    assert b"".join(jn.dht_payloads()) == gold["dht"].tobytes()


def test_scan_bytes_equal_pillow():
    """Byte for byte against libjpeg through Pillow, same quality, 4:2:0, a restart interval an MCU row, the standard
    Huffman tables."""
    pytest.importorskip("PIL")
    for case in jn.cases():
        img, mine, _ = _encoded(case)
        assert jn.scan_of(mine) == jn.scan_of(_pillow(img, case[4])), case[0]


def test_tables_equal_pillow():
    pytest.importorskip("PIL")
    for q in (1, 30, 49, 50, 75, 95, 100):
        segs, _ = jn.segments(_pillow(jn.case_image(8, 8, "noise"), q))
        assert [p for m, p in segs if m == 0xDB] == jn.dqt_payloads(q), q
        assert [p for m, p in segs if m == 0xC4] == jn.dht_payloads()
        dri = [p for m, p in segs if m == 0xDD]
        assert dri == [b"\x00\x01"]


def test_pillow_decodes_the_stream():
    """Pillow opens the oracle's whole stream, and the picture equals its decode of its own stream: the same
    coefficients and tables decode alike."""
    pytest.importorskip("PIL")
    from PIL import Image
    for case in jn.cases():
        img, mine, _ = _encoded(case)
        a = Image.open(io.BytesIO(mine))
        assert a.size == (case[2], case[1]) and a.mode == "RGB"
        b = Image.open(io.BytesIO(_pillow(img, case[4])))
        assert np.array_equal(np.asarray(a), np.asarray(b)), case[0]


def test_header_layout():
    hdr = jn.header(272, 1024, 75)
    segs, _ = jn.segments(hdr + b"\xff\xd9")
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert len(hdr) == 629
    sof = segs[3][1]
    assert sof == bytes([8, 1, 16, 4, 0, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert segs[8][1] == (64).to_bytes(2, "big")


def test_quantiser_multiply_and_shift_is_the_division():
    """kernels/jpeg.hip quantises with ((|c| + 4 q) >> 3) * r >> 20, r = floor(2^20 / q) + 1, in 32 bits
    (svx_jpeg_host.h). It is (|c| + (8 q >> 1)) / (8 q) for every q in 1..255 and every |c| < 2^14. The DCT's
    outputs are far inside: samples of +-128 give |DC| <= 8192 and, through the 2-D basis, |AC| < 8192 as well (the
    orthonormal coefficient is at most 128 * 2.83 * 2.83 = 1024, the output 8 times that); the largest over the
    case list is asserted below. No product leaves 32 bits."""
    c = np.arange(1 << 14, dtype=np.uint64)[None, :]
    q = np.arange(1, 256, dtype=np.uint64)[:, None]
    r = (np.uint64(1 << 20) // q) + np.uint64(1)
    prod = ((c + 4 * q) >> np.uint64(3)) * r
    assert int(prod.max()) < 1 << 32
    assert np.array_equal(prod >> np.uint64(20), (c + ((8 * q) >> np.uint64(1))) // (8 * q))
    assert int(r.max()) < 1 << 21 and int(q.max()) < 1 << 8          # r | q << 21 fits a word
    worst = 0
    for content in jn.CONTENTS:
        img = jn.case_image(40, 76, content)
        y, cb, cr = jn.ycc(img)
        yp = np.pad(y, ((0, 8), (0, 4)), mode="edge")
        worst = max(worst, int(np.abs(jn.fdct(jn._blocks(yp))).max()))
    assert 0 < worst < 1 << 14, worst


# ---- the AVI container -----------------------------------------------------------------------------------------
def _chunks(buf, start, end):
    """[(fourcc, payload offset, size)] of the chunks in buf[start:end], sizes checked against the range."""
    out, i = [], start
    while i < end:
        cc, n = struct.unpack_from("<4sI", buf, i)
        assert i + 8 + n <= end, (cc, i, n, end)
        out.append((cc, i + 8, n))
        i += 8 + n + (n & 1)
    assert i == end or i == end + 1
    return out


def test_avi_container(tmp_path):
    """VideoWriter.write_encoded on three streams (one of odd length), walked by a small RIFF parser."""
    from svx import video
    from svx._abi import SvxError
    streams = [jn.encode(jn.case_image(8, 8, "noise", seed=s), 75) for s in range(3)]
    streams[1] += b"\x00" * (1 - (len(streams[1]) & 1))          # make one odd ...
    streams[2] += b"\x00" * (len(streams[2]) & 1)                # ... and one even
    assert len(streams[1]) & 1 and not len(streams[2]) & 1
    path = tmp_path / "out.avi"
    assert video.VideoWriter_fourcc(*"MJPG") == 0x47504A4D
    with pytest.raises(SvxError):
        video.VideoWriter(str(path), video.VideoWriter_fourcc(*"XVID"), 8, (1024, 272))
    vw = video.VideoWriter(str(path), video.VideoWriter_fourcc(*"MJPG"), 8, (1024, 272))
    assert vw.isOpened()
    for s in streams:
        vw.write_encoded(s)
    with pytest.raises(SvxError):
        vw.write_encoded(b"not a jpeg")
    vw.release()
    assert not vw.isOpened()
    vw.release()
    buf = path.read_bytes()
    riff, size, form = struct.unpack_from("<4sI4s", buf, 0)
    assert (riff, form) == (b"RIFF", b"AVI ") and size == len(buf) - 8
    top = _chunks(buf, 12, len(buf))
    assert [c[0] for c in top] == [b"LIST", b"LIST", b"idx1"]
    (_, hdrl_at, hdrl_n), (_, movi_at, movi_n), (_, idx_at, idx_n) = top
    assert buf[hdrl_at:hdrl_at + 4] == b"hdrl" and buf[movi_at:movi_at + 4] == b"movi"
    hdrl = _chunks(buf, hdrl_at + 4, hdrl_at + hdrl_n)
    assert [c[0] for c in hdrl] == [b"avih", b"LIST"]
    avih = struct.unpack_from("<14I", buf, hdrl[0][1])
    assert hdrl[0][2] == 56 and avih[0] == 125000 and avih[3] & 0x10 and avih[4] == 3 and avih[6] == 1
    assert avih[8:10] == (1024, 272) and avih[7] == max(map(len, streams))
    strl_at, strl_n = hdrl[1][1], hdrl[1][2]
    assert buf[strl_at:strl_at + 4] == b"strl"
    strl = _chunks(buf, strl_at + 4, strl_at + strl_n)
    assert [c[0] for c in strl] == [b"strh", b"strf"] and strl[0][2] == 56 and strl[1][2] == 40
    strh = struct.unpack_from("<4s4sIHHIIIIIIiI4h", buf, strl[0][1])
    assert strh[:2] == (b"vids", b"MJPG") and (strh[6], strh[7]) == (1, 8) and strh[9] == 3    # scale, rate, length
    assert strh[-2:] == (1024, 272)
    strf = struct.unpack_from("<IiiHH4sI", buf, strl[1][1])
    assert strf == (40, 1024, 272, 1, 24, b"MJPG", 1024 * 272 * 3)
    frames = _chunks(buf, movi_at + 4, movi_at + movi_n)
    assert [c[0] for c in frames] == [b"00dc"] * 3
    for (_, at, n), s in zip(frames, streams):
        assert buf[at:at + n] == s
    assert frames[2][1] - 8 == frames[1][1] + len(streams[1]) + 1      # the odd stream is padded
    assert idx_n == 48
    for k, (_, at, n) in enumerate(frames):
        cc, flags, off, ln = struct.unpack_from("<4sIII", buf, idx_at + 16 * k)
        assert cc == b"00dc" and flags & 0x10 and ln == n
        assert movi_at + off == at - 8                                  # from the 'movi' tag to the chunk header
    # a rate / scale pair for a fractional rate
    vw = video.VideoWriter(str(tmp_path / "b.avi"), "MJPG", 29.97, (8, 8))
    vw.release()
    b = (tmp_path / "b.avi").read_bytes()
    assert struct.unpack_from("<II", b, b.index(b"strh") + 8 + 20) == (100, 2997)
    assert b[-8:] == struct.pack("<4sI", b"idx1", 0)


def test_avi_refuses_to_pass_4_gib(tmp_path):
    from svx import video
    from svx._abi import SvxError
    vw = video.VideoWriter(str(tmp_path / "big.avi"), "MJPG", 8, (8, 8))
    vw._pos = (1 << 32) - 4096                     # as if that much had been written
    with pytest.raises(SvxError):
        vw.write_encoded(jn.encode(jn.case_image(8, 8, "noise"), 75) + b"\0" * 4096)
    vw._pos = 0
    vw.release()


def test_functions_sets_unchanged():
    """The recording adds no drop-in for the `functions` module: cv2.VideoWriter is not one of its attributes."""
    from svx import dropin
    assert "VideoWriter" not in dropin.PATCHED and "jpeg_encode" not in dropin.PATCHED
    assert set(dropin.PINNED) | set(dropin.UNPINNED) <= set(dropin.PATCHED)
