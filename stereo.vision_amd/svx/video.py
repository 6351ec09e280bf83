"""The MJPG recording of the reference's loop (loop.py:49-54,82-89): cv2.VideoWriter(name, MJPG, 8, (1024, 272)),
write(image), release(), with the pictures encoded on the GPU (include/svx.h, sv_jpeg_encode / sv_batch_jpeg;
DESIGN §7.11) and a plain RIFF AVI written here.

    video_writer = svx.video.VideoWriter(name, svx.video.VideoWriter_fourcc(*"MJPG"), 8, (1024, 272))
    video_writer.write(image)          # a host BGR picture, encoded on the device
    video_writer.write_batch(batch)    # or a device batch's streams (Batch.jpeg() / FrameLoop(road="video"))
    video_writer.release()

The file: RIFF 'AVI ' { LIST 'hdrl' { 'avih', LIST 'strl' { 'strh' vids/MJPG, 'strf' BITMAPINFOHEADER } },
LIST 'movi' { '00dc' chunks padded to even length }, 'idx1' }. The frame count and the sizes are patched on release().
One RIFF only (no OpenDML): a write that would take the file past 4 GiB raises. The JPEG streams are libjpeg's bytes
at the same settings; parity with cv2's own MJPG encoder and its container details is unpinned.

And its counterpart, the playback: cv2.VideoCapture's surface over such a file, the frames decoded on
the GPU (sv_jpeg_decode / sv_jpeg_decode_many) to libjpeg-turbo's pixels.

    cap = svx.video.VideoCapture(name)
    n, fps = int(cap.get(svx.video.CAP_PROP_FRAME_COUNT)), cap.get(svx.video.CAP_PROP_FPS)
    ok, frame = cap.read()             # (h, w, 3) uint8 BGR; (False, None) past the end or for a malformed frame
    frames = cap.read_batch(64)        # the next 64 frames in one upload and one read-back
    cap.set(svx.video.CAP_PROP_POS_FRAMES, 0)
    cap.release()

The reader takes one RIFF 'AVI ' whose first stream is MJPG video: 'hdrl' ('avih', 'strh', 'strf'), a 'movi' list of
'00dc' / '00db' chunks (inside 'rec ' lists too), 'idx1' when present (offsets from the 'movi' tag or from the
file's start), otherwise a walk of the 'movi' list; 'JUNK' and other streams' chunks are skipped. Another codec or an
OpenDML file (a second RIFF, 'AVIX') raises SvxError. Parity with cv2's own MJPG decoder is unpinned.
"""
import struct
from fractions import Fraction

import numpy as np

from ._abi import SvxError

_LIMIT = (1 << 32) - 1           # a RIFF size field
_AVIF_HASINDEX = 0x10
_AVIIF_KEYFRAME = 0x10
_HDRL = 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))   # the hdrl list's payload
_MOVI_AT = 12 + 8 + _HDRL          # file offset of LIST 'movi'


# cv2's property ids
CAP_PROP_POS_FRAMES = 1
CAP_PROP_FRAME_WIDTH = 3
CAP_PROP_FRAME_HEIGHT = 4
CAP_PROP_FPS = 5
CAP_PROP_FOURCC = 6
CAP_PROP_FRAME_COUNT = 7


def VideoWriter_fourcc(c1, c2, c3, c4):  # noqa: N802  (cv2's name)
    """cv2.VideoWriter_fourcc: the four characters as a little-endian int."""
    return ord(c1) | ord(c2) << 8 | ord(c3) << 16 | ord(c4) << 24


class VideoWriter:
    """cv2.VideoWriter for MJPG in an AVI (loop.py:49-54,82-89). fourcc: VideoWriter_fourcc(*"MJPG") (or "MJPG"), any
    other raises SvxError. fps: a rate / scale pair is stored (8 -> 8 / 1, 29.97 -> 2997 / 100). frameSize: (w, h).
    quality: the JPEG quality of write() (1..100; 75, the default of cv2's writer as far as known, unpinned)."""

    def __init__(self, filename, fourcc, fps, frameSize, isColor=True, quality=75):  # noqa: N803
        if isinstance(fourcc, str):
            fourcc = VideoWriter_fourcc(*fourcc)
        if int(fourcc) != VideoWriter_fourcc(*"MJPG"):
            raise SvxError(f"svx.video.VideoWriter writes MJPG only, not fourcc {int(fourcc):#x}")
        w, h = (int(v) for v in frameSize)
        if not (1 <= w <= 4096 and 1 <= h <= 4096):
            raise SvxError(f"frame size {(w, h)} outside 1..4096")
        rate = Fraction(fps).limit_denominator(100000)
        if rate <= 0:
            raise SvxError(f"fps must be positive, got {fps}")
        self.size, self.quality = (w, h), int(quality)
        self._rate, self._scale = rate.numerator, rate.denominator
        self._index = []          # (offset from 'movi', length) of every frame
        self._pos = 0             # bytes of the movi list's payload behind the 'movi' tag
        self._max = 0
        try:
            self._f = open(filename, "wb")
        except OSError:
            self._f = None        # cv2's writer reports this through isOpened()
            return
        self._f.write(self._header())

    def isOpened(self):  # noqa: N802
        return self._f is not None

    def _header(self):
        w, h = self.size
        n, movi = len(self._index), 4 + self._pos
        idx = 16 * n
        riff = 4 + (8 + _HDRL) + (8 + movi) + (8 + idx)
        usec = (1000000 * self._scale + self._rate // 2) // self._rate
        bps = min(_LIMIT, self._max * self._rate // self._scale)
        out = struct.pack("<4sI4s", b"RIFF", riff, b"AVI ")
        out += struct.pack("<4sI4s", b"LIST", _HDRL, b"hdrl")
        out += struct.pack("<4sI14I", b"avih", 56, usec, bps, 0, _AVIF_HASINDEX, n, 0, 1, self._max, w, h, 0, 0, 0, 0)
        out += struct.pack("<4sI4s", b"LIST", 4 + (8 + 56) + (8 + 40), b"strl")
        out += struct.pack("<4sI4s4sIHHIIIIIIiI4h", b"strh", 56, b"vids", b"MJPG", 0, 0, 0, 0, self._scale, self._rate,
                           0, n, self._max, -1, 0, 0, 0, w, h)
        out += struct.pack("<4sIIiiHH4sIiiII", b"strf", 40, 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        out += struct.pack("<4sI4s", b"LIST", movi, b"movi")
        assert len(out) == _MOVI_AT + 12
        return out

    def write_encoded(self, stream):
        """One frame that is already a JPEG stream (bytes)."""
        if self._f is None:
            return
        data = bytes(stream)
        if data[:2] != b"\xff\xd8":
            raise SvxError("write_encoded takes a JPEG stream (it starts with SOI)")
        pad = len(data) & 1
        # what the file would be with this frame and the index behind it
        total = _MOVI_AT + 12 + self._pos + 8 + len(data) + pad + 8 + 16 * (len(self._index) + 1)
        if total > _LIMIT:
            raise SvxError("the AVI would pass 4 GiB (one RIFF, no OpenDML): release() and start another file")
        self._f.write(struct.pack("<4sI", b"00dc", len(data)) + data + b"\0" * pad)
        self._index.append((4 + self._pos, len(data)))
        self._pos += 8 + len(data) + pad
        self._max = max(self._max, len(data))

    def write(self, image):
        """A host picture, (h, w, 3) uint8 BGR (or (h, w) grey), encoded on the device. A picture of another size
        than the writer's is ignored, as cv2's writer ignores it."""
        if self._f is None:
            return
        from . import dropin
        a = np.asarray(image)
        if a.ndim < 2 or (a.shape[1], a.shape[0]) != self.size:
            return
        self.write_encoded(dropin.jpeg_encode(a, self.quality))

    def write_batch(self, b):
        """The streams of a device batch (after Batch.jpeg(), or a batch of FrameLoop(road="video")), in frame order,
        read through the pack in one copy. A frame that overflowed its slot raises before anything is written."""
        if self._f is None:
            return
        if (b.W, b.H // 2) != self.size:
            raise SvxError(f"the batch's tiles are {(b.W, b.H // 2)}, the writer's frames {self.size}")
        sizes = b.jpeg_sizes()
        bad = np.flatnonzero(sizes < 0)
        if bad.size:
            raise SvxError(f"frame {int(bad[0])}'s stream needs {-int(sizes[bad[0]])} bytes and overflowed its slot: "
                           "run jpeg() with a larger cap")
        for s in b.read_jpegs():
            self.write_encoded(s)

    def release(self):
        """The index, then the frame count and the sizes into the headers; closes the file."""
        if self._f is None:
            return
        f, self._f = self._f, None
        try:
            f.write(struct.pack("<4sI", b"idx1", 16 * len(self._index)))
            f.write(b"".join(struct.pack("<4sIII", b"00dc", _AVIIF_KEYFRAME, off, n) for off, n in self._index))
            f.seek(0)
            f.write(self._header())
        finally:
            f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


def _avi_index(f):
    """(frames as (file offset, length), w, h, rate, scale) of an open AVI file; SvxError for what is not one RIFF
    'AVI ' with MJPG video in its first stream."""
    f.seek(0, 2)
    size = f.tell()
    f.seek(0)
    head = f.read(12)
    if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
        raise SvxError("not a RIFF 'AVI ' file")
    info, movi, idx = {}, None, None
    pos = 12
    while pos + 8 <= size:
        f.seek(pos)
        cc, n = struct.unpack("<4sI", f.read(8))
        if cc == b"RIFF":
            raise SvxError("an OpenDML file (a second RIFF, 'AVIX'): one RIFF 'AVI ' only")
        body = pos + 8
        if cc == b"LIST":
            kind = f.read(4)
            if kind == b"hdrl":
                _parse_hdrl(f.read(max(0, min(n, size - body) - 4)), info)
            elif kind == b"movi":
                movi = (body, min(body + n, size))       # from the 'movi' tag to the list's end
        elif cc == b"idx1":
            idx = f.read(min(n, size - body))
        pos = body + n + (n & 1)
    if "handler" not in info or movi is None:
        raise SvxError("an AVI without a video stream header or a 'movi' list")
    codecs = {info["handler"].upper(), info.get("compression", b"MJPG").upper()}
    if info["type"] != b"vids" or codecs != {b"MJPG"}:
        raise SvxError(f"the first stream is {info['type']!r} / {info['handler']!r} / "
                       f"{info.get('compression')!r}, not MJPG video")
    frames = _frames_from_idx(f, idx, movi, size) if idx else None
    if frames is None:
        frames = _frames_from_movi(f, movi)
    return frames, info.get("w", 0), info.get("h", 0), info.get("rate", 0), info.get("scale", 1)


def _parse_hdrl(buf, info):
    """The first stream's 'strh' and 'strf' (and 'avih' for the size when 'strf' gives none) out of an 'hdrl' list."""
    i = 0
    while i + 8 <= len(buf):
        cc, n = struct.unpack_from("<4sI", buf, i)
        if cc == b"LIST":                 # 'strl': its chunks follow
            i += 12
            continue
        p = buf[i + 8:i + 8 + n]
        if cc == b"avih" and len(p) >= 40:
            info.setdefault("w", struct.unpack_from("<I", p, 32)[0])
            info.setdefault("h", struct.unpack_from("<I", p, 36)[0])
        elif cc == b"strh" and "handler" not in info and len(p) >= 28:
            info["type"], info["handler"] = p[:4], p[4:8]
            info["scale"], info["rate"] = struct.unpack_from("<II", p, 20)
        elif cc == b"strf" and "compression" not in info and "handler" in info and len(p) >= 20:
            w, h = struct.unpack_from("<ii", p, 4)
            info["w"], info["h"], info["compression"] = w, abs(h), p[16:20]
        i += 8 + n + (n & 1)


def _frames_from_idx(f, idx, movi, size):
    """The video frames of an 'idx1', offsets taken from the 'movi' tag or from the file's start, whichever finds the
    first frame's chunk; None when neither does."""
    ent = [struct.unpack_from("<4sIII", idx, i) for i in range(0, len(idx) - 15, 16)]
    ent = [(off, n) for cc, _, off, n in ent if cc in (b"00dc", b"00db")]
    if not ent:
        return []
    for base in (movi[0], 0):
        f.seek(base + ent[0][0])
        head = f.read(8)
        if len(head) == 8 and head[:4] in (b"00dc", b"00db") and struct.unpack("<I", head[4:])[0] == ent[0][1]:
            break
    else:
        return None
    frames = [(base + off + 8, n) for off, n in ent]
    return frames if all(at + n <= size for at, n in frames) else None


def _frames_from_movi(f, movi):
    pos, end, frames = movi[0] + 4, movi[1], []
    while pos + 8 <= end:
        f.seek(pos)
        cc, n = struct.unpack("<4sI", f.read(8))
        if cc == b"LIST":                 # 'rec ': its chunks follow
            pos += 12
            continue
        if cc in (b"00dc", b"00db") and pos + 8 + n <= end:
            frames.append((pos + 8, n))
        pos += 8 + n + (n & 1)
    return frames


class VideoCapture:
    """cv2.VideoCapture over an MJPG AVI (the files VideoWriter writes, and other writers' of the same kind), frames
    decoded on the GPU. A file that cannot be opened gives isOpened() == False, as cv2's does; one that is not an
    MJPG AVI raises SvxError."""

    def __init__(self, filename):
        self._f, self._frames, self._pos = None, [], 0
        self._size, self._rate, self._scale = (0, 0), 0, 1
        try:
            self._f = open(filename, "rb")
        except OSError:
            return
        try:
            self._frames, w, h, self._rate, self._scale = _avi_index(self._f)
        except Exception:
            self._f.close()
            self._f = None
            raise
        self._size = (w, h)

    def isOpened(self):  # noqa: N802
        return self._f is not None

    def get(self, prop):
        if self._f is None:
            return 0.0
        if prop == CAP_PROP_POS_FRAMES:
            return float(self._pos)
        if prop == CAP_PROP_FRAME_COUNT:
            return float(len(self._frames))
        if prop == CAP_PROP_FRAME_WIDTH:
            return float(self._size[0])
        if prop == CAP_PROP_FRAME_HEIGHT:
            return float(self._size[1])
        if prop == CAP_PROP_FPS:
            return self._rate / self._scale if self._scale else 0.0
        if prop == CAP_PROP_FOURCC:
            return float(VideoWriter_fourcc(*"MJPG"))
        return 0.0

    def set(self, prop, value):
        """CAP_PROP_POS_FRAMES: the frame the next read() returns (0 .. the frame count)."""
        if self._f is None or prop != CAP_PROP_POS_FRAMES or not 0 <= int(value) <= len(self._frames):
            return False
        self._pos = int(value)
        return True

    def read_encoded(self):
        """The next frame's JPEG stream (bytes), or None past the end."""
        if self._f is None or self._pos >= len(self._frames):
            return None
        at, n = self._frames[self._pos]
        self._pos += 1
        self._f.seek(at)
        return self._f.read(n)

    def read(self):
        """(True, the next frame as (h, w, 3) uint8 BGR), or (False, None) past the end, for a frame that is no
        baseline 4:2:0 JPEG and for one whose scan is malformed (the position moves on)."""
        s = self.read_encoded()
        if s is None:
            return False, None
        from . import dropin
        try:
            frame, status = dropin.jpeg_decode(s, with_status=True)
        except SvxError:
            return False, None
        return (True, frame) if status == 0 else (False, None)

    def read_batch(self, n, with_status=False):
        """The next min(n, frames left) frames as (m, h, w, 3) uint8, decoded in one upload and one read-back; they
        must share one size. A malformed frame raises SvxError, unless with_status is set: then the result is
        (frames, (m,) int32 statuses)."""
        streams = []
        while len(streams) < int(n):
            s = self.read_encoded()
            if s is None:
                break
            streams.append(s)
        if not streams:
            frames, status = np.empty((0, self._size[1], self._size[0], 3), np.uint8), np.zeros(0, np.int32)
        else:
            from . import dropin
            frames, status = dropin.jpeg_decode_many(streams)
        if with_status:
            return frames, status
        bad = np.flatnonzero(status)
        if bad.size:
            raise SvxError(f"frame {self._pos - len(streams) + int(bad[0])} has a malformed scan "
                           f"(status {int(status[bad[0]])})")
        return frames

    def release(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
