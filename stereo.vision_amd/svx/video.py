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
