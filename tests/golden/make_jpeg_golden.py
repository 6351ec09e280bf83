"""Writes tests/golden/jpeg.npz: for every case of tests/jpeg_numpy.cases(), the entropy-coded segment (the bytes
after the SOS header, before EOI) that Pillow / libjpeg-turbo writes for the case's picture at its quality with
4:2:0, restart_marker_rows=1 and optimize=False; for scans over 16 KB only the length and a 16-hex sha256. Also the
DQT payloads at the three qualities and the DHT payloads. Needs Pillow; run by hand:

    python tests/golden/make_jpeg_golden.py

The pin then travels to machines without Pillow (tests/test_jpeg_cpu.py, tests/test_gpu_jpeg.py)."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_numpy as jn  # noqa: E402

LIMIT = 16384


def pillow_stream(bgr, quality):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, "JPEG", quality=quality, subsampling="4:2:0",
                                                                restart_marker_rows=1, optimize=False)
    return buf.getvalue()


def main():
    out = {}
    for name, h, w, content, q in jn.cases():
        segs, scan = jn.segments(pillow_stream(jn.case_image(h, w, content), q))
        out[name + "/len"] = np.int64(len(scan))
        out[name + "/sha"] = np.array(jn.digest(scan))
        if len(scan) <= LIMIT:
            out[name + "/scan"] = np.frombuffer(scan, np.uint8)
    for q in jn.QUALITIES:
        segs, _ = jn.segments(pillow_stream(jn.case_image(8, 8, "noise"), q))
        out[f"dqt/q{q}"] = np.frombuffer(b"".join(p for m, p in segs if m == 0xDB), np.uint8)
    out["dht"] = np.frombuffer(b"".join(p for m, p in segs if m == 0xC4), np.uint8)
    path = os.path.join(HERE, "jpeg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(jn.cases()), "cases")


if __name__ == "__main__":
    main()
