"""Writes tests/golden/jpeg_decode.npz: what Pillow / libjpeg-turbo decodes.

  <case>/shape, <case>/sha   for every case of tests/jpeg_numpy.cases(): the (h, w, 3) BGR picture Pillow decodes
                             from jn.encode(case picture, quality), as its shape and a 16-hex sha256
  <case>/bgr                 ... and the pixels themselves where the picture is at most 16 KB
  pil/<variant>/stream, bgr  streams Pillow itself wrote from 40 x 76 and 17 x 33 noise (custom Huffman tables,
                             restart intervals that are no MCU rows, more than eight intervals, none at all) with
                             the pixels Pillow decodes from them

Needs Pillow; run by hand:

    python tests/golden/make_jpeg_decode_golden.py

The pin then travels to machines without Pillow (tests/test_jpeg_decode_cpu.py, tests/test_gpu_jpeg_decode.py)."""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_numpy as jn  # noqa: E402

LIMIT = 16384
VARIANTS = {
    "optimize": dict(optimize=True),
    "blocks3": dict(restart_marker_blocks=3),
    "blocks1": dict(restart_marker_blocks=1),         # 15 intervals at 40 x 76: RSTn wraps
    "plain": dict(),
    "optimize-rows1": dict(optimize=True, restart_marker_rows=1),
}
VARIANT_SHAPES = [(40, 76), (17, 33)]


def pillow_decode(stream):
    pic = Image.open(io.BytesIO(stream))
    pic.load()
    return np.ascontiguousarray(np.asarray(pic.convert("RGB"))[:, :, ::-1])


def sha(bgr):
    return hashlib.sha256(np.ascontiguousarray(bgr).tobytes()).hexdigest()[:16]


def variant_names():
    return [f"{h}x{w}-{v}" for h, w in VARIANT_SHAPES for v in VARIANTS]


def main():
    out = {}
    for name, h, w, content, q in jn.cases():
        bgr = pillow_decode(jn.encode(jn.case_image(h, w, content), q))
        out[name + "/shape"] = np.array(bgr.shape, np.int64)
        out[name + "/sha"] = np.array(sha(bgr))
        if bgr.size <= LIMIT:
            out[name + "/bgr"] = bgr
    for h, w in VARIANT_SHAPES:
        img = jn.case_image(h, w, "noise", seed=3)
        for v, kw in VARIANTS.items():
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(buf, "JPEG", quality=80, subsampling="4:2:0",
                                                                        **kw)
            out[f"pil/{h}x{w}-{v}/stream"] = np.frombuffer(buf.getvalue(), np.uint8)
            out[f"pil/{h}x{w}-{v}/bgr"] = pillow_decode(buf.getvalue())
    path = os.path.join(HERE, "jpeg_decode.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(jn.cases()), "cases")


if __name__ == "__main__":
    main()
