#!/usr/bin/env python3
"""Glyph-tip fixtures from the REFERENCE's own getNormalVectorLine (functions.py:396-416).

DEVELOPMENT MACHINE ONLY (needs /root/reference; never on the GPU machine):
    PYTHONDONTWRITEBYTECODE=1 python3 -B tests/golden/make_hull_golden.py

hull_glyph.json — the camera constants the reference module holds and, for a few dozen (centre, abc, d) cases, what
functions.getNormalVectorLine(centre, abc, disparity) returns with disparity[cy, cx] = d (uint8): the two ints, or
"raises" where it raises (d == 0: the division gives inf and int() refuses the nan that follows; a zero plane:
int(inf)). The function is pure Python and runs unmodified behind the cv2 stub. Recorded results only.
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, REPO]
from make_golden import load_reference  # noqa: E402

H, W = 544, 1024


def cases():
    rng = np.random.default_rng(20261020)
    out = []
    for i in range(40):
        cx, cy = int(rng.integers(0, W)), int(rng.integers(0, H))
        abc = [float(rng.normal(0, 0.05)), float(rng.normal(-0.6, 0.3)), float(rng.normal(0.05, 0.05))]
        d = int(rng.integers(1, 256))
        out.append((cx, cy, abc, d))
    out += [(0, 0, [0.01, -0.5, 0.04], 1), (W - 1, H - 1, [0.01, -0.5, 0.04], 255), (474, 262, [0.0, -1.0, 0.0], 64),
            (475, 262, [1e-9, -1e-9, 1e-9], 7), (100, 500, [-3.0, 2.0, 9.0], 128),
            (512, 300, [0.01, -0.5, 0.04], 0), (3, 3, [0.2, 0.1, -0.4], 0),      # d == 0
            (512, 300, [0.0, 0.0, 0.0], 50)]                                     # a zero plane: Z = 0
    return out


def main():
    f = load_reference()
    warnings.simplefilter("ignore")
    out = {"camera": [f.camera_focal_length_px, f.stereo_camera_baseline_m, f.image_centre_w, f.image_centre_h],
           "shape": [H, W], "cases": []}
    for cx, cy, abc, d in cases():
        disp = np.zeros((H, W), np.uint8)
        disp[cy, cx] = d
        try:
            r = f.getNormalVectorLine((cx, cy), np.array(abc, np.float64), disp)
            r = [int(r[0]), int(r[1])]
        except Exception:   # noqa: BLE001 (the reference's caller catches Exception too, stereovision.py:205)
            r = "raises"
        out["cases"].append({"centre": [cx, cy], "abc": abc, "d": d, "tip": r})
    with open(os.path.join(HERE, "hull_glyph.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(len(out["cases"]), "cases,", sum(c["tip"] == "raises" for c in out["cases"]), "raise")


if __name__ == "__main__":
    main()
