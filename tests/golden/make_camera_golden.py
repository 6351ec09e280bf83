#!/usr/bin/env python3
"""Reference-run fixture at cameras other than the reference's own.

CONTAINER ONLY (needs /root/reference):
    PYTHONDONTWRITEBYTECODE=1 python3 -B tests/golden/make_camera_golden.py

The reference reads its four camera constants when its functions are called (functions.py:181-207), so
setting those module attributes runs its UNMODIFIED chain (make_golden.run_chain: projectDisparityTo3d ->
calculatePointErrors -> computePlanarThreshold -> calculateColourHistogram -> filterPointsByHistogram ->
project3DPointsTo2DImagePoints) under another camera. Only inputs' seeds and outputs are saved:

* camera.npz  — for every camera of camera_inputs.CAMERAS, the chain at step 2 on frame 0 of the 72 x 152
                shape under the planes "some" and "tight": plane_points, hist, the three counts; and the
                back-projection deltas dx[x][d], dy[y][d] over the frame's even x and y, measured through
                the reference's projection + back-projection as deltas.npz was. For near_int also the full
                arrays: xyz and mask_xyz (raw float64), rgb, keep_idx, keep2_idx.
* camera.json — the camera tuples, planes, shape and seed, and for the other three cameras the digests of
                xyz / rgb.

Both files are written byte for byte the same by every run (fixed zip timestamps, sorted keys).
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, REPO]
from make_golden import digest, load_reference, run_chain  # noqa: E402
import camera_inputs as ci  # noqa: E402


def set_camera(F, cam):
    F.camera_focal_length_px, F.stereo_camera_baseline_m, F.image_centre_w, F.image_centre_h = cam


def measured_deltas(F, H, W):
    """dx[x][d] for even x and dy[y][d] for even y (int8, 0 elsewhere): the int32 back-projection of the
    reference's projection minus the source coordinate, every d in 1..255 (make_golden.py, part 5)."""
    img = np.zeros((510, W), np.uint8)
    for i in range(255):
        img[2 * i, :] = i + 1
    back = np.array(F.project3DPointsTo2DImagePoints(F.projectDisparityTo3d(img, 128)), np.int32)
    gx = np.arange(0, W - 1, 2)
    dx = np.zeros((W, 256), np.int8)
    xs, ds = np.tile(gx, 255), np.repeat(np.arange(1, 256), len(gx))
    assert np.abs(back[:, 0] - xs).max() <= 1
    dx[xs, ds] = back[:, 0] - xs
    img = np.zeros((H, 512), np.uint8)
    for j in range(256):
        img[:, 2 * j] = min(j + 1, 255)
    back = np.array(F.project3DPointsTo2DImagePoints(F.projectDisparityTo3d(img, 128)), np.int32)
    gy = np.arange(0, H - 1, 2)
    dy = np.zeros((H, 256), np.int8)
    ys, ds = np.repeat(gy, 256), np.tile(np.minimum(np.arange(1, 257), 255), len(gy))
    assert np.abs(back[:, 1] - ys).max() <= 1
    dy[ys, ds] = back[:, 1] - ys
    return dx, dy


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps and order: the same bytes on every run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    F = load_reference()
    default = (F.camera_focal_length_px, F.stereo_camera_baseline_m, F.image_centre_w, F.image_centre_h)
    H, W = ci.FIXTURE_SHAPE
    disp, bgr = ci.frame(H, W, 0)
    arrays = {}
    meta = {"cameras": {k: list(v) for k, v in ci.CAMERAS.items()}, "shape": [H, W], "seed": ci.SEED,
            "frame": {"disp": digest(disp), "bgr": digest(bgr)}, "step": 2, "planes": {}, "digests": {}}
    try:
        for cname, cam in ci.CAMERAS.items():
            set_camera(F, cam)
            meta["planes"][cname] = {}
            for pname in ci.FIXTURE_PLANES:
                abc, pthr, hthr = ci.plane_case(cam, pname)
                r = run_chain(F, disp, bgr, np.array(abc), point_thr=pthr, hist_thr=hthr)
                counts = (len(r["xyz"]), len(r["keep_idx"]), len(r["keep2_idx"]))
                meta["planes"][cname][pname] = {"abc": list(abc), "point_thr": pthr, "hist_thr": hthr,
                                                "counts": list(counts)}
                pre = f"{cname}_{pname}_"
                arrays[pre + "plane_points"] = r["plane_points"]
                arrays[pre + "hist"] = r["hist"]
                arrays[pre + "counts"] = np.array(counts, np.int64)
                if cname == "near_int":
                    arrays[pre + "keep_idx"] = r["keep_idx"]
                    arrays[pre + "keep2_idx"] = r["keep2_idx"]
                print(cname, pname, counts)
            if cname == "near_int":   # plane-independent: the projection itself
                arrays[cname + "_xyz"] = r["xyz"]
                arrays[cname + "_mask_xyz"] = r["mask_xyz"]
                arrays[cname + "_rgb"] = r["rgb"]
            meta["digests"][cname] = {"xyz": digest(r["xyz"]), "rgb": digest(r["rgb"]),
                                      "mask_xyz": digest(r["mask_xyz"])}
            dx, dy = measured_deltas(F, H, W)
            arrays[cname + "_dx_even"] = dx
            arrays[cname + "_dy_even"] = dy
            meta["digests"][cname].update(dx=digest(dx), dy=digest(dy), dx_neg=int((dx == -1).sum()),
                                          dy_neg=int((dy == -1).sum()))
    finally:
        set_camera(F, default)
    save_npz(os.path.join(HERE, "camera.npz"), arrays)
    with open(os.path.join(HERE, "camera.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("camera.npz", os.path.getsize(os.path.join(HERE, "camera.npz")), "bytes")


if __name__ == "__main__":
    main()
