"""Probe: the general-scale resize per 4096 frames, by device events, medians of seven calls after three
warm-up calls — resize_disp 390 x 889 -> 544 x 1024 on a cropped batch; 544 x 1024 -> 544 x 1024 (the identity) and
Batch.tile() on a 544 x 1024 batch, alternating in the same process; a device-to-device copy of the resize's output
bytes between HIP events on a stream of its own — with the bytes a frame by this file's own count (source rows read
once, destination written), the rates, the ratio to the copy and the ratio of the rate to tile()'s. Then one
sv_images_tile host call (dropin.images_tile) of the 544 x 1024 five-picture list with a 390 x 889 disparity, by the
host clock: it includes the copies in and out. --frames N takes batches of N frames. Prints one JSON record; --out
FILE also writes it there."""
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "stereo.vision_amd")]
from svx import _abi, batch as svb, dropin, io  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def med(v):
    return round(float(np.median(v)), 4)


def resize_bytes(sh, sw, dh, dw):
    """Bytes of one grey frame the resize must move: every source row once, the destination once (the tables are
    read once a launch, not a frame)."""
    return {"source_read": sh * sw, "destination_written": dh * dw, "total": sh * sw + dh * dw}


def tile_bytes(H, W, road_bits):
    """tools/_probe_tile.py's count of the tile kernel's bytes a frame."""
    rows = 2 * (H // 4)
    return 3 * W * H + 3 * W * rows + W * rows + (W // 8 if road_bits else W) * rows * 2 + W // 8 * rows + \
        3 * W * (H // 2)


def copy_ms(nbytes, warm=3, reps=7):
    """A device-to-device hipMemcpyAsync of nbytes between two HIP events, on a stream of its own."""
    _abi.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    P = ctypes.c_void_p

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")
    src, dst, st, e0, e1 = P(), P(), P(), P(), P()
    ok(hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(nbytes)))
    ok(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(nbytes)))
    ok(hip.hipMemset(src, 1, ctypes.c_size_t(nbytes)))
    ok(hip.hipStreamCreate(ctypes.byref(st)))
    ok(hip.hipEventCreate(ctypes.byref(e0)))
    ok(hip.hipEventCreate(ctypes.byref(e1)))
    out = []
    for rep in range(warm + reps):
        ok(hip.hipEventRecord(e0, st))
        ok(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(nbytes), 3, st))   # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, st))
        ok(hip.hipEventSynchronize(e1))
        t = ctypes.c_float(0)
        ok(hip.hipEventElapsedTime(ctypes.byref(t), e0, e1))
        if rep >= warm:
            out.append(float(t.value))
    for e in (e0, e1):
        ok(hip.hipEventDestroy(e))
    ok(hip.hipStreamDestroy(st))
    ok(hip.hipFree(src))
    ok(hip.hipFree(dst))
    return out


frames = int(arg("--frames", "4096"))
H, W, CH, CW = 544, 1024, 390, 889
out = {"frames": frames}
rng = np.random.default_rng(710)

# the cropped batch: 390 x 889 at a row stride of 896 -> 544 x 1024
with svb.Batch(frames, CH, CW, step=1, with_bgr=False) as b:
    d = rng.integers(0, 256, (CH, CW)).astype(np.uint8)
    for f in range(frames):                # a few distinct frames, rolled: the content does not change the traffic
        b.upload(f, np.roll(d, f % 7, axis=1) if f < 8 else d)
    up = []
    for rep in range(10):
        b.resize_disp((H, W), sync=True)
        if rep >= 3:
            up.append(b.resize_disp_ms())
parts = resize_bytes(CH, CW, H, W)
gb_up = frames * parts["total"] / 1e9
out["crop_to_display"] = {"shape": [CH, CW, H, W], "ms": med(up), "all": [round(x, 3) for x in up],
                          "bytes_per_frame": parts, "gb": round(gb_up, 3), "tb_per_s": round(gb_up / med(up), 3)}
print("crop_to_display", json.dumps(out["crop_to_display"]), flush=True)

# the identity and tile() on a 544 x 1024 batch, alternating
masks = io.load_masks(os.path.join(REPO, "tests", "golden", "masks"))
with svb.Batch(frames, step=1, with_bgr=True, with_points=True) as b:
    b.pipeline_mode("resident")
    b.road_bits(True)
    b.synth(0)
    b.road_mask(masks["road_threshold_mask"])
    b.pipeline()
    b.road_raster(sync=True)
    b.road_clean(sync=True)
    b.road_hull(sync=True)
    b.result(sync=True)
    ident, til = [], []
    for rep in range(10):
        b.resize_disp((H, W), sync=True)
        b.tile(sync=True)
        if rep >= 3:
            ident.append(b.resize_disp_ms())
            til.append(b.tile_ms())
iparts = resize_bytes(H, W, H, W)
gb_id = frames * iparts["total"] / 1e9
gb_tile = frames * tile_bytes(H, W, True) / 1e9
out["identity"] = {"shape": [H, W, H, W], "ms": med(ident), "all": [round(x, 3) for x in ident],
                   "bytes_per_frame": iparts, "gb": round(gb_id, 3), "tb_per_s": round(gb_id / med(ident), 3)}
out["tile"] = {"ms": med(til), "all": [round(x, 3) for x in til], "bytes_per_frame": tile_bytes(H, W, True),
               "gb": round(gb_tile, 3), "tb_per_s": round(gb_tile / med(til), 3)}
print("identity", json.dumps(out["identity"]), flush=True)
print("tile", json.dumps(out["tile"]), flush=True)

# the floor: a device-to-device copy of the resize's output bytes (it reads and writes them: twice the bytes)
cp = copy_ms(frames * H * W)
gb_cp = 2 * frames * H * W / 1e9
out["copy"] = {"bytes": frames * H * W, "ms": med(cp), "all": [round(x, 3) for x in cp],
               "tb_per_s": round(gb_cp / med(cp), 3)}
for k in ("crop_to_display", "identity"):
    out[k]["ratio_to_copy"] = round(out[k]["ms"] / out["copy"]["ms"], 3)
    out[k]["rate_ratio_to_tile"] = round(out[k]["tb_per_s"] / out["tile"]["tb_per_s"], 3)
print("copy", json.dumps(out["copy"]), flush=True)

# one host call of batchImages' five-picture list with the cropped disparity: copies in and out included
pics = [rng.integers(0, 256, s).astype(np.uint8) for s in ((CH, CW), (H, W, 3), (H, W), (H, W), (H, W, 3))]
wall = []
for rep in range(10):
    t0 = time.perf_counter()
    t = dropin.images_tile(pics, (H, W))
    if rep >= 3:
        wall.append((time.perf_counter() - t0) * 1e3)
out["images_tile_host_call"] = {"list": "390x889 grey, 544x1024 BGR, grey, grey, BGR", "out_shape": list(t.shape),
                                "ms_host_clock_with_copies": med(wall), "all": [round(x, 3) for x in wall]}
if "--out" in sys.argv:
    os.makedirs(os.path.dirname(os.path.abspath(arg("--out", ""))), exist_ok=True)
    with open(arg("--out", ""), "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps(out))
