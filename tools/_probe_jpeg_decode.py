"""Probe: the JPEG decoder on a batch of 272 x 1024 tiles at quality 75 (4096 synthetic frames of
544 x 1024 unless --frames N), one process:
 - encode: Batch.jpeg by device events (median of five calls after two warm-ups): the yardstick;
 - decode: sv_jpeg_decode_many of those streams, its four kernels by device events (marker scan, entropy walk,
   chroma planes, picture; median of --reps calls after a warm-up), the host's wall time of the whole call, and a
   check of frames across the chunk borders against the one-stream entry;
 - a device-to-device copy of the decoded bytes (hipMemcpyAsync, device events);
 - the host link: --pairs stereo pairs of that shape into a batch as JPEG streams (Batch.decode_bgr_pair: parse,
   upload, decode) against the same pairs as raw pixels (Batch.upload_bgr_pair), alternating, host wall time.
The synthetic frames' upper halves are uniform noise: a hard case, not a road scene. Prints one JSON record;
--out FILE writes it."""
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


frames = int(arg("--frames", "4096"))
reps = int(arg("--reps", "3"))
npairs = min(int(arg("--pairs", "256")), frames // 2)
quality = 75
H, W = 544, 1024
h, w = H // 2, W
raw = h * w * 3
masks = io.load_masks(os.path.join(REPO, "tests", "golden", "masks"))
out = {"frames": frames, "quality": quality, "tile": [h, w], "raw_bytes_per_frame": raw}

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
    b.tile(sync=True)
    enc = []
    for rep in range(7):
        b.jpeg(quality, sync=True)
        if rep >= 2:
            enc.append(b.jpeg_ms())
    if (b.jpeg_sizes() < 0).any():
        raise SystemExit("a stream overflowed the default slot")
    buf, offsets, total = b.read_jpegs_packed()
    check_tiles = {f: b.read_tile(f) for f in (0, frames - 1)}
offs = np.concatenate([offsets, [total]]).astype(np.int64)
out["encode_ms"] = med(enc)
out["encode_all"] = [round(x, 3) for x in enc]
out["stream_bytes_mean"] = round(total / frames, 1)
out["share_of_raw"] = round(total / frames / raw, 4)
print("encode", json.dumps(out), flush=True)

pics = np.empty((frames, h, w, 3), np.uint8)
status = np.empty(frames, np.int32)
stage, wall = [], []
for rep in range(reps + 1):
    t0 = time.perf_counter()
    _abi.call("sv_jpeg_decode_many", 0, _abi.ptr(buf), _abi.ptr(offs), frames, h, w, _abi.ptr(pics), _abi.ptr(status))
    t1 = time.perf_counter()
    if rep >= 1:
        stage.append(dropin.jpeg_decode_stage_ms())
        wall.append((t1 - t0) * 1e3)
if status.any():
    raise SystemExit(f"decode statuses: {np.flatnonzero(status)[:8].tolist()}")
checked = sorted({0, frames - 1, *range(1023, frames, 1024), *range(1024, frames, 1024)})
for f in checked:
    if not np.array_equal(pics[f], dropin.jpeg_decode(buf[offs[f]:offs[f + 1]].tobytes())):
        raise SystemExit(f"frame {f}: the batch's picture differs from the one-stream entry's")
err = {f: int(np.abs(pics[f].astype(np.int32) - t).max()) for f, t in check_tiles.items()}
names = ("scan", "entropy", "chroma", "picture")
st = {n: med([s[i] for s in stage]) for i, n in enumerate(names)}
dec_ms = round(sum(st.values()), 4)
out["decode"] = {"stage_ms": st, "decode_ms": dec_ms, "all": [[round(v, 3) for v in s] for s in stage],
                 "ratio_to_encode": round(dec_ms / out["encode_ms"], 3),
                 "entropy_over_encode": round(st["entropy"] / out["encode_ms"], 3),
                 "gpixels_per_s": round(frames * h * w / dec_ms / 1e6, 3), "call_wall_ms": med(wall),
                 "frames_checked_against_one_stream_entry": checked, "max_abs_error_against_the_tile": err}
print("decode", json.dumps(out["decode"]), flush=True)

if "--no-copy" not in sys.argv:
    hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")
    src, dst, e0, e1 = (ctypes.c_void_p() for _ in range(4))
    nbytes = ctypes.c_size_t(frames * raw)
    ok(hip.hipMalloc(ctypes.byref(src), nbytes))
    ok(hip.hipMalloc(ctypes.byref(dst), nbytes))
    ok(hip.hipMemset(src, 1, nbytes))
    ok(hip.hipEventCreate(ctypes.byref(e0)))
    ok(hip.hipEventCreate(ctypes.byref(e1)))
    ms = []
    for rep in range(10):
        t = ctypes.c_float(0)
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyAsync(dst, src, nbytes, 3, None))      # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ok(hip.hipEventElapsedTime(ctypes.byref(t), e0, e1))
        if rep >= 3:
            ms.append(t.value)
    out["d2d_copy_of_pictures_ms"] = med(ms)
    for p in (src, dst):
        ok(hip.hipFree(p))
    for e in (e0, e1):
        ok(hip.hipEventDestroy(e))

# the host link: pairs as streams against pairs as pixels
if npairs > 0:
    ls = [buf[offs[f]:offs[f + 1]].tobytes() for f in range(npairs)]
    rs = [buf[offs[f]:offs[f + 1]].tobytes() for f in range(npairs, 2 * npairs)]
    t_dec, t_up, k_ms = [], [], []
    with svb.Batch(npairs, h, w, step=1, with_bgr=False) as b:
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            st2 = b.decode_bgr_pair(0, ls, rs)
            t1 = time.perf_counter()
            for f in range(npairs):
                b.upload_bgr_pair(f, pics[f], pics[npairs + f])
            t2 = time.perf_counter()
            if rep >= 1:
                t_dec.append((t1 - t0) * 1e3)
                t_up.append((t2 - t1) * 1e3)
                k_ms.append(b.decode_ms())
        if st2.any():
            raise SystemExit("pair decode statuses")
    sbytes = int(offs[2 * npairs] - offs[0])
    out["host_link"] = {"pairs": npairs, "stream_bytes": sbytes, "raw_bytes": 2 * npairs * raw,
                        "decode_bgr_pair_ms": med(t_dec), "of_which_kernels_ms": med(k_ms),
                        "upload_bgr_pair_ms": med(t_up), "ratio": round(med(t_dec) / med(t_up), 3)}
if "--out" in sys.argv:
    with open(arg("--out", ""), "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps(out))
