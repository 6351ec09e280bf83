"""Probe: the ground grid per 4096 frames of 544 x 1024, on the synthetic frames' obstacle stage —
road_hull(), obstacle_list() and ground_grid() at the default grid by device events in the same run (median of three
calls after a warm-up); a device-to-device copy of the bytes the stage must move (the two bitmaps, the disparity and
the output) as the yardstick, by device events too; and by the host clock read_ground_nearest() against the read-back
of one frame's obstacle image (the first call and a second one: the first device-to-host copy of a process into
pageable memory pays a set-up of its own). A second, smaller batch (--heavy-frames, default 512) holds frames of one
constant disparity, road all over: every pixel of a bitmap word in one cell and a row in a handful, the heaviest
collisions the LDS atomics can meet. --frames N takes a batch of N frames. --variant-lib PATH also runs this probe in a
child process on another build of the library (SVX_LIB; the throw-away build with one LDS atomic a pixel) and records
its ground_grid ms beside this build's. Prints one JSON record; --out FILE also writes it there."""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "stereo.vision_amd")]
from svx import batch as svb, io  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def med(v):
    return round(float(np.median(v)), 4)


def d2d_copy_ms(nbytes, reps=4):
    """ms of a hipMemcpyAsync device-to-device of nbytes, by events: the median of reps - 1 after a warm-up."""
    hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    src, dst, e0, e1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")
    ok(hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(nbytes)))
    ok(hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(nbytes)))
    ok(hip.hipMemset(src, 1, ctypes.c_size_t(nbytes)))
    ok(hip.hipEventCreate(ctypes.byref(e0)))
    ok(hip.hipEventCreate(ctypes.byref(e1)))
    out = []
    for rep in range(reps):
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(nbytes), 3, None))   # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = ctypes.c_float(0)
        ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
        if rep:
            out.append(ms.value)
    for p in (src, dst):
        ok(hip.hipFree(p))
    for e in (e0, e1):
        ok(hip.hipEventDestroy(e))
    return out


masks = io.load_masks(os.path.join(REPO, "tests", "golden", "masks"))
frames = int(arg("--frames", "4096"))
H, W, NX, NZ = 544, 1024, 64, 128
out = {"lib": os.path.basename(os.environ.get("SVX_LIB", "")) or "libsvx.so", "frames": frames, "shape": [H, W],
       "grid": [-8.0, 0.0, 0.25, NX, NZ]}

with svb.Batch(frames, step=1, with_bgr=True, with_points=True) as b:
    b.pipeline_mode("resident")
    b.road_bits(True)
    b.synth(0)
    b.road_mask(masks["road_threshold_mask"])
    b.pipeline()
    b.road_raster(sync=True)
    b.road_clean(sync=True)
    hull, lists, grids = [], [], []
    for rep in range(4):                       # the first round warms up (and allocates the buffers and the mapping)
        b.road_hull(sync=True)
        b.obstacle_list(sync=True)
        b.ground_grid(sync=True)
        if rep:
            hull.append(b.road_hull_ms())
            lists.append(b.obstacle_list_ms())
            grids.append(b.ground_grid_ms())
    tf = time.perf_counter()
    b.read_ground_nearest()
    t0 = time.perf_counter()
    profile = b.read_ground_nearest()
    t1 = time.perf_counter()
    img = b.read_road_hull(0)["obstacles"]
    t2 = time.perf_counter()
    one = b.read_ground_grid(0)
    t3 = time.perf_counter()
    infos = np.stack([b.read_ground_grid(f)["info"] for f in range(0, frames, max(frames // 64, 1))])
    moved = frames * (2 * H * (W // 32) * 4 + H * W + (2 * NX * NZ + NX + 4) * 4)
    copy = d2d_copy_ms(moved)
    out["ground_grid"] = {
        "road_hull_ms": med(hull), "road_hull_all": [round(x, 3) for x in hull],
        "obstacle_list_ms": med(lists), "obstacle_list_all": [round(x, 3) for x in lists],
        "ground_grid_ms": med(grids), "ground_grid_all": [round(x, 3) for x in grids],
        "ratio_to_road_hull": round(med(grids) / med(hull), 2),
        "bytes_moved": int(moved), "d2d_copy_of_those_bytes_ms": med(copy), "d2d_copy_all": [round(x, 3) for x in copy],
        "ratio_to_d2d_copy": round(med(grids) / med(copy), 2),
        "read_ground_nearest_ms_host": round((t1 - t0) * 1e3, 3),
        "read_ground_nearest_first_call_ms_host": round((t0 - tf) * 1e3, 3), "nearest_bytes_of_the_batch": int(profile.nbytes),
        "read_one_obstacle_image_ms_host": round((t2 - t1) * 1e3, 3), "obstacle_image_bytes": int(img.size),
        "read_one_frame_grid_ms_host": round((t3 - t2) * 1e3, 3),
        "occupied_columns_per_frame_mean": round(float((profile >= 0).sum(axis=1).mean()), 2),
        "info_mean_of_sampled_frames": [round(float(x), 1) for x in infos.mean(axis=0)],
        "obstacle_cells_of_frame_0": int((one["obst"] > 0).sum()), "road_cells_of_frame_0": int((one["road"] > 0).sum())}

heavy = int(arg("--heavy-frames", "512"))
if heavy > 0:
    frame = np.full((H, W), 100, np.uint8)
    bgr = np.full((H, W, 3), 90, np.uint8)
    with svb.Batch(heavy, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode("resident")
        b.road_bits(True)
        for f in range(heavy):
            b.upload(f, frame, bgr)
        b.pipeline(plane=(0.0, 0.0, 0.01), point_thr=1e9, hist_thr=2)   # the road image is every pixel with d > 0
        b.road_raster(sync=True)
        b.road_clean(sync=True)
        b.road_hull(sync=True)
        ms = []
        for rep in range(4):
            b.ground_grid(sync=True)
            if rep:
                ms.append(b.ground_grid_ms())
        g0 = b.read_ground_grid(0)
        out["constant_disparity"] = {
            "frames": heavy, "d": 100, "ground_grid_ms": med(ms), "ground_grid_all": [round(x, 3) for x in ms],
            "ms_per_4096_frames": round(med(ms) * 4096 / heavy, 3), "info_of_frame_0": [int(x) for x in g0["info"]],
            "road_cells_of_frame_0": int((g0["road"] > 0).sum()), "largest_cell_of_frame_0": int(g0["road"].max())}

variant = arg("--variant-lib", "")
if variant:
    env = dict(os.environ, SVX_LIB=os.path.abspath(variant))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--frames", str(frames), "--heavy-frames",
                        str(heavy)], env=env,
                       capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise RuntimeError(f"the variant's probe failed ({p.returncode}): {p.stderr[-2000:]}")
    v = json.loads(p.stdout.strip().splitlines()[-1])
    same = all(out["ground_grid"][k] == v["ground_grid"][k] for k in
               ("info_mean_of_sampled_frames", "occupied_columns_per_frame_mean", "obstacle_cells_of_frame_0"))
    out["per_pixel_atomic_variant"] = {
        "lib": v["lib"], "ground_grid_ms": v["ground_grid"]["ground_grid_ms"],
        "ground_grid_all": v["ground_grid"]["ground_grid_all"], "same_results": bool(same),
        "run_aggregated_over_per_pixel": round(out["ground_grid"]["ground_grid_ms"] / v["ground_grid"]["ground_grid_ms"], 3)}
    if heavy > 0:
        vc, oc = v["constant_disparity"], out["constant_disparity"]
        out["per_pixel_atomic_variant"]["constant_disparity"] = {
            "ground_grid_ms": vc["ground_grid_ms"], "ground_grid_all": vc["ground_grid_all"],
            "same_results": vc["info_of_frame_0"] == oc["info_of_frame_0"]
            and vc["largest_cell_of_frame_0"] == oc["largest_cell_of_frame_0"],
            "run_aggregated_over_per_pixel": round(oc["ground_grid_ms"] / vc["ground_grid_ms"], 3)}
if "--out" in sys.argv:
    os.makedirs(os.path.dirname(os.path.abspath(arg("--out", ""))), exist_ok=True)
    with open(arg("--out", ""), "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps(out))
