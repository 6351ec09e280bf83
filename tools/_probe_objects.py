"""Probe: the obstacle list per 4096 frames of 544 x 1024, on the synthetic frames' obstacle stage —
road_hull() and obstacle_list() by device events in the same run (median of three calls after a warm-up, at the
defaults min_area 70 / cap 16 and at min_area 1 / cap 32), and by the host clock the read-back of all 4096 lists
against one frame's obstacle image. --frames N takes a batch of N frames. Prints one JSON record; --out FILE also
writes it there."""
import json
import os
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


masks = io.load_masks(os.path.join(REPO, "tests", "golden", "masks"))
frames = int(arg("--frames", "4096"))
out = {"lib": os.path.basename(os.environ.get("SVX_LIB", "")) or "libsvx.so", "frames": frames, "shape": [544, 1024]}

with svb.Batch(frames, step=1, with_bgr=True, with_points=True) as b:
    b.pipeline_mode("resident")
    b.road_bits(True)
    b.synth(0)
    b.road_mask(masks["road_threshold_mask"])
    b.pipeline()
    b.road_raster(sync=True)
    b.road_clean(sync=True)
    hull, lists, hard = [], [], []
    for rep in range(4):                       # the first round warms up (and allocates the scratch)
        b.road_hull(sync=True)
        b.obstacle_list(sync=True)
        if rep:
            hull.append(b.road_hull_ms())
            lists.append(b.obstacle_list_ms())
        b.obstacle_list(min_area=1, cap=32, sync=True)
        if rep:
            hard.append(b.obstacle_list_ms())
    b.obstacle_list(sync=True)
    t0 = time.perf_counter()
    got = [b.read_obstacle_list(f) for f in range(frames)]
    t1 = time.perf_counter()
    img = b.read_road_hull(0)["obstacles"]
    t2 = time.perf_counter()
    b.obstacle_list(sync=True)
    t3 = time.perf_counter()
    b.read_obstacle_list(0)                    # the one device copy every later read is served from
    t4 = time.perf_counter()
    ns = np.array([n for n, _ in got])
    areas = np.array([int(e["area"].sum()) for _, e in got])
    out["obstacle_list"] = {
        "road_hull_ms": med(hull), "road_hull_all": [round(x, 3) for x in hull],
        "obstacle_list_ms": med(lists), "obstacle_list_all": [round(x, 3) for x in lists],
        "ratio_to_road_hull": round(med(lists) / med(hull), 2),
        "obstacle_list_min_area_1_cap_32_ms": med(hard), "min_area_1_cap_32_all": [round(x, 3) for x in hard],
        "read_all_lists_ms_host": round((t1 - t0) * 1e3, 2), "first_read_one_copy_ms_host": round((t4 - t3) * 1e3, 3),
        "read_one_obstacle_image_ms_host": round((t2 - t1) * 1e3, 2),
        "list_bytes_of_the_batch": int(frames * (16 * 56 + 4)), "obstacle_image_bytes": int(img.size),
        "components_per_frame_mean_max": [round(float(ns.mean()), 2), int(ns.max())],
        "listed_area_per_frame_mean": round(float(areas.mean()), 1),
        "obstacle_share_of_frame_0": round(float((img != 0).mean()), 4)}
if "--out" in sys.argv:
    os.makedirs(os.path.dirname(os.path.abspath(arg("--out", ""))), exist_ok=True)
    with open(arg("--out", ""), "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps(out))
