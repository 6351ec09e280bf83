"""Probe: the obstacle stage per 4096 frames of 544 x 1024 — road_hull() by device events beside
road_clean(), on the synthetic frames' cleaned images — and the frame loop's ms per batch with road="clean" against
road="obstacles" (alternating rounds of 16 timed batches in one process). --modes clean times road="clean" alone
(for a library built from the parent commit, chosen with SVX_LIB, on the same box); --frames N takes batches of N
frames, --rounds 0 skips the frame loop. Prints one JSON record; --out FILE also writes it there."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "stereo.vision_amd")]
from svx import batch as svb, io  # noqa: E402
from svx.loop import STAGES, FrameLoop  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


masks = io.load_masks(os.path.join(REPO, "tests", "golden", "masks"))
road_mask, carmask = masks["road_threshold_mask"], masks["carmask"]
modes = arg("--modes", "clean,obstacles").split(",")
rounds = int(arg("--rounds", "3"))
out = {"lib": os.path.basename(os.environ.get("SVX_LIB", "")) or "libsvx.so"}
frames = int(arg("--frames", "4096"))


def med(v):
    return round(float(np.median(v)), 4)


if "obstacles" in modes:
    with svb.Batch(frames, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode("resident")
        b.road_bits(True)
        b.synth(0)
        b.road_mask(road_mask)
        clean, hull, wall = [], [], []
        for rep in range(10):
            b.pipeline()
            b.road_raster(sync=True)
            b.road_clean(sync=True)
            t0 = time.perf_counter()
            b.road_hull(sync=True)
            t1 = time.perf_counter()
            if rep >= 3:
                clean.append(b.road_clean_ms()[1])
                hull.append(b.road_hull_ms())
                wall.append((t1 - t0) * 1e3)
        sample = [b.read_road_hull(f, images=False) for f in (0, frames // 4, frames * 5 // 8, frames - 1)]
        out["road_hull"] = {"road_hull_ms": med(hull), "road_hull_all": [round(x, 3) for x in hull],
                            "road_hull_ms_host": med(wall), "road_clean_ms": med(clean),
                            "hull_vertices_of_four_frames": [len(r["hull"]) for r in sample],
                            "valid_of_those": [r["valid"] for r in sample]}
    print("road_hull", json.dumps(out["road_hull"]), flush=True)

warm, reps = 2, 16
loops = {m: [] for m in modes}
stage = {}
for rnd in range(rounds):
    for road in modes:
        with FrameLoop(frames, slots=2, source="caller", carmask=carmask, road=road, road_mask=road_mask) as loop:
            seq = None
            for i in range(warm + reps):
                if i == warm:
                    loop.wait(seq)
                    t0 = time.perf_counter()
                if i < 2:
                    loop.acquire().synth(i * frames)
                seq = loop.submit(i * frames)
            loop.wait(seq)
            ms = (time.perf_counter() - t0) / reps * 1e3
            tls = [loop.timeline(q) for q in (seq - 1, seq)]
            stage[road] = {name: round(float(np.mean([tl[name][1] - tl[name][0] for tl in tls])), 3) for name in STAGES}
        loops[road].append(round(ms, 3))
        print("loop", road, rnd, round(ms, 3), json.dumps(stage[road]), flush=True)
out["frame_loop_ms_per_batch"] = loops
out["frame_loop_stage_ms"] = stage
if "--out" in sys.argv:
    with open(arg("--out", ""), "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps(out))
