"""Probe: the road clean-up per 4096 frames of 544 x 1024 — the clean-up kernel and road_clean() as
a whole by device events, the road pass beside it by a host clock around a synchronise — and the frame loop's ms per
batch with road="walk" against road="clean" (two alternating rounds of 16 timed batches). Prints one JSON record;
--out FILE also writes it there."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "stereo.vision_amd")]
from svx import batch as svb, io  # noqa: E402
from svx.loop import STAGES, FrameLoop  # noqa: E402

masks = io.load_masks(os.path.join(REPO, "tests", "golden", "masks"))
road_mask, carmask = masks["road_threshold_mask"], masks["carmask"]
out = {}
frames = 4096


def med(v):
    return round(float(np.median(v)), 4)


for label, step, bits in (("bitmap_step1", 1, True), ("packed_step1", 1, False), ("packed_step2", 2, False)):
    with svb.Batch(frames, step=step, with_bgr=True, with_points=True) as b:
        b.pipeline_mode("resident")
        b.road_bits(bits)
        b.synth(0)
        b.road_mask(road_mask)
        road, kern, total, wall = [], [], [], []
        for rep in range(8):
            b.pipeline()
            t0 = time.perf_counter()
            b.road_raster(sync=True)
            t1 = time.perf_counter()
            b.road_clean(sync=True)
            t2 = time.perf_counter()
            k, t = b.road_clean_ms()
            if rep >= 3:
                road.append((t1 - t0) * 1e3)
                wall.append((t2 - t1) * 1e3)
                kern.append(k)
                total.append(t)
        n = [len(b.read_road_clean(f, walk=True)[1]) for f in (0, 1000, 4095)]
        out[label] = {"road_pass_ms_host": med(road), "road_pass_all": [round(x, 3) for x in road],
                      "clean_kernel_ms": med(kern), "clean_kernel_all": [round(x, 3) for x in kern],
                      "road_clean_ms": med(total), "road_clean_all": [round(x, 3) for x in total],
                      "road_clean_ms_host": med(wall), "clean_pixels_of_frames_0_1000_4095": n}
    print(label, json.dumps(out[label]), flush=True)

warm, reps = 2, 16
loops = {"walk": [], "clean": []}
stage = {}
for rnd in range(2):
    for road in ("walk", "clean"):
        kw = dict(road_mask=road_mask) if road == "clean" else {}
        with FrameLoop(frames, slots=2, source="caller", carmask=carmask, road=road, **kw) as loop:
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
            a, bb = tls
            lo, hi = max(bb["draw"][0], a["pipeline"][0]), min(bb["draw"][1], a["road"][1])
            stage[road]["draw_overlap_ms"] = round(max(0.0, hi - lo), 3)
            stage[road]["next_draw_ms"] = round(bb["draw"][1] - bb["draw"][0], 3)
        loops[road].append(round(ms, 3))
        print("loop", road, rnd, round(ms, 3), json.dumps(stage[road]), flush=True)
out["frame_loop_ms_per_batch"] = loops
out["frame_loop_stage_ms"] = stage
if "--out" in sys.argv:
    with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
        json.dump(out, fh, indent=1)
print(json.dumps(out))
