"""Probe: the result image per 4096 frames of 544 x 1024 — result() by device events (medians of
seven calls after three warm-ups) beside road_hull(), on the synthetic frames; with the diagnostic library
(SVX_LIB=.../libsvx_diag.so) also its floor, a device-to-device copy of the same frames' BGR into the result buffer
between the same events in the same process (SVX_RESULT_COPY=1) — and the frame loop's ms per batch with
road="obstacles" against road="result" (alternating rounds of 16 timed batches in one process). --modes obstacles
times road="obstacles" alone (for a library built from the parent commit, chosen with SVX_LIB, on the same box);
--frames N takes batches of N frames, --rounds 0 skips the frame loop. Prints one JSON record; --out FILE also
writes it there."""
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
modes = arg("--modes", "obstacles,result").split(",")
rounds = int(arg("--rounds", "3"))
lib = os.path.basename(os.environ.get("SVX_LIB", "")) or "libsvx.so"
out = {"lib": lib}
frames = int(arg("--frames", "4096"))
diag = "diag" in lib


def med(v):
    return round(float(np.median(v)), 4)


if "result" in modes:
    with svb.Batch(frames, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode("resident")
        b.road_bits(True)
        b.synth(0)
        b.road_mask(road_mask)
        b.pipeline()
        b.road_raster(sync=True)
        b.road_clean(sync=True)
        hull, res, copy, wall = [], [], [], []
        for rep in range(10):
            b.road_hull(sync=True)
            t0 = time.perf_counter()
            b.result(sync=True)
            t1 = time.perf_counter()
            if rep >= 3:
                hull.append(b.road_hull_ms())
                res.append(b.result_ms())
                wall.append((t1 - t0) * 1e3)
            if diag:                      # the floor, alternating with the kernel
                os.environ["SVX_RESULT_COPY"] = "1"
                b.result(sync=True)
                os.environ["SVX_RESULT_COPY"] = "0"
                if rep >= 3:
                    copy.append(b.result_ms())
        b.result(sync=True)
        sample = [b.read_road_hull(f, images=False) for f in (0, frames // 4, frames * 5 // 8, frames - 1)]
        gb = 2 * frames * 544 * 1024 * 3 / 1e9
        out["result"] = {"result_ms": med(res), "result_all": [round(x, 3) for x in res],
                         "result_ms_host": med(wall), "road_hull_ms": med(hull), "gb_in_and_out": round(gb, 3),
                         "tb_per_s": round(gb / med(res), 3),
                         "hull_vertices_of_four_frames": [len(r["hull"]) for r in sample],
                         "valid_of_those": [r["valid"] for r in sample],
                         "obstacle_share_of_frame_0": round(float((b.read_road_hull(0)["obstacles"] != 0).mean()), 4)}
        if copy:
            out["result"].update({"copy_ms": med(copy), "copy_all": [round(x, 3) for x in copy],
                                  "ratio_to_copy": round(med(res) / med(copy), 3)})
    print("result", json.dumps(out["result"]), flush=True)

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
