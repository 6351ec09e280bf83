"""Probe: the image tile per 4096 frames of 544 x 1024 — tile() by device events (medians of seven
calls after three warm-ups) alternating with result() in the same process, on the synthetic frames, with the bytes
the tile kernel must move per frame by this file's own count and the rate they imply beside result()'s — and the
frame loop's ms per batch with road="result" against road="tile" (alternating rounds of 16 timed batches in one
process). --modes result times road="result" alone (for a library built from the parent commit, chosen with
SVX_LIB, on the same box); --frames N takes batches of N frames, --rounds 0 skips the frame loop, --bits 0 reads the
raw road picture as u8 (no pipeline bitmap). Prints one JSON record; --out FILE also writes it there."""
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


def tile_bytes(H, W, road_bits, clean_bits):
    """Bytes of one frame the tile kernel must move, by picture. The stack's pictures are sampled at rows 4 q + 1 and
    4 q + 2 only: half the rows of each; disparity and BGR belong to the top half of the tile (H / 4 output rows),
    the two road pictures to the bottom half. A bitmap row is W / 8 bytes."""
    rows = 2 * (H // 4)                                  # source rows read of a picture of the stack
    parts = {"result_read": 3 * W * H,                   # 2 rows of 3 W for each of the H / 2 output rows
             "bgr_read": 3 * W * rows, "disparity_read": W * rows,
             "road_read": (W // 8 if road_bits else W) * rows * 2,     # the map's quadrant and its own
             "cleaned_read": (W // 8 if clean_bits else W) * rows,
             "tile_written": 3 * W * (H // 2)}
    parts["total"] = sum(parts.values())
    return parts


masks = io.load_masks(os.path.join(REPO, "tests", "golden", "masks"))
road_mask, carmask = masks["road_threshold_mask"], masks["carmask"]
modes = arg("--modes", "result,tile").split(",")
rounds = int(arg("--rounds", "3"))
bits = arg("--bits", "1") == "1"
lib = os.path.basename(os.environ.get("SVX_LIB", "")) or "libsvx.so"
out = {"lib": lib}
frames = int(arg("--frames", "4096"))
H, W = 544, 1024


def med(v):
    return round(float(np.median(v)), 4)


if "tile" in modes:
    with svb.Batch(frames, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode("resident")
        b.road_bits(bits)
        b.synth(0)
        b.road_mask(road_mask)
        b.pipeline()
        b.road_raster(sync=True)
        b.road_clean(sync=True)
        b.road_hull(sync=True)
        res, til, wall = [], [], []
        for rep in range(10):                # alternating: result(), then tile()
            b.result(sync=True)
            t0 = time.perf_counter()
            b.tile(sync=True)
            t1 = time.perf_counter()
            if rep >= 3:
                res.append(b.result_ms())
                til.append(b.tile_ms())
                wall.append((t1 - t0) * 1e3)
        parts = tile_bytes(H, W, bits, True)
        gb_tile = frames * parts["total"] / 1e9
        gb_res = 2 * frames * H * W * 3 / 1e9
        out["tile"] = {"tile_ms": med(til), "tile_all": [round(x, 3) for x in til], "tile_ms_host": med(wall),
                       "result_ms": med(res), "result_all": [round(x, 3) for x in res],
                       "road_source": "bitmap" if bits else "u8", "cleaned_source": "bitmap",
                       "bytes_per_frame": parts, "gb_tile": round(gb_tile, 3), "gb_result": round(gb_res, 3),
                       "tile_tb_per_s": round(gb_tile / med(til), 3), "result_tb_per_s": round(gb_res / med(res), 3),
                       "rate_ratio_tile_to_result": round((gb_tile / med(til)) / (gb_res / med(res)), 3),
                       "road_share_of_frame_0": round(float((b.read_road(0) != 0).mean()), 4)}
    print("tile", json.dumps(out["tile"]), flush=True)

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
