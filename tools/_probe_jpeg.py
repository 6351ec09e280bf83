"""Probe: the JPEG stage per batch of 272 x 1024 tiles (4096 frames of 544 x 1024 unless --frames N).
 - encode: jpeg(75) by device events (medians of seven calls after three warm-ups) alternating with tile() in the
   same process, beside a device-to-device copy of the tiles' bytes (hipMemcpyAsync, device events);
 - bytes a frame: mean, maximum, and the share of frames that overflowed the default slot. The synthetic frames'
   upper halves are uniform noise: a hard case, not a road scene;
 - read-back into pooled page-locked memory (sv_host_alloc): the packed streams in one copy against the same
   batch's raw tiles, frame by frame;
 - the frame loop's ms per batch with road="tile" against road="video" (alternating rounds of 16 timed batches).
--modes tile times road="tile" alone (for a library built from the parent commit, chosen with SVX_LIB, on the same
box); --rounds 0 skips the frame loop; --no-copy skips the device-to-device copy. Prints one JSON record; --out FILE writes it."""
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "stereo.vision_amd")]
from svx import _abi, batch as svb, io  # noqa: E402
from svx.loop import STAGES, FrameLoop  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def med(v):
    return round(float(np.median(v)), 4)


masks = io.load_masks(os.path.join(REPO, "tests", "golden", "masks"))
road_mask, carmask = masks["road_threshold_mask"], masks["carmask"]
modes = arg("--modes", "tile,video").split(",")
rounds = int(arg("--rounds", "3"))
frames = int(arg("--frames", "4096"))
quality = int(arg("--quality", "75"))
lib = os.path.basename(os.environ.get("SVX_LIB", "")) or "libsvx.so"
out = {"lib": lib, "frames": frames, "quality": quality}
H, W = 544, 1024
raw = (H // 2) * W * 3

if "video" in modes:
    with svb.Batch(frames, step=1, with_bgr=True, with_points=True) as b:
        b.pipeline_mode("resident")
        b.road_bits(True)
        b.synth(0)
        b.road_mask(road_mask)
        b.pipeline()
        b.road_raster(sync=True)
        b.road_clean(sync=True)
        b.road_hull(sync=True)
        b.result(sync=True)
        til, jpg, wall = [], [], []
        for rep in range(10):                # alternating: tile(), then jpeg()
            b.tile(sync=True)
            t0 = time.perf_counter()
            b.jpeg(quality, sync=True)
            t1 = time.perf_counter()
            if rep >= 3:
                til.append(b.tile_ms())
                jpg.append(b.jpeg_ms())
                wall.append((t1 - t0) * 1e3)
        sizes = b.jpeg_sizes().astype(np.int64)
        need = np.abs(sizes)
        # the frames go through the scratch in chunks: the first and last frame of the batch and the frames either
        # side of every 1024 must equal the host entry's stream of the same tile
        from svx import dropin
        checked = sorted({f for f in (0, frames - 1, *range(1023, frames, 1024), *range(1024, frames, 1024))
                          if sizes[f] > 0})
        for f in checked:
            if b.read_jpeg(f) != dropin.jpeg_encode(b.read_tile(f), quality):
                raise SystemExit(f"frame {f}: the batch's stream differs from the host entry's")
        rec = {"jpeg_ms": med(jpg), "jpeg_all": [round(x, 3) for x in jpg], "jpeg_ms_host": med(wall),
               "tile_ms": med(til), "tile_all": [round(x, 3) for x in til], "raw_bytes_per_frame": raw,
               "bytes_per_frame_mean": round(float(need.mean()), 1), "bytes_per_frame_max": int(need.max()),
               "share_of_raw_mean": round(float(need.mean()) / raw, 4), "default_slot": raw // 2,
               "overflowed_share": round(float((sizes < 0).mean()), 6), "frames_checked_against_host_entry": checked,
               "gpixels_per_s": round(frames * (H // 2) * W / med(jpg) / 1e6, 3),
               "note": "synthetic frames: the upper half of every frame is uniform noise (a hard case, no road scene)"}
        if "--no-copy" not in sys.argv:
            # the HIP runtime the library itself is linked to, called directly: two buffers of the tiles' size
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
            rec["d2d_copy_of_tiles_ms"] = med(ms)
            for p in (src, dst):
                ok(hip.hipFree(p))
            for e in (e0, e1):
                ok(hip.hipEventDestroy(e))
        # read-back into page-locked memory: the packed streams in one copy, the raw tiles frame by frame
        total = int(np.maximum(sizes, 0).sum())
        pk = _abi.pinned_empty((max(total, 1),), np.uint8)
        offs = np.empty(frames, np.int64)
        tot = ctypes.c_int64(0)
        t_pack, t_read = [], []
        for rep in range(5):
            t0 = time.perf_counter()
            _abi.call("sv_batch_jpeg_pack", b._h, 1)
            t1 = time.perf_counter()
            _abi.call("sv_batch_read_jpeg_packed", b._h, _abi.ptr(pk), pk.size, _abi.ptr(offs), ctypes.byref(tot))
            t2 = time.perf_counter()
            if rep >= 1:
                t_pack.append((t1 - t0) * 1e3)
                t_read.append((t2 - t1) * 1e3)
        nraw = min(frames, 512)                      # the raw tiles of the first 512 frames (3.4 GB for 4096)
        tiles = _abi.pinned_empty((nraw, H // 2, W, 3), np.uint8)
        t_raw = []
        for rep in range(4):
            t0 = time.perf_counter()
            for f in range(nraw):
                _abi.call("sv_batch_read_tile", b._h, f, _abi.ptr(tiles[f]))
            if rep >= 1:
                t_raw.append((time.perf_counter() - t0) * 1e3)
        rec["readback"] = {"packed_bytes": total, "pack_ms_host": med(t_pack), "packed_read_ms": med(t_read),
                           "packed_gb_per_s": round(total / med(t_read) / 1e6, 3), "raw_frames": nraw,
                           "raw_bytes": nraw * raw, "raw_read_ms": med(t_raw),
                           "raw_gb_per_s": round(nraw * raw / med(t_raw) / 1e6, 3),
                           "raw_read_ms_scaled_to_batch": round(med(t_raw) * frames / nraw, 3)}
        out["jpeg"] = rec
    print("jpeg", json.dumps(out["jpeg"]), flush=True)

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
