"""Probe: the rectification per batch of 544 x 1024 BGR pairs — Batch.rectify() by device events
(median of three calls after a warm-up, a fresh synth_bgr_pair() before each: a second call without one is refused),
with the maps of the barrel model plus a 1 degree rotation on the left eye and minus 1 degree on the right; and as the
yardstick a device-to-device copy of the bytes it must move, by device events too: both eyes' pictures read and both
written, so a copy of frames x 2 x Hp x Wp x 3 bytes, which reads and writes 4 x Hp x Wp x 3 a frame. --frames N
takes a batch of N frames (default 4096: 2 x 2 stores of 6.8 GB with the second store). The measurement runs in a
child process; --variant-lib PATH runs it in a second child on another build of the library (SVX_LIB; the throw-away
build whose workgroups take one picture each, so that the map is read again for every picture) and records its ms
beside this build's. Prints one JSON record; --out FILE also writes it there."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "stereo.vision_amd"), os.path.join(REPO, "tests")]


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def med(v):
    return round(float(np.median(v)), 4)


def d2d_copy_ms(nbytes, reps=4):
    """ms of a hipMemcpyAsync device-to-device of nbytes, by events: the reps - 1 after a warm-up."""
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


def measure(frames):
    import hashlib

    import rectify_numpy as rn
    from svx import batch as svb, dropin
    H, W = 544, 1024
    K, D, _, P = rn.models((H, W))["barrel"]
    left = dropin.rectify_map(K, D, rn.rot("y", 1.0), P, (H, W))
    right = dropin.rectify_map(K, D, rn.rot("y", -1.0), P, (H, W))
    out = {"lib": os.path.basename(os.environ.get("SVX_LIB", "")) or "libsvx.so", "frames": frames, "pair_shape": [H, W],
           "maps": "barrel k1 = -0.3, rotated +1 / -1 degree about y",
           "entries_with_all_taps_inside": [round(float((rn.taps_inside(m[0], H, W) == 4).mean()), 4)
                                            for m in (left, right)]}
    ms = []
    with svb.Batch(frames, H, W, step=1, with_bgr=False) as b:
        b.rectify_maps(left, right)
        for rep in range(4):                   # the first round warms up (and allocates the second store)
            b.synth_bgr_pair(0)
            b.rectify(sync=True)
            if rep:
                ms.append(b.rectify_ms())
        last = frames - 1
        got = b.read_bgr_pair(last)
        b.synth_bgr_pair(0)
        raw = b.read_bgr_pair(last)
        out["last_frame_equals_oracle"] = bool(np.array_equal(got[0], rn.remap(raw[0], *left))
                                               and np.array_equal(got[1], rn.remap(raw[1], *right)))
        out["last_frame_sha256"] = hashlib.sha256(got[0].tobytes() + got[1].tobytes()).hexdigest()[:16]
    copied = frames * 2 * H * W * 3
    copy = d2d_copy_ms(copied)
    out.update({"rectify_ms": med(ms), "rectify_all": [round(x, 3) for x in ms],
                "bytes_read_plus_written": 2 * copied, "d2d_copy_bytes": copied,
                "d2d_copy_ms": med(copy), "d2d_copy_all": [round(x, 3) for x in copy],
                "ratio_to_d2d_copy": round(med(ms) / med(copy), 3),
                "tb_per_s": round(2 * copied / (med(ms) * 1e-3) / 1e12, 3),
                "map_bytes_both_eyes": 2 * 6 * H * W})
    return out


def child(frames, lib=None):
    env = dict(os.environ)
    if lib:
        env["SVX_LIB"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--frames", str(frames)], env=env,
                       capture_output=True, text=True, timeout=420)
    if p.returncode != 0:
        raise RuntimeError(f"the probe's child failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    frames = int(arg("--frames", "4096"))
    if "--child" in sys.argv:
        print(json.dumps(measure(frames)))
        sys.exit(0)
    out = child(frames)
    variant = arg("--variant-lib", "")
    if variant:
        v = child(frames, variant)
        out["map_reread_per_picture_variant"] = {
            "lib": v["lib"], "rectify_ms": v["rectify_ms"], "rectify_all": v["rectify_all"],
            "same_results": v["last_frame_sha256"] == out["last_frame_sha256"],
            "maps_in_registers_over_reread": round(out["rectify_ms"] / v["rectify_ms"], 3)}
    if "--out" in sys.argv:
        os.makedirs(os.path.dirname(os.path.abspath(arg("--out", ""))), exist_ok=True)
        with open(arg("--out", ""), "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))
