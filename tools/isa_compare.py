#!/usr/bin/env python3
"""Per-kernel comparison of two trees' gfx950 device code (CPU only: it compiles, it runs nothing).

    tools/isa_compare.py PARENT_TREE THIS_TREE [--diag] [-j N] > profiles/<pr>/isa_compare.txt

Every unit of each tree's csrc/Makefile SRCS is compiled device-only with that tree's own FLAGS line (--diag: plus
-DSVX_DIAG, the diagnostic library's build), which gives a plain gfx950 ELF per unit. Units whose two ELFs are
byte-identical are named in one line. Then, per kernel of every unit: the function's bytes, its 64-byte kernel descriptor
(all but the code entry offset, which only says where the function lies) and its metadata entry are compared as
bytes and text; nothing is disassembled. Lines are SAME / DIFF / GONE (parent only) / NEW (this tree only).
The exit status is 0 only if no line is DIFF, GONE or NEW.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = "/opt/rocm/llvm/bin"
DEVICE_ONLY = ["--cuda-device-only", "-fuse-cuid=none", "--no-gpu-bundle-output", "-c"]


def make_vars(csrc):
    """The Makefile's plain assignments, expanded ($(EXTRA) and anything unknown: empty)."""
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    raw = dict(re.findall(r"^(\w+)\s*\??=\s*(.*)$", text, re.M))

    def expand(s):
        return re.sub(r"\$\((\w+)\)", lambda m: expand(raw.get(m.group(1), "")), s)

    return expand(raw["HIPCC"]), expand(raw["FLAGS"]).split(), expand(raw["SRCS"]).split()


def compile_unit(csrc, hipcc, flags, unit, out):
    subprocess.run([hipcc, *flags, *DEVICE_ONLY, unit, "-o", out], cwd=csrc, check=True)
    return out


def readelf(*args):
    return subprocess.run([f"{LLVM}/llvm-readelf", "--wide", *args], check=True, capture_output=True, text=True).stdout


def kernels(elf):
    """name -> (function bytes, descriptor bytes without the entry offset, metadata text, metadata numbers)."""
    data = open(elf, "rb").read()
    sect = {}   # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+\S+\s+([0-9a-f]{16})\s+([0-9a-f]+)\s", readelf("-S", elf), re.M):
        sect[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    sym = {}
    for line in readelf("--symbols", elf).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            addr, off = sect[int(f[6])]
            start = int(f[1], 16) - addr + off
            sym[f[7]] = data[start:start + int(f[2])]
    notes = readelf("--notes", elf)
    meta = {}
    for entry in re.split(r"^  - (?=\.)", notes.split("amdhsa.kernels:")[-1].split("\namdhsa.target")[0], flags=re.M)[1:]:
        meta[re.search(r"\.name:\s+(\S+)", entry).group(1)] = entry
    out = {}
    for name, entry in meta.items():
        kd = sym[name + ".kd"]
        assert len(kd) == 64, (name, len(kd))
        num = {k: int(re.search(rf"\.{k}:\s+(\d+)", entry).group(1))
               for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")}
        out[name] = (sym[name], kd[:16] + kd[24:], entry, num)
    return out


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    if not names or not filt:   # no demangler: the mangled names
        return {n: n for n in names}
    res = subprocess.run([filt], input="\n".join(names), check=True, capture_output=True, text=True)
    return {n: d.removeprefix("void ").replace("svx::", "", 1).replace("(anonymous namespace)::", "", 1)
            for n, d in zip(names, res.stdout.splitlines())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--diag", action="store_true", help="compare the diagnostic build (-DSVX_DIAG)")
    ap.add_argument("-j", type=int, default=min(8, len(os.sched_getaffinity(0))))
    a = ap.parse_args()
    trees = [os.path.join(os.path.abspath(t), "stereo.vision_amd", "csrc") for t in (a.parent, a.this)]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.j) as pool:
        jobs = []   # per tree: unit -> future of its ELF
        for ti, csrc in enumerate(trees):
            hipcc, flags, srcs = make_vars(csrc)
            if a.diag:
                flags = flags + ["-DSVX_DIAG"]
            jobs.append({u: pool.submit(compile_unit, csrc, hipcc, flags, u,
                                        os.path.join(tmp, f"{ti}_{u.replace('/', '_')}.elf")) for u in srcs})
        units = list(jobs[0]) + [u for u in jobs[1] if u not in jobs[0]]
        elfs = {u: [j[u].result() if u in j else None for j in jobs] for u in units}
        build = "diagnostic build, -DSVX_DIAG" if a.diag else "release build"
        print(f"# Device-only compiles (gfx950, each tree's Makefile FLAGS, {build}, -fuse-cuid=none) of the parent "
              "tree and this tree, per kernel:")
        print("# SAME = equal function bytes, equal kernel descriptor (all but the code entry offset) and equal "
              "metadata; GONE = in the parent only; NEW = in this tree only")
        same_units = [u for u in units if all(elfs[u]) and open(elfs[u][0], "rb").read() == open(elfs[u][1], "rb").read()]
        print("# byte-identical code objects in both trees: " + " ".join(same_units))
        count = dict(SAME=0, DIFF=0, GONE=0, NEW=0)
        for u in units:
            old, new = (kernels(e) if e else {} for e in elfs[u])
            names = demangle(sorted(set(old) | set(new)))
            if not names:   # a host-only unit
                continue
            print(f"== {u}")
            print(f"kernels: parent {len(old)}  new {len(new)}")
            for n in sorted(names, key=names.get):
                if n not in new or n not in old:
                    tag = "GONE" if n in old else "NEW "
                    print(f"  {tag}   {len((old.get(n) or new[n])[0]):6d} B  {names[n][:100]}")
                    count[tag.strip()] += 1
                    continue
                o, w = old[n], new[n]
                tag = "SAME" if o[:3] == w[:3] else "DIFF"
                count[tag] += 1
                nums = " ".join(f"{lab} {o[3][k]}->{w[3][k]}" for lab, k in (
                    ("vgpr", "vgpr_count"), ("sgpr", "sgpr_count"), ("lds", "group_segment_fixed_size"),
                    ("scratch", "private_segment_fixed_size")))
                what = "code" if o[0] != w[0] or tag == "SAME" else "meta"
                print(f"  {tag}   {what} {len(o[0]):6d}->{len(w[0]):6d} B kd {'=' if o[1] == w[1] else '!'} {nums}  "
                      f"{names[n][:85]}")
        print("# " + "  ".join(f"{k} {v}" for k, v in count.items()))
    return 0 if not (count["DIFF"] or count["GONE"] or count["NEW"]) else 1


if __name__ == "__main__":
    sys.exit(main())
