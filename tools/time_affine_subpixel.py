#!/usr/bin/env python3
"""Timing of affine sub-pixel refinement (stereo.affine_subpixel, affine_subpixel.hip) on a 4096^2 stretched LoG pair.

Input: the stretched scene of tests/refimpl (right = left stretched by 3 %, so the true disparity is fractional and
known), its rounded true disparity as the integer starting point, PREFILTER_LOG 1.4, max_pyramid_levels = 2.  Kernels
15 x 15 and 35 x 35, blocks 1024^2 and 256^2.  Reports wall time from device events after one warm-up call, Mpix/s,
fixpoint rounds and window-loop iterations counted by the kernel, VALU instructions of the window loop from the ISA, the
refinement's share of the vector issue rate (78.6 T lane-ops/s, MI355X_MICROARCH.md) and the CPU restatement's ns per
pixel on 16 threads over a crop.
usage: python tools/time_affine_subpixel.py [--size 4096] [--no-cpu] [--no-isa]"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))


def window_loop_valu():
    """VALU instructions per trip of the deepest loop of affine_refine_kernel with the most VALU work (the window loop)."""
    src = os.path.join(ROOT, "visionworkbench_amd", "csrc", "affine_subpixel.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "aff.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src), "--cuda-device-only", "-S",
                               src, "-o", out], stderr=subprocess.DEVNULL)
        lines = open(out).read().splitlines()
    inside, loops, cur, depth = False, collections.defaultdict(collections.Counter), None, {}
    for line in lines:
        if re.match(r"^_Z\S+:", line):
            inside = "affine_refine_kernel" in line
            continue
        if not inside:
            continue
        m = re.search(r"Header=(BB\S+) Depth=(\d+)", line)
        if m and (line.startswith(".L") or line.startswith("; %bb")):
            cur = m.group(1)
            depth[cur] = int(m.group(2))
            continue
        if line.startswith(".L") and ":" in line:
            h = line.split(":")[0][1:]
            cur = h if h in loops or "Loop Header" in line else None
            continue
        if "This Inner Loop Header" in line:
            continue
        if cur and line.startswith("\t") and not line.startswith("\t;") and not line.startswith("\t."):
            op = line.split()[0]
            loops[cur]["valu" if op.startswith("v_") else "other"] += 1
    deepest = max(depth.values())
    best = max(((h, c) for h, c in loops.items() if depth.get(h) == deepest), key=lambda kv: kv[1]["valu"])
    return best[0], best[1]["valu"], best[1]["other"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-isa", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import affine_ref
    from visionworkbench_amd import stereo
    n = args.size
    left, right, d, true = affine_ref.stretched_scene(n, n)
    lt, rt, dt_ = (torch.from_numpy(a).cuda() for a in (left, right, d))
    valu = None if args.no_isa else window_loop_valu()
    if valu:
        print("ISA: window loop %s: %d VALU + %d other instructions per trip" % valu)
    rows = []
    for k in (15, 35):
        for b in (1024, 256):
            st = []
            stereo.affine_subpixel(dt_, lt, rt, 2, 1.4, (k, k), 2, block_size=(b, b))   # warm-up
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = stereo.affine_subpixel(dt_, lt, rt, 2, 1.4, (k, k), 2, block_size=(b, b), stats=st)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            o = out.cpu().numpy()
            v = o[..., 2] > 0
            inner = (slice(64, -64), slice(64, -64))
            mae = float(np.abs(o[..., 0] - true)[inner][v[inner]].mean())
            mae0 = float(np.abs(d[..., 0] - true)[inner].mean())
            lane_ops = st[2] * k * k * (valu[1] if valu else 0)
            share = lane_ops / (ms * 1e-3) / 78.6e12 if valu else float("nan")
            rows.append((k, b, ms, n * n / ms / 1e3, st[0], st[1], st[2], share, mae0, mae))
            print("k %2d block %4d: %9.1f ms  %8.2f Mpix/s  rounds sum %d max %d  iterations %d  VALU share %.3f  MAE %.3f -> %.3f"
                  % rows[-1], flush=True)
    if not args.no_cpu:
        crop = 512
        l2, r2, d2, _ = affine_ref.stretched_scene(crop, crop)
        tiles = affine_ref.tiles_for(crop, crop, (128, 128))
        for k in (15, 35):
            t0 = time.time()
            ths = [threading.Thread(target=affine_ref.pyramid_subpixel, args=(d2, l2, r2, 2, 1.4, (k, k), 2),
                                    kwargs={"tiles": [t]}) for t in tiles]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            s = time.time() - t0
            print("CPU restatement, %d^2 crop in 16 tiles of 128^2 on 16 threads, k %d: %.2f s = %.0f ns per pixel" % (crop, k, s, s / crop ** 2 * 1e9))


if __name__ == "__main__":
    main()
