#!/usr/bin/env python3
"""Timing of the Lucas-Kanade and Bayes-EM sub-pixel refiners (stereo.lk_subpixel / bayes_em_subpixel, lk_refine_kernel /
em_refine_kernel in affine_subpixel.hip) on a 4096^2 stretched LoG pair scaled to [0, 1].

Input: the stretched scene of tests/refimpl scaled to [0, 1] (pyr_ref.unit_scene: right = left stretched by 3 %, so the
true disparity is fractional and known), its rounded true disparity as the integer start, PREFILTER_LOG 1.4,
max_pyramid_levels = 2.  Kernels 15 x 15 and 35 x 35, blocks 1024^2 and 256^2.  Reports wall time from device events
after one warm-up call, Mpix/s, fixpoint rounds and window passes counted by the kernel, VALU and FP64 instructions per
trip of the window loop from the ISA, MAE against the true disparity and the CPU restatement's ns per pixel on 16 threads
over a crop.
usage: python tools/time_pyramid_subpixel.py --algorithm lk|em [--size 4096] [--no-cpu] [--no-isa] [--kernels 15,35]
       [--blocks 1024,256]"""
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

KERNEL = {"lk": "lk_refine_kernel", "em": "em_refine_kernel"}


def window_loop_isa(kernel):
    """(loop label, VALU, FP64 VALU, other) per trip of the deepest loop of `kernel` with the most VALU work."""
    src = os.path.join(ROOT, "visionworkbench_amd", "csrc", "affine_subpixel.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "pyr.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src), "--cuda-device-only", "-S",
                               src, "-o", out], stderr=subprocess.DEVNULL)
        lines = open(out).read().splitlines()
    inside, loops, cur, depth = False, collections.defaultdict(collections.Counter), None, {}
    for line in lines:
        if re.match(r"^_Z\S+:", line):
            inside = kernel in line
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
            if op.startswith("v_"):
                loops[cur]["valu"] += 1
                if op.endswith("_f64") or "_f64_" in op:
                    loops[cur]["f64"] += 1
            else:
                loops[cur]["other"] += 1
    deepest = max(depth.values())
    best = max(((h, c) for h, c in loops.items() if depth.get(h) == deepest), key=lambda kv: kv[1]["valu"])
    return best[0], best[1]["valu"], best[1]["f64"], best[1]["other"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--algorithm", choices=["lk", "em"], required=True)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--kernels", default="15,35")
    ap.add_argument("--blocks", default="1024,256")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-isa", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import pyr_ref
    alg = args.algorithm
    isa = None if args.no_isa else window_loop_isa(KERNEL[alg])
    if isa:
        print("ISA: %s window loop %s: %d VALU (%d FP64) + %d other instructions per trip" % ((KERNEL[alg],) + isa), flush=True)
    kernels = [int(k) for k in args.kernels.split(",")]
    blocks = [int(b) for b in args.blocks.split(",")]
    if args.size > 0:
        import torch
        from visionworkbench_amd import stereo
        fn = stereo.lk_subpixel if alg == "lk" else stereo.bayes_em_subpixel
        n = args.size
        left, right, d, true = pyr_ref.unit_scene(n, n)
        lt, rt, dt_ = (torch.from_numpy(a).cuda() for a in (left, right, d))
        for k in kernels:
            for b in blocks:
                st = []
                fn(dt_, lt, rt, 2, 1.4, (k, k), 2, block_size=(b, b))   # warm-up
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(dt_, lt, rt, 2, 1.4, (k, k), 2, block_size=(b, b), stats=st)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1)
                o = out.cpu().numpy()
                v = o[..., 2] > 0
                inner = (slice(64, -64), slice(64, -64))
                mae = float(np.abs(o[..., 0] - true)[inner][v[inner]].mean())
                mae0 = float(np.abs(d[..., 0] - true)[inner].mean())
                print("%s k %2d block %4d: %9.1f ms  %8.2f Mpix/s  rounds sum %d max %d  window passes %d (%.2f per pixel)  "
                      "invalid %.4f  MAE %.3f -> %.3f" % (alg, k, b, ms, n * n / ms / 1e3, st[0], st[1], st[2], st[2] / n / n,
                                                         1 - v.mean(), mae0, mae), flush=True)
    if not args.no_cpu:
        crop = 256 if alg == "em" else 512
        l2, r2, d2, _ = pyr_ref.unit_scene(crop, crop)
        tiles = pyr_ref.tiles_for(crop, crop, (crop // 4, crop // 4))
        code = 0 if alg == "lk" else 2
        for k in kernels:
            t0 = time.time()
            ths = [threading.Thread(target=pyr_ref.pyramid_subpixel, args=(d2, l2, r2, 2, 1.4, (k, k), 2),
                                    kwargs={"tiles": [t], "algorithm": code}) for t in tiles]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            s = time.time() - t0
            print("CPU restatement, %d^2 crop in 16 tiles of %d^2 on 16 threads, k %d: %.2f s = %.0f ns per pixel"
                  % (crop, crop // 4, k, s, s / crop ** 2 * 1e9), flush=True)


if __name__ == "__main__":
    main()
