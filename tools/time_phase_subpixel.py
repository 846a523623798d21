#!/usr/bin/env python3
"""Timing of the phase sub-pixel refiner (stereo.phase_subpixel, phase_refine_kernel in phase_subpixel.hip) on a 4096^2
stretched LoG pair scaled to [0, 1].

Input: pyr_ref.unit_scene (right = left stretched by 3 %, the true disparity fractional and known), its rounded true
disparity as the start, PREFILTER_LOG 1.4, max_pyramid_levels = 0 (phase_subpixel's default), accuracy 20, blocks 1024^2,
kernels 15 x 15 and 35 x 35.  Reports wall time from device events after one warm-up call, Mpix/s, the share of the FP32
vector peak (157.3 TFLOP/s) the stated FLOP count reaches, and the CPU restatement's time per pixel on 16 threads over a
crop, and the GPU's multiple of it.

FLOP count of one valid pixel, K x K window, as the kernel does the work (2 FLOP per fma, the rest not counted): three
forward DFTs (the left patch once, the right patch per call), each K^2 outputs of a K-term real row sum (2 fma) and K^2 of a
K-term complex column sum (4 fma): 6 K^3 fma; per call the padded inverse, 2K^2 outputs of a K-term complex sum (4 fma)
and 4K^2 real outputs of a K-term sum (2 fma): 16 K^3 fma; per call with a pad factor p > 2 (up = ceil(1.5 p)) the
partial upsample, up K outputs of a K-term complex sum and up^2 of a K-term complex sum (4 fma each).
usage: python tools/time_phase_subpixel.py [--size 4096] [--kernels 15,35] [--block 1024] [--accuracy 20] [--no-cpu]"""
import argparse
import math
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))

PEAK_FP32 = 157.3e12


def flop_per_pixel(k, accuracy):
    fma = 18 * k ** 3 + 2 * 16 * k ** 3
    for p in (int(accuracy / 2), accuracy):      # C integer division (toward zero)
        if p > 2:
            up = math.ceil(1.5 * p)
            fma += 4 * up * k * k + 4 * up * up * k
    return 2 * fma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--kernels", default="15,35")
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--accuracy", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import phase_ref
    import pyr_ref
    kernels = [int(k) for k in args.kernels.split(",")]
    acc, b = args.accuracy, args.block
    cpu_ns = {}
    if not args.no_cpu:
        crop = 256
        l2, r2, d2, _ = pyr_ref.unit_scene(crop, crop)
        tiles = pyr_ref.tiles_for(crop, crop, (crop // 4, crop // 4))
        for k in kernels:
            t0 = time.time()
            ths = [threading.Thread(target=phase_ref.phase_subpixel, args=(d2, l2, r2, 2, 1.4, (k, k), 0, acc),
                                    kwargs={"tiles": [t], "threads": 1}) for t in tiles]
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            s = time.time() - t0
            cpu_ns[k] = s / crop ** 2 * 1e9
            print("CPU restatement, %d^2 crop in 16 tiles of %d^2 on 16 threads, k %d: %.2f s = %.0f ns per pixel"
                  % (crop, crop // 4, k, s, cpu_ns[k]), flush=True)
    if args.size > 0:
        import torch
        from visionworkbench_amd import stereo
        n = args.size
        left, right, d, true = pyr_ref.unit_scene(n, n)
        lt, rt, dt_ = (torch.from_numpy(a).cuda() for a in (left, right, d))
        for k in kernels:
            st = []
            stereo.phase_subpixel(dt_, lt, rt, 2, 1.4, (k, k), 0, acc, block_size=(b, b))   # warm-up
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = stereo.phase_subpixel(dt_, lt, rt, 2, 1.4, (k, k), 0, acc, block_size=(b, b), stats=st)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            o = out.cpu().numpy()
            v = o[..., 2] > 0
            inner = (slice(64, -64), slice(64, -64))
            mae = float(np.abs(o[..., 0] - true)[inner][v[inner]].mean())
            mae0 = float(np.abs(d[..., 0] - true)[inner].mean())
            fl = flop_per_pixel(k, acc) * st[0]
            line = ("phase k %2d acc %d block %4d: %9.1f ms  %8.2f Mpix/s  refined %d invalidated %d  %.2f MFLOP/pixel  "
                    "%.1f TFLOP/s = %.1f %% of FP32 peak  invalid %.4f  MAE %.3f -> %.3f"
                    % (k, acc, b, ms, n * n / ms / 1e3, st[0], st[1], flop_per_pixel(k, acc) / 1e6, fl / ms / 1e9,
                       100 * fl / ms / 1e-3 / PEAK_FP32, 1 - v.mean(), mae0, mae))
            if k in cpu_ns:
                line += "  %.0fx the 16-thread restatement" % (cpu_ns[k] / (ms * 1e6 / n / n))
            print(line, flush=True)


if __name__ == "__main__":
    main()
