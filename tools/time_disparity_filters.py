#!/usr/bin/env python3
"""Timing of the disparity post-filters (disparity_filters.hip) on a 4096^2 map in 1024^2 boxes.

Per filter, window size and semantics: the device time from torch events after one warm-up call (tensors resident; the
call's one stream synchronisation for the box table included), Mpix/s, and beside it the 16-thread CPU restatement
(tests/refimpl/disparity_filters_ref.cc) on a sampled 2048^2 crop in 512^2 boxes (16 boxes, one per thread: the
restatement is serial within a box) and the GPU's multiple of it.  For the snapshot kernels also the compulsory bytes
(disparity in + out 24 B per pixel, texture in 4 B; texture_measure 4 + 4 B) / time as a fraction of 8 TB/s.  For the
k^2 kernels (texture_measure, the smoothing at texture 0, the median's selection sweeps) window samples per second and
the VALU instructions per sample that the vector issue ceiling (256 CUs x 4 SIMDs x one wave64 instruction per 4 cycles
x 2.4 GHz = 3.93e13 lane-instructions/s) allows at that rate.  A sample is one window element visited once:
texture_measure visits 2 k^2 per pixel (3 k^2 double adds), the smoothing k^2, the median's bisection (33 or 34) k^2.
usage: python tools/time_disparity_filters.py [--size 4096] [--no-cpu] [--only median,neighbor,texture,smooth]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))

ISSUE = 256 * 4 * 64 / 4 * 2.4e9
HBM = 8.0e12


def tile(img, n):
    reps = [-(-n // img.shape[0]), -(-n // img.shape[1])] + [1] * (img.ndim - 2)
    return np.ascontiguousarray(np.tile(img, reps)[:n, :n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", default="median,neighbor,texture,smooth")
    args = ap.parse_args()
    import torch
    import disparity_filters_ref as dfr
    from visionworkbench_amd import stereo
    n, b = args.size, args.block
    only = args.only.split(",")
    d = tile(dfr.float_scene(1111, 1033, seed=90), n)
    di = tile(dfr.int_scene(1111, 1033, seed=92), n)
    img = tile(dfr.image_scene(1111, 1033, seed=93), n)
    zero = np.zeros((n, n), np.float32)            # texture 0: every valid pixel smooths over the largest window
    crop, cb = min(2048, n), min(512, n)
    dt, dit, it, zt = (torch.from_numpy(a).cuda() for a in (d, di, img, zero))

    def cpu(fn):
        if args.no_cpu:
            return None
        t0 = time.time()
        fn()
        return (time.time() - t0) / crop ** 2 * 1e9

    def gpu(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        del out
        return e0.elapsed_time(e1)

    def report(name, ms, cpu_ns, bytes_px=None, samples_px=None):
        line = "%-34s %9.2f ms  %9.1f Mpix/s" % (name, ms, n * n / ms / 1e3)
        if bytes_px:
            line += "  %.1f %% of 8 TB/s on %d compulsory B/pixel" % (100 * bytes_px * n * n / (ms * 1e-3) / HBM, bytes_px)
        if samples_px:
            rate = samples_px * n * n / (ms * 1e-3)
            line += "  %.1f Gsamples/s = the issue ceiling at %.0f VALU per sample" % (rate / 1e9, ISSUE / rate)
        if cpu_ns is not None:
            line += "  CPU %.0f ns/pixel, GPU %.0fx" % (cpu_ns, cpu_ns / (ms * 1e6 / n / n))
        print(line, flush=True)

    for sem in ("snapshot", "reference"):
        snap = sem == "snapshot"
        if "median" in only:
            for k in (3, 5, 9, 15):
                c = cpu(lambda: dfr.disparity_median_filter(d[:crop, :crop].copy(), k, sem, block_size=(cb, cb)))
                ms = gpu(lambda: stereo.disparity_median_filter(dt, k, sem, block_size=(b, b)))
                report("median k %2d %s" % (k, sem), ms, c, 24 if snap else None, 33.5 * k * k if snap else None)
        if "neighbor" in only:
            c = cpu(lambda: dfr.disparity_neighbor_filter(di[:crop, :crop].copy(), sem, block_size=(cb, cb)))
            ms = gpu(lambda: stereo.disparity_neighbor_filter(dit, sem, block_size=(b, b)))
            report("neighbour %s" % sem, ms, c, 24 if snap else None)
        if "smooth" in only:
            for k in (11, 13, 31):
                c = cpu(lambda: dfr.texture_preserving_disparity_filter(d[:crop, :crop].copy(), zero[:crop, :crop], 0.15, k, sem,
                                                                        block_size=(cb, cb)))
                ms = gpu(lambda: stereo.texture_preserving_disparity_filter(dt, zt, 0.15, k, sem, block_size=(b, b)))
                report("smoothing max %2d texture 0 %s" % (k, sem), ms, c, 28 if snap else None, k * k if snap else None)
    if "texture" in only:
        for k in (3, 9, 15, 31):
            c = cpu(lambda: dfr.texture_measure(img[:crop, :crop], k, block_size=(cb, cb)))
            ms = gpu(lambda: stereo.texture_measure(it, k, block_size=(b, b)))
            report("texture_measure k %2d" % k, ms, c, 8, 2 * k * k)


if __name__ == "__main__":
    main()
