#!/usr/bin/env python3
"""Timing of the local outlier filters (outlier_filters.hip) and std_dev_image on a 4096^2 float disparity map.

Per method and window (3, 11, 31 across: half kernels 1, 5, 15): the device time from torch events around `reps` calls
after one warm-up call (tensors resident, no stats: no synchronisation inside the call), the median and the spread of
the repetitions, Mpix/s, and beside it the 16-thread CPU restatement (tests/refimpl/outlier_filters_ref.cc, threaded by
rows) on the same host, run once on a crop of the same map (2048^2; 1024^2 at window 31) and scaled per pixel, and the
GPU's multiple of it.  The mean filter is timed in both semantics, each method also as its clean-up composition at
window 11, and std_dev_image at sizes 3, 11, 31.
usage: python tools/time_outlier_filters.py [--size 4096] [--reps 5] [--no-cpu] [--only mean,stddev,plane,image]
       [--markdown FILE]   (also writes the table to FILE)"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))

ARGS = {"mean": (1.0,), "stddev": (1.5, 0.3), "plane": (1.5, 0.2)}


def tile(img, n):
    reps = [-(-n // img.shape[0]), -(-n // img.shape[1])] + [1] * (img.ndim - 2)
    return np.ascontiguousarray(np.tile(img, reps)[:n, :n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only", default="mean,stddev,plane,image")
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    import torch
    import outlier_filters_ref as ofr
    from visionworkbench_amd import stereo
    assert torch.cuda.is_available(), "timing needs a GPU"
    n = args.size
    only = args.only.split(",")
    d = tile(ofr.float_scene(1111, 1033, seed=90), n)
    img = tile(ofr.image_scene(1111, 1033, seed=93), n)
    dt, it = torch.from_numpy(d).cuda(), torch.from_numpy(img).cuda()
    plain = {"mean": stereo.rm_outliers_using_mean, "stddev": stereo.rm_outliers_using_stddev, "plane": stereo.rm_outliers_using_plane}
    clean = {"mean": stereo.disparity_cleanup_using_mean, "stddev": stereo.disparity_cleanup_using_stddev,
             "plane": stereo.disparity_clean_using_plane}
    rows = []

    def cpu(fn, crop):
        if args.no_cpu:
            return None
        t0 = time.time()
        fn(min(crop, n))
        return (time.time() - t0) / min(crop, n) ** 2 * 1e9

    def gpu(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            del out
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), min(ms), max(ms)

    def report(name, t, cpu_ns):
        ms, lo, hi = t
        gpu_ns = ms * 1e6 / n / n
        row = [name, "%.2f" % ms, "%.2f - %.2f" % (lo, hi), "%.1f" % (n * n / ms / 1e3),
               "not run" if cpu_ns is None else "%.0f" % cpu_ns, "not run" if cpu_ns is None else "%.0f x" % (cpu_ns / gpu_ns)]
        rows.append(row)
        print("%-44s %9s ms (%s)  %9s Mpix/s  CPU %s ns/pixel  GPU %s" % tuple(row), flush=True)

    for method in ("mean", "stddev", "plane"):
        if method not in only:
            continue
        for half in (1, 5, 15):
            crop = 1024 if half == 15 else 2048
            for sem in (("reference", "skip") if method == "mean" else ("reference",)):
                kw = {"semantics": sem} if method == "mean" else {}
                c = cpu(lambda m: ofr.rm_outliers(method, d[:m, :m], half, half, *ARGS[method], semantics=sem), crop)
                t = gpu(lambda: plain[method](dt, half, half, *ARGS[method], **kw))
                report("%s %dx%d%s" % (method, 2 * half + 1, 2 * half + 1, " " + sem if method == "mean" else ""), t, c)
        c = cpu(lambda m: ofr.rm_outliers(method, d[:m, :m], 5, 5, *ARGS[method], cleanup=True), 2048)
        t = gpu(lambda: clean[method](dt, 5, 5, *ARGS[method]))
        report("%s 11x11 with clean-up" % method, t, c)
    if "image" in only:
        for k in (3, 11, 31):
            c = cpu(lambda m: ofr.std_dev_image(img[:m, :m], k, k, "zero"), 2048)
            t = gpu(lambda: stereo.std_dev_image(it, k, k, "zero"))
            report("std_dev_image %dx%d" % (k, k), t, c)
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("| filter, %d x %d float map | GPU ms (median of %d) | min - max ms | Mpix/s | CPU 16 threads ns/pixel | GPU / CPU |\n"
                    % (n, n, args.reps))
            f.write("|---|---|---|---|---|---|\n")
            for row in rows:
                f.write("| " + " | ".join(row) + " |\n")


if __name__ == "__main__":
    main()
