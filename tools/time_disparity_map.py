#!/usr/bin/env python3
"""Timing of the operators of disparity_map.hip on a 4096^2 map, tensors resident on the device.

Per operator and pixel type: the device time of one call (torch events around `--repeat` back-to-back calls after one
warm-up call, divided by the count; the median of `--windows` such windows and their spread), the effective bandwidth
(the compulsory bytes of the operator, counted from the shapes below, over that time) and its share of 8 TB/s, and
beside it the single-thread CPU restatement (tests/refimpl/disparity_map_ref.cc) on the same host and the same map.
Compulsory bytes per INPUT pixel: a disparity pixel is 12 B.
  get_disparity_range 12 (read);  disparity_range_mask, transform_disparities, 24 (read + write);
  intersect_mask_and_data 36;  missing_pixel_image 15;  disparity_subsample 12 + 3 (a quarter of the pixels written);
  disparity_upsample 12 + 48;  disparity_transform_image 12 + 4 + 4 (the gathered right image counted once).
get_disparity_range is timed with a device result (no host copy); range_mask without stats.
usage: python tools/time_disparity_map.py [--size 4096] [--no-cpu] [--repeat 20] [--windows 5]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))

HBM = 8.0e12


def tile(img, n):
    reps = [-(-n // img.shape[0]), -(-n // img.shape[1])] + [1] * (img.ndim - 2)
    return np.ascontiguousarray(np.tile(img, reps)[:n, :n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    import torch
    import disparity_map_ref as ref
    from visionworkbench_amd import BBox2i, stereo
    if not torch.cuda.is_available():
        sys.exit("time_disparity_map: no GPU; nothing is measured without one")
    n = args.size
    maps = {"f32": tile(ref.float_scene(1111, 1033, seed=90), n), "i32": tile(ref.int_scene(1111, 1033, seed=92), n)}
    others = {"f32": tile(ref.float_scene(1111, 1033, seed=94), n), "i32": tile(ref.int_scene(1111, 1033, seed=95), n)}
    right = tile(ref.image_scene(1111, 1033, seed=93), n)
    warp_d = tile(ref.warp_scene(1111, 1033, seed=96), n)
    mn, mx = (40, 30), (n - 20, n - 10)
    m = ref.PROJECTIVE
    box = BBox2i(100, 200, n, n)

    def cpu(fn):
        if args.no_cpu:
            return None
        t0 = time.time()
        fn()
        return (time.time() - t0) * 1e3

    def gpu(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.repeat):
                out = fn()
            e1.record()
            torch.cuda.synchronize()
            del out
            times.append(e0.elapsed_time(e1) / args.repeat)
        return float(np.median(times)), min(times), max(times)

    def report(name, t, cpu_ms, bytes_px):
        ms, lo, hi = t
        gbs = bytes_px * n * n / (ms * 1e-3) / 1e9
        line = "%-40s %8.3f ms (%.3f - %.3f)  %7.0f GB/s on %2d B/pixel = %4.1f %% of 8 TB/s" % (
            name, ms, lo, hi, gbs, bytes_px, 100 * gbs * 1e9 / HBM)
        if cpu_ms is not None:
            line += "  CPU %8.1f ms, GPU %.0fx" % (cpu_ms, cpu_ms / ms)
        print(line, flush=True)

    for key in ("f32", "i32"):
        d, o = maps[key], others[key]
        dt, ot = torch.from_numpy(d).cuda(), torch.from_numpy(o).cuda()
        report("get_disparity_range %s" % key, gpu(lambda: stereo.get_disparity_range(dt, device_result=True)),
               cpu(lambda: ref.get_disparity_range(d)), 12)
        report("disparity_range_mask %s" % key, gpu(lambda: stereo.disparity_range_mask(dt, mn, mx)),
               cpu(lambda: ref.disparity_range_mask(d, mn, mx)), 24)
        report("transform_disparities functor %s" % key, gpu(lambda: stereo.transform_disparities(dt, m)),
               cpu(lambda: ref.transform_disparities(d, m)), 24)
        report("transform_disparities subregion round %s" % key, gpu(lambda: stereo.transform_disparities_subregion(True, box, m, dt)),
               cpu(lambda: ref.transform_disparities(d, m, "subregion_round", 100, 200)), 24)
        report("intersect_mask_and_data %s" % key, gpu(lambda: stereo.intersect_mask_and_data(dt, ot)),
               cpu(lambda: ref.intersect_mask_and_data(d, o)), 36)
        report("missing_pixel_image %s" % key, gpu(lambda: stereo.missing_pixel_image(dt)), cpu(lambda: ref.missing_pixel_image(d)), 15)
        report("disparity_subsample %s" % key, gpu(lambda: stereo.disparity_subsample(dt)), cpu(lambda: ref.disparity_subsample(d)), 15)
        report("disparity_upsample %s" % key, gpu(lambda: stereo.disparity_upsample(dt)), cpu(lambda: ref.disparity_upsample(d)), 60)
        del dt, ot
    rt, wt = torch.from_numpy(right).cuda(), torch.from_numpy(warp_d).cuda()
    report("disparity_transform_image", gpu(lambda: stereo.disparity_transform_image(rt, wt)),
           cpu(lambda: ref.disparity_transform_image(right, warp_d)), 20)


if __name__ == "__main__":
    main()
