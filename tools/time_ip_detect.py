#!/usr/bin/env python3
"""Timing of interest-point detection and description on the GPU (csrc/ip_detect.hip, csrc/ip_describe.hip): the image resident
on the device, IntegralAutoGainDetector with 1 000 points per 1024 x 1024 tile, then SGrad.

Per stage: the device time from the HIP events the library puts around its launches (vwgpu_profile_enable), summed over the
launches of one call; the median and the range over `--windows` calls after a warm-up call.  Cases: one 1024 x 1024 tile and
the 16 tiles of a 4096 x 4096 image (--sizes).  Next to each figure the stage's stated bound at --clock-mhz and
the fraction of it that was reached, and with --cpu the single-thread time of the CPU restatement
(tests/refimpl/ip_detect_ref.cc) on this host for one 1024 x 1024 tile (its result is what the GPU's must equal).
With --obalog the OBALoG detector (threshold 0.01) is timed as well, which adds the orientation stage.

The bounds, per 1024 x 1024 tile of w x h pixels, S = 8 scales, n candidates, p points:
  integral     latency: ceil(h / 64) bands x (w + 63) steps x 4 dependent vector instructions x 4 cycles (a lone wave issues one
               vector instruction per 4 cycles); tiles run side by side, so the bound of a call is that of one tile
  planes       the bytes that must move: S planes written and the integral read once, at 8 TB/s
  extrema      S planes read once, at 8 TB/s
  cull         n^2 comparisons of 3 vector operations over 256 CUs x 64 lanes per clock
  orientation  p x (113 samples x 12 taps x 4 loads) 4-byte loads at one load per lane per clock over 256 CUs x 64 lanes
  sgrad        latency: (42 + 63) steps x 16 cycles of the support's integral + 180 x 2 x 4 cycles of the serial norm, per point,
               over 1024 SIMDs with one wave each
usage: python tools/time_ip_detect.py [--sizes 1024,4096] [--windows 7] [--clock-mhz 2400] [--cpu] [--obalog]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))

STAGES = ("ip_integral", "ip_planes", "ip_extrema", "ip_cull", "ip_orientation", "ip_crop", "ip_sgrad")


def image_of(size):
    """The 256 x 256 test scene repeated, with fresh noise so that no two tiles are equal."""
    import ip_detect_scenes as sc
    base = sc.scene(256, 256, 21)
    rng = np.random.RandomState(size)
    img = np.tile(base, (size // 256, size // 256)) + 0.01 * rng.uniform(-1, 1, (size, size))
    return np.ascontiguousarray(np.clip(img, 0, 1), np.float32)


def bounds(size, stats, points, clock_hz):
    tiles = (size // 1024) ** 2
    w = h = 1024
    lanes = 256 * 64
    n = max(s[1] for s in stats)
    return {
        "ip_integral": (h // 64) * (w + 63) * 16 / clock_hz,
        "ip_planes": tiles * (8 * 4 * w * h + 4 * (w + 1) * (h + 1)) / 8e12,
        "ip_extrema": tiles * 8 * 4 * w * h / 8e12,
        "ip_cull": sum(float(s[1]) ** 2 * 3 for s in stats) / lanes / clock_hz,
        "ip_orientation": points * 113 * 12 * 4 / lanes / clock_hz,
        "ip_crop": tiles * 2 * 4 * 1200 * 1200 / 8e12,
        "ip_sgrad": points * (105 * 16 + 180 * 2 * 4) / 1024 / clock_hz,
    }, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--clock-mhz", type=float, default=2400.0)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--obalog", action="store_true")
    args = ap.parse_args()
    import torch
    import visionworkbench_amd as vwa
    from visionworkbench_amd import interest_point as ipm
    ctx = vwa.Context(0)
    clock = args.clock_mhz * 1e6
    for size in [int(s) for s in args.sizes.split(",")]:
        img = image_of(size)
        dimg = torch.from_numpy(img).cuda()
        dets = [("iagd", ipm.IntegralAutoGainDetector(1000))]
        if args.obalog:
            dets.append(("obalog", ipm.IntegralInterestPointDetector(ipm.OBALoGInterestOperator(0.01), max_points=1000)))
        for name, det in dets:
            gen = ipm.SGradDescriptorGenerator()
            rows = {s: [] for s in STAGES}
            total, stats, ip = [], [], None
            for window in range(args.windows + 1):
                ctx.profile_enable(True)
                ctx.profile_reset()
                stats = []
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ip = ipm.detect_interest_points(dimg, det, 1000, ctx=ctx, stats=stats)
                ip = ipm.describe_interest_points(dimg, gen, ip, ctx=ctx)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                got = {}
                for stage, ms in ctx.profile_read():
                    got[stage] = got.get(stage, 0.0) + ms
                ctx.profile_enable(False)
                if window == 0:
                    continue      # warm-up: arenas grow, code objects load
                total.append(wall * 1e3)
                for s in STAGES:
                    rows[s].append(got.get(s, 0.0))
            bound, most = bounds(size, stats, len(ip), clock)
            print("%d x %d, %s + sgrad: %d tiles, %d points, candidates per tile at most %d, wall %.2f ms (median of %d, host included)"
                  % (size, size, name, len(stats), len(ip), most, float(np.median(total)), args.windows))
            for s in STAGES:
                v = np.array(rows[s])
                if not v.any():
                    continue
                med = float(np.median(v))
                print("  %-15s %9.3f ms  [%8.3f .. %8.3f]  bound %9.4f ms  fraction %.4f"
                      % (s, med, v.min(), v.max(), bound[s] * 1e3, bound[s] * 1e3 / med))
    if args.cpu:
        import ip_detect_ref as ref
        img = image_of(1024)
        t0 = time.perf_counter()
        ref.integral(img)
        t1 = time.perf_counter()
        f, st = ref.detect(img, ref.IAGD, max_points=1000, desired=1000)
        t2 = time.perf_counter()
        ip = ipm.InterestPoints(f["x"], f["y"], np.zeros((f["x"].size, 0), np.float32), scale=f["scale"])
        ref.describe(img, ipm.description_crop(ip, 42), ip.x, ip.y, ip.scale, ip.orientation, ref.SGRAD)
        t3 = time.perf_counter()
        print("CPU restatement, one 1024 x 1024 tile, one thread: integral %.1f ms, detect (integral, planes, extrema, cull) %.1f ms, "
              "sgrad of %d points %.1f ms" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, len(ip), (t3 - t2) * 1e3))
    ctx.close()


if __name__ == "__main__":
    main()
