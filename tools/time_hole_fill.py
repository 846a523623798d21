#!/usr/bin/env python3
"""Timing of the hole filling on the GPU (csrc/hole_fill.hip), images resident on the device.

Three measurements, each the median of `--windows` windows of HIP events (through torch) around `--repeat` back-to-back
calls after a warm-up call, divided by the count, with the spread of the windows:
  1. fill_holes_grass on a --size x --size float disparity map with planted holes of mixed size (rectangles of 1 .. 64
     pixels a side, four fifths of their pixels invalid), hole_fill_len 10, 30 and 64; beside it the time of the CPU
     restatement (tests/refimpl/hole_fill_ref.cc, one thread) on the same host and input, and a word-for-word comparison of
     the two results.  With --both-forms also with VWGPU_OPT_INPAINT_OVERLAP = 0, one form after the other.
  2. One 64 x 64 hole alone in a 70 x 70 map: the latency case (one workgroup of one wavefront).
  3. grassfire (uint8 source) and blob_index (float disparity) at --size, as a fraction of a device-to-device copy of the
     bytes each reads and writes, timed in the same run (no data-sheet number enters).
usage: python tools/time_hole_fill.py [--size 4096] [--repeat 5] [--windows 5] [--both-forms] [--no-cpu]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))


def planted(n, seed=5, count=None):
    rng = np.random.RandomState(seed)
    hole = np.zeros((n, n), bool)
    count = count if count is not None else (n * n) // 8192
    for _ in range(count):
        side = int(rng.choice([1, 2, 3, 5, 8, 10, 16, 24, 30, 48, 64], p=[.2, .15, .15, .12, .1, .08, .07, .05, .04, .02, .02]))
        bw, bh = rng.randint(max(1, side // 2), side + 1, 2)
        x, y = rng.randint(2, n - bw - 2), rng.randint(2, n - bh - 2)
        hole[y:y + bh, x:x + bw] |= rng.uniform(size=(bh, bw)) < 0.8
    return hole


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--both-forms", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    import hole_fill_ref as ref
    import visionworkbench_amd as vwa
    from visionworkbench_amd import core, image
    if not torch.cuda.is_available():
        sys.exit("time_hole_fill: no GPU; nothing is measured without one")
    ctx = vwa.Context(0)

    def windows(fn, repeat=args.repeat):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(repeat):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b) / repeat)
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    def show(name, t, extra=""):
        print("%-52s %10.3f ms  (windows %.3f .. %.3f) %s" % (name, t[0], t[1], t[2], extra), flush=True)

    n = args.size
    base = ref.float_map(n, n, 3)
    hole = planted(n)
    src = ref.punch(base, hole, None)
    d = torch.from_numpy(src).cuda()
    out = torch.empty_like(d)
    print("fill_holes_grass, %d x %d float disparity, %d invalid pixels" % (n, n, int(hole.sum())))
    for L in (10, 30, 64):
        forms = [(1, "")] + ([(0, " no overlap")] if args.both_forms else [])
        for overlap, tag in forms:
            ctx.set_option(core.OPT_INPAINT_OVERLAP, overlap)
            t = windows(lambda: image.fill_holes_grass(d, L, out=out, ctx=ctx))
            filled = int(((out[..., 2] != 0) & (d[..., 2] == 0)).sum().item())
            show("  L = %2d%s: GPU" % (L, tag), t, "%d pixels filled" % filled)
        ctx.set_option(core.OPT_INPAINT_OVERLAP, 1)
        if not args.no_cpu:
            t0 = time.perf_counter()
            want = ref.fill_holes_grass(src, L)
            cpu = (time.perf_counter() - t0) * 1e3
            print("  L = %2d: CPU restatement %38.1f ms   equal words: %s" % (L, cpu, bool(np.array_equal(want, out.cpu().numpy()))), flush=True)

    print("one 64 x 64 hole in 70 x 70 (PixelMask<float> and float disparity)")
    for kind in (1, 3):
        one = np.zeros((70, 70), bool)
        one[3:67, 3:67] = True
        s1 = ref.punch(ref.float_map(70, 70, kind), one, None)
        d1 = torch.from_numpy(s1).cuda()
        o1 = torch.empty_like(d1)
        forms = [(1, "")] + ([(0, " no overlap")] if args.both_forms else [])
        for overlap, tag in forms:
            ctx.set_option(core.OPT_INPAINT_OVERLAP, overlap)
            show("  kind %d%s: GPU" % (kind, tag), windows(lambda: image.fill_holes_grass(d1, 64, out=o1, ctx=ctx), 2))
        ctx.set_option(core.OPT_INPAINT_OVERLAP, 1)
        if not args.no_cpu:
            t0 = time.perf_counter()
            want = ref.fill_holes_grass(s1, 64)
            cpu = (time.perf_counter() - t0) * 1e3
            print("  kind %d: CPU restatement %37.1f ms   equal words: %s" % (kind, cpu, bool(np.array_equal(want, o1.cpu().numpy()))), flush=True)

    print("grassfire and blob_index at %d x %d against a copy of their bytes" % (n, n))
    mask = torch.from_numpy((~hole).astype(np.uint8)).cuda()
    g = torch.empty((n, n), dtype=torch.int32, device="cuda")
    for ib in (False, True):
        t = windows(lambda: ctx.check(ctx._lib.vwgpu_grassfire_dev(ctx._h, 0, mask.data_ptr(), n, n, 0, int(ib), g.data_ptr(), 0)))
        nbytes = n * n * 5      # one uint8 read, one int32 written
        a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        c = windows(lambda: b.copy_(a))
        show("  grassfire ignore_borders %d" % ib, t, "copy of %d bytes %.3f ms: %.1f x" % (nbytes, c[0], t[0] / c[0]))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for invert in (False, True):
        cnt = image.blob_index(d, invert=invert, ctx=ctx).count
        t = windows(lambda: image.blob_index(d, invert=invert, capacity=cnt, ctx=ctx))
        nbytes = n * n * 16     # one 12-byte pixel read, one int32 label written
        a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        c = windows(lambda: b.copy_(a))
        show("  blob_index invert %d (%d blobs)" % (invert, cnt), t, "copy of %d bytes %.3f ms: %.1f x" % (nbytes, c[0], t[0] / c[0]))
    ctx.close()


if __name__ == "__main__":
    main()
