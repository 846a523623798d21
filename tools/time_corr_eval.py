#!/usr/bin/env python3
"""Timing of disparity quality evaluation (stereo.corr_eval, ce_eval_kernel in corr_eval.hip) on a 4096^2 pair.

Input: corr_eval_ref.scene (a smooth positive texture pair, right = left moved by (-3.3, 0.6) plus noise; a smooth
fractional 2-D disparity around that shift, 8 % invalid pixels), 1024^2 tiles, metrics ncc and parabola_curvature at
7 x 7, 15 x 15 and 35 x 35.  Reports the device time from torch events after one warm-up call (tensors resident, the
call's one stream synchronisation included), Mpix/s, window samples per second, and the VALU instructions per sample
that the vector issue ceiling (256 CUs x 4 SIMDs x one wave64 instruction per 4 cycles x 2.4 GHz = 3.93e13
lane-instructions/s) allows at that rate, to hold against the inner loop's count from the ISA (`hipcc -S` of
corr_eval.hip, tools/isa_loop.py).  A sample is one (c, r) step of one NCC patch: ncc evaluates kx ky per
valid pixel, parabola_curvature 5 kx ky when the centre NCC is >= 0.  With the CPU restatement (tests/refimpl/corr_eval_ref.cc) on
16 threads over the 1024^2 tiles of a sampled 512^2 crop, it prints the GPU's multiple of it.
usage: python tools/time_corr_eval.py [--size 4096] [--kernels 7,15,35] [--metrics ncc,parabola_curvature] [--no-cpu]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))

ISSUE = 256 * 4 * 64 / 4 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--kernels", default="7,15,35")
    ap.add_argument("--metrics", default="ncc,parabola_curvature")
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    import corr_eval_ref
    from visionworkbench_amd import stereo
    kernels = [int(k) for k in args.kernels.split(",")]
    metrics = args.metrics.split(",")
    n, b = args.size, args.block
    left, right, d, _, _ = corr_eval_ref.scene(n, n, seed=21)
    crop = 512
    cpu_ns = {}
    if not args.no_cpu:
        for m in metrics:
            for k in kernels:
                t0 = time.time()
                corr_eval_ref.corr_eval(left[:crop, :crop], right, d[:crop, :crop], (k, k), m, block_size=(b, b), threads=16)
                cpu_ns[m, k] = (time.time() - t0) / crop ** 2 * 1e9
                print("CPU restatement %s k %d, %d^2 crop on 16 threads: %.0f ns per pixel" % (m, k, crop, cpu_ns[m, k]),
                      flush=True)
    lt, rt, dt_ = (torch.from_numpy(a).cuda() for a in (left, right, d))
    for m in metrics:
        for k in kernels:
            st = []
            stereo.corr_eval(lt, rt, dt_, (k, k), m, block_size=(b, b))   # warm-up
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = stereo.corr_eval(lt, rt, dt_, (k, k), m, block_size=(b, b), stats=st)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            samples = st[0] * k * k * (5 if m != "ncc" else 1)
            line = ("%-18s k %2d block %4d: %8.2f ms  %8.1f Mpix/s  evaluated %d valid %d  %.2f Gsamples/s"
                    % (m, k, b, ms, n * n / ms / 1e3, st[0], st[1], samples / ms / 1e6))
            line += "  = the issue ceiling at %.0f VALU per sample" % (ISSUE / (samples / (ms * 1e-3)))
            if (m, k) in cpu_ns:
                line += "  %.0fx the 16-thread restatement" % (cpu_ns[m, k] / (ms * 1e6 / n / n))
            print(line, flush=True)
            del out


if __name__ == "__main__":
    main()
