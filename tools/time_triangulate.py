#!/usr/bin/env python3
"""Timing of stereo triangulation (csrc/triangulate.hip) on a 4096^2 float32 disparity map, tensors resident on the device
and outputs allocated once.

Per case: the device time of one vwgpu_stereo_triangulate_dev call (HIP events through torch around `--repeat` back-to-back
calls after a warm-up call, divided by the count; the median of `--windows` such windows and their spread), the compulsory
bytes per pixel over that time, and the ratio to a device-to-device copy of the SAME number of bytes timed in the same
run, which is the yardstick (no data-sheet number enters).  Compulsory bytes per pixel: 12 read + 24 xyz (+ 8 error + 24
error vector).  Cases: the null-distortion pinhole pair with xyz only, with every output, with the statistics; a pair
with Tsai lenses; a CAHV pair; the universe radius on the point image (24 read + 24 written); a pair with each of the FOV,
fisheye, Brown-Conrady, adjustable Tsai and Photometrix lenses on both cameras (--no-lenses leaves them out).
usage: python tools/time_triangulate.py [--size 4096] [--repeat 20] [--windows 5]"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--no-lenses", action="store_true", help="only the cases without the any-lens instantiations")
    args = ap.parse_args()
    import torch
    import triangulate_ref as ref
    import visionworkbench_amd as vwa
    from visionworkbench_amd import camera
    if not torch.cuda.is_available():
        sys.exit("time_triangulate: no GPU; nothing is measured without one")
    n = args.size
    # a smooth surface in front of a converging pair whose principal point is the image centre; f scales with the image
    null1, null2 = ref.pinhole_pair(n, n, f=500.0 * n / 70.0)
    lens = camera.TsaiLensDistortion(*ref.MILD_TSAI)
    tsai1, tsai2 = ref.pinhole_pair(n, n, f=500.0 * n / 70.0, distortion1=lens, distortion2=lens)
    cahv1, cahv2 = ref.cahv_of(null1), ref.cahv_of(null2)
    d = ref._depth_disparity(null1, null2, n, n, seed=3).astype(np.float32)
    d[np.random.default_rng(4).random((n, n)) < 0.04, 2] = 0
    dt = torch.from_numpy(d).cuda()
    xyz = torch.empty((n, n, 3), dtype=torch.float64, device="cuda")
    err = torch.empty((n, n), dtype=torch.float64, device="cuda")
    vec = torch.empty((n, n, 3), dtype=torch.float64, device="cuda")
    words = torch.zeros(3, dtype=torch.int64, device="cuda")
    ctx = vwa.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = ctx._lib

    def triangulate(c1, c2, every, stats):
        def call():
            ctx.check(lib.vwgpu_stereo_triangulate_dev(
                ctx._h, 1, dt.data_ptr(), n, n, 0, 0, 0, ctypes.byref(camera.descriptor_of(c1)), ctypes.byref(camera.descriptor_of(c2)),
                0.0, 0, xyz.data_ptr(), 0, err.data_ptr() if every else None, 0, vec.data_ptr() if every else None, 0,
                words.data_ptr() if stats else None))
        return call

    def gpu(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.repeat):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / args.repeat)
        return float(np.median(times)), min(times), max(times)

    copies = {}

    def copy_ms(bytes_px):
        """A device-to-device copy that reads and writes bytes_px * n * n bytes in all (half of them each way)."""
        if bytes_px not in copies:
            half = bytes_px * n * n // 2
            src, dst = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            src.zero_()
            copies[bytes_px] = gpu(lambda: dst.copy_(src))[0]
            del src, dst
        return copies[bytes_px]

    def report(name, t, bytes_px):
        ms, lo, hi = t
        gbs = bytes_px * n * n / (ms * 1e-3) / 1e9
        c = copy_ms(bytes_px)
        print("%-44s %8.3f ms (%.3f - %.3f)  %6.0f GB/s on %2d B/pixel;  copy of the same bytes %8.3f ms = %6.0f GB/s;  ratio %.2f" % (
            name, ms, lo, hi, gbs, bytes_px, c, bytes_px * n * n / (c * 1e-3) / 1e9, c / ms), flush=True)

    print("%d x %d float32 disparity map, %s" % (n, n, torch.cuda.get_device_name(0)))
    report("pinhole pair (no lens), xyz", gpu(triangulate(null1, null2, False, False)), 36)
    report("pinhole pair (no lens), xyz + error + errvec", gpu(triangulate(null1, null2, True, False)), 68)
    report("pinhole pair (no lens), xyz + statistics", gpu(triangulate(null1, null2, False, True)), 36)
    report("pinhole pair (Tsai lenses), xyz", gpu(triangulate(tsai1, tsai2, False, False)), 36)
    report("pinhole pair (Tsai lenses), xyz + error + errvec", gpu(triangulate(tsai1, tsai2, True, False)), 68)
    report("CAHV pair, xyz", gpu(triangulate(cahv1, cahv2, False, False)), 36)
    out, origin = torch.empty_like(xyz), np.zeros(3)

    def universe():
        ctx.check(lib.vwgpu_universe_radius_dev(ctx._h, xyz.data_ptr(), 3, n, n, 0, origin.ctypes.data, 11.0, 13.0, out.data_ptr(), 0, None))
    report("universe_radius, 3 channels", gpu(universe), 48)
    if args.no_lenses:
        ctx.close()
        return
    # one camera per lens of the any-lens instantiations; Brown-Conrady and Photometrix work in focal-plane units (pixels here)
    lenses = (("FOV", camera.FovLensDistortion([0.9])), ("fisheye", camera.FisheyeLensDistortion([-0.05, 0.01, -0.003, 0.001])),
              ("Brown-Conrady", camera.BrownConradyDistortion([-0.6, -0.2, 0.13e-8, -0.52e-16, 0, 0.55e-9, 0, 0.201])),
              ("adjustable Tsai", camera.AdjustableTsaiLensDistortion([-0.1, 0.02, -0.003, 1e-3, -2e-3, 0.01])),
              ("Photometrix", camera.PhotometrixLensDistortion([0.6, -0.3, -5e-9, 2e-16, -1e-24, 1e-9, -2e-9, 0, 0])))
    for name, lens_k in lenses:
        cam1, cam2 = ref.pinhole_pair(n, n, f=500.0 * n / 70.0, distortion1=lens_k, distortion2=lens_k)
        report("pinhole pair (%s lenses), xyz" % name, gpu(triangulate(cam1, cam2, False, False)), 36)
    ctx.close()


if __name__ == "__main__":
    main()
