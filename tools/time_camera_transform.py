#!/usr/bin/env python3
"""Timing of the epipolar resampling (csrc/camera_transform.hip): a 4096^2 float32 output from a 4096^2 source, tensors
resident on the device and outputs allocated once.

Per case: the device time of one vwgpu_camera_transform_dev call (HIP events through torch around `--repeat` back-to-back
calls after a warm-up call, divided by the count; the median of `--windows` such windows and their spread), the compulsory
bytes per pixel over that time (4 read + 4 written, 5 + 5 with masks), and the ratio to a device-to-device copy of the
SAME number of bytes timed in the same run, which is the yardstick (no data-sheet number enters).  Cases: pinhole ->
pinhole with the point-to-pixel check on and off, a Tsai source with the check on (the Newton loop) and off, CAHV -> CAHV,
the masked form, and a CAHVOR and a CAHVORE source (the reference's test cameras scaled to the frame) into their own
linearisation, masked and not, with the re-distortion (CAHV -> CAHVOR / CAHVORE) beside them, and a pinhole with each of
the FOV, fisheye, Brown-Conrady, adjustable Tsai and Photometrix lenses as the source with the check on and off and as the
destination (--no-lenses leaves them out).  VWGPU_LIBRARY selects another build of the library (make -C visionworkbench_amd/csrc ct16: the
16 x 16 workgroup footprint).
usage: python tools/time_camera_transform.py [--size 4096] [--repeat 20] [--windows 5]"""
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
    import epipolar_ref as ref
    import triangulate_ref as tri
    import visionworkbench_amd as vwa
    from visionworkbench_amd import _lib, camera
    if not torch.cuda.is_available():
        sys.exit("time_camera_transform: no GPU; nothing is measured without one")
    n = args.size
    # a source and a rectified camera at one centre that look nearly the same way: all but a rim of the output taps the source
    rot_s, rot_d = tri.rot_y(3.0) @ ref.rot_x(-2.0), tri.rot_y(1.0) @ ref.rot_x(1.5)
    f, c = 1.0 * n, n / 2.0
    lens = camera.TsaiLensDistortion(*ref.MILD_TSAI)
    src = camera.PinholeModel(ref.CENTER, rot_s, f, f, c, c)
    src_tsai = camera.PinholeModel(ref.CENTER, rot_s, f, f, c, c, distortion=lens)
    dst = camera.PinholeModel(ref.CENTER, rot_d, 1.05 * f, 1.05 * f, c, c)
    img = torch.rand((n, n), dtype=torch.float32, device="cuda")
    mask = (torch.rand((n, n), device="cuda") >= 0.1).to(torch.uint8)
    out = torch.empty((n, n), dtype=torch.float32, device="cuda")
    omask = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    ctx = vwa.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    lib = ctx._lib

    def transform(s, d, check, masked):
        ms, md = camera.matrix_of(s), camera.matrix_of(d)

        def call():
            ctx.check(lib.vwgpu_camera_transform_dev(
                ctx._h, img.data_ptr(), n, n, 0, mask.data_ptr() if masked else None, 0, ctypes.byref(camera.descriptor_of(s)),
                None if ms is None else ms.ctypes.data, ctypes.byref(camera.descriptor_of(d)), None if md is None else md.ctypes.data,
                n, n, 0, 0, 0.0, 0, int(check), out.data_ptr(), 0, omask.data_ptr() if masked else None, 0, None))
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
            a, b = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            a.zero_()
            copies[bytes_px] = gpu(lambda: b.copy_(a))[0]
            del a, b
        return copies[bytes_px]

    def report(name, t, bytes_px):
        ms, lo, hi = t
        gbs = bytes_px * n * n / (ms * 1e-3) / 1e9
        cp = copy_ms(bytes_px)
        print("%-44s %8.3f ms (%.3f - %.3f)  %6.0f GB/s on %2d B/pixel;  copy of the same bytes %8.3f ms = %6.0f GB/s;  ratio %.2f" % (
            name, ms, lo, hi, gbs, bytes_px, cp, bytes_px * n * n / (cp * 1e-3) / 1e9, cp / ms), flush=True)

    print("%d x %d float32 output from a %d x %d source, %s, library %s" % (n, n, n, n, torch.cuda.get_device_name(0),
                                                                            os.path.relpath(_lib.LIB_PATH, ROOT)))
    report("pinhole -> pinhole, check on", gpu(transform(src, dst, True, False)), 8)
    report("pinhole -> pinhole, check off", gpu(transform(src, dst, False, False)), 8)
    report("Tsai src -> pinhole, check on", gpu(transform(src_tsai, dst, True, False)), 8)
    report("Tsai src -> pinhole, check off", gpu(transform(src_tsai, dst, False, False)), 8)
    report("CAHV -> CAHV", gpu(transform(tri.cahv_of(src), tri.cahv_of(dst), True, False)), 8)
    report("pinhole -> pinhole, check on, masked", gpu(transform(src, dst, True, True)), 10)
    # CAHVOR / CAHVORE: the fixture cameras of the tests (1024^2 frames) scaled to n, into their own linearisation
    import cahvor_ref
    for name, make in (("CAHVOR", cahvor_ref.cahvor), ("CAHVORE", cahvor_ref.cahvore)):
        raw = make(n / 1024.0)
        lin = camera.linearize_camera(raw, (n, n))
        report("%s -> CAHV" % name, gpu(transform(raw, lin, True, False)), 8)
        report("%s -> CAHV, masked" % name, gpu(transform(raw, lin, True, True)), 10)
        report("CAHV -> %s" % name, gpu(transform(lin, raw, True, False)), 8)
    if args.no_lenses:
        ctx.close()
        return
    # one camera per lens of the any-lens instantiations; Brown-Conrady and Photometrix work in focal-plane units (pixels here)
    lenses = (("FOV", camera.FovLensDistortion([0.9])), ("fisheye", camera.FisheyeLensDistortion([-0.05, 0.01, -0.003, 0.001])),
              ("Brown-Conrady", camera.BrownConradyDistortion([-0.6, -0.2, 0.13e-8, -0.52e-16, 0, 0.55e-9, 0, 0.201])),
              ("adjustable Tsai", camera.AdjustableTsaiLensDistortion([-0.1, 0.02, -0.003, 1e-3, -2e-3, 0.01])),
              ("Photometrix", camera.PhotometrixLensDistortion([0.6, -0.3, -5e-9, 2e-16, -1e-24, 1e-9, -2e-9, 0, 0])))
    for name, lens_k in lenses:
        cam = camera.PinholeModel(ref.CENTER, rot_s, f, f, c, c, distortion=lens_k)
        report("%s src -> pinhole, check on" % name, gpu(transform(cam, dst, True, False)), 8)
        report("%s src -> pinhole, check off" % name, gpu(transform(cam, dst, False, False)), 8)
        report("pinhole -> %s dst, check on" % name, gpu(transform(dst, cam, True, False)), 8)
    ctx.close()


if __name__ == "__main__":
    main()
