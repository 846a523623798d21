#!/usr/bin/env python3
"""Timing of vw::transform on the GPU (csrc/transform.hip): float32 images of --size x --size resident on the device, outputs
allocated once.

Per case: the device time of one vwgpu_transform_image_dev call (HIP events through torch around `--repeat` back-to-back
calls after a warm-up call, divided by the count; the median of `--windows` such windows and their spread), and the ratio
to a device-to-device copy of the OUTPUT's bytes (4 per pixel, 5 with a mask) timed in the same run, which is the yardstick
(no data-sheet number enters).  Cases: a near-identity homography (size x size from size x size) and resample 0.5
(size/2 x size/2 from size x size), for the three interpolations, unmasked and masked, over ZeroEdgeExtension; and for
bilinear a fractional translation beside vwgpu_disparity_warp on the constant disparity that gives the same pixels.

--other PATH names a second build of the library (make -C visionworkbench_amd/csrc tfscalar: the interior bicubic rows as
four dword loads each instead of one 16-byte load).  Both builds then run every case in the same process, window by window in
turn, so that a drift of the machine hits both alike.
usage: python tools/time_transform.py [--size 4096] [--repeat 20] [--windows 7] [--other tools/libexp/libvwgpu_tfscalar.so]"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class OtherLibrary(object):
    """A second build of libvwgpu.so with a context of its own on the current torch stream."""

    def __init__(self, path, stream):
        P, I, PD = ctypes.c_void_p, ctypes.c_int, ctypes.c_ssize_t
        self.lib = ctypes.CDLL(path)
        self.lib.vwgpu_create.argtypes = [ctypes.POINTER(P), I]
        self.lib.vwgpu_set_stream.argtypes = [P, P]
        self.lib.vwgpu_destroy.argtypes = [P]
        self.lib.vwgpu_destroy.restype = None
        self.lib.vwgpu_transform_image_dev.argtypes = [P, P, I, I, PD, P, PD, P, I, P, I, I, I, I, P, PD, P, PD]
        self.h = P()
        assert self.lib.vwgpu_create(ctypes.byref(self.h), 0) == 0
        assert self.lib.vwgpu_set_stream(self.h, stream) == 0

    def close(self):
        self.lib.vwgpu_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--other", default=None, help="a second build of the library to alternate with")
    args = ap.parse_args()
    import torch
    import visionworkbench_amd as vwa
    from visionworkbench_amd import _lib
    from visionworkbench_amd import transform as tf
    if not torch.cuda.is_available():
        sys.exit("time_transform: no GPU; nothing is measured without one")
    n = args.size
    img = torch.rand((n, n), dtype=torch.float32, device="cuda")
    mask = (torch.rand((n, n), device="cuda") >= 0.1).to(torch.uint8)
    out = torch.empty((n, n), dtype=torch.float32, device="cuda")
    omask = torch.empty((n, n), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx = vwa.Context(0)
    ctx.set_stream(stream)
    builds = [("shipped", ctx._lib, ctx._h)]
    other = None
    if args.other:
        other = OtherLibrary(os.path.abspath(args.other), stream)
        builds.append((os.path.basename(args.other), other.lib, other.h))

    def image_call(lib, h, tx, w, hh, interp, masked):
        steps = tf.descriptors_of(tx)
        arr = (_lib.Transform * len(steps))(*steps)
        params = _lib.TransformParams(interp, 0, 0.0, 0, 0, 0.0, 0)

        def call():
            rc = lib.vwgpu_transform_image_dev(h, img.data_ptr(), n, n, 0, mask.data_ptr() if masked else None, 0, arr, len(steps),
                                               ctypes.byref(params), w, hh, 0, 0, out.data_ptr(), 0, omask.data_ptr() if masked else None, 0)
            assert rc == 0, rc
        return call

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.repeat):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.repeat

    def gpu(fns):
        """The functions window by window in turn: [(median, min, max)] in their order."""
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        times = [[] for _ in fns]
        for _ in range(args.windows):
            for k, fn in enumerate(fns):
                times[k].append(window(fn))
        return [(float(np.median(t)), min(t), max(t)) for t in times]

    copies = {}

    def copy_ms(nbytes):
        """A device-to-device copy that reads nbytes and writes nbytes."""
        if nbytes not in copies:
            a, b = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            a.zero_()
            copies[nbytes] = gpu([lambda: b.copy_(a)])[0]
            del a, b
        return copies[nbytes]

    def report(name, t, nbytes):
        ms, lo, hi = t
        cp, clo, chi = copy_ms(nbytes)
        print("%-58s %8.3f ms (%.3f - %.3f);  copy of the output's bytes %7.3f ms (%.3f - %.3f);  copy / call %.2f" % (
            name, ms, lo, hi, cp, clo, chi, cp / ms), flush=True)

    print("%d x %d float32 source, %s, library %s" % (n, n, torch.cuda.get_device_name(0), os.path.relpath(_lib.LIB_PATH, ROOT)))
    k = 1.0 / n
    homography = tf.HomographyTransform([[1.01, 0.02, -1.5], [-0.01, 0.99, 2.0], [0.4 * k * 1e-2, -0.8 * k * 1e-2, 1.0]])
    cases = (("homography", homography, n, n), ("resample 0.5", tf.ResampleTransform(0.5, 0.5), n // 2, n // 2))
    for cname, tx, w, h in cases:
        for iname, interp in (("nearest", 0), ("bilinear", 1), ("bicubic", 2)):
            for masked in (False, True):
                res = gpu([image_call(lib, hd, tx, w, h, interp, masked) for _, lib, hd in builds])
                for (bname, _, _), t in zip(builds, res):
                    report("%s, %s%s [%s]" % (cname, iname, ", masked" if masked else "", bname), t, w * h * (5 if masked else 4))
    # bilinear over ZeroEdgeExtension beside vwgpu_disparity_warp on a constant disparity: the same pixels from another kernel
    dx, dy = 0.375, -1.25
    disp = torch.zeros((n, n, 3), dtype=torch.float32, device="cuda")
    disp[..., 0], disp[..., 1], disp[..., 2] = dx, dy, 1.0

    def warp():
        assert ctx._lib.vwgpu_disparity_warp_dev(ctx._h, img.data_ptr(), n, n, 0, disp.data_ptr(), n, n, 0, out.data_ptr(), 0) == 0
    fns = [image_call(ctx._lib, ctx._h, tf.TranslateTransform(-dx, -dy), n, n, 1, False), warp]
    fns[0]()
    torch.cuda.synchronize()
    first = out.clone()
    warp()
    torch.cuda.synchronize()
    print("translate and disparity_warp give the same pixels: %s" % bool(torch.equal(first, out)))
    res = gpu(fns)
    report("translate (0.375, -1.25), bilinear", res[0], n * n * 4)
    report("vwgpu_disparity_warp, constant disparity", res[1], n * n * 4)
    print("translate / disparity_warp: %.2f" % (res[0][0] / res[1][0]))
    if other:
        other.close()
    ctx.close()


if __name__ == "__main__":
    main()
