#!/usr/bin/env python3
"""Timing of interest-point matching on the GPU (csrc/ip_match.hip): descriptor matrices resident on the device, outputs
allocated once.

Per case: the device time of one vwgpu_ip_match_dev call (HIP events through torch around `--repeat` back-to-back calls after
a warm-up call, divided by the count; the median of `--windows` such windows and their spread).  Cases: L2 SIMPLE with
K = 128 and HAMMING SIMPLE with K = 64, at N1 = N2 = 2 000 and 20 000 (--sizes).  Next to each L2 time: the issue floor of the
specified arithmetic, N1 * N2 * K * 3 vector operations (subtract, multiply, add; no FMA by specification) over
256 CUs x 64 lanes per clock at --clock-mhz (the device's maximum engine clock by default: the runtime reports no clock through
torch, and a loaded chip runs below it, so the fraction is the pessimistic one), and the fraction of it that was reached.  With --cpu the
single-thread time of the CPU restatement (tests/refimpl/ip_match_ref.cc) at the smallest size on this host, whose result
the GPU's must equal word for word.

--other PATH names a second build of the library (make -C visionworkbench_amd/csrc ipvariant IPM_FLAGS=-DIPM_CHUNK=512 IPM_NAME=chunk512, say).
Both builds then run every case in the same process, window by window in turn, so that a drift of the machine hits both alike.
usage: python tools/time_ip_match.py [--sizes 2000,20000] [--repeat 5] [--windows 7] [--clock-mhz 2400] [--cpu] [--other tools/libexp/libvwgpu_ip_chunk512.so]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))


class OtherLibrary(object):
    """A second build of libvwgpu.so with a context of its own on the current torch stream."""

    def __init__(self, path, stream):
        P, I, PD = ctypes.c_void_p, ctypes.c_int, ctypes.c_ssize_t
        self.lib = ctypes.CDLL(path)
        self.lib.vwgpu_create.argtypes = [ctypes.POINTER(P), I]
        self.lib.vwgpu_set_stream.argtypes = [P, P]
        self.lib.vwgpu_destroy.argtypes = [P]
        self.lib.vwgpu_destroy.restype = None
        self.lib.vwgpu_ip_match_chunk.argtypes = [I]
        self.lib.vwgpu_ip_match_dev.argtypes = [P, P, I, PD, P, I, PD, I, P, P, P, P, P, P, P, P]
        self.h = P()
        assert self.lib.vwgpu_create(ctypes.byref(self.h), 0) == 0
        assert self.lib.vwgpu_set_stream(self.h, stream) == 0

    def close(self):
        self.lib.vwgpu_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,20000")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="the clock of the issue floor (MI355X: 2400 MHz at most)")
    ap.add_argument("--cpu", action="store_true", help="also time the CPU restatement at the smallest size and compare the results")
    ap.add_argument("--other", default=None, help="a second build of the library to alternate with")
    args = ap.parse_args()
    import torch
    import visionworkbench_amd as vwa
    from visionworkbench_amd import _lib
    if not torch.cuda.is_available():
        sys.exit("time_ip_match: no GPU; nothing is measured without one")
    sizes = [int(s) for s in args.sizes.split(",")]
    stream = torch.cuda.current_stream().cuda_stream
    ctx = vwa.Context(0)
    ctx.set_stream(stream)
    builds = [("shipped", ctx._lib, ctx._h)]
    other = None
    if args.other:
        other = OtherLibrary(os.path.abspath(args.other), stream)
        builds.append((os.path.basename(args.other), other.lib, other.h))
    props = torch.cuda.get_device_properties(0)
    clock_hz = args.clock_mhz * 1e6
    print("%s, %d CUs, issue floor at %.0f MHz, library %s" % (props.name, props.multi_processor_count, clock_hz / 1e6,
                                                         os.path.relpath(_lib.LIB_PATH, ROOT)))
    for name, lib, _ in builds:
        print("  %s: %d candidates per workgroup at N2 = %d" % (name, lib.vwgpu_ip_match_chunk(sizes[-1]), sizes[-1]))

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

    rng = np.random.RandomState(7)
    for metric, k in ((0, 128), (1, 64)):
        for n in sizes:
            if metric == 0:
                h1, h2 = rng.random_sample((n, k)).astype(np.float32), rng.random_sample((n, k)).astype(np.float32)
            else:
                h1, h2 = rng.randint(0, 256, (n, k)).astype(np.uint8), rng.randint(0, 256, (n, k)).astype(np.uint8)
            hp1, hp2 = rng.randint(0, 2, n).astype(np.uint8), rng.randint(0, 2, n).astype(np.uint8)
            d1, d2, p1, p2 = (torch.from_numpy(a).cuda() for a in (h1, h2, hp1, hp2))
            index = torch.empty(n, dtype=torch.int32, device="cuda")
            dist = torch.empty((n, 2), dtype=torch.float32, device="cuda")
            P = _lib.IpMatchParams(metric, 0, 0.8, 0, 0, (ctypes.c_double * 4)(0, 0, 0, 0))

            def call_of(lib, h):
                def call():
                    rc = lib.vwgpu_ip_match_dev(h, d1.data_ptr(), n, k, d2.data_ptr(), n, k, k, p1.data_ptr(), p2.data_ptr(), None, None,
                                                ctypes.byref(P), index.data_ptr(), dist.data_ptr(), None)
                    assert rc == 0, rc
                return call
            res = gpu([call_of(lib, h) for _, lib, h in builds])
            what = "%s SIMPLE, K = %d, N1 = N2 = %d" % ("L2" if metric == 0 else "HAMMING", k, n)
            for (bname, _, _), (ms, lo, hi) in zip(builds, res):
                line = "%-44s [%s] %9.3f ms (%.3f - %.3f)" % (what, bname, ms, lo, hi)
                if metric == 0:
                    floor_ms = float(n) * n * k * 3 / (256 * 64 * clock_hz) * 1e3
                    line += ";  issue floor %.3f ms, reached %.3f of it" % (floor_ms, floor_ms / ms)
                print(line, flush=True)
            if args.cpu and n == min(sizes):
                import ip_match_ref as ref
                ref.lib()
                t0 = time.perf_counter()
                want = ref.match(h1, h2, 0.8, metric=metric, pol1=hp1, pol2=hp2)
                cpu_ms = (time.perf_counter() - t0) * 1e3
                builds[0][1].vwgpu_ip_match_dev(builds[0][2], d1.data_ptr(), n, k, d2.data_ptr(), n, k, k, p1.data_ptr(), p2.data_ptr(), None, None,
                                                ctypes.byref(P), index.data_ptr(), dist.data_ptr(), None)
                torch.cuda.synchronize()
                equal = np.array_equal(index.cpu().numpy(), want[0]) and np.array_equal(dist.cpu().numpy(), want[1])
                print("%-44s CPU restatement, one thread: %.1f ms; the GPU's index and distances equal it: %s" % (what, cpu_ms, equal), flush=True)
    if other:
        other.close()
    ctx.close()


if __name__ == "__main__":
    main()
