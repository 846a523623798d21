"""ctypes binding of the CPU restatement of vw::stereo::corr_eval (corr_eval_ref.cc; test infrastructure), the C++ view
program (corr_eval_view.cc) and the scenes of the corr_eval tests."""
import ctypes
import os
import subprocess

import numpy as np

from affine_ref import tiles_for

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
METRICS = {"ncc": 0, "stddev": 1, "parabola_curvature": 2, "cramer_rao": 3}
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "corr_eval_ref.mk"])
    return os.path.join(HERE, "libcorr_eval_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        _LIB.cer_corr_eval.argtypes = [p, i, i, p, p, p, p, i, i, i, i, i, i, i, i, f, p, i, p, i, p]
        _LIB.cer_corr_eval.restype = i
    return _LIB


def corr_eval(left, right, disparity, kernel_size, metric, sample_rate=1, round_to_int=False, prefilter_mode=0,
              prefilter_kernel_width=0.0, left_valid=None, right_valid=None, block_size=None, tiles=None, threads=16):
    """Returns (out (rows, cols, 2) float32 {value, valid}, [evaluated, valid, tiles, degenerate tiles]).  Pixels outside
    the tiles are zero.  Raises ValueError("... rc N") on the restatement's error codes (1 argument, 2 non-finite
    disparity, 3 outside int32, 4 a patch outside its left crop)."""
    d = np.ascontiguousarray(disparity, np.float32)
    l = np.ascontiguousarray(left, np.float32)
    r = np.ascontiguousarray(right, np.float32)
    if d.ndim != 3 or d.shape[2] != 3 or d.shape[:2] != l.shape:
        raise ValueError("cer_corr_eval: left image and disparity must have the same dimensions (rc 1)")
    h, w = l.shape
    lv = None if left_valid is None else np.ascontiguousarray(np.asarray(left_valid) != 0, np.uint8)
    rv = None if right_valid is None else np.ascontiguousarray(np.asarray(right_valid) != 0, np.uint8)
    t = np.ascontiguousarray(tiles if tiles is not None else tiles_for(w, h, block_size), np.int32).reshape(-1, 4)
    out = np.zeros((h, w, 2), np.float32)
    st = (ctypes.c_longlong * 4)()
    rc = lib().cer_corr_eval(d.ctypes.data, w, h, l.ctypes.data, None if lv is None else lv.ctypes.data, r.ctypes.data,
                             None if rv is None else rv.ctypes.data, r.shape[1], r.shape[0], int(kernel_size[0]),
                             int(kernel_size[1]), METRICS.get(metric, -1), int(sample_rate), 1 if round_to_int else 0,
                             int(prefilter_mode), float(prefilter_kernel_width), t.ctypes.data, len(t), out.ctypes.data,
                             int(threads), st)
    if rc:
        raise ValueError("cer_corr_eval: rc %d" % rc)
    return out, list(st)


def scene(w, h, rw=None, rh=None, shift=(-3.3, 0.6), seed=5, masks=False):
    """A smooth positive texture pair (right(x + sx, y + sy) ~ left(x, y)) and a smooth fractional 2-D disparity near
    `shift` with ~8 % invalid pixels (their stored values random); masks=True adds ~5 % masked pixels to both images."""
    rw, rh = rw or w, rh or h
    rng = np.random.RandomState(seed)

    def tex(x, y):
        v = np.zeros_like(x)
        for _ in range(10):
            fx, fy, ph = rng.uniform(0.05, 0.4), rng.uniform(0.05, 0.4), rng.uniform(0, 6.3)
            v += np.sin(fx * x + fy * y + ph) * rng.uniform(0.3, 1.0)
        return v

    state = rng.get_state()
    yl, xl = np.mgrid[0:h, 0:w].astype(np.float64)
    left = (tex(xl, yl) * 20 + 100).astype(np.float32)
    rng.set_state(state)
    yr, xr = np.mgrid[0:rh, 0:rw].astype(np.float64)
    right = (tex(xr - shift[0], yr - shift[1]) * 20 + 100 + rng.normal(0, 0.5, (rh, rw))).astype(np.float32)
    d = np.zeros((h, w, 3), np.float32)
    d[..., 0] = shift[0] + 0.7 * np.sin(xl / 17.0) * np.cos(yl / 23.0)
    d[..., 1] = shift[1] + 0.5 * np.cos(xl / 19.0 + yl / 29.0)
    d[..., 2] = 1
    bad = rng.uniform(size=(h, w)) < 0.08
    d[bad, 2] = 0
    d[bad, 0] = rng.uniform(-50, 50, bad.sum())
    d[bad, 1] = rng.uniform(-50, 50, bad.sum())
    if not masks:
        return left, right, d, None, None
    lv = (rng.uniform(size=(h, w)) > 0.05).astype(np.uint8)
    rv = (rng.uniform(size=(rh, rw)) > 0.05).astype(np.uint8)
    return left, right, d, lv, rv


def build_view_program():
    """Compiles corr_eval_view.cc (vwlite headers + libvwgpu.so) with its own command."""
    exe = os.path.join(HERE, "corr_eval_view")
    src = os.path.join(HERE, "corr_eval_view.cc")
    lib_dir = os.path.join(ROOT, "visionworkbench_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "visionworkbench_amd", "vwlite"), "-o", exe, src, "-L" + lib_dir,
                           "-lvwgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
