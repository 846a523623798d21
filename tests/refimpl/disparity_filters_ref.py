"""ctypes binding of the CPU restatement of the disparity post-filters of Stereo/Algorithms.h
(disparity_filters_ref.cc; test infrastructure), the C++ program (disparity_filters_view.cc) and the scenes of the tests."""
import ctypes
import os
import subprocess

import numpy as np

from affine_ref import tiles_for

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SEMANTICS = {"reference": 0, "snapshot": 1}
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "disparity_filters_ref.mk"])
    return os.path.join(HERE, "libdisparity_filters_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
        _LIB.dfr_median.argtypes = [p, i, i, i, i, p, i, p, i, p]
        _LIB.dfr_neighbor.argtypes = [p, i, i, i, p, i, p, i, p]
        _LIB.dfr_smooth.argtypes = [p, i, i, p, f, i, i, p, i, p, i, p]
        _LIB.dfr_texture.argtypes = [p, i, i, i, d, d, p, i, p, i, p]
    return _LIB


def _boxes(w, h, block_size, tiles):
    return np.ascontiguousarray(tiles if tiles is not None else tiles_for(w, h, block_size), np.int32).reshape(-1, 4)


def _buffer(disparity, dtype):
    """The image the restatement works on: the caller's own array when it already is a C-contiguous array of `dtype`
    (reference semantics then modify it, as the reference modifies disparity_in), else a copy."""
    d = disparity if (isinstance(disparity, np.ndarray) and disparity.dtype == dtype and disparity.flags.c_contiguous
                      and disparity.flags.writeable) else np.array(disparity, dtype, order="C")
    if d.ndim != 3 or d.shape[2] != 3:
        raise ValueError("disparity must be (rows, cols, 3)")
    return d


def _finish(name, rc, out, changed, stats):
    if rc:
        raise ValueError("%s: rc %d" % (name, rc))
    if stats is not None:
        stats[:] = [changed.value]
    return out


def disparity_median_filter(disparity, kernel_size, semantics="reference", block_size=None, tiles=None, stats=None,
                            threads=16):
    d = _buffer(disparity, np.float32)
    h, w = d.shape[:2]
    t = _boxes(w, h, block_size, tiles)
    out = np.empty_like(d)
    ch = ctypes.c_longlong(0)
    rc = lib().dfr_median(d.ctypes.data, w, h, int(kernel_size), SEMANTICS[semantics], t.ctypes.data, len(t),
                          out.ctypes.data, int(threads), ctypes.addressof(ch))
    return _finish("dfr_median", rc, out, ch, stats)


def disparity_neighbor_filter(disparity, semantics="reference", block_size=None, tiles=None, stats=None, threads=16):
    d = _buffer(disparity, np.int32)
    h, w = d.shape[:2]
    t = _boxes(w, h, block_size, tiles)
    out = np.empty_like(d)
    ch = ctypes.c_longlong(0)
    rc = lib().dfr_neighbor(d.ctypes.data, w, h, SEMANTICS[semantics], t.ctypes.data, len(t), out.ctypes.data,
                            int(threads), ctypes.addressof(ch))
    return _finish("dfr_neighbor", rc, out, ch, stats)


def texture_preserving_disparity_filter(disparity, texture, texture_max=0.15, max_kernel_size=11, semantics="reference",
                                        block_size=None, tiles=None, stats=None, threads=16):
    d = _buffer(disparity, np.float32)
    h, w = d.shape[:2]
    tex = np.ascontiguousarray(texture, np.float32)
    if tex.shape != (h, w):
        raise ValueError("dfr_smooth: texture and disparity sizes differ (rc 1)")
    t = _boxes(w, h, block_size, tiles)
    out = np.empty_like(d)
    ch = ctypes.c_longlong(0)
    rc = lib().dfr_smooth(d.ctypes.data, w, h, tex.ctypes.data, float(texture_max), int(max_kernel_size),
                          SEMANTICS[semantics], t.ctypes.data, len(t), out.ctypes.data, int(threads), ctypes.addressof(ch))
    return _finish("dfr_smooth", rc, out, ch, stats)


def texture_measure(image, kernel_size=9, gradient_weight=0.5, stddev_weight=0.5, block_size=None, tiles=None, stats=None,
                    threads=16):
    """(rows, cols) float32 scores, zero outside the boxes; stats receives [largest score]."""
    img = np.ascontiguousarray(image, np.float32)
    h, w = img.shape
    t = _boxes(w, h, block_size, tiles)
    out = np.zeros((h, w), np.float32)
    mx = ctypes.c_float(0)
    rc = lib().dfr_texture(img.ctypes.data, w, h, int(kernel_size), float(gradient_weight), float(stddev_weight),
                           t.ctypes.data, len(t), out.ctypes.data, int(threads), ctypes.addressof(mx))
    if rc:
        raise ValueError("dfr_texture: rc %d" % rc)
    if stats is not None:
        stats[:] = [mx.value]
    return out


def float_scene(w, h, seed=3, invalid=0.08, hole=True):
    """A smooth fractional 2-D disparity with SGM-like speckle, ~8 % invalid pixels whose stored values are random (NaN
    among them) and, with hole=True, a fully invalid rectangle."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.zeros((h, w, 3), np.float32)
    d[..., 0] = -6.0 + 3.0 * np.sin(x / 13.0) * np.cos(y / 17.0) + np.floor(x / 9.0) * 0.25
    d[..., 1] = 0.8 * np.cos(x / 19.0 + y / 11.0)
    speck = rng.uniform(size=(h, w)) < 0.05
    d[speck, 0] += rng.uniform(-20, 20, speck.sum()).astype(np.float32)
    d[speck, 1] += rng.uniform(-5, 5, speck.sum()).astype(np.float32)
    d[..., 2] = 1
    bad = rng.uniform(size=(h, w)) < invalid
    if hole:
        bad[h // 3:h // 3 + max(h // 4, 1), w // 4:w // 4 + max(w // 3, 1)] = True
    d[bad, 2] = 0
    d[bad, 0] = rng.uniform(-50, 50, bad.sum())
    d[bad, 1] = rng.uniform(-50, 50, bad.sum())
    nan = bad & (rng.uniform(size=(h, w)) < 0.2)
    d[nan, 0] = np.nan
    return d


def int_scene(w, h, seed=4):
    """An integer SGM-like map (piecewise constant with steps) with planted isolated outliers, holes, and checkerboard
    stretches where two candidates tie."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = np.zeros((h, w, 3), np.int32)
    d[..., 0] = -8 + x // 11 + y // 23
    d[..., 1] = (x + y) // 37 - 1
    d[..., 2] = 1
    out = rng.uniform(size=(h, w)) < 0.04
    d[out, 0] += rng.randint(-9, 10, out.sum())
    hole = rng.uniform(size=(h, w)) < 0.06
    d[hole, 2] = 0
    d[hole, 0] = rng.randint(-99, 99, hole.sum())
    d[hole, 1] = rng.randint(-99, 99, hole.sum())
    tie = (y >= h // 2) & (y < h // 2 + 6)
    d[tie, 0] = np.where((x + y)[tie] % 2 == 0, 3, 4)
    d[tie, 1] = 0
    d[tie, 2] = 1
    return d


def image_scene(w, h, seed=6, integer=False):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 100 + 40 * np.sin(x / 7.0) * np.cos(y / 9.0) + rng.normal(0, 6, (h, w)) * (x > w / 2)
    return (np.round(v) if integer else v).astype(np.float32)


def build_view_program():
    """Compiles disparity_filters_view.cc (vwlite headers + libvwgpu.so) with its own command."""
    exe = os.path.join(HERE, "disparity_filters_view")
    src = os.path.join(HERE, "disparity_filters_view.cc")
    lib_dir = os.path.join(ROOT, "visionworkbench_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "visionworkbench_amd", "vwlite"), "-o", exe, src, "-L" + lib_dir,
                           "-lvwgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
