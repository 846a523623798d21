"""ctypes binding of the CPU restatement of the local outlier filters of Stereo/DisparityMap.h and std_dev_image
(outlier_filters_ref.cc; test infrastructure), the C++ program (outlier_filters_view.cc) and the scenes of the tests."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
METHODS = {"mean": 0, "stddev": 1, "plane": 2}
SEMANTICS = {"reference": 0, "skip": 1}
EDGES = {"constant": 0, "zero": 1}
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "outlier_filters_ref.mk"])
    return os.path.join(HERE, "liboutlier_filters_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        _LIB.ofr_rm_outliers.argtypes = [i, i, p, i, i, i, i, d, d, i, i, p, i, p]
        _LIB.ofr_std_dev_image.argtypes = [p, i, i, i, i, i, p, i]
    return _LIB


def rm_outliers(method, disparity, half_h, half_v, p0, p1=0.0, cleanup=False, semantics="reference", stats=None, threads=16):
    """method 'mean' (p0 = max_mean_diff), 'stddev' or 'plane' (p0 = pixel_threshold, p1 = rejection_threshold) on a
    (rows, cols, 3) int32 or float32 image; stats receives [rejected by the filter, rejected by the clean-up pass]."""
    if disparity.dtype not in (np.int32, np.float32):
        raise ValueError("disparity must be int32 or float32")
    d = np.ascontiguousarray(disparity)
    if d.ndim != 3 or d.shape[2] != 3:
        raise ValueError("disparity must be (rows, cols, 3)")
    h, w = d.shape[:2]
    out = np.empty_like(d)
    st = (ctypes.c_longlong * 2)()
    rc = lib().ofr_rm_outliers(METHODS[method], 0 if d.dtype == np.int32 else 1, d.ctypes.data, w, h, int(half_h), int(half_v),
                               float(p0), float(p1), int(bool(cleanup)), SEMANTICS[semantics], out.ctypes.data, int(threads),
                               ctypes.addressof(st))
    if rc:
        raise ValueError("ofr_rm_outliers: rc %d" % rc)
    if stats is not None:
        stats[:] = list(st)
    return out


def std_dev_image(image, kernel_width, kernel_height, edge="zero", threads=16):
    img = np.ascontiguousarray(image, np.float32)
    h, w = img.shape
    out = np.empty_like(img)
    rc = lib().ofr_std_dev_image(img.ctypes.data, w, h, int(kernel_width), int(kernel_height), EDGES[edge], out.ctypes.data,
                                 int(threads))
    if rc:
        raise ValueError("ofr_std_dev_image: rc %d" % rc)
    return out


def float_scene(w, h, seed=3, noise=0.15, outliers=0.03, invalid=0.06, hole=True):
    """A smooth ramp plus noise with planted outliers, ~6 % invalid pixels whose stored values are random and, with
    hole=True, a fully invalid rectangle."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.zeros((h, w, 3), np.float32)
    d[..., 0] = -6.0 + 0.11 * x - 0.07 * y + 1.5 * np.sin(x / 13.0) * np.cos(y / 17.0) + rng.normal(0, noise, (h, w))
    d[..., 1] = 0.8 * np.cos(x / 19.0 + y / 11.0) + 0.02 * y + rng.normal(0, noise, (h, w))
    out = rng.uniform(size=(h, w)) < outliers
    d[out, 0] += rng.uniform(-25, 25, out.sum()).astype(np.float32)
    d[out, 1] += rng.uniform(-8, 8, out.sum()).astype(np.float32)
    d[..., 2] = 1
    bad = rng.uniform(size=(h, w)) < invalid
    if hole:
        bad[h // 3:h // 3 + max(h // 4, 1), w // 4:w // 4 + max(w // 3, 1)] = True
    d[bad, 2] = 0
    d[bad, 0] = rng.uniform(-50, 50, bad.sum())
    d[bad, 1] = rng.uniform(-50, 50, bad.sum())
    return d


def int_scene(w, h, seed=4, huge=1000000):
    """Integer disparities (piecewise constant with steps) with planted outliers of magnitude `huge` and holes."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = np.zeros((h, w, 3), np.int32)
    d[..., 0] = -8 + x // 7 + y // 13 + rng.randint(-1, 2, (h, w))
    d[..., 1] = (x + y) // 17 - 1
    d[..., 2] = 1
    out = rng.uniform(size=(h, w)) < 0.03
    d[out, 0] = rng.choice([-huge, huge], out.sum())
    out = rng.uniform(size=(h, w)) < 0.01
    d[out, 1] = huge
    hole = rng.uniform(size=(h, w)) < 0.06
    d[hole, 2] = 0
    d[hole, 0] = rng.randint(-99, 99, hole.sum())
    d[hole, 1] = rng.randint(-99, 99, hole.sum())
    return d


def sparse_scene(w, h, dtype, seed=5):
    """An all-invalid block that holds single valid pixels, inside a valid surround."""
    d = float_scene(w, h, seed, hole=False) if dtype == np.float32 else int_scene(w, h, seed, huge=500)
    d[h // 5:h - h // 5, w // 5:w - w // 5, 2] = 0
    rng = np.random.RandomState(seed + 1)
    for _ in range(max(3, w * h // 150)):
        d[rng.randint(h // 5, h - h // 5), rng.randint(w // 5, w - w // 5), 2] = 1
    return d


def image_scene(w, h, seed=6):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return (100 + 40 * np.sin(x / 7.0) * np.cos(y / 9.0) + rng.normal(0, 6, (h, w)) * (x > w / 2)).astype(np.float32)


def build_view_program():
    """Compiles outlier_filters_view.cc (vwlite headers + libvwgpu.so) with its own command."""
    exe = os.path.join(HERE, "outlier_filters_view")
    src = os.path.join(HERE, "outlier_filters_view.cc")
    lib_dir = os.path.join(ROOT, "visionworkbench_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "visionworkbench_amd", "vwlite"), "-o", exe, src, "-L" + lib_dir,
                           "-lvwgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
