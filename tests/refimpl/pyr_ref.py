"""ctypes binding of the CPU restatement of PyramidSubpixelView with SUBPIXEL_LUCAS_KANADE and SUBPIXEL_BAYES_EM (pyr_ref.cc;
test infrastructure), the C++ view program of lk_subpixel / bayes_em_subpixel and the exhaustive exp check program."""
import ctypes
import os
import subprocess

import numpy as np

import affine_ref
from affine_ref import cascade_scene, read_pfm, stretched_scene, tiles_for, top_left_hole_scene, write_pfm  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "pyr_ref.mk"])
    return os.path.join(HERE, "libpyr_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        _LIB.pyr_pyramid_subpixel.argtypes = [p, i, i, p, p, i, i, i, f, i, i, i, i, p, i, p, i, p]
        _LIB.pyr_pyramid_subpixel.restype = i
    return _LIB


def pyramid_subpixel(disparity, left, right, prefilter_mode, prefilter_width, kernel_size, max_pyramid_levels=2,
                     block_size=None, inplace=True, algorithm=2, tiles=None):
    """Returns (out (rows, cols, 3) float32, window passes).  Pixels outside the tiles are zero."""
    d = np.ascontiguousarray(disparity, np.float32)
    l = np.ascontiguousarray(left, np.float32)
    r = np.ascontiguousarray(right, np.float32)
    h, w = l.shape
    t = np.ascontiguousarray(tiles if tiles is not None else tiles_for(w, h, block_size), np.int32).reshape(-1, 4)
    out = np.zeros((h, w, 3), np.float32)
    it = ctypes.c_longlong(0)
    rc = lib().pyr_pyramid_subpixel(d.ctypes.data, w, h, l.ctypes.data, r.ctypes.data, r.shape[1], r.shape[0],
                                    int(prefilter_mode), float(prefilter_width), int(kernel_size[0]), int(kernel_size[1]),
                                    int(max_pyramid_levels), int(algorithm), t.ctypes.data, len(t), out.ctypes.data,
                                    1 if inplace else 0, ctypes.byref(it))
    if rc:
        raise ValueError("pyr_pyramid_subpixel: rc %d" % rc)
    return out, it.value


def unit_scene(w, h, seed=3):
    """stretched_scene with both images scaled by one affine map to [0, 1], as Ames Stereo Pipeline feeds stereo."""
    left, right, d, true = stretched_scene(w, h, seed=seed)
    lo, hi = min(left.min(), right.min()), max(left.max(), right.max())
    return ((left - lo) / (hi - lo)).astype(np.float32), ((right - lo) / (hi - lo)).astype(np.float32), d, true


def unit_top_left_hole_scene(w=96, h=80, kernel=(7, 7), step=11):
    left, right, d, where = top_left_hole_scene(w, h, kernel, step)
    lo, hi = min(left.min(), right.min()), max(left.max(), right.max())
    return ((left - lo) / (hi - lo)).astype(np.float32), ((right - lo) / (hi - lo)).astype(np.float32), d, where


def build_view_program():
    """Compiles pyr_view.cc (vwlite headers + libvwgpu.so) with its own command."""
    exe = os.path.join(HERE, "pyr_view")
    src = os.path.join(HERE, "pyr_view.cc")
    lib = os.path.join(ROOT, "visionworkbench_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "visionworkbench_amd", "vwlite"), "-o", exe, src, "-L" + lib, "-lvwgpu",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def build_exp_check():
    """hipcc-builds em_exp_check.hip (the device header em_exp.h, evaluated on the GPU or on the host)."""
    exe = os.path.join(HERE, "em_exp_check")
    src = os.path.join(HERE, "em_exp_check.hip")
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread",
                           "-I" + os.path.join(ROOT, "visionworkbench_amd", "csrc"), "-o", exe, src])
    return exe


def _unit(left, right):
    lo, hi = min(left.min(), right.min()), max(left.max(), right.max())
    return ((left - lo) / (hi - lo)).astype(np.float32), ((right - lo) / (hi - lo)).astype(np.float32)


def unit_cascade_scene(w, h, seed=5):
    """cascade_scene with both images scaled to [0, 1]."""
    left, right, d, true = cascade_scene(w, h, seed)
    left, right = _unit(left, right)
    return left, right, d, true
