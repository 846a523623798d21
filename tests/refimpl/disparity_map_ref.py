"""ctypes binding of the CPU restatement of the operators of Stereo/DisparityMap.h on a finished disparity map
(disparity_map_ref.cc; test infrastructure), the C++ program (disparity_map_view.cc) and the scenes of the tests."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SEMANTICS = {"reference": 0, "fixed": 1}
MODES = {"functor": 0, "subregion": 1, "subregion_round": 2}
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "disparity_map_ref.mk"])
    return os.path.join(HERE, "libdisparity_map_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        _LIB.dmr_get_disparity_range.argtypes = [i, p, i, i, p]
        _LIB.dmr_disparity_range_mask.argtypes = [i, p, i, i, i, i, p, p, i, p, p]
        _LIB.dmr_transform_disparities.argtypes = [i, p, i, i, i, i, p, i, p]
        _LIB.dmr_disparity_subsample.argtypes = [i, p, i, i, p]
        _LIB.dmr_disparity_upsample.argtypes = [i, p, i, i, p]
        _LIB.dmr_missing_pixel_image.argtypes = [i, p, i, i, p]
        _LIB.dmr_intersect_mask_and_data.argtypes = [i, p, p, i, i, p]
        _LIB.dmr_disparity_transform_reverse.argtypes = [p, i, i, d, d, p]
        _LIB.dmr_disparity_transform_reverse.restype = None
        _LIB.dmr_disparity_warp.argtypes = [p, i, i, p, i, i, p]
    return _LIB


def _disp(disparity):
    if disparity.dtype not in (np.int32, np.float32):
        raise ValueError("disparity must be int32 or float32")
    d = np.ascontiguousarray(disparity)
    if d.ndim != 3 or d.shape[2] != 3:
        raise ValueError("disparity must be (rows, cols, 3)")
    return d, (0 if d.dtype == np.int32 else 1), d.shape[1], d.shape[0]


def _ok(rc, what):
    if rc:
        raise ValueError("%s: rc %d" % (what, rc))


def get_disparity_range(disparity):
    """float32[4] {min.x, min.y, max.x, max.y} over the valid pixels, zeros without any."""
    d, t, w, h = _disp(disparity)
    out = np.zeros(4, np.float32)
    _ok(lib().dmr_get_disparity_range(t, d.ctypes.data, w, h, out.ctypes.data), "dmr_get_disparity_range")
    return out


def disparity_range_mask(disparity, mn, mx, semantics="reference", x0=0, y0=0, stats=None):
    d, t, w, h = _disp(disparity)
    out = np.empty_like(d)
    lo, hi = np.asarray(mn, np.float64).copy(), np.asarray(mx, np.float64).copy()
    n = ctypes.c_longlong(0)
    _ok(lib().dmr_disparity_range_mask(t, d.ctypes.data, w, h, int(x0), int(y0), lo.ctypes.data, hi.ctypes.data,
                                       SEMANTICS[semantics], out.ctypes.data, ctypes.addressof(n)), "dmr_disparity_range_mask")
    if stats is not None:
        stats[:] = [n.value]
    return out


def transform_disparities(disparity, matrix, mode="functor", x0=0, y0=0):
    """matrix: the APPLIED 3 x 3 matrix (for the functor overload with HomographyTransform(H): inverse(H))."""
    d, t, w, h = _disp(disparity)
    out = np.empty_like(d)
    m = np.ascontiguousarray(matrix, np.float64).reshape(9)
    _ok(lib().dmr_transform_disparities(t, d.ctypes.data, w, h, int(x0), int(y0), m.ctypes.data, MODES[mode], out.ctypes.data),
        "dmr_transform_disparities")
    return out


def disparity_subsample(disparity):
    d, t, w, h = _disp(disparity)
    out = np.empty((1 + (h - 1) // 2, 1 + (w - 1) // 2, 3), d.dtype)
    _ok(lib().dmr_disparity_subsample(t, d.ctypes.data, w, h, out.ctypes.data), "dmr_disparity_subsample")
    return out


def disparity_upsample(disparity):
    d, t, w, h = _disp(disparity)
    out = np.empty((2 * h, 2 * w, 3), d.dtype)
    _ok(lib().dmr_disparity_upsample(t, d.ctypes.data, w, h, out.ctypes.data), "dmr_disparity_upsample")
    return out


def missing_pixel_image(disparity):
    d, t, w, h = _disp(disparity)
    out = np.empty((h, w, 3), np.uint8)
    _ok(lib().dmr_missing_pixel_image(t, d.ctypes.data, w, h, out.ctypes.data), "dmr_missing_pixel_image")
    return out


def intersect_mask_and_data(data, mask):
    d, t, w, h = _disp(data)
    m, tm, wm, hm = _disp(mask)
    if (t, w, h) != (tm, wm, hm):
        raise ValueError("data and mask differ in type or size")
    out = np.empty_like(d)
    _ok(lib().dmr_intersect_mask_and_data(t, d.ctypes.data, m.ctypes.data, w, h, out.ctypes.data), "dmr_intersect_mask_and_data")
    return out


def disparity_transform_reverse(disparity, px, py):
    """DisparityTransform(disparity).reverse((px, py))."""
    d, t, w, h = _disp(disparity)
    if t != 1:
        raise ValueError("DisparityTransform takes a float32 disparity")
    out = np.zeros(2, np.float64)
    lib().dmr_disparity_transform_reverse(d.ctypes.data, w, h, float(px), float(py), out.ctypes.data)
    return out


def disparity_transform_image(right, disparity):
    """transform(right, DisparityTransform(disparity))."""
    r = np.ascontiguousarray(right, np.float32)
    d, t, w, h = _disp(disparity)
    if t != 1 or r.ndim != 2:
        raise ValueError("a (rows, cols) float32 image and a float32 disparity")
    out = np.empty_like(r)
    _ok(lib().dmr_disparity_warp(r.ctypes.data, r.shape[1], r.shape[0], d.ctypes.data, w, h, out.ctypes.data), "dmr_disparity_warp")
    return out


def inverse3(H):
    """The plain 3 x 3 adjugate inverse the C++ and Python layers use for HomographyTransform(H)."""
    from visionworkbench_amd import stereo
    return stereo.HomographyTransform(H).inverse_matrix


def float_scene(w, h, seed=3, invalid=0.1, spread=6.0):
    """A smooth float disparity with noise; ~10 % invalid pixels whose stored values are random."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.zeros((h, w, 3), np.float32)
    d[..., 0] = -spread + 0.13 * x - 0.05 * y + 1.5 * np.sin(x / 5.0) * np.cos(y / 7.0) + rng.normal(0, 0.4, (h, w))
    d[..., 1] = 2.0 * np.cos(x / 9.0 + y / 4.0) + 0.03 * y + rng.normal(0, 0.4, (h, w))
    d[..., 2] = 1
    bad = rng.uniform(size=(h, w)) < invalid
    d[bad, 2] = 0
    d[bad, 0] = rng.uniform(-50, 50, bad.sum())
    d[bad, 1] = rng.uniform(-50, 50, bad.sum())
    return d


def int_scene(w, h, seed=4, invalid=0.1):
    """Integer disparities of both signs; ~10 % invalid pixels whose stored values are random."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    d = np.zeros((h, w, 3), np.int32)
    d[..., 0] = -9 + x // 5 - y // 11 + rng.randint(-3, 4, (h, w))
    d[..., 1] = (x + y) // 13 - 3 + rng.randint(-2, 3, (h, w))
    d[..., 2] = 1
    bad = rng.uniform(size=(h, w)) < invalid
    d[bad, 2] = 0
    d[bad, 0] = rng.randint(-99, 99, bad.sum())
    d[bad, 1] = rng.randint(-99, 99, bad.sum())
    return d


def scene(w, h, dtype, seed=3):
    return float_scene(w, h, seed) if dtype == np.float32 else int_scene(w, h, seed)


def image_scene(w, h, seed=6):
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return (100 + 40 * np.sin(x / 7.0) * np.cos(y / 9.0) + rng.normal(0, 6, (h, w))).astype(np.float32)


def warp_scene(dw, dh, seed=7):
    """A float disparity for the warp: fractional offsets, integer offsets (also in one coordinate only), offsets that
    lead outside any small image, and invalid pixels."""
    rng = np.random.RandomState(seed)
    d = np.zeros((dh, dw, 3), np.float32)
    d[..., 0] = rng.uniform(-4, 4, (dh, dw))
    d[..., 1] = rng.uniform(-3, 3, (dh, dw))
    kind = rng.randint(0, 8, (dh, dw))
    d[kind == 0, 0] = np.round(d[kind == 0, 0])
    d[kind == 0, 1] = np.round(d[kind == 0, 1])
    d[kind == 1, 0] = np.round(d[kind == 1, 0])
    d[kind == 2, 1] = np.round(d[kind == 2, 1])
    d[kind == 3, 0] += rng.choice([-3000.0, 3000.0], (kind == 3).sum())
    d[kind == 4, 1] += rng.choice([-3000.0, 3000.0], (kind == 4).sum())
    d[..., 2] = 1
    d[kind == 5, 2] = 0
    return d


AFFINE = np.array([[1.00679, -0.0125401, 116.812], [0.00788373, 0.996033, -1.93039], [0, 0, 1]], np.float64)   # TestDisparity.cxx Transform2
PROJECTIVE = np.array([[0.98, 0.03, -4.5], [-0.02, 1.01, 2.25], [1.5e-4, -0.9e-4, 1.0]], np.float64)
TRANSLATION = np.array([[1, 0, 45], [0, 1, -30], [0, 0, 1]], np.float64)   # TestDisparity.cxx Transform1


def build_view_program():
    """Compiles disparity_map_view.cc (vwlite headers + libvwgpu.so) with its own command."""
    exe = os.path.join(HERE, "disparity_map_view")
    src = os.path.join(HERE, "disparity_map_view.cc")
    lib_dir = os.path.join(ROOT, "visionworkbench_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "visionworkbench_amd", "vwlite"), "-o", exe, src, "-L" + lib_dir,
                           "-lvwgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
