"""ctypes binding of the CPU restatement of vw::stereo::phase_subpixel (phase_ref.cc; test infrastructure), its pieces
(fftshift, pad_fourier_transform, phase_correlation_subpixel) and the C++ view program of phase_subpixel (phase_view.cc)."""
import ctypes
import os
import subprocess

import numpy as np

from affine_ref import tiles_for

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "phase_ref.mk"])
    return os.path.join(HERE, "libphase_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        _LIB.phr_fftshift.argtypes = [p, i, i, i, i, p]
        _LIB.phr_fftshift.restype = None
        _LIB.phr_pad_fourier_transform.argtypes = [p, i, i, i, i, p]
        _LIB.phr_pad_fourier_transform.restype = None
        _LIB.phr_percentile_u8.argtypes = [p, i, p]
        _LIB.phr_percentile_u8.restype = None
        _LIB.phr_phase_correlation.argtypes = [p, p, i, i, i, p]
        _LIB.phr_phase_correlation.restype = None
        _LIB.phr_phase_subpixel.argtypes = [p, i, i, p, p, i, i, i, f, i, i, i, i, p, i, p, i, p]
        _LIB.phr_phase_subpixel.restype = i
    return _LIB


def fftshift(a, reverse=False):
    """vw::fftshift of a (rows, cols) or (rows, cols, ch) float32 array."""
    a = np.ascontiguousarray(a, np.float32)
    ch = 1 if a.ndim == 2 else a.shape[2]
    out = np.empty_like(a)
    lib().phr_fftshift(a.ctypes.data, a.shape[0], a.shape[1], ch, 1 if reverse else 0, out.ctypes.data)
    return out


def pad_fourier_transform(spec, new_width, new_height):
    """vw::pad_fourier_transform of a complex (rows, cols) spectrum; returns complex64 (new_height, new_width)."""
    s = np.ascontiguousarray(np.asarray(spec, np.complex64))
    out = np.empty((new_height, new_width), np.complex64)
    lib().phr_pad_fourier_transform(s.ctypes.data, s.shape[0], s.shape[1], new_width, new_height, out.ctypes.data)
    return out


def percentile_u8(a):
    """get_dft's percentile_scale_convert(a, 0.02, 0.98) as float32 values 0..255, same shape."""
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty_like(a)
    lib().phr_percentile_u8(a.ctypes.data, a.size, out.ctypes.data)
    return out


def phase_correlation(left, right, pad_factor):
    """phase_correlation_subpixel of two equal (rows, cols) patches: the offset (x, y) as two float32."""
    l = np.ascontiguousarray(left, np.float32)
    r = np.ascontiguousarray(right, np.float32)
    assert l.shape == r.shape
    off = np.zeros(2, np.float32)
    lib().phr_phase_correlation(l.ctypes.data, r.ctypes.data, l.shape[0], l.shape[1], int(pad_factor), off.ctypes.data)
    return off


def phase_subpixel(disparity, left, right, prefilter_mode, prefilter_width, kernel_size, max_pyramid_levels=0,
                   phase_subpixel_accuracy=20, block_size=None, tiles=None, threads=16):
    """Returns (out (rows, cols, 3) float32, [pixels refined, pixels invalidated, tiles]).  Pixels outside the tiles are
    zero."""
    d = np.ascontiguousarray(disparity, np.float32)
    l = np.ascontiguousarray(left, np.float32)
    r = np.ascontiguousarray(right, np.float32)
    h, w = l.shape
    t = np.ascontiguousarray(tiles if tiles is not None else tiles_for(w, h, block_size), np.int32).reshape(-1, 4)
    out = np.zeros((h, w, 3), np.float32)
    st = (ctypes.c_longlong * 3)()
    rc = lib().phr_phase_subpixel(d.ctypes.data, w, h, l.ctypes.data, r.ctypes.data, r.shape[1], r.shape[0],
                                  int(prefilter_mode), float(prefilter_width), int(kernel_size[0]), int(kernel_size[1]),
                                  int(max_pyramid_levels), int(phase_subpixel_accuracy), t.ctypes.data, len(t),
                                  out.ctypes.data, int(threads), st)
    if rc:
        raise ValueError("phr_phase_subpixel: rc %d" % rc)
    return out, list(st)


def shifted_texture(w, h, shift, seed=7, seed_disparity=(-2.6, -1.3)):
    """A smooth random texture in [0, 1] and the same texture moved by `shift` = (sx, sy): right(x + sx, y + sy) =
    left(x, y), sampled exactly from a band-limited sum of sinusoids.  The seed disparity map is uniform, valid and
    fractional; the true disparity is `shift`."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    left = np.zeros((h, w))
    right = np.zeros((h, w))
    for _ in range(24):
        fx, fy = rng.uniform(-0.35, 0.35, 2)
        ph, amp = rng.uniform(0, 2 * np.pi), rng.uniform(0.2, 1.0)
        left += amp * np.cos(fx * xx + fy * yy + ph)
        right += amp * np.cos(fx * (xx - shift[0]) + fy * (yy - shift[1]) + ph)
    lo, hi = min(left.min(), right.min()), max(left.max(), right.max())
    left = ((left - lo) / (hi - lo)).astype(np.float32)
    right = ((right - lo) / (hi - lo)).astype(np.float32)
    d = np.zeros((h, w, 3), np.float32)
    d[..., 0], d[..., 1], d[..., 2] = seed_disparity[0], seed_disparity[1], 1.0
    return left, right, d


def build_view_program():
    """Compiles phase_view.cc (vwlite headers + libvwgpu.so) with its own command."""
    exe = os.path.join(HERE, "phase_view")
    src = os.path.join(HERE, "phase_view.cc")
    lib_dir = os.path.join(ROOT, "visionworkbench_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "visionworkbench_amd", "vwlite"), "-o", exe, src, "-L" + lib_dir,
                           "-lvwgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
