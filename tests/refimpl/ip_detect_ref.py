"""ctypes binding of the CPU restatement of the OBALoG detectors and the SGrad descriptors (ip_detect_ref.cc; test
infrastructure)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
IAGD, OBALOG = 0, 1
SGRAD, SGRAD2 = 0, 1
_LIB = None
_FIELDS = (("x", np.float32), ("y", np.float32), ("ix", np.int32), ("iy", np.int32), ("orientation", np.float32), ("scale", np.float32),
           ("interest", np.float32))


def same(got, want, what=""):
    """Exact equality of every word; NaNs by position."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), "%s: NaNs in different places" % what
        got, want = np.where(gn, 0, got), np.where(wn, 0, want)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d words differ, first at %s: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "ip_detect_ref.mk"])
    return os.path.join(HERE, "libip_detect_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, d, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float, ctypes.c_longlong
        _LIB.idr_integral.argtypes = [p, i, i, ll, p]
        _LIB.idr_integral.restype = None
        _LIB.idr_box_at.argtypes = [p, i, i, i, i, p, p]
        _LIB.idr_box_at.restype = f
        _LIB.idr_box_filter.argtypes = [p, i, i, i, p, p, p]
        _LIB.idr_box_filter.restype = None
        _LIB.idr_plane.argtypes = [p, i, i, i, p]
        _LIB.idr_plane.restype = None
        _LIB.idr_harris_outside.restype = ll
        _LIB.idr_atan2f.argtypes = [f, f, i]
        _LIB.idr_atan2f.restype = f
        _LIB.idr_haar.argtypes = [p, i, i, d, d, f, i]
        _LIB.idr_haar.restype = f
        _LIB.idr_orientation.argtypes = [p, i, i, i, i, f, i]
        _LIB.idr_orientation.restype = f
        _LIB.idr_detect.argtypes = [p, ll, i, i, i, i, i, i, d, i, i, i, i, p, p, p, p, p, p, p, p]
        _LIB.idr_describe.argtypes = [p, ll, i, i, p, i, p, p, p, p, i, p]
        _LIB.idr_describe.restype = None
    return _LIB


def integral(image):
    img = np.ascontiguousarray(image, np.float32)
    h, w = img.shape
    out = np.empty((h + 1, w + 1), np.float32)
    lib().idr_integral(img.ctypes.data, w, h, w, out.ctypes.data)
    return out


def _boxes(boxes, weights):
    return np.ascontiguousarray(boxes, np.int32).reshape(-1, 4), np.ascontiguousarray(weights, np.float32).reshape(-1)


def box_at(integ, x, y, boxes, weights):
    """apply_box_filter_at_point at integral(x, y); boxes rows are start x, start y, width, height."""
    b, wt = _boxes(boxes, weights)
    integ = np.ascontiguousarray(integ, np.float32)
    return float(lib().idr_box_at(integ.ctypes.data, integ.shape[1] - 1, int(x), int(y), len(wt), b.ctypes.data, wt.ctypes.data))


def box_filter(integ, boxes, weights):
    b, wt = _boxes(boxes, weights)
    integ = np.ascontiguousarray(integ, np.float32)
    h, w = integ.shape[0] - 1, integ.shape[1] - 1
    out = np.empty((h, w), np.float32)
    lib().idr_box_filter(integ.ctypes.data, w, h, len(wt), b.ctypes.data, wt.ctypes.data, out.ctypes.data)
    return out


def plane(integ, scale):
    integ = np.ascontiguousarray(integ, np.float32)
    h, w = integ.shape[0] - 1, integ.shape[1] - 1
    out = np.empty((h, w), np.float32)
    lib().idr_plane(integ.ctypes.data, w, h, int(scale), out.ctypes.data)
    return out


def harris_outside():
    return int(lib().idr_harris_outside())


def atan2f(y, x, libm=False):
    return np.float32(lib().idr_atan2f(float(np.float32(y)), float(np.float32(x)), int(libm)))


def haar(integ, x, y, size, vertical=False):
    integ = np.ascontiguousarray(integ, np.float32)
    return np.float32(lib().idr_haar(integ.ctypes.data, integ.shape[1], integ.shape[0], float(x), float(y), float(size), int(vertical)))


def orientation(integ, ix, iy, scale, libm=False):
    integ = np.ascontiguousarray(integ, np.float32)
    return np.float32(lib().idr_orientation(integ.ctypes.data, integ.shape[1], integ.shape[0], int(ix), int(iy), float(np.float32(scale)), int(libm)))


def detect(image, detector, scales=8, threshold=0.05, max_points=0, desired=0, libm=False, rect=None):
    """(fields dict, stats [extrema, passed, written]) of process_image on the crop `rect` = (x, y, w, h) (the whole image by default),
    the points shifted by the crop's origin."""
    img = np.ascontiguousarray(image, np.float32)
    x0, y0, w, h = (0, 0, img.shape[1], img.shape[0]) if rect is None else rect
    cap = max(1, ((w + 1) // 2) * ((h + 1) // 2) * max(1, scales - 2))
    out = {name: np.empty(cap, dtype) for name, dtype in _FIELDS}
    stats = (ctypes.c_int * 3)()
    n = lib().idr_detect(img.ctypes.data, img.shape[1], x0, y0, w, h, detector, scales, float(threshold), max_points, desired, int(libm), cap,
                         *[out[name].ctypes.data for name, _ in _FIELDS], stats)
    assert n >= 0
    return {name: v[:n].copy() for name, v in out.items()}, list(stats)


def detect_tiles(image, detector, rects, desired, **kw):
    """The tile loop of detect_interest_points: the tiles' points appended in order."""
    parts = [detect(image, detector, desired=d, rect=r, **kw)[0] for r, d in zip(rects, desired)]
    return {name: np.concatenate([p[name] for p in parts]) for name, _ in _FIELDS}


def describe(image, crop, x, y, scale, orientation_, kind):
    img = np.ascontiguousarray(image, np.float32)
    rect = np.ascontiguousarray(crop, np.int32).reshape(4)
    arrs = [np.ascontiguousarray(v, np.float32).reshape(-1) for v in (x, y, scale, orientation_)]
    n = arrs[0].size
    desc = np.zeros((n, 180 if kind == SGRAD else 128), np.float32)
    lib().idr_describe(img.ctypes.data, img.shape[1], img.shape[1], img.shape[0], rect.ctypes.data, n, *[a.ctypes.data for a in arrs], kind,
                       desc.ctypes.data)
    return desc


def build_view_program():
    """Compiles ip_detect_view.cc (vwlite headers + libvwgpu.so) by ip_detect_view.mk."""
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "ip_detect_view.mk"])
    return os.path.join(HERE, "ip_detect_view")
