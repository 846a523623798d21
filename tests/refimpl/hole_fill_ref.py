"""ctypes binding of the CPU restatement of grassfire, the blob index, ErodeView, InpaintView, fill_holes_grass and
fill_nodata_with_avg (hole_fill_ref.cc; test infrastructure), the C++ program (hole_fill_view.cc) and the scenes of the
tests."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EDGES = {"reference": 0, "fixed": 1}
_SRC = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1, np.dtype(np.float32): 2}
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "hole_fill_ref.mk"])
    return os.path.join(HERE, "libhole_fill_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint
        _LIB.hfr_grassfire.argtypes = [i, p, i, i, i, p]
        _LIB.hfr_blob_index.argtypes = [i, p, i, i, i, i, i, p, p, i, ctypes.POINTER(ctypes.c_int)]
        _LIB.hfr_blob_sizes.argtypes = [i, p, i, i, u, p]
        _LIB.hfr_erode_blobs.argtypes = [i, p, i, i, i, p]
        _LIB.hfr_inpaint.argtypes = [i, p, i, i, p, p, i, i, p, i, p]
        _LIB.hfr_fill_holes_grass.argtypes = [i, p, i, i, i, i, p]
        _LIB.hfr_fill_nodata_with_avg.argtypes = [p, i, i, i, p]
    return _LIB


def kind_of(img):
    """The pixel kind of an array: (rows, cols) uint8, (rows, cols, 2) float32, (rows, cols, 3) int32 / float32."""
    if img.ndim == 2 and img.dtype == np.uint8:
        return 0
    if img.ndim == 3 and img.shape[2] == 2 and img.dtype == np.float32:
        return 1
    if img.ndim == 3 and img.shape[2] == 3 and img.dtype in (np.int32, np.float32):
        return 2 if img.dtype == np.int32 else 3
    raise ValueError("not a masked image: %s %s" % (img.shape, img.dtype))


def _ok(rc, what):
    if rc:
        raise ValueError("%s: rc %d" % (what, rc))


def grassfire(src, ignore_borders=False):
    s = np.ascontiguousarray(src)
    out = np.empty(s.shape, np.int32)
    _ok(lib().hfr_grassfire(_SRC[s.dtype], s.ctypes.data, s.shape[1], s.shape[0], int(ignore_borders), out.ctypes.data), "hfr_grassfire")
    return out


def blob_index(img, invert=False, max_area=0, wipe_size=0, capacity=None):
    """(labels int32 (rows, cols), table int32 (count, 5) {min.x, min.y, max.x, max.y, size}); capacity: rows of the
    table offered, a too small one gives (-6, count)."""
    a = np.ascontiguousarray(img)
    h, w = a.shape[:2]
    labels = np.empty((h, w), np.int32)
    n = ctypes.c_int(0)
    cap = ((w + 1) // 2) * ((h + 1) // 2) if capacity is None else int(capacity)
    table = np.zeros((max(cap, 1), 5), np.int32)
    rc = lib().hfr_blob_index(kind_of(a), a.ctypes.data, w, h, int(invert), int(max_area), int(wipe_size), labels.ctypes.data,
                              table.ctypes.data, cap, ctypes.byref(n))
    if rc == -6:
        return -6, n.value
    _ok(rc, "hfr_blob_index")
    return labels, table[:n.value].copy()


def blob_sizes(img, limit=0xffffffff):
    a = np.ascontiguousarray(img)
    out = np.empty(a.shape[:2], np.uint32)
    _ok(lib().hfr_blob_sizes(kind_of(a), a.ctypes.data, a.shape[1], a.shape[0], int(limit), out.ctypes.data), "hfr_blob_sizes")
    return out


def erode_blobs(img, max_area):
    a = np.ascontiguousarray(img)
    out = np.empty_like(a)
    _ok(lib().hfr_erode_blobs(kind_of(a), a.ctypes.data, a.shape[1], a.shape[0], int(max_area), out.ctypes.data), "hfr_erode_blobs")
    return out


def inpaint(img, labels, table, use_grassfire=True, default=None, semantics="reference"):
    a = np.ascontiguousarray(img)
    lab, tab = np.ascontiguousarray(labels, np.int32), np.ascontiguousarray(table, np.int32).reshape(-1, 5)
    dflt = np.zeros(3, np.float32) if default is None else np.ascontiguousarray(default, np.float32)
    out = np.empty_like(a)
    _ok(lib().hfr_inpaint(kind_of(a), a.ctypes.data, a.shape[1], a.shape[0], lab.ctypes.data, tab.ctypes.data, tab.shape[0],
                          int(use_grassfire), dflt.ctypes.data, EDGES[semantics], out.ctypes.data), "hfr_inpaint")
    return out


def fill_holes_grass(img, hole_fill_len, semantics="reference"):
    a = np.ascontiguousarray(img)
    out = np.empty_like(a)
    _ok(lib().hfr_fill_holes_grass(kind_of(a), a.ctypes.data, a.shape[1], a.shape[0], int(hole_fill_len), EDGES[semantics],
                                   out.ctypes.data), "hfr_fill_holes_grass")
    return out


def fill_nodata_with_avg(img, kernel_size):
    a = np.ascontiguousarray(img, np.float32)
    out = np.empty_like(a)
    _ok(lib().hfr_fill_nodata_with_avg(a.ctypes.data, a.shape[1], a.shape[0], int(kernel_size), out.ctypes.data), "hfr_fill_nodata_with_avg")
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------

def float_map(w, h, kind, seed=5):
    """A smooth all-valid map of a float kind (1: {value, valid}, 3: {dx, dy, valid}) with noise."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    c = 1 if kind == 1 else 2
    d = np.zeros((h, w, c + 1), np.float32)
    d[..., 0] = -6 + 0.13 * x - 0.05 * y + 1.5 * np.sin(x / 5.0) * np.cos(y / 7.0) + rng.normal(0, 0.4, (h, w))
    if c == 2:
        d[..., 1] = 2.0 * np.cos(x / 9.0 + y / 4.0) + 0.03 * y + rng.normal(0, 0.4, (h, w))
    d[..., c] = 1
    return d


def as_kind(valid, kind, seed=9):
    """An image of the given kind with the given validity (bool (rows, cols)) and random stored values everywhere."""
    rng = np.random.RandomState(seed)
    h, w = valid.shape
    if kind == 0:
        return np.where(valid, rng.randint(1, 256, (h, w)), 0).astype(np.uint8)
    if kind == 1:
        d = rng.uniform(-50, 50, (h, w, 2)).astype(np.float32)
        d[..., 1] = valid
        return d
    if kind == 2:
        d = rng.randint(-99, 99, (h, w, 3)).astype(np.int32)
        d[..., 2] = np.where(valid, 0x7fffffff, 0)
        return d
    d = rng.uniform(-50, 50, (h, w, 3)).astype(np.float32)
    d[..., 2] = valid
    return d


def punch(img, hole, stored=None, seed=11):
    """Invalidates the pixels of the bool mask `hole` in a float-kind image; stored: None = random in +-1e3, else the
    value the holes keep.  Returns a new image."""
    rng = np.random.RandomState(seed)
    out = img.copy()
    c = img.shape[2] - 1
    n = int(hole.sum())
    for k in range(c):
        out[hole, k] = rng.uniform(-1e3, 1e3, n).astype(np.float32) if stored is None else np.float32(stored)
    out[hole, c] = 0
    return out


def build_view_program():
    """Compiles hole_fill_view.cc (vwlite headers + libvwgpu.so) with its own command."""
    exe = os.path.join(HERE, "hole_fill_view")
    src = os.path.join(HERE, "hole_fill_view.cc")
    lib_dir = os.path.join(ROOT, "visionworkbench_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "visionworkbench_amd", "vwlite"), "-o", exe, src, "-L" + lib_dir,
                           "-lvwgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
