"""ctypes binding of the CPU restatement of vw::transform (transform_ref.cc; test infrastructure) and the scenes of the
tests.  A map is a vwgpu_transform descriptor (visionworkbench_amd._lib.Transform, whose layout the restatement shares);
the scenes make theirs with the restatement's own tfr_make / tfr_rotate / tfr_invert, so both sides are handed the same
inverse matrices."""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from visionworkbench_amd import _lib as vw_lib  # noqa: E402

IDENTITY, TRANSLATE, RESAMPLE, AFFINE, HOMOGRAPHY = range(5)
NEAREST, BILINEAR, BICUBIC = range(3)
INTERPS = {"nearest": NEAREST, "bilinear": BILINEAR, "bicubic": BICUBIC}
ZERO, VALUE, CONSTANT, PERIODIC, CYLINDRICAL, REFLECT, LINEAR = range(7)
EDGES = {"zero": ZERO, "value": VALUE, "constant": CONSTANT, "periodic": PERIODIC, "cylindrical": CYLINDRICAL, "reflect": REFLECT,
         "linear": LINEAR}
FORWARD, REVERSE = 0, 1
C_INTEGER, C_ALL_INSIDE, C_SOME_OUTSIDE, C_NAN_HUGE, C_NODATA, C_OTHER_TAP = 1, 2, 4, 8, 16, 32
_LIB = None


def same(got, want, what=""):
    """Exact equality of every word; NaNs by position."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype.kind != "f":
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: %d words differ, first at %s: got %r, want %r" % (
            what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaNs in different places" % what
    g, w = got.copy(), want.copy()
    g[gn], w[wn] = 0, 0
    bits = {8: np.uint64, 4: np.uint32}[got.dtype.itemsize]
    bad = np.argwhere(g.view(bits) != w.view(bits))
    assert bad.size == 0, "%s: %d words differ, first at %s: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "transform_ref.mk"])
    return os.path.join(HERE, "libtransform_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, d, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float, ctypes.c_longlong
        _LIB.tfr_make.argtypes = [i, p, i, p]
        _LIB.tfr_rotate.argtypes = [d, d, d, p]
        _LIB.tfr_invert.argtypes = [p, p]
        _LIB.tfr_points.argtypes = [p, i, i, p, ll, p]
        _LIB.tfr_image.argtypes = [p, i, i, p, p, i, i, i, f, i, i, f, i, i, i, i, i, p, p, p]
        assert _LIB.tfr_desc_size() == ctypes.sizeof(vw_lib.Transform)
    return _LIB


def make(kind, params=()):
    """(rc, descriptor) of the restatement's tfr_make; the descriptor is all 0xff bytes beforehand, to show what a refusal leaves."""
    d = vw_lib.Transform()
    ctypes.memset(ctypes.addressof(d), 0xff, ctypes.sizeof(d))
    p = np.ascontiguousarray(params, np.float64).reshape(-1)
    rc = lib().tfr_make(int(kind), p.ctypes.data if p.size else None, int(p.size), ctypes.addressof(d))
    return rc, d


def made(kind, params=()):
    rc, d = make(kind, params)
    assert rc == 0, (kind, params)
    return d


def rotate(theta, cx, cy):
    d = vw_lib.Transform()
    assert lib().tfr_rotate(theta, cx, cy, ctypes.addressof(d)) == 0
    return d


def invert(desc):
    d = vw_lib.Transform()
    assert lib().tfr_invert(ctypes.addressof(desc), ctypes.addressof(d)) == 0
    return d


def by_hand(kind, fwd=(), rev=()):
    """A descriptor filled word by word."""
    d = vw_lib.Transform()
    d.kind = kind
    for k, v in enumerate(fwd):
        d.fwd[k] = v
    for k, v in enumerate(rev):
        d.rev[k] = v
    return d


def _array(steps):
    steps = list(steps)
    return (vw_lib.Transform * len(steps))(*steps), len(steps)


def points(steps, direction, pts):
    """(rc, out) of the restatement's chain on (n, 2) points."""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 2)
    out = np.empty_like(p)
    arr, n = _array(steps)
    rc = lib().tfr_points(arr, n, direction, p.ctypes.data, p.shape[0], out.ctypes.data)
    return rc, out


def image(img, steps, size, x0=0, y0=0, interp=BILINEAR, edge=ZERO, edge_value=0.0, edge_valid=False, mask=None, nodata=None):
    """A dict: out (h, w) float32, mask (h, w) uint8 (always computed: without a source mask every source pixel is valid),
    classes (h, w) int32 of C_* bits, rc.  nodata: None or (value, valid)."""
    src = np.ascontiguousarray(img, np.float32)
    sh, sw = src.shape
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    w, h = int(size[0]), int(size[1])
    out, omask, cls = np.empty((h, w), np.float32), np.empty((h, w), np.uint8), np.empty((h, w), np.int32)
    arr, n = _array(steps)
    nd = (0, 0.0, 0) if nodata is None else (1, float(nodata[0]), int(bool(nodata[1])))
    rc = lib().tfr_image(src.ctypes.data, sw, sh, None if m is None else m.ctypes.data, arr, n, int(interp), int(edge), float(edge_value),
                         int(bool(edge_valid)), nd[0], nd[1], nd[2], w, h, int(x0), int(y0), out.ctypes.data, omask.ctypes.data,
                         cls.ctypes.data)
    return {"out": out, "mask": omask, "classes": cls, "rc": rc}


def at(img, qx, qy, interp, edge, **kw):
    """The interpolation of the edge-extended image at the real position (qx, qy): a translation by (-qx, -qy) seen at (0, 0)."""
    r = image(img, [made(TRANSLATE, (-qx, -qy))], (1, 1), interp=interp, edge=edge, **kw)
    assert r["rc"] == 0
    return float(r["out"][0, 0])


# ---- scenes ----------------------------------------------------------------------------------------------------------------

SOURCE_SIZES = [(1, 1), (2, 3), (17, 1), (37, 23), (70, 45)]      # (cols, rows)
OUTPUT_SIZES = [(70, 9), (130, 11)]                                # neither a multiple of 64 x 4


def source_image(size, seed=3):
    """(image (rows, cols) float32, mask uint8 255 / 0): smooth texture plus noise; about a tenth of the pixels invalid,
    with values of their own (a masked tap forms its value whatever the validity)."""
    w, h = size
    rng = np.random.default_rng(seed + 131 * w + h)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 100.0 + 40.0 * np.sin(xs / 5.0) * np.cos(ys / 7.0) + rng.uniform(-5, 5, (h, w))
    mask = (rng.random((h, w)) >= 0.1).astype(np.uint8) * 255
    return img.astype(np.float32), mask


def sample_image():
    """The 2 x 3 image 1..6 of the reference's unit tests."""
    return np.array([[1, 2], [3, 4], [5, 6]], np.float32)


W0_REV = (0.5, 0.0, 0.0, 0.0, 0.25, 0.0, 1.0 / 64, 0.0, -0.25)      # w = x / 64 - 1 / 4: exactly 0 in column 16


def scenes():
    """name -> dict(src=(cols, rows), steps=[descriptors], size=(w, h), x0, y0): every map of the GPU test over an output box
    that straddles the source's border."""
    rot = rotate(0.3, 34.5, 22.0)
    shear = made(AFFINE, (1.1, 0.2, -0.1, 0.9, 3.5, -2.25))
    return {
        "identity": dict(src=(70, 45), steps=[made(IDENTITY)], size=(130, 11), x0=-25, y0=-4),
        "int_translate": dict(src=(70, 45), steps=[made(TRANSLATE, (3.0, -2.0))], size=(130, 11), x0=-25, y0=-4),
        "frac_translate": dict(src=(70, 45), steps=[made(TRANSLATE, (0.375, -1.25))], size=(130, 11), x0=-25, y0=-4),
        "resample_2": dict(src=(37, 23), steps=[made(RESAMPLE, (2.0, 2.0))], size=(130, 11), x0=-25, y0=-3),
        "resample_half": dict(src=(70, 45), steps=[made(RESAMPLE, (0.5, 0.5))], size=(70, 9), x0=-10, y0=-2),
        "resize_odd": dict(src=(37, 23), steps=[made(RESAMPLE, (51 / 37.0, 9 / 23.0))], size=(70, 9), x0=-9, y0=-2),
        "rotate": dict(src=(70, 45), steps=[rot], size=(130, 11), x0=-25, y0=14),
        "shear": dict(src=(70, 45), steps=[shear], size=(130, 11), x0=-20, y0=-3),
        "homography": dict(src=(70, 45), steps=[made(HOMOGRAPHY, (1.01, 0.02, -1.5, -0.01, 0.99, 2.0, 1e-4, -2e-4, 1.0))], size=(130, 11),
                           x0=-25, y0=-4),
        "w_zero": dict(src=(70, 45), steps=[by_hand(HOMOGRAPHY, rev=W0_REV)], size=(130, 11), x0=0, y0=0),
        "chain3": dict(src=(70, 45), steps=[made(TRANSLATE, (2.5, -1.0)), rotate(0.2, 30.0, 20.0), made(RESAMPLE, (1.25, 0.8))],
                       size=(130, 11), x0=-20, y0=-3),
        "inverse": dict(src=(70, 45), steps=[invert(shear)], size=(130, 11), x0=-10, y0=20),
    }


INTEGER_ONLY = ("identity", "int_translate", "resample_half")     # every position an integer: one tap, whatever the interpolation


def scene_result(name, interp, masked, edge=ZERO, edge_value=0.0, edge_valid=False, nodata=None):
    s = scenes()[name]
    img, mask = source_image(s["src"])
    return image(img, s["steps"], s["size"], s["x0"], s["y0"], interp=interp, edge=edge, edge_value=edge_value, edge_valid=edge_valid,
                 mask=mask if masked else None, nodata=nodata)


# ---- the C++ program -----------------------------------------------------------------------------------------------------

def build_view_program():
    """Compiles transform_view.cc (vwlite headers + libvwgpu.so) by transform_view.mk."""
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "transform_view.mk"])
    return os.path.join(HERE, "transform_view")
