"""ctypes binding of the CPU restatement of the CAHVOR and CAHVORE cameras (cahvor_ref.cc; test infrastructure) and the
cameras and scenes of the tests.  Cameras are visionworkbench_amd.camera models or descriptors; nothing here calls the
library's arithmetic: the models only carry their parameters."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
from visionworkbench_amd import _lib as vw_lib  # noqa: E402
from visionworkbench_amd import camera as vw_camera  # noqa: E402

FORWARD, REVERSE = 0, 1
ST_OK, ST_NOT_CONVERGED, ST_THETA = 0, 1, 2
RC_ARGUMENT, RC_LOGIC = -1, -5
VIEW, MODEL = 0, 1
_LIB = None
GOLDEN = os.path.join(ROOT, "tests", "golden")


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "cahvor_ref.mk"])
    return os.path.join(HERE, "libcahvor_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, d, f, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float, ctypes.c_longlong
        _LIB.cvr_pixel_to_vector.argtypes = [p, d, d, p, p]
        _LIB.cvr_point_to_pixel.argtypes = [p, p, p]
        _LIB.cvr_linearize.argtypes = [p, i, i, i, i, p]
        _LIB.cvr_camera_transform.argtypes = [p, i, i, p, p, p, i, i, i, i, f, i, p, p, p, p, p, p]
        _LIB.cvr_transform_points.argtypes = [p, p, i, p, ll, p, p]
        _LIB.cvr_stereo_triangulate.argtypes = [p, i, i, i, i, p, p, d, i, p, p, p, p, p]
        assert _LIB.trr_camera_size() == ctypes.sizeof(vw_lib.Camera)
    return _LIB


def _cam(c):
    return ctypes.addressof(vw_camera.descriptor_of(c))


def pixel_to_vector(cam, pix):
    """(ray (3,), status, Newton steps)"""
    out, passes = np.zeros(3), ctypes.c_int(0)
    st = lib().cvr_pixel_to_vector(_cam(cam), float(pix[0]), float(pix[1]), out.ctypes.data, ctypes.addressof(passes))
    return out, st, passes.value


def point_to_pixel(cam, point):
    """(pixel (2,), status)"""
    p, out = np.ascontiguousarray(point, np.float64), np.zeros(2)
    st = lib().cvr_point_to_pixel(_cam(cam), p.ctypes.data, out.ctypes.data)
    return out, st


def linearize(cam, in_size, out_size=None):
    """(descriptor of the CAHV camera, rc)"""
    out_size = in_size if out_size is None else out_size
    d = vw_lib.Camera()
    rc = lib().cvr_linearize(_cam(cam), int(in_size[0]), int(in_size[1]), int(out_size[0]), int(out_size[1]), ctypes.addressof(d))
    return d, rc


def cahv_model(d):
    return vw_camera.CAHVModel(list(d.center), list(d.A), list(d.H), list(d.V))


def linearize_model(cam, in_size, out_size=None):
    d, rc = linearize(cam, in_size, out_size)
    assert rc == 0
    return cahv_model(d)


def camera_transform(image, src, dst, size=None, mask=None, edge=(0, False), x0=0, y0=0):
    """A dict: out (h, w) float32, mask (h, w) uint8 (always computed), q (h, w, 2) the source positions, status and passes
    (h, w) int32, failed and theta (counts), rc."""
    img = np.ascontiguousarray(image, np.float32)
    sh, sw = img.shape
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    w, h = (sw, sh) if size is None else (int(size[0]), int(size[1]))
    out, omask = np.empty((h, w), np.float32), np.empty((h, w), np.uint8)
    q, status, passes = np.empty((h, w, 2)), np.empty((h, w), np.int32), np.empty((h, w), np.int32)
    counts = np.zeros(2, np.int64)
    rc = lib().cvr_camera_transform(img.ctypes.data, sw, sh, None if m is None else m.ctypes.data, _cam(src), _cam(dst), w, h, int(x0),
                                    int(y0), float(edge[0]), int(bool(edge[1])), out.ctypes.data, omask.ctypes.data, q.ctypes.data,
                                    status.ctypes.data, passes.ctypes.data, counts.ctypes.data)
    return {"out": out, "mask": omask, "q": q, "status": status, "passes": passes, "failed": int(counts[0]), "theta": int(counts[1]),
            "rc": rc}


def transform_points(src, dst, direction, points):
    """(out (n, 2), failed, theta, rc)"""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 2)
    out, counts = np.empty_like(p), np.zeros(2, np.int64)
    rc = lib().cvr_transform_points(_cam(src), _cam(dst), direction, p.ctypes.data, p.shape[0], out.ctypes.data, counts.ctypes.data)
    return out, int(counts[0]), int(counts[1]), rc


class Stats(ctypes.Structure):
    _fields_ = [("point_count", ctypes.c_longlong), ("max_error", ctypes.c_double), ("sum_error", ctypes.c_double)]


def stereo_triangulate(disp, cam1, cam2, semantics=VIEW, angle_tol=0.0):
    """disp (h, w, 3) float32 {dx, dy, valid}.  A dict: xyz, error, errvec, angle, stats (point_count, max_error, sum_error)."""
    d = np.ascontiguousarray(disp, np.float32)
    h, w = d.shape[:2]
    xyz, err, ev, ang = np.empty((h, w, 3)), np.empty((h, w)), np.empty((h, w, 3)), np.empty((h, w))
    st = Stats()
    rc = lib().cvr_stereo_triangulate(d.ctypes.data, w, h, 0, 0, _cam(cam1), _cam(cam2), float(angle_tol), int(semantics), xyz.ctypes.data,
                                      err.ctypes.data, ev.ctypes.data, ctypes.addressof(st), ang.ctypes.data)
    assert rc == 0
    return {"xyz": xyz, "error": err, "errvec": ev, "angle": ang, "stats": (st.point_count, st.max_error, st.sum_error)}


# ---- cameras ---------------------------------------------------------------------------------------------------------------

def golden():
    with open(os.path.join(GOLDEN, "cahvor_cameras.json")) as f:
        return json.load(f)


def _scaled(H, V, A, s):
    """H' = s H + ((s - 1) / 2) A: the camera of the same frame sampled s times as densely (pixel centres at integers)."""
    H, V, A = (np.array(x, np.float64) for x in (H, V, A))
    return s * H + ((s - 1) / 2) * A, s * V + ((s - 1) / 2) * A


def cahvor(s=1.0, R=None, C=None):
    """The reference's ForwardReverse CAHVOR camera (a 1024^2 frame), scaled by s."""
    g = golden()["cahvor"]
    H, V = _scaled(g["H"], g["V"], g["A"], s)
    return vw_camera.CAHVORModel(g["C"] if C is None else C, g["A"], H, V, g["O"], g["R"] if R is None else R)


def cahvore(s=1.0, R=None, T=None, P=None, C=None, unit_O=False):
    """The reference's ForwardReverse CAHVORE camera (a 1024^2 frame, T = 3, P = 0.37), scaled by s.  Its O has six digits
    and a norm of 1 - 4e-7, more than the 1e-8 of the small-angle branch: unit_O normalises it."""
    g = golden()["cahvore"]
    H, V = _scaled(g["H"], g["V"], g["A"], s)
    O = np.array(g["O"], np.float64)
    if unit_O:
        O = O / np.sqrt(O @ O)
    return vw_camera.CAHVOREModel(g["C"] if C is None else C, g["A"], H, V, O, g["R"] if R is None else R, g["E"],
                                  T=g["T"] if T is None else T, P=g["P"] if P is None else P)


def axis_pixel(cam):
    """The pixel whose ray is the optical axis O of a CAHVOR[E] camera."""
    return np.array([cam.O @ cam.H / (cam.O @ cam.A), cam.O @ cam.V / (cam.O @ cam.A)])


SW, SH = 96, 80          # the small frame of the GPU tests
SCALE = SW / 1024.0


def small(kind, **kw):
    """The fixture camera of `kind` for a 96-wide frame (the rows scale with it; 80 of them are used)."""
    return (cahvor if kind == "cahvor" else cahvore)(SCALE, **kw)


def source_image(seed=11):
    """(image (SH, SW) float32 in [0, 1], mask uint8), about a tenth of the pixels invalid."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:SH, 0:SW].astype(np.float64)
    img = 0.5 + 0.3 * np.sin(xs / 6.0) * np.cos(ys / 5.0) + rng.uniform(-0.15, 0.15, (SH, SW))
    mask = (rng.random((SH, SW)) >= 0.1).astype(np.uint8) * 255
    return np.clip(img, 0, 1).astype(np.float32), mask


def turned(cahv, deg_h, deg_v=0.0):
    """The CAHV camera turned about its own vertical (and horizontal) image axis by the given angles: same centre."""
    A, H, V = cahv.A, cahv.H, cahv.V
    hc, vc = H @ A, V @ A
    hp, vp = H - hc * A, V - vc * A
    hs, vs = np.sqrt(hp @ hp), np.sqrt(vp @ vp)
    h1, v1 = hp / hs, vp / vs
    a, b = np.deg2rad(deg_h), np.deg2rad(deg_v)
    A2 = np.cos(a) * A + np.sin(a) * h1
    h2 = np.cos(a) * h1 - np.sin(a) * A
    A3 = np.cos(b) * A2 + np.sin(b) * v1
    v3 = np.cos(b) * v1 - np.sin(b) * A2
    return vw_camera.CAHVModel(cahv.C, A3, hs * h2 + hc * A3, vs * v3 + vc * A3)


STRONG_R = (0.001, -0.05, 0.5)      # some pixels of a 37 x 29 image leave the Newton loop in pass 0, others in pass 2


def theta_pair():
    """(src, dst): a P = 1 CAHVORE source under its own linearisation turned by 110 degrees; for part of the output
    theta * |P| exceeds pi / 2."""
    src = small("cahvore", T=1)
    return src, turned(linearize_model(src, (SW, SH)), 110.0)


def scene_points(cam, n=240, seed=5):
    """Points 8 to 14 in front of `cam`, spread over its field of view."""
    rng = np.random.default_rng(seed)
    A = cam.A / np.sqrt(cam.A @ cam.A)
    hp = cam.H - (cam.H @ A) * A
    vp = cam.V - (cam.V @ A) * A
    h1, v1 = hp / np.sqrt(hp @ hp), vp / np.sqrt(vp @ vp)
    depth = rng.uniform(8, 14, n)
    return cam.C + depth[:, None] * A + rng.uniform(-2.5, 2.5, n)[:, None] * h1 + rng.uniform(-2.0, 2.0, n)[:, None] * v1


def stereo_pair(kind, **kw):
    """Two cameras of `kind` for the small frame, 0.4 apart along the image's horizontal axis."""
    left = small(kind, **kw)
    A = left.A
    hp = left.H - (left.H @ A) * A
    right = small(kind, C=left.C + 0.4 * hp / np.sqrt(hp @ hp), **kw)
    return left, right


def scene_disparity(kind, w=33, h=21, seed=9, **kw):
    """(disp (h, w, 3) float32, left, right): the disparities of w x h scene points, 8 to 14 away along the left rays of the
    map's pixels, projected by the restatement into the right camera; sub-pixel noise in both components makes the rays
    skew.  About one pixel in sixteen is invalid."""
    left, right = stereo_pair(kind, **kw)
    rng = np.random.default_rng(seed)
    d = np.zeros((h, w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            ray, st, _ = pixel_to_vector(left, (x, y))
            assert st == ST_OK
            q, st = point_to_pixel(right, left.C + rng.uniform(8, 14) * ray)
            assert st == ST_OK
            d[y, x] = (q[0] - x + rng.uniform(-0.3, 0.3), q[1] - y + rng.uniform(-0.3, 0.3), rng.random() >= 1 / 16)
    return d, left, right


# ---- the C++ program -------------------------------------------------------------------------------------------------------

def build_view_program():
    """Compiles cahvor_view.cc (vwlite headers + libvwgpu.so) with its makefile fragment."""
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "cahvor_view.mk"])
    return os.path.join(HERE, "cahvor_view")
