"""ctypes binding of the CPU restatement of two-camera triangulation (triangulate_ref.cc; test infrastructure), the C++
program (triangulate_view.cc) and the scenes of the tests.  Cameras are visionworkbench_amd.camera models or their flat
descriptors (struct vwgpu_camera)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from visionworkbench_amd import _lib as vw_lib  # noqa: E402
from visionworkbench_amd import camera as vw_camera  # noqa: E402

SEMANTICS = {"view": 0, "model": 1}
LAYOUTS = {"dxdyv": 0x000, "dxdy": 0x100, "dv": 0x200, "d": 0x300}
WORDS = {"dxdyv": 3, "dxdy": 2, "dv": 2, "d": 1}
# classes[..., 0]: what became of a pixel; classes[..., 1:3]: how the Tsai solver of camera 1 / 2 left
PX_INVALID, PX_NAN, PX_INVALID_PIXEL, PX_PARALLEL, PX_REFLECTED, PX_POINT = range(6)
EXIT_NONE, EXIT_STEP, EXIT_DET, EXIT_NAN, EXIT_PASSES = range(5)
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "triangulate_ref.mk"])
    return os.path.join(HERE, "libtriangulate_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        _LIB.trr_pinhole_camera.argtypes = [p, p, d, d, d, d, p, p, p, d, i, p, p]
        _LIB.trr_stereo_triangulate.argtypes = [i, p, i, i, i, i, p, p, d, i, p, p, p, p, p]
        _LIB.trr_convergence_angle.argtypes = [i, p, i, i, i, i, p, p, i, p]
        _LIB.trr_universe_radius.argtypes = [p, i, i, i, p, d, d, p, p]
        _LIB.trr_pixel_to_vector.argtypes = [p, d, d, p, p]
        _LIB.trr_pixel_to_vector.restype = None
        _LIB.trr_tsai_distorted.argtypes = [p, d, d, p]
        _LIB.trr_tsai_distorted.restype = None
        _LIB.trr_tsai_undistorted.argtypes = [p, d, d, p, p]
        _LIB.trr_tsai_undistorted.restype = None
        assert _LIB.trr_camera_size() == ctypes.sizeof(vw_lib.Camera)
    return _LIB


def _cam(c):
    return ctypes.addressof(vw_camera.descriptor_of(c))


def _disp(disparity, layout):
    d = np.ascontiguousarray(disparity)
    if d.dtype not in (np.int32, np.float32):
        raise ValueError("disparity must be int32 or float32")
    if layout is None:
        layout = "d" if d.ndim == 2 else {3: "dxdyv", 2: "dxdy"}[d.shape[2]]
    if (d.ndim != 2) if WORDS[layout] == 1 else (d.ndim != 3 or d.shape[2] != WORDS[layout]):
        raise ValueError("disparity shape does not fit layout %r" % layout)
    return d, (0 if d.dtype == np.int32 else 1), LAYOUTS[layout], d.shape[1], d.shape[0]


def pinhole_descriptor(center, rotation, fu, fv, cu, cv, u=(1, 0, 0), v=(0, 1, 0), w=(0, 0, 1), distortion=None, pixel_pitch=1.0):
    """The restatement's own rebuild_camera_matrix; raises ValueError where the reference asserts."""
    a = [np.ascontiguousarray(np.array(x, np.float64).reshape(-1)) for x in (center, rotation, u, v, w)]
    dist = None if distortion is None else np.ascontiguousarray(np.array(distortion, np.float64))
    out = vw_lib.Camera()
    rc = lib().trr_pinhole_camera(a[0].ctypes.data, a[1].ctypes.data, fu, fv, cu, cv, a[2].ctypes.data, a[3].ctypes.data,
                                  a[4].ctypes.data, pixel_pitch, 0 if dist is None else 1, None if dist is None else dist.ctypes.data,
                                  ctypes.addressof(out))
    if rc:
        raise ValueError("trr_pinhole_camera: rc %d" % rc)
    return out


def stereo_triangulate(disparity, cam1, cam2, x0=0, y0=0, angle_tol=0.0, semantics="view", layout=None):
    """Returns a dict: xyz (h, w, 3), error (h, w), errvec (h, w, 3), stats [point_count, max_error, sum_error] and
    classes (h, w, 3) int32."""
    d, t, lay, w, h = _disp(disparity, layout)
    xyz, err, vec = np.empty((h, w, 3)), np.empty((h, w)), np.empty((h, w, 3))
    cls = np.empty((h, w, 3), np.int32)
    st = vw_lib.TriangulateStats()
    rc = lib().trr_stereo_triangulate(t, d.ctypes.data, w, h, int(x0), int(y0), _cam(cam1), _cam(cam2), float(angle_tol),
                                      SEMANTICS[semantics] | lay, xyz.ctypes.data, err.ctypes.data, vec.ctypes.data,
                                      ctypes.addressof(st), cls.ctypes.data)
    if rc:
        raise ValueError("trr_stereo_triangulate: rc %d" % rc)
    return {"xyz": xyz, "error": err, "errvec": vec, "stats": [int(st.point_count), float(st.max_error), float(st.sum_error)],
            "classes": cls}


def convergence_angle(disparity, cam1, cam2, x0=0, y0=0, semantics="model", layout=None):
    d, t, lay, w, h = _disp(disparity, layout)
    out = np.empty((h, w))
    rc = lib().trr_convergence_angle(t, d.ctypes.data, w, h, int(x0), int(y0), _cam(cam1), _cam(cam2), SEMANTICS[semantics] | lay,
                                     out.ctypes.data)
    if rc:
        raise ValueError("trr_convergence_angle: rc %d" % rc)
    return out


def universe_radius(points, origin, near_radius=0.0, far_radius=float(np.finfo(np.float64).max), stats=None):
    p = np.ascontiguousarray(points, np.float64)
    out = np.empty_like(p)
    o = np.ascontiguousarray(np.array(origin, np.float64))
    counts = (ctypes.c_longlong * 2)()
    rc = lib().trr_universe_radius(p.ctypes.data, p.shape[2], p.shape[1], p.shape[0], o.ctypes.data, float(near_radius),
                                   float(far_radius), out.ctypes.data, counts)
    if rc:
        raise ValueError("trr_universe_radius: rc %d" % rc)
    if stats is not None:
        stats[:] = list(counts)
    return out


def pixel_to_vector(cam, pix):
    out, how = np.empty(3), ctypes.c_int(0)
    lib().trr_pixel_to_vector(_cam(cam), float(pix[0]), float(pix[1]), out.ctypes.data, ctypes.addressof(how))
    return out


def tsai_distorted(cam, pix):
    out = np.empty(2)
    lib().trr_tsai_distorted(_cam(cam), float(pix[0]), float(pix[1]), out.ctypes.data)
    return out


def tsai_undistorted(cam, pix):
    """(undistorted pixel, how the solver left)"""
    out, how = np.empty(2), ctypes.c_int(0)
    lib().trr_tsai_undistorted(_cam(cam), float(pix[0]), float(pix[1]), out.ctypes.data, ctypes.addressof(how))
    return out, how.value


# ---- scenes --------------------------------------------------------------------------------------------------------------

def rot_y(deg):
    a = deg * (math.pi / 180.0)   # the C library's cos and sin, as triangulate_view.cc uses them
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def pinhole_pair(w=70, h=45, f=500.0, toe_in=2.5, distortion1=None, distortion2=None):
    """A converging pair: baseline 1 along x, each camera turned toe_in degrees towards the other, principal point at the
    image centre."""
    cu, cv = w / 2.0, h / 2.0
    return (vw_camera.PinholeModel((0, 0, 0), rot_y(toe_in), f, f, cu, cv, distortion=distortion1),
            vw_camera.PinholeModel((1, 0, 0), rot_y(-toe_in), f, f, cu, cv, distortion=distortion2))


def cahv_of(pin, flip_v=False):
    """The CAHV camera of an undistorted pinhole.  With the pinhole's own axes dot(cross(V, H), A) < 0 and pixel_to_vector
    takes its sign flip; flip_v=True turns the image's v axis round (rows counted upwards), the other handedness."""
    r = pin.rotation
    hvec, vvec, a = r[:, 0], (-r[:, 1] if flip_v else r[:, 1]), r[:, 2]
    return vw_camera.CAHVModel(pin.center, a, pin.fu * hvec + pin.cu * a, pin.fv * vvec + pin.cv * a)


def _depth_disparity(cam1, cam2, w, h, seed, depth0=12.0, noise=0.3):
    """Disparities of a smooth depth surface seen from cam1 (an undistorted pinhole with the default frame), plus sub-pixel
    noise in both components (skew rays)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    k_inv = np.linalg.inv(np.array([[cam1.fu, 0, cam1.cu], [0, cam1.fv, cam1.cv], [0, 0, 1.0]]))
    rays = np.stack([xs, ys, np.ones_like(xs)], axis=-1) @ (cam1.rotation @ k_inv).T
    rays /= np.linalg.norm(rays, axis=-1, keepdims=True)
    depth = depth0 + 2.0 * np.sin(xs / 11.0) + np.cos(ys / 7.0)
    pts = cam1.camera_center() + rays * depth[..., None]
    q = np.concatenate([pts, np.ones((h, w, 1))], axis=-1) @ cam2.camera_matrix().T
    d = np.zeros((h, w, 3), np.float64)
    d[..., 0], d[..., 1] = q[..., 0] / q[..., 2] - xs, q[..., 1] / q[..., 2] - ys
    d[..., :2] += rng.uniform(-noise, noise, (h, w, 2))
    d[..., 2] = 1
    return d


def _disparity_to(cam1, cam2, x, y, depth):
    """The disparity at left pixel (x, y) of the point `depth` along its ray (negative: behind the camera)."""
    px2 = cam2.point_to_pixel(cam1.camera_center() + pixel_to_vector(cam1, (x, y)) * depth)
    return px2[0] - x, px2[1] - y


def main_scene(w=70, h=45, seed=7, dtype=np.float32, cams=None):
    """(disparity, cam1, cam2): the converging pinhole pair over a smooth depth surface, with one or more
    pixels of every class stamped in where the image is large enough: invalid, NaN (float), right pixel at
    (-1e8, -1e8), nearly parallel rays, a point behind the cameras."""
    ideal = pinhole_pair(w, h)                   # the disparities are this pair's, whichever cameras are handed back
    cam1, cam2 = cams if cams is not None else ideal
    d = _depth_disparity(ideal[0], ideal[1], w, h, seed)
    rng = np.random.default_rng(seed + 1)
    d[rng.random((h, w)) < 0.04, 2] = 0          # invalid pixels keep their stored disparity
    if w > 8 and h > 16:
        d[16, 8] = (-1e8 - 8, -1e8 - 16, 1)      # exactly representable in float32, and 8 + dx == -1e8 in float and double
    if w > 20 and h > 10:
        far = _disparity_to(ideal[0], ideal[1], 20, 10, 1e7)
        d[10, 20] = (far[0], far[1], 1)           # nearly parallel
        near = _disparity_to(ideal[0], ideal[1], 21, 10, 12.0)
        d[10, 21] = (2 * far[0] - near[0] - 20, far[1], 1)   # the rays diverge: the closest points lie behind the cameras
    out = d.astype(dtype) if dtype == np.float32 else np.round(d).astype(np.int32)
    if dtype == np.float32 and w > 5 and h > 3:
        out[3, 5] = (np.nan, 0.25, 1)
        out[3, 4] = (0.5, np.nan, 1)
    return out, cam1, cam2


# a lens whose radial term turns over inside the image (1 + 3 k1 r^2 = 0 at r = 1 / 16, 32 pixels from the centre): the
# Jacobian is singular on that circle and pixels beyond it have no undistorted counterpart, so the solver's fallbacks run
WILD_TSAI = (-256.0 / 3.0, 0.0, 0.0, 0.0, 0.0)
MILD_TSAI = (-0.28, 0.09, 1.1e-3, -6e-4, 0.013)


def tsai_scene(w=70, h=45, seed=11):
    """(disparity, cam1, cam2): f = 512 and the principal point at (32, 22), so that left pixel (64, 22) sits on the
    singular circle of cam1's lens; cam2 has a mild lens."""
    cam1 = vw_camera.PinholeModel((0, 0, 0), rot_y(2.5), 512.0, 512.0, 32.0, 22.0, distortion=vw_camera.TsaiLensDistortion(*WILD_TSAI))
    cam2 = vw_camera.PinholeModel((1, 0, 0), rot_y(-2.5), 512.0, 512.0, 32.0, 22.0, distortion=vw_camera.TsaiLensDistortion(*MILD_TSAI))
    ideal = (vw_camera.PinholeModel((0, 0, 0), rot_y(2.5), 512.0, 512.0, 32.0, 22.0),
             vw_camera.PinholeModel((1, 0, 0), rot_y(-2.5), 512.0, 512.0, 32.0, 22.0))
    d = _depth_disparity(ideal[0], ideal[1], w, h, seed)
    rng = np.random.default_rng(seed + 1)
    d[rng.random((h, w)) < 0.04, 2] = 0
    return d.astype(np.float32), cam1, cam2


def relayout(disparity, layout):
    """A {dx, dy, valid} map in another pixel form (the scalar forms keep dx)."""
    if layout == "dxdyv":
        return disparity
    if layout == "dxdy":
        return np.ascontiguousarray(disparity[..., :2])
    if layout == "dv":
        return np.ascontiguousarray(disparity[..., [0, 2]])
    return np.ascontiguousarray(disparity[..., 0])


# ---- the C++ program -----------------------------------------------------------------------------------------------------

def build_view_program():
    """Compiles triangulate_view.cc (vwlite headers + libvwgpu.so) with its own command."""
    exe = os.path.join(HERE, "triangulate_view")
    src = os.path.join(HERE, "triangulate_view.cc")
    lib_dir = os.path.join(ROOT, "visionworkbench_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "visionworkbench_amd", "vwlite"), "-o", exe, src, "-L" + lib_dir,
                           "-lvwgpu", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe
