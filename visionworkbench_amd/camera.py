"""The part of vw::camera that triangulation and epipolar rectification need: PinholeModel with the null, Tsai, FOV,
fisheye, Brown-Conrady, adjustable Tsai or Photometrix lens distortion and its .tsai files, CAHVModel, CAHVORModel and
CAHVOREModel, epipolar(), linearize_camera, resize_epipolar_cameras_to_fit, CameraTransform and camera_transform.

Each model is a host object that produces the flat camera descriptor of the C ABI (struct vwgpu_camera, include/vwgpu.h)
and, for a pinhole, the 3 x 4 camera matrix that travels beside it; the rays and projections themselves are computed on
the device (stereo.stereo_triangulate, camera_transform, CameraTransform).  point_to_pixel is a host convenience in numpy
(scene building, tests); the models and epipolar() need no GPU.
"""
import ctypes
import re

import numpy as np

from . import _lib
from ._operands import Operands
from .core import ArgumentErr, BBox2i, IOErr, LogicErr, NoImplErr

CAMERA_PINHOLE, CAMERA_CAHV, CAMERA_CAHVOR, CAMERA_CAHVORE = 0, 1, 3, 4      # 2 is unassigned and refused (include/vwgpu.h)
DISTORTION_NULL, DISTORTION_TSAI = 0, 1
DISTORTION_FOV, DISTORTION_FISHEYE, DISTORTION_BROWN_CONRADY, DISTORTION_ADJUSTABLE_TSAI, DISTORTION_PHOTOMETRIX = 2, 3, 4, 6, 7   # 5 is refused


def _g17(v):
    return "%.17g" % v          # std::setprecision(17): the digits that survive double -> text -> double


def _read_fields(lines, names, missing_ok=()):
    """read_fields_in_vec (src/vw/Camera/LensDistortion.cc:52-92): `name = value` lines in any order, others ignored."""
    found = {}
    for line in lines:
        t = line.replace("=", " ").split()
        if len(t) >= 2:
            try:
                found[t[0]] = float(t[1])
            except ValueError:
                pass
    out = []
    for n in names:
        if n not in found and n not in missing_ok:
            raise IOErr("LensDistortion: Could not read a value for %s." % n)
        out.append(found.get(n, 0.0))
    return out


def _vec3(v, what):
    a = np.array(v, np.float64).reshape(-1)
    if a.size != 3:
        raise ArgumentErr("%s must have three elements" % what)
    return np.ascontiguousarray(a)


class LensDistortion(object):
    """vw::camera::LensDistortion (src/vw/Camera/LensDistortion.h): the parameters of one lens.  The two coordinate
    functions take a PinholeModel and a point in focal-plane units (pixel * pixel_pitch) and run, on the host, the
    functions the kernels run (vwgpu_lens_coordinates)."""
    KIND, NAME, PARAM_NAMES = None, None, ()

    def _set(self, params):
        self.params = np.ascontiguousarray(np.array(params, np.float64).reshape(-1))
        if self.PARAM_NAMES and self.params.size != len(self.PARAM_NAMES):
            raise IOErr("%s: Incorrect number of parameters was passed in." % type(self).__name__)

    def name(self):
        return self.NAME

    def distortion_parameters(self):
        return self.params.copy()

    def _coordinates(self, cam, direction, p):
        if cam.distortion is not self:
            raise ArgumentErr("%s: the camera carries another lens" % type(self).__name__)
        pts = np.ascontiguousarray(np.array(p, np.float64))
        if pts.ndim < 1 or pts.shape[-1] != 2:
            raise ArgumentErr("%s: the points must be (..., 2) {x, y}" % type(self).__name__)
        out = np.empty_like(pts)
        rc = _lib.load().vwgpu_lens_coordinates(ctypes.byref(cam.descriptor), direction, pts.ctypes.data, pts.size // 2,
                                                out.ctypes.data, None)
        if rc == -5:
            raise LogicErr("LensDistortion: Did not converge.")
        if rc != 0:
            raise ArgumentErr("%s: bad arguments" % type(self).__name__)
        return out

    def distorted_coordinates(self, cam, p):
        return self._coordinates(cam, 0, p)

    def undistorted_coordinates(self, cam, p):
        return self._coordinates(cam, 1, p)

    def write(self, f):
        for n, v in zip(self.PARAM_NAMES, self.params):
            f.write("%s = %s\n" % (n, _g17(v)))

    @classmethod
    def read(cls, lines):
        return cls(_read_fields(lines, cls.PARAM_NAMES))


class FovLensDistortion(LensDistortion):
    """vw::camera::FovLensDistortion (src/vw/Camera/LensDistortion.cc:418-530): the one-parameter wide-angle lens; k1 must
    be positive (IOErr)."""
    KIND, NAME, PARAM_NAMES = 2, "FOV", ("k1",)

    def __init__(self, params):
        self._set(np.atleast_1d(params))
        if not self.params[0] > 0:
            raise IOErr("FovLensDistortion: The distortion coefficient must be positive.")


class FisheyeLensDistortion(LensDistortion):
    """vw::camera::FisheyeLensDistortion (src/vw/Camera/LensDistortion.cc:532-673): k1, k2, k3, k4."""
    KIND, NAME, PARAM_NAMES = 3, "FISHEYE", ("k1", "k2", "k3", "k4")

    def __init__(self, params):
        self._set(params)


class BrownConradyDistortion(LensDistortion):
    """vw::camera::BrownConradyDistortion (src/vw/Camera/LensDistortion.cc:675-775): BrownConradyDistortion(params) with
    the eight numbers xp, yp, k1, k2, k3, p1, p2, phi, or BrownConradyDistortion(principal, radial, centering, angle)."""
    KIND, NAME, PARAM_NAMES = 4, "BrownConrady", ("xp", "yp", "k1", "k2", "k3", "p1", "p2", "phi")

    def __init__(self, params, radial=None, centering=None, angle=None):
        if radial is not None:
            params = list(np.atleast_1d(params)) + list(radial) + list(centering) + [angle]
        if np.size(params) != 8:
            raise ArgumentErr("BrownConradyDistortion: requires constructor input of size 8.")
        self._set(params)

    def write(self, f):
        for n, v in zip(self.PARAM_NAMES, self.params):            # :746-756: two blanks before `=`, but for phi
            f.write("%s%s= %s\n" % (n, " " if n == "phi" else "  ", _g17(v)))


class AdjustableTsaiLensDistortion(LensDistortion):
    """vw::camera::AdjustableTsaiLensDistortion (src/vw/Camera/LensDistortion.cc:777-917): n - 3 even radial coefficients,
    two tangential ones and alpha; 4 <= n, and n <= 13 is what the camera descriptor holds."""
    KIND, NAME = 6, "AdjustableTSAI"

    def __init__(self, params):
        self._set(params)
        if self.params.size <= 3:
            raise ArgumentErr("Requires at least 4 coefficients for distortion. Last 3 are always the distortion coefficients and "
                              "alpha. All leading elements are even radial distortion coefficients.")
        if self.params.size > 13:
            raise NoImplErr("AdjustableTsaiLensDistortion: more than 13 coefficients do not fit the camera descriptor")

    def write(self, f):
        def vec(v):
            return "Vector%d(%s)" % (len(v), ",".join(_g17(x) for x in v))
        f.write("Radial Coeff: %s\nTangential Coeff: %s\nAlpha: %s\n" % (vec(self.params[:-3]), vec(self.params[-3:-1]), _g17(self.params[-1])))

    @classmethod
    def read(cls, lines):
        """AdjustableTsaiLensDistortion::read (:889-913): the three-line form."""
        text = "\n".join(lines)
        m = re.match(r"\s*Radial\s+Coeff:\s*Vector(\d+)\(([^)]*)\)\s*Tangential\s+Coeff:\s*Vector(\d+)\(([^)]*)\)\s*Alpha:\s*(\S+)", text)
        if m is None:
            raise IOErr("AdjustableTsaiLensDistortion::read(): Could not read vector params.")
        try:
            radial, tangential = [float(t) for t in m.group(2).split(",")], [float(t) for t in m.group(4).split(",")]
            alpha = float(m.group(5))
        except ValueError:
            raise IOErr("AdjustableTsaiLensDistortion::read(): Could not read vector params.")
        if len(radial) != int(m.group(1)) or len(tangential) != int(m.group(3)):
            raise IOErr("AdjustableTsaiLensDistortion::read(): Could not read vector params.")
        return cls(radial + tangential + [alpha])


class PhotometrixLensDistortion(LensDistortion):
    """vw::camera::PhotometrixLensDistortion (src/vw/Camera/LensDistortion.cc:919-1013): xp, yp, k1, k2, k3, p1, p2, b1, b2
    (b1 and b2 are not used, as in the reference)."""
    KIND, NAME, PARAM_NAMES = 7, "Photometrix", ("xp", "yp", "k1", "k2", "k3", "p1", "p2", "b1", "b2")

    def __init__(self, params):
        self._set(params)


class TsaiLensDistortion(LensDistortion):
    """vw::camera::TsaiLensDistortion (src/vw/Camera/LensDistortion.cc:225-400): parameters k1, k2, p1, p2, k3."""
    KIND, NAME, PARAM_NAMES = 1, "TSAI", ("k1", "k2", "p1", "p2", "k3")

    def __init__(self, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
        self.params = np.array([k1, k2, p1, p2, k3], np.float64)

    @classmethod
    def read(cls, lines):
        return cls(*_read_fields(lines, cls.PARAM_NAMES, missing_ok=("k3",)))

    def distorted_coordinates(self, cam, p):
        """TsaiLensDistortion::distorted_coordinates (:345-369) of an undistorted pixel (in units of the focal length)."""
        if cam.fu < 1e-300 or cam.fv < 1e-300:
            return np.array([np.inf, np.inf])
        k1, k2, p1, p2, k3 = self.params
        x, y = (p[0] - cam.cu) / cam.fu, (p[1] - cam.cv) / cam.fv
        r2 = x * x + y * y
        rdist = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
        dx = x * rdist + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
        dy = y * rdist + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
        return np.array([dx * cam.fu + cam.cu, dy * cam.fv + cam.cv])


class PinholeModel(object):
    """vw::camera::PinholeModel(center, rotation, fu, fv, cu, cv, u, v, w, distortion, pixel_pitch)
    (src/vw/Camera/PinholeModel.h): rotation is the camera-to-world matrix, (u, v, w) the image-plane frame (the default
    +x right, +y down, +z forward).  distortion: None (NullLensDistortion) or a LensDistortion (Tsai, FOV, fisheye, Brown-Conrady, adjustable Tsai,
    Photometrix).  u, v, w that fail the reference's orthonormality asserts raise ArgumentErr."""

    def __init__(self, center, rotation, fu, fv, cu, cv, u=(1, 0, 0), v=(0, 1, 0), w=(0, 0, 1), distortion=None, pixel_pitch=1.0):
        self.center = _vec3(center, "PinholeModel: the camera center")
        self.rotation = np.ascontiguousarray(np.array(rotation, np.float64))
        if self.rotation.shape != (3, 3):
            raise ArgumentErr("PinholeModel: the rotation must be 3 x 3")
        self.fu, self.fv, self.cu, self.cv = float(fu), float(fv), float(cu), float(cv)
        self.u, self.v, self.w = _vec3(u, "PinholeModel: u"), _vec3(v, "PinholeModel: v"), _vec3(w, "PinholeModel: w")
        if distortion is not None and not isinstance(distortion, LensDistortion):
            raise ArgumentErr("PinholeModel: the lens distortion must be None or a LensDistortion")
        self.distortion = distortion
        self.pixel_pitch = float(pixel_pitch)
        self.descriptor = _lib.Camera()
        tsai = isinstance(distortion, TsaiLensDistortion)
        params = distortion.params if tsai else None
        rc = _lib.load().vwgpu_pinhole_camera(
            self.center.ctypes.data, self.rotation.ctypes.data, self.fu, self.fv, self.cu, self.cv, self.u.ctypes.data,
            self.v.ctypes.data, self.w.ctypes.data, self.pixel_pitch, DISTORTION_TSAI if tsai else DISTORTION_NULL,
            params.ctypes.data if params is not None else None, ctypes.byref(self.descriptor))
        if rc != 0:
            raise ArgumentErr("PinholeModel: u, v, w must be orthonormal")
        if distortion is not None and not tsai:
            rc = _lib.load().vwgpu_camera_set_lens(ctypes.byref(self.descriptor), distortion.KIND, distortion.params.ctypes.data,
                                                   int(distortion.params.size))
            if rc != 0:
                raise ArgumentErr("PinholeModel: the parameters of the %s lens are refused" % distortion.name())
        self.matrix = np.empty((3, 4), np.float64)
        rc = _lib.load().vwgpu_pinhole_camera_matrix(
            self.center.ctypes.data, self.rotation.ctypes.data, self.fu, self.fv, self.cu, self.cv, self.u.ctypes.data,
            self.v.ctypes.data, self.w.ctypes.data, self.pixel_pitch, DISTORTION_TSAI if tsai else DISTORTION_NULL,
            params.ctypes.data if params is not None else None, self.matrix.ctypes.data)
        if rc != 0:
            raise ArgumentErr("PinholeModel: u, v, w must be orthonormal")

    def camera_center(self, pix=None):
        return self.center.copy()

    def camera_matrix(self):
        """The 3 x 4 matrix K [uvw R^T | -uvw R^T C] of rebuild_camera_matrix (src/vw/Camera/PinholeModel.cc:593-603), in the
        bits the reference's products give (vwgpu_pinhole_camera_matrix): what the device projects with."""
        return self.matrix.copy()

    def focal_length(self):
        return np.array([self.fu, self.fv])

    def point_offset(self):
        return np.array([self.cu, self.cv])

    def set_point_offset(self, offset):
        """PinholeModel::set_point_offset: the descriptor and the camera matrix are rebuilt."""
        self.__init__(self.center, self.rotation, self.fu, self.fv, offset[0], offset[1], self.u, self.v, self.w, self.distortion,
                      self.pixel_pitch)

    def point_to_pixel(self, point):
        """PinholeModel::point_to_pixel without its round-trip check (src/vw/Camera/PinholeModel.cc:370-413); LogicErr where
        the lens's distorted_coordinates does not converge."""
        q = self.camera_matrix() @ np.append(_vec3(point, "point_to_pixel: the point"), 1.0)
        pix = q[:2] / q[2]
        if self.distortion is not None:
            pix = self.distortion.distorted_coordinates(self, pix)
        return pix / self.pixel_pitch

    def pixel_to_vector(self, pix):
        """PinholeModel::pixel_to_vector (src/vw/Camera/PinholeModel.cc:422-430)."""
        u = np.array(pix, np.float64).reshape(2) * self.pixel_pitch
        if self.distortion is not None:
            u = LensDistortion.undistorted_coordinates(self.distortion, self, u)
        m, x, y = list(self.descriptor.inv_camera_transform), float(u[0]), float(u[1])
        v = [0.0 + m[3 * i] * x + m[3 * i + 1] * y + m[3 * i + 2] * 1.0 for i in range(3)]       # a dot_prod per row, from zero
        n = float(np.sqrt(0.0 + v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
        return np.array([v[0] / n, v[1] / n, v[2] / n])

    @classmethod
    def read(cls, path):
        """PinholeModel::read (src/vw/Camera/PinholeModel.cc:119-304): a .tsai file of any version, with or without the
        PINHOLE line, the pitch line and the name of the lens (an old file without a name holds Tsai parameters)."""
        try:
            with open(path) as f:
                lines = f.read().split("\n")
        except OSError as e:
            raise IOErr("PinholeModel::read_file: Could not open file: %s (%s)" % (path, e))
        k, version = 0, 1
        if "VERSION" in lines[0]:
            m = re.match(r"VERSION_(\d+)", lines[0])
            version = int(m.group(1)) if m else 1
            k = 1
            if version == 4:
                if len(lines) < 2 or "PINHOLE" not in lines[1]:
                    raise ArgumentErr("PinholeModel::read_file: Expected PINHOLE type, but got type %s" % (lines[1] if len(lines) > 1 else ""))
                k = 2
        elif re.match(r"fu\s*=", lines[0]) is None:
            raise IOErr("PinholeModel::read_file(): A Pinhole camera file must start either with the VERSION line or the focal "
                        "length. Got instead:\n%s\n" % lines[0])
        vals = {}
        for name, count in (("fu", 1), ("fv", 1), ("cu", 1), ("cv", 1), ("u_direction", 3), ("v_direction", 3), ("w_direction", 3),
                            ("C", 3), ("R", 9)):
            t = lines[k].replace("=", " = ").split() if k < len(lines) else []
            try:
                if t[:2] != [name, "="] or len(t) < 2 + count:
                    raise ValueError
                vals[name] = [float(x) for x in t[2:2 + count]]
            except ValueError:
                raise IOErr("PinholeModel::read_file(): Could not read %s" % name)
            k += 1
        pitch = 1.0
        if k < len(lines) and "pitch" in lines[k]:
            try:
                pitch = float(lines[k].replace("=", " ").split()[1])
            except (ValueError, IndexError):
                raise IOErr("PinholeModel::read_file(): Could not read the pixel pitch")
            k += 1
        elif version > 2:
            raise IOErr("PinholeModel::read_file(): Pitch value required in this file version!")
        # construct_lens_distortion (:264-304): the first name the line holds, whatever its case, in the reference's order
        line = lines[k].lower() if k < len(lines) else ""
        lens = None
        for name, kind in (("NULL", None), ("BrownConrady", BrownConradyDistortion), ("AdjustableTSAI", AdjustableTsaiLensDistortion),
                           ("Photometrix", PhotometrixLensDistortion), ("RPC", "RPC"), ("FOV", FovLensDistortion),
                           ("FISHEYE", FisheyeLensDistortion), ("TSAI", TsaiLensDistortion)):
            if name.lower() in line:
                lens = (kind,)
                break
        if lens is None:
            if version > 2:
                raise IOErr("PinholeModel::read_file(): Distortion name required in this file version!")
            lens = (TsaiLensDistortion,)
        else:
            k += 1
        if lens[0] == "RPC":
            raise NoImplErr("PinholeModel::read_file(): the RPC lens distortion is not implemented")
        distortion = lens[0].read(lines[k:]) if lens[0] is not None else None
        return cls(vals["C"], np.array(vals["R"]).reshape(3, 3), vals["fu"][0], vals["fv"][0], vals["cu"][0], vals["cv"][0],
                   vals["u_direction"], vals["v_direction"], vals["w_direction"], distortion, pitch)

    def write(self, path):
        """PinholeModel::write (src/vw/Camera/PinholeModel.cc:306-347): VERSION_4 with 17 significant digits, into `path` with
        the extension .tsai; returns the path written."""
        path = re.sub(r"\.[^./\\]*$", "", str(path)) + ".tsai" if re.search(r"\.[^./\\]*$", str(path)) else str(path) + ".tsai"

        def row(v):
            return " ".join(_g17(x) for x in np.array(v).reshape(-1))
        try:
            with open(path, "w") as f:
                f.write("VERSION_4\nPINHOLE\n")
                f.write("fu = %s\nfv = %s\ncu = %s\ncv = %s\n" % tuple(_g17(x) for x in (self.fu, self.fv, self.cu, self.cv)))
                f.write("u_direction = %s\nv_direction = %s\nw_direction = %s\n" % (row(self.u), row(self.v), row(self.w)))
                f.write("C = %s\nR = %s\npitch = %s\n" % (row(self.center), row(self.rotation), _g17(self.pixel_pitch)))
                f.write("%s\n" % (self.distortion.name() if self.distortion is not None else "NULL"))
                if self.distortion is not None:
                    self.distortion.write(f)
        except OSError as e:
            raise IOErr("PinholeModel::write: Could not open file: %s (%s)" % (path, e))
        return path


class CAHVModel(object):
    """vw::camera::CAHVModel(C, A, H, V) (src/vw/Camera/CAHVModel.h)."""

    def __init__(self, C, A, H, V):
        self.C, self.A, self.H, self.V = (_vec3(x, "CAHVModel: " + n) for x, n in ((C, "C"), (A, "A"), (H, "H"), (V, "V")))
        d = self.descriptor = _lib.Camera()
        d.kind = CAMERA_CAHV
        d.center[:] = self.C
        d.A[:] = self.A
        d.H[:] = self.H
        d.V[:] = self.V

    def camera_center(self, pix=None):
        return self.C.copy()

    def point_to_pixel(self, point):
        """CAHVModel::point_to_pixel (src/vw/Camera/CAHVModel.cc:167-171)."""
        p = _vec3(point, "point_to_pixel: the point") - self.C
        d = p @ self.A
        return np.array([p @ self.H / d, p @ self.V / d])


def _read_vectors(path, names, who):
    """The `X = a b c` lines of the reference's camera files in the order `names`, after anything that precedes `C =`
    (src/vw/Camera/CAHVORModel.cc:30-78)."""
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise IOErr("%s: Could not read file: %s (%s)" % (who, path, e))
    start = re.search(r"C\s*=", text)
    if start is None:
        raise IOErr("%s: Could not read file: %s" % (who, path))
    tokens = text[start.start():].replace("=", " = ").split()
    out, k = {}, 0
    for name, count in names:
        if tokens[k:k + 2] != [name, "="] or len(tokens) < k + 2 + count:
            raise IOErr("%s: Could not read %s vector" % (who, name))
        try:
            out[name] = [float(t) for t in tokens[k + 2:k + 2 + count]]
        except ValueError:
            raise IOErr("%s: Could not read %s vector" % (who, name))
        k += 2 + count
    return out


def _g20(v):
    return "%.20g" % v          # std::ofstream with precision(20)


def _write_vectors(path, rows, who):
    try:
        with open(path, "w") as f:
            for name, v in rows:
                f.write("%s = %s\n" % (name, " ".join(_g20(x) for x in np.atleast_1d(v))))
    except OSError as e:
        raise IOErr("%s: Could not write file: %s (%s)" % (who, path, e))


def _normalize(v):
    return v / np.sqrt(v @ v)


class CAHVORModel(object):
    """vw::camera::CAHVORModel(C, A, H, V, O, R) (src/vw/Camera/CAHVORModel.h): CAHV with radial distortion about the axis O
    with the coefficients R.  The rays and projections of the device are the reference's bits; pixel_to_vector and
    point_to_pixel here are a host convenience in numpy."""

    def __init__(self, C, A, H, V, O, R):
        self.C, self.A, self.H, self.V, self.O, self.R = (_vec3(x, "CAHVORModel: " + n) for x, n in zip((C, A, H, V, O, R), "CAHVOR"))
        self.descriptor = _lib.Camera()
        rc = _lib.load().vwgpu_cahvor_camera(self.C.ctypes.data, self.A.ctypes.data, self.H.ctypes.data, self.V.ctypes.data,
                                             self.O.ctypes.data, self.R.ctypes.data, ctypes.byref(self.descriptor))
        if rc != 0:
            raise ArgumentErr("CAHVORModel: bad arguments")

    def type(self):
        return "CAHVOR"

    def camera_center(self, pix=None):
        return self.C.copy()

    def pixel_to_vector(self, pix):
        """CAHVORModel::pixel_to_vector (src/vw/Camera/CAHVORModel.cc:297-348)."""
        rr = _normalize(np.cross(self.V - pix[1] * self.A, self.H - pix[0] * self.A))
        if np.cross(self.V, self.H) @ self.A < 0:
            rr = -rr
        omega = rr @ self.O
        lam = rr - omega * self.O
        tau = lam @ lam / (omega * omega)
        k1, k3, k5 = 1 + self.R[0], self.R[1] * tau, self.R[2] * tau * tau
        u = 1.0 - (self.R[0] + k3 + k5)
        for _ in range(20):
            u2 = u * u
            poly = ((k5 * u2 + k3) * u2 + k1) * u - 1
            deriv = (5 * k5 * u2 + 3 * k3) * u2 + k1
            if deriv <= 0:
                break
            du = poly / deriv
            u -= du
            if abs(du) < 1e-6:
                break
        return _normalize(rr - (1 - u) * lam)

    def point_to_pixel(self, point):
        """CAHVORModel::point_to_pixel (src/vw/Camera/CAHVORModel.cc:431-448)."""
        vec = _vec3(point, "point_to_pixel: the point") - self.C
        omega = vec @ self.O
        lam = vec - omega * self.O
        tau = lam @ lam / (omega * omega)
        mu = self.R[0] + self.R[1] * tau + self.R[2] * tau * tau
        pp = vec + mu * lam
        alpha = pp @ self.A
        return np.array([pp @ self.H / alpha, pp @ self.V / alpha])

    @classmethod
    def read(cls, path):
        """CAHVORModel(filename) (src/vw/Camera/CAHVORModel.cc:30-78)."""
        v = _read_vectors(path, [(n, 3) for n in "CAHVOR"], "CAHVORModel")
        return cls(*(v[n] for n in "CAHVOR"))

    def write(self, path):
        """CAHVORModel::write (src/vw/Camera/CAHVORModel.cc:93-112): 20 significant digits."""
        _write_vectors(path, [(n, getattr(self, n)) for n in "CAHVOR"], "CAHVORModel")


class CAHVOREModel(object):
    """vw::camera::CAHVOREModel(C, A, H, V, O, R, E, T, P) (src/vw/Camera/CAHVOREModel.cc:105-132): the fisheye member of the
    family, with the moving entrance pupil E and the linearity P.  T = 1 (perspective) sets P = 1, T = 2 (fisheye) sets
    P = 0, T = 3 (general) takes P; without T, P itself is given.  P outside [0, 1] or another T raises ArgumentErr."""

    def __init__(self, C, A, H, V, O, R, E, T=None, P=1.0):
        names = "CAHVORE"
        self.C, self.A, self.H, self.V, self.O, self.R, self.E = (_vec3(x, "CAHVOREModel: " + n) for x, n in zip((C, A, H, V, O, R, E), names))
        T = 3 if T is None else T
        if T not in (1, 2, 3):
            raise ArgumentErr("Unknown CAHVORE type: %r" % (T,))
        self.descriptor = _lib.Camera()
        rc = _lib.load().vwgpu_cahvore_camera(self.C.ctypes.data, self.A.ctypes.data, self.H.ctypes.data, self.V.ctypes.data,
                                              self.O.ctypes.data, self.R.ctypes.data, self.E.ctypes.data, int(T), float(P),
                                              ctypes.byref(self.descriptor))
        if rc != 0:
            raise ArgumentErr("Invalid P value: %r" % (P,))
        self.P = float(self.descriptor.distortion[0])

    def type(self):
        return "CAHVORE"

    def camera_center(self, pix=None):
        return self.C.copy()

    def pixel_to_vector(self, pix):
        """CAHVOREModel::pixel_to_vector (src/vw/Camera/CAHVOREModel.cc:167-228); LogicErr where it does not converge."""
        w3 = np.cross(self.V - pix[1] * self.A, self.H - pix[0] * self.A)
        rp = w3 / (self.A @ np.cross(self.V, self.H))
        zetap = rp @ self.O
        lam3 = rp - zetap * self.O
        chip = np.sqrt(lam3 @ lam3) / zetap
        if chip < 1e-8:
            return self.O.copy()
        chi, dchi, R = chip, 1.0, self.R
        for n in range(102):
            if n > 100:
                raise LogicErr("CAHVOREModel: Did not converge.")
            if abs(dchi) < 1e-8:
                break
            with np.errstate(all="ignore"):
                deriv = (1 + R[0]) + 3 * R[1] * chi ** 2 + 5 * R[2] * chi ** 4
                dchi = ((1 + R[0]) * chi + R[1] * chi ** 3 + R[2] * chi ** 5 - chip) / deriv
            chi -= dchi
        P = self.P
        theta = np.arcsin(P * chi) / P if P < -1e-15 else np.arctan(P * chi) / P if P > 1e-15 else chi
        return np.sin(theta) * _normalize(lam3) + np.cos(theta) * self.O

    def point_to_pixel(self, point):
        """CAHVOREModel::point_to_pixel (src/vw/Camera/CAHVOREModel.cc:232-301); LogicErr where it throws."""
        p_c = _vec3(point, "point_to_pixel: the point") - self.C
        zeta = p_c @ self.O
        lam3 = p_c - zeta * self.O
        lam = np.sqrt(lam3 @ lam3)
        theta, dtheta, E, R, P = np.arctan2(lam, zeta), 1.0, self.E, self.R, self.P
        for n in range(102):
            if n > 100:
                raise LogicErr("CAHVOREModel: Did not converge.")
            if abs(dtheta) < 1e-8:
                break
            c, s, t2, t3, t4 = np.cos(theta), np.sin(theta), theta ** 2, theta ** 3, theta ** 4
            ups = zeta * c + lam * s - (1 - c) * (E[0] + E[1] * t2 + E[2] * t4) - (theta - s) * (2 * E[1] * theta + 4 * E[2] * t3)
            dtheta = (zeta * s - lam * c - (theta - s) * (E[0] + E[1] * t2 + E[2] * t4)) / ups
            theta -= dtheta
        if theta * abs(P) > np.pi / 2:
            raise LogicErr("CAHVOREModel: Theta out of bounds.")
        if theta < 1e-8:
            rp = p_c
        else:
            chi = np.sin(P * theta) / P if P < -1e-15 else np.tan(P * theta) / P if P > 1e-15 else theta
            mu = R[0] + chi * chi * (R[1] + chi * chi * R[2])
            rp = (lam / chi) * self.O + (1 + mu) * lam3
        alpha = rp @ self.A
        return np.array([rp @ self.H / alpha, rp @ self.V / alpha])

    @classmethod
    def read(cls, path):
        """CAHVOREModel(filename) (src/vw/Camera/CAHVOREModel.cc:38-103)."""
        v = _read_vectors(path, [(n, 3) for n in "CAHVORE"] + [("T", 1), ("P", 1)], "CAHVOREModel")
        t = v["T"][0]
        if t != int(t):
            raise IOErr("CAHVOREModel: could not read T element")
        return cls(*(v[n] for n in "CAHVORE"), T=int(t), P=v["P"][0])

    def write(self, path):
        """CAHVOREModel::write (src/vw/Camera/CAHVOREModel.cc:139-165): the T line follows P (0 -> 2, 1 -> 1, else 3)."""
        t = 2 if self.P == 0 else 1 if self.P == 1 else 3
        _write_vectors(path, [(n, getattr(self, n)) for n in "CAHVORE"] + [("T", t), ("P", self.P)], "CAHVOREModel")


def linearize_camera(model, in_size, out_size=None):
    """vw::camera::linearize_camera(model, in_size, out_size) for a CAHVORModel (src/vw/Camera/CAHVORModel.cc:460-547) or a
    CAHVOREModel (src/vw/Camera/CAHVOREModel.cc:303-381): the CAHVModel with the same centre that covers the common field
    of view of a frame of in_size = (cols, rows), for an image of out_size (in_size by default).  A CAHVORE landmark ray
    that does not converge raises LogicErr.  Host arithmetic in the library, no GPU."""
    if not isinstance(model, (CAHVORModel, CAHVOREModel)):
        raise ArgumentErr("linearize_camera: expected a CAHVORModel or a CAHVOREModel")
    out_size = in_size if out_size is None else out_size
    d = _lib.Camera()
    rc = _lib.load().vwgpu_linearize_camera(ctypes.byref(model.descriptor), int(in_size[0]), int(in_size[1]), int(out_size[0]),
                                            int(out_size[1]), ctypes.byref(d))
    if rc == -5:
        raise LogicErr("CAHVOREModel: Did not converge.")
    if rc != 0:
        raise ArgumentErr("linearize_camera: the sizes must be positive")
    return CAHVModel(list(d.center), list(d.A), list(d.H), list(d.V))


def linearize_camera_transform(image, src, mask=None, edge=(0, False), ctx=None):
    """linearize_camera_transform(image, src_camera, edge, BilinearInterpolation()) (src/vw/Camera/CameraTransform.h:185-225):
    the image of a CAHVORModel or CAHVOREModel as its own linearisation at the image's size sees it.  Returns
    (image, cahv) or, with a mask, (image, mask, cahv)."""
    if image.ndim != 2:
        raise ArgumentErr("linearize_camera_transform: the image must be (rows, cols)")
    size = (int(image.shape[1]), int(image.shape[0]))
    cahv = linearize_camera(src, size, size)
    out = camera_transform(image, src, cahv, mask=mask, edge=edge, ctx=ctx)
    return out + (cahv,) if mask is not None else (out, cahv)


def descriptor_of(camera):
    """The struct vwgpu_camera of a camera model, or the structure itself."""
    if isinstance(camera, _lib.Camera):
        return camera
    d = getattr(camera, "descriptor", None)
    if not isinstance(d, _lib.Camera):
        raise ArgumentErr("expected a PinholeModel, a CAHV, CAHVOR or CAHVORE model or a camera descriptor, not %r" % (camera,))
    return d


def matrix_of(camera):
    """The camera matrix that goes beside a descriptor: a (3, 4) float64 array for a PinholeModel, None for the CAHV family."""
    return getattr(camera, "matrix", None)


def _ptr(a):
    return None if a is None else a.ctypes.data


def epipolar(cam0, cam1):
    """vw::camera::epipolar(src0, src1, dst0, dst1) for two PinholeModels (src/vw/Camera/PinholeModel.cc:679-732) or two
    CAHVModels (src/vw/Camera/CAHVModel.cc:297-337): the two rectified cameras.  Cameras without a baseline raise
    ArgumentErr.  Host arithmetic in the library, no GPU."""
    lib = _lib.load()
    if isinstance(cam0, PinholeModel) and isinstance(cam1, PinholeModel):
        rot, focal, offset, pitch = np.empty((3, 3)), np.empty(2), np.empty(2), ctypes.c_double(0)
        f0, o0, f1, o1 = cam0.focal_length(), cam0.point_offset(), cam1.focal_length(), cam1.point_offset()
        rc = lib.vwgpu_epipolar_pinhole(cam0.center.ctypes.data, cam0.rotation.ctypes.data, f0.ctypes.data, o0.ctypes.data, cam0.pixel_pitch,
                                        cam1.center.ctypes.data, cam1.rotation.ctypes.data, f1.ctypes.data, o1.ctypes.data, cam1.pixel_pitch,
                                        rot.ctypes.data, focal.ctypes.data, offset.ctypes.data, ctypes.addressof(pitch))
        if rc != 0:
            raise ArgumentErr("epipolar: the two cameras have the same centre")
        return tuple(PinholeModel(c.center, rot, focal[0], focal[1], offset[0], offset[1], pixel_pitch=pitch.value) for c in (cam0, cam1))
    if isinstance(cam0, CAHVModel) and isinstance(cam1, CAHVModel):
        d0, d1 = _lib.Camera(), _lib.Camera()
        rc = lib.vwgpu_epipolar_cahv(ctypes.byref(cam0.descriptor), ctypes.byref(cam1.descriptor), ctypes.byref(d0), ctypes.byref(d1))
        if rc != 0:
            raise ArgumentErr("epipolar: the two cameras have the same centre")
        return tuple(CAHVModel(list(d.center), list(d.A), list(d.H), list(d.V)) for d in (d0, d1))
    raise ArgumentErr("epipolar: expected two PinholeModels or two CAHVModels")


FORWARD, REVERSE = 0, 1


class CameraTransform(object):
    """vw::camera::CameraTransform<Src, Dst>(src, dst) (src/vw/Camera/CameraTransform.h:43-79) for arrays of points:
    forward maps pixels of src to pixels of dst, reverse the other way; both on the device.  The two cameras must share
    their centre (LogicErr otherwise).  check: PinholeModel::set_do_point_to_pixel_check of the camera projected into; a
    point that fails it raises LogicErr for numpy points, and becomes a NaN pair for tensors."""

    def __init__(self, src, dst, check=True, ctx=None):
        self.src, self.dst, self.check, self.ctx = src, dst, bool(check), ctx

    def _run(self, direction, points):
        ops = Operands("CameraTransform", points, self.ctx)
        p = ops.image(points, np.float64)
        if p.ndim < 1 or int(p.shape[-1]) != 2:
            raise ArgumentErr("CameraTransform: the points must be (..., 2) {x, y}")
        n = 1
        for k in p.shape[:-1]:
            n *= int(k)
        if n <= 0:
            raise ArgumentErr("CameraTransform: no points")
        out = ops.empty(tuple(p.shape), np.float64)
        ops.call("camera_transform_points", ctypes.byref(descriptor_of(self.src)), _ptr(matrix_of(self.src)),
                 ctypes.byref(descriptor_of(self.dst)), _ptr(matrix_of(self.dst)), direction, int(self.check), ops.ptr(p), n, ops.ptr(out),
                 None)
        return out

    def forward(self, points):
        return self._run(FORWARD, points)

    def reverse(self, points):
        return self._run(REVERSE, points)


def camera_transform(image, src, dst, size=None, mask=None, edge=(0, False), x0=0, y0=0, check=True, ctx=None, failed=None):
    """camera_transform(image, src_camera, dst_camera, size, edge, BilinearInterpolation()) rasterised
    (src/vw/Camera/CameraTransform.h:123-183): the (rows, cols) float32 image as the camera dst sees it.  size: (cols, rows)
    of the result, the image's own by default; x0, y0: the image coordinates of its pixel (0, 0).  mask: an optional
    validity mask of the image (PixelMask<float>); the result is then (image, uint8 mask 255 / 0), valid where every tap
    is.  edge = (value, valid): the ValueEdgeExtension pixel; (0, False) is ZeroEdgeExtension.  check: the source
    PinholeModel's point-to-pixel check (on by default, as in the reference); a failing pixel becomes the edge pixel, and
    a numpy call then raises LogicErr with the reference's message, where a tensor call goes on without synchronising.
    The same holds where a CAHVOREModel on either side throws (no convergence, theta out of bounds).  A CAHVORModel or
    CAHVOREModel goes with a CAHVModel, in either role; any other pair with one of them raises NoImplErr.
    failed: an int64[1] CUDA tensor that receives the count of such pixels.  numpy in -> numpy out, CUDA tensors in -> CUDA
    tensors out on the current torch stream."""
    ops = Operands("camera_transform", image, ctx)
    if image.ndim != 2:
        raise ArgumentErr("camera_transform: the image must be (rows, cols)")
    img = ops.image(image, np.float32, rows=True)
    sh, sw = int(img.shape[0]), int(img.shape[1])
    m = ops.nonzero_u8(mask, same_device=True)
    if m is not None and tuple(m.shape) != (sh, sw):
        raise ArgumentErr("camera_transform: the mask must have the image's shape")
    w, h = (sw, sh) if size is None else (int(size[0]), int(size[1]))
    if sw <= 0 or sh <= 0 or w <= 0 or h <= 0:
        raise ArgumentErr("camera_transform: empty image")
    out = ops.empty((h, w), np.float32)
    out_mask = ops.empty((h, w), np.uint8) if m is not None else None
    cnt = None
    if failed is not None:
        if not ops.tensor:
            raise ArgumentErr("camera_transform: failed is an int64[1] CUDA tensor, with a CUDA image")
        cnt = ops.ptr(ops.image(failed, np.int64, in_place=True))
    ops.call("camera_transform", ops.ptr(img), sw, sh, ops.row_stride(img), ops.ptr(m), 0, ctypes.byref(descriptor_of(src)),
             _ptr(matrix_of(src)), ctypes.byref(descriptor_of(dst)), _ptr(matrix_of(dst)), w, h, int(x0), int(y0), float(edge[0]),
             int(bool(edge[1])), int(bool(check)), ops.ptr(out), 0, ops.ptr(out_mask), 0, cnt)
    return out if m is None else (out, out_mask)


def _roi_perimeter(roi):
    """The points compute_transformed_bbox_fast visits (src/vw/Image/Transform.h:279-301), in its order."""
    x0, y0, x1, y1 = roi.min[0], roi.min[1], roi.max[0], roi.max[1]
    xs, ys = np.arange(x0, x1, dtype=np.float64), np.arange(y0, y1, dtype=np.float64)
    return np.concatenate([np.stack([xs, np.full_like(xs, y0)], 1), np.stack([xs, np.full_like(xs, y1 - 1)], 1),
                           np.stack([np.full_like(ys, x0), ys], 1), np.stack([np.full_like(ys, x1 - 1), ys], 1)])


def compute_transformed_bbox_fast(roi, transform):
    """compute_transformed_bbox_fast(roi, transform) (src/vw/Image/Transform.h:272-315): (min, max) of the BBox2f grown by
    the forward-transformed perimeter of the BBox2i roi; the box is float, a coordinate is compared in double and stored
    rounded to float (src/vw/Math/BBox.tcc:82-97)."""
    pts = np.asarray(transform.forward(_roi_perimeter(roi)))
    fmax = np.finfo(np.float32).max
    lo, hi = np.array([fmax, fmax], np.float32), np.array([-fmax, -fmax], np.float32)    # BBox(): empty
    for p in pts:
        for i in (0, 1):
            if p[i] > float(hi[i]):
                hi[i] = np.float32(p[i])
            if p[i] < float(lo[i]):
                lo[i] = np.float32(p[i])
    return lo, hi


def resize_epipolar_cameras_to_fit(cam1, cam2, epi1, epi2, roi1, roi2, ctx=None):
    """vw::camera::resize_epipolar_cameras_to_fit (src/vw/Camera/EpipolarUtils.cc:37-76): shifts the point offset of the two
    rectified pinholes so that the transformed ROIs (BBox2i) begin at column and row 0; returns (epi1, epi2, size1, size2)
    with the new cameras and the (cols, rows) needed to hold each transformed image."""
    boxes = [compute_transformed_bbox_fast(roi, CameraTransform(c, e, ctx=ctx)) for c, e, roi in ((cam1, epi1, roi1), (cam2, epi2, roi2))]
    min_col = min(float(boxes[0][0][0]), float(boxes[1][0][0]))
    min_row = min(float(boxes[0][0][1]), float(boxes[1][0][1]))
    point_offset = epi1.point_offset()
    center_adjust = np.array([min_col, min_row]) * epi1.pixel_pitch
    new = []
    for e in (epi1, epi2):
        n = PinholeModel(e.center, e.rotation, e.fu, e.fv, e.cu, e.cv, e.u, e.v, e.w, e.distortion, e.pixel_pitch)
        n.set_point_offset(point_offset - center_adjust)
        new.append(n)
    sizes = []
    for c, e, roi in ((cam1, new[0], roi1), (cam2, new[1], roi2)):
        _, hi = compute_transformed_bbox_fast(roi, CameraTransform(c, e, ctx=ctx))
        sizes.append((int(hi[0]), int(hi[1])))       # Vector2i = a float vector: truncation
    return new[0], new[1], sizes[0], sizes[1]


__all__ = ["PinholeModel", "LensDistortion", "TsaiLensDistortion", "FovLensDistortion", "FisheyeLensDistortion", "BrownConradyDistortion",
           "AdjustableTsaiLensDistortion", "PhotometrixLensDistortion", "CAHVModel", "CAHVORModel", "CAHVOREModel", "linearize_camera",
           "linearize_camera_transform", "descriptor_of", "matrix_of", "epipolar", "CameraTransform",
           "camera_transform", "compute_transformed_bbox_fast", "resize_epipolar_cameras_to_fit", "BBox2i"]
