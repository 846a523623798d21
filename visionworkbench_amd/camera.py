"""The part of vw::camera that triangulation needs: PinholeModel with the null or the Tsai lens distortion and CAHVModel.

Each model is a host object that produces the flat camera descriptor of the C ABI (struct vwgpu_camera, include/vwgpu.h);
the rays themselves are computed on the device inside stereo.stereo_triangulate / stereo.StereoModel.  point_to_pixel and
the camera matrix are host conveniences in numpy (scene building, tests); nothing here needs a GPU.
"""
import ctypes

import numpy as np

from . import _lib
from .core import ArgumentErr

CAMERA_PINHOLE, CAMERA_CAHV = 0, 1
DISTORTION_NULL, DISTORTION_TSAI = 0, 1


def _vec3(v, what):
    a = np.array(v, np.float64).reshape(-1)
    if a.size != 3:
        raise ArgumentErr("%s must have three elements" % what)
    return np.ascontiguousarray(a)


class TsaiLensDistortion(object):
    """vw::camera::TsaiLensDistortion (src/vw/Camera/LensDistortion.cc:225-400): parameters k1, k2, p1, p2, k3."""

    def __init__(self, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
        self.params = np.array([k1, k2, p1, p2, k3], np.float64)

    def distortion_parameters(self):
        return self.params.copy()

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
    +x right, +y down, +z forward).  distortion: None (NullLensDistortion) or a TsaiLensDistortion.  u, v, w that fail the
    reference's orthonormality asserts raise ArgumentErr."""

    def __init__(self, center, rotation, fu, fv, cu, cv, u=(1, 0, 0), v=(0, 1, 0), w=(0, 0, 1), distortion=None, pixel_pitch=1.0):
        self.center = _vec3(center, "PinholeModel: the camera center")
        self.rotation = np.ascontiguousarray(np.array(rotation, np.float64))
        if self.rotation.shape != (3, 3):
            raise ArgumentErr("PinholeModel: the rotation must be 3 x 3")
        self.fu, self.fv, self.cu, self.cv = float(fu), float(fv), float(cu), float(cv)
        self.u, self.v, self.w = _vec3(u, "PinholeModel: u"), _vec3(v, "PinholeModel: v"), _vec3(w, "PinholeModel: w")
        if distortion is not None and not isinstance(distortion, TsaiLensDistortion):
            raise ArgumentErr("PinholeModel: the lens distortion must be None or a TsaiLensDistortion")
        self.distortion = distortion
        self.pixel_pitch = float(pixel_pitch)
        self.descriptor = _lib.Camera()
        params = distortion.params if distortion is not None else None
        rc = _lib.load().vwgpu_pinhole_camera(
            self.center.ctypes.data, self.rotation.ctypes.data, self.fu, self.fv, self.cu, self.cv, self.u.ctypes.data,
            self.v.ctypes.data, self.w.ctypes.data, self.pixel_pitch, DISTORTION_TSAI if distortion is not None else DISTORTION_NULL,
            params.ctypes.data if params is not None else None, ctypes.byref(self.descriptor))
        if rc != 0:
            raise ArgumentErr("PinholeModel: u, v, w must be orthonormal")

    def camera_center(self, pix=None):
        return self.center.copy()

    def camera_matrix(self):
        """The 3 x 4 matrix K [uvw R^T | -uvw R^T C] of rebuild_camera_matrix (src/vw/Camera/PinholeModel.cc:593-603)."""
        uvw = np.stack([self.u, self.v, self.w])
        ext = np.empty((3, 4))
        ext[:, :3] = uvw @ self.rotation.T
        ext[:, 3] = uvw @ (-self.rotation.T) @ self.center
        k = np.array([[self.fu, 0, self.cu], [0, self.fv, self.cv], [0, 0, 1.0]])
        return k @ ext

    def point_to_pixel(self, point):
        """PinholeModel::point_to_pixel without its round-trip check (src/vw/Camera/PinholeModel.cc:370-413)."""
        q = self.camera_matrix() @ np.append(_vec3(point, "point_to_pixel: the point"), 1.0)
        pix = q[:2] / q[2]
        if self.distortion is not None:
            pix = self.distortion.distorted_coordinates(self, pix)
        return pix / self.pixel_pitch


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


def descriptor_of(camera):
    """The struct vwgpu_camera of a camera model, or the structure itself."""
    if isinstance(camera, _lib.Camera):
        return camera
    d = getattr(camera, "descriptor", None)
    if not isinstance(d, _lib.Camera):
        raise ArgumentErr("expected a PinholeModel, a CAHVModel or a camera descriptor, not %r" % (camera,))
    return d


__all__ = ["PinholeModel", "TsaiLensDistortion", "CAHVModel", "descriptor_of"]
