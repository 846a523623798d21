// camera_rays.h — the part of vw::camera the kernels share: the small fp64 vector helpers in the reference's expression
// order and pixel_to_vector of PinholeModel with the null and the Tsai lens (src/vw/Camera/PinholeModel.cc:422-434,
// src/vw/Camera/LensDistortion.cc:260-400 over src/vw/Math/NewtonRaphson.cc:58-119) and of CAHVModel
// (src/vw/Camera/CAHVModel.cc:173-189).  Used by triangulate.hip and camera_transform.hip; internal linkage, so every
// translation unit compiles its own copy.
#pragma once
#include <cmath>

#include "vwgpu_internal.h"

namespace {

// which code a kernel carries for one camera: a pinhole without lens distortion, a pinhole whose distortion kind is read
// at run time, CAHV
enum { TR_CAM_PINHOLE_NULL = 0, TR_CAM_PINHOLE = 1, TR_CAM_CAHV = 2 };

struct tr_v3 { double x, y, z; };
struct tr_v2 { double x, y; };

__host__ __device__ inline double tr_dot(const tr_v3& a, const tr_v3& b) { return 0.0 + a.x * b.x + a.y * b.y + a.z * b.z; }
__host__ __device__ inline tr_v3 tr_cross(const tr_v3& a, const tr_v3& b) {
  return tr_v3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__host__ __device__ inline tr_v3 tr_sub(const tr_v3& a, const tr_v3& b) { return tr_v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ inline double tr_norm(const tr_v3& a) { return sqrt(0.0 + a.x * a.x + a.y * a.y + a.z * a.z); }
__host__ __device__ inline double tr_norm(const tr_v2& a) { return sqrt(0.0 + a.x * a.x + a.y * a.y); }
__host__ __device__ inline tr_v3 tr_normalize(const tr_v3& a) {
  const double n = tr_norm(a);
  return tr_v3{a.x / n, a.y / n, a.z / n};
}
__host__ __device__ inline tr_v3 tr_load3(const double* p) { return tr_v3{p[0], p[1], p[2]}; }

// TsaiDistortionNorm (LensDistortion.cc:260-276)
__device__ inline tr_v2 tr_tsai_norm(const tr_v2& P, const double* distortion) {
  double x = P.x;
  double y = P.y;
  double k1 = distortion[0];
  double k2 = distortion[1];
  double p1 = distortion[2];
  double p2 = distortion[3];
  double k3 = distortion[4];
  double r2 = x * x + y * y;
  double rdist = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
  double x_out = x * rdist + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x));
  double y_out = y * rdist + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y);
  return tr_v2{x_out, y_out};
}

// TsaiDistortionJacobian (LensDistortion.cc:286-324)
__device__ inline void tr_tsai_jacobian(const tr_v2& P, const double* distortion, double* jacobian) {
  double x = P.x;
  double y = P.y;
  double k1 = distortion[0];
  double k2 = distortion[1];
  double p1 = distortion[2];
  double p2 = distortion[3];
  double k3 = distortion[4];
  double r2 = x * x + y * y;
  double dr2dx = 2.0 * x;
  double dr2dy = 2.0 * y;
  double rdist = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
  jacobian[0] = rdist
              + x * (k1 * dr2dx + k2 * dr2dx * 2.0 * r2 + k3 * dr2dx * 3.0 * r2 * r2)
              + 2.0 * p1 * y + p2 * (dr2dx + 4.0 * x);
  jacobian[1] = x * (k1 * dr2dy + k2 * dr2dy * 2.0 * r2 + k3 * dr2dy * 3.0 * r2 * r2)
              + 2.0 * p1 * x  + p2 * dr2dy;
  jacobian[2] = y * (k1 * dr2dx + k2 * dr2dx * 2.0 * r2 + k3 * dr2dx * 3.0 * r2 * r2)
              + (p1 * dr2dx + 2.0 * p2 * y);
  jacobian[3] = rdist
              + y * (k1 * dr2dy + k2 * dr2dy * 2.0 * r2 + k3 * dr2dy * 3.0 * r2 * r2)
              + p1 * (dr2dy + 4.0 * y) + 2.0 * p2 * x;
}

// NewtonRaphson::solve (NewtonRaphson.cc:58-119) with guessX = outY = the normalised distorted pixel, tol = 1e-9
__device__ inline tr_v2 tr_newton_tsai(const tr_v2& outY, const double* distortion) {
  tr_v2 X = outY;
  tr_v2 bestX = X;
  double best_err = 1.7976931348623157e308;   // std::numeric_limits<double>::max()
  int count = 1;
  const int maxTries = 20;
  while (count < maxTries) {
    const tr_v2 FX = tr_tsai_norm(X, distortion);
    const tr_v2 F{FX.x - outY.x, FX.y - outY.y};
    const double nF = tr_norm(F);
    if (nF != nF) return bestX;
    if (nF < best_err) {
      best_err = nF;
      bestX = X;
    }
    double J[4];
    tr_tsai_jacobian(X, distortion, J);
    const double det = J[0] * J[3] - J[1] * J[2];
    if (fabs(det) < 1e-6 || det != det) return bestX;
    tr_v2 DX;
    DX.x = (J[3] * F.x - J[1] * F.y) / det;
    DX.y = (J[0] * F.y - J[2] * F.x) / det;
    X.x = X.x - DX.x;
    X.y = X.y - DX.y;
    if (tr_norm(DX) < 1e-9) return X;
    count++;
  }
  return bestX;
}

// TsaiLensDistortion::undistorted_coordinates (LensDistortion.cc:371-400)
__device__ inline tr_v2 tr_tsai_undistort(const vwgpu_camera& c, const tr_v2& p) {
  if (c.fu < 1e-300 || c.fv < 1e-300) return tr_v2{HUGE_VAL, HUGE_VAL};
  const tr_v2 p0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const tr_v2 U = tr_newton_tsai(p0, c.distortion);
  double ux = U.x, uy = U.y;
  ux = ux * c.fu + c.cu;
  uy = uy * c.fv + c.cv;
  return tr_v2{ux, uy};
}

// pixel_to_vector of the camera kinds a kernel carries
// `flip`: the handedness test of CAHVModel::pixel_to_vector, dot(cross(V, H), A) < 0 — the same for every pixel, so the
// host evaluates it once (tr_cahv_flips)
template <int CAM>
__device__ inline tr_v3 tr_ray(const vwgpu_camera& c, const tr_v2& pix, bool flip) {
  if (CAM == TR_CAM_CAHV) {
    // CAHVModel::pixel_to_vector (CAHVModel.cc:173-185)
    const tr_v3 A = tr_load3(c.A), H = tr_load3(c.H), V = tr_load3(c.V);
    const tr_v3 a{V.x - pix.y * A.x, V.y - pix.y * A.y, V.z - pix.y * A.z};
    const tr_v3 b{H.x - pix.x * A.x, H.y - pix.x * A.y, H.z - pix.x * A.z};
    tr_v3 vec = tr_normalize(tr_cross(a, b));
    if (flip) {
      vec.x *= -1.0;
      vec.y *= -1.0;
      vec.z *= -1.0;
    }
    return vec;
  }
  // PinholeModel::pixel_to_vector (PinholeModel.cc:422-430)
  tr_v2 u{pix.x * c.pixel_pitch, pix.y * c.pixel_pitch};
  if (CAM != TR_CAM_PINHOLE_NULL && c.distortion_kind == VWGPU_DISTORTION_TSAI) u = tr_tsai_undistort(c, u);
  const tr_v3 p{u.x, u.y, 1.0};
  const double* m = c.inv_camera_transform;
  return tr_normalize(tr_v3{tr_dot(tr_load3(m), p), tr_dot(tr_load3(m + 3), p), tr_dot(tr_load3(m + 6), p)});
}

}  // namespace
