// camera_rays.h — the part of vw::camera the kernels share: the small fp64 vector helpers in the reference's expression
// order and pixel_to_vector of PinholeModel with the null and the Tsai lens (src/vw/Camera/PinholeModel.cc:422-434,
// src/vw/Camera/LensDistortion.cc:260-400 over src/vw/Math/NewtonRaphson.cc:58-119) and of CAHVModel
// (src/vw/Camera/CAHVModel.cc:173-189), and both directions of CAHVORModel (src/vw/Camera/CAHVORModel.cc:297-348, :431-448)
// and CAHVOREModel (src/vw/Camera/CAHVOREModel.cc:167-301), which the host's linearize_camera runs as well.  Used by
// triangulate.hip and camera_transform.hip; internal linkage, so every translation unit compiles its own copy.
#pragma once
#include <cmath>

#include "vwgpu_internal.h"

namespace {

// which code a kernel carries for one camera: a pinhole without lens distortion, a pinhole whose distortion kind is read
// at run time, CAHV, CAHVOR, CAHVORE
enum { TR_CAM_PINHOLE_NULL = 0, TR_CAM_PINHOLE = 1, TR_CAM_CAHV = 2, TR_CAM_CAHVOR = 3, TR_CAM_CAHVORE = 4 };
// how a CAHVORE function left: its result, or one of the reference's two throws
enum { TR_OK = 0, TR_NOT_CONVERGED = 1, TR_THETA_OUT_OF_BOUNDS = 2 };

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

// the two kinds that are paired only with CAHV (camera transform) or with their own kind (triangulation)
inline bool tr_new_kind(const vwgpu_camera& c) { return c.kind == VWGPU_CAMERA_CAHVOR || c.kind == VWGPU_CAMERA_CAHVORE; }
inline const char* tr_kind_name(const vwgpu_camera& c) {
  return c.kind == VWGPU_CAMERA_CAHVORE ? "CAHVORE" : c.kind == VWGPU_CAMERA_CAHVOR ? "CAHVOR" : c.kind == VWGPU_CAMERA_CAHV ? "CAHV" : "Pinhole";
}

// O, R, E and the linearity P of a CAHVOR / CAHVORE descriptor: storage only a pinhole uses (include/vwgpu.h)
__host__ __device__ inline tr_v3 tr_cam_O(const vwgpu_camera& c) { return tr_load3(c.inv_camera_transform); }
__host__ __device__ inline tr_v3 tr_cam_R(const vwgpu_camera& c) { return tr_load3(c.inv_camera_transform + 3); }
__host__ __device__ inline tr_v3 tr_cam_E(const vwgpu_camera& c) { return tr_load3(c.inv_camera_transform + 6); }
__host__ __device__ inline double tr_cam_P(const vwgpu_camera& c) { return c.distortion[0]; }

// CAHVORModel::pixel_to_vector without partials (CAHVORModel.cc:297-348).  Neither exit of the Newton loop on
// k5 u^5 + k3 u^3 + k1 u = 1 is a failure: after 20 passes, or with deriv <= 0, the current u is used.
__host__ __device__ inline tr_v3 tr_cahvor_ray(const vwgpu_camera& c, const tr_v2& pix, bool flip) {
  const tr_v3 A = tr_load3(c.A), H = tr_load3(c.H), V = tr_load3(c.V), O = tr_cam_O(c), R = tr_cam_R(c);
  const tr_v3 a{V.x - pix.y * A.x, V.y - pix.y * A.y, V.z - pix.y * A.z};
  const tr_v3 b{H.x - pix.x * A.x, H.y - pix.x * A.y, H.z - pix.x * A.z};
  tr_v3 rr = tr_normalize(tr_cross(a, b));
  if (flip) rr = tr_v3{-1.0 * rr.x, -1.0 * rr.y, -1.0 * rr.z};
  const double omega = tr_dot(rr, O);
  const tr_v3 lambda{rr.x - omega * O.x, rr.y - omega * O.y, rr.z - omega * O.z};
  const double tau = tr_dot(lambda, lambda) / (omega * omega);
  const double k1 = 1 + R.x;
  const double k3 = R.y * tau;
  const double k5 = R.z * tau * tau;
  double u = 1.0 - (R.x + k3 + k5);
  for (int i = 0; i < 20; ++i) {
    const double u_2 = u * u;
    const double poly = ((k5 * u_2 + k3) * u_2 + k1) * u - 1;
    const double deriv = (5 * k5 * u_2 + 3 * k3) * u_2 + k1;
    if (deriv <= 0) break;
    const double du = poly / deriv;
    u -= du;
    if (fabs(du) < 1.0e-6) break;
  }
  const double s = 1 - u;
  return tr_normalize(tr_v3{rr.x - s * lambda.x, rr.y - s * lambda.y, rr.z - s * lambda.z});
}

// CAHVORModel::point_to_pixel without partials (CAHVORModel.cc:431-448): closed form
__host__ __device__ inline tr_v2 tr_cahvor_project(const vwgpu_camera& c, const tr_v3& point) {
  const tr_v3 O = tr_cam_O(c), R = tr_cam_R(c);
  const tr_v3 vec = tr_sub(point, tr_load3(c.center));
  const double omega = tr_dot(vec, O);
  const tr_v3 lambda{vec.x - omega * O.x, vec.y - omega * O.y, vec.z - omega * O.z};
  const double tau = tr_dot(lambda, lambda) / (omega * omega);
  const double mu = R.x + (R.y * tau) + (R.z * tau * tau);
  const tr_v3 pp_c{vec.x + mu * lambda.x, vec.y + mu * lambda.y, vec.z + mu * lambda.z};
  const double alpha = tr_dot(pp_c, tr_load3(c.A));
  return tr_v2{tr_dot(pp_c, tr_load3(c.H)) / alpha, tr_dot(pp_c, tr_load3(c.V)) / alpha};
}

// CAHVOREModel::pixel_to_vector (CAHVOREModel.cc:167-228).  The loop on chi tests n > 100 (the throw) before the step, so
// it makes at most 101 updates; a lane that has converged leaves the loop and idles.  E does not enter the ray.
__host__ __device__ inline int tr_cahvore_ray(const vwgpu_camera& c, const tr_v2& pix, tr_v3& result) {
  const tr_v3 A = tr_load3(c.A), H = tr_load3(c.H), V = tr_load3(c.V), O = tr_cam_O(c), R = tr_cam_R(c);
  const double P = tr_cam_P(c);
  const tr_v3 a{V.x - pix.y * A.x, V.y - pix.y * A.y, V.z - pix.y * A.z};
  const tr_v3 b{H.x - pix.x * A.x, H.y - pix.x * A.y, H.z - pix.x * A.z};
  const tr_v3 w3 = tr_cross(a, b);
  const double f = 1 / tr_dot(A, tr_cross(V, H));
  const tr_v3 rp{f * w3.x, f * w3.y, f * w3.z};
  const double zetap = tr_dot(rp, O);
  const tr_v3 lambdap3{rp.x - zetap * O.x, rp.y - zetap * O.y, rp.z - zetap * O.z};
  const double lambdap = tr_norm(lambdap3);
  const double chip = lambdap / zetap;
  result = O;
  if (chip < 1e-8) return TR_OK;   // approximations for small angles
  double chi = chip;
  double dchi = 1;
  bool converged = false;
  for (int n = 0; n <= 100; ++n) {
    if (fabs(dchi) < 1e-8) {
      converged = true;
      break;
    }
    const double chi2 = chi * chi;
    const double chi3 = chi * chi2;
    const double chi4 = chi * chi3;
    const double chi5 = chi * chi4;
    const double deriv = (1 + R.x) + 3 * R.y * chi2 + 5 * R.z * chi4;
    dchi = ((1 + R.x) * chi + R.y * chi3 + R.z * chi5 - chip) / deriv;
    chi -= dchi;
  }
  if (!converged) return TR_NOT_CONVERGED;
  const double linchi = P * chi;
  double theta;
  if (P < -1e-15) theta = asin(linchi) / P;
  else if (P > 1e-15) theta = atan(linchi) / P;
  else theta = chi;
  const tr_v3 l = tr_normalize(lambdap3);
  const double st = sin(theta), ct = cos(theta);
  result = tr_v3{st * l.x + ct * O.x, st * l.y + ct * O.y, st * l.z + ct * O.z};
  return TR_OK;
}

// CAHVOREModel::point_to_pixel (CAHVOREModel.cc:232-301)
__host__ __device__ inline int tr_cahvore_project(const vwgpu_camera& c, const tr_v3& point, tr_v2& pix) {
  const tr_v3 O = tr_cam_O(c), R = tr_cam_R(c), E = tr_cam_E(c);
  const double P = tr_cam_P(c);
  const tr_v3 p_c = tr_sub(point, tr_load3(c.center));
  const double zeta = tr_dot(p_c, O);
  const tr_v3 lambda3{p_c.x - zeta * O.x, p_c.y - zeta * O.y, p_c.z - zeta * O.z};
  const double lambda = tr_norm(lambda3);
  double theta = atan2(lambda, zeta);
  double dtheta = 1;
  bool converged = false;
  for (int n = 0; n <= 100; ++n) {
    if (fabs(dtheta) < 1e-8) {
      converged = true;
      break;
    }
    const double costh = cos(theta);
    const double sinth = sin(theta);
    const double theta2 = theta * theta;
    const double theta3 = theta * theta2;
    const double theta4 = theta * theta3;
    const double upsilon = zeta * costh + lambda * sinth
      - (1 - costh) * (E.x + E.y * theta2 + E.z * theta4)
      - (theta - sinth) * (2 * E.y * theta + 4 * E.z * theta3);
    dtheta = (zeta * sinth - lambda * costh - (theta - sinth) * (E.x + E.y * theta2 + E.z * theta4)) / upsilon;
    theta -= dtheta;
  }
  if (!converged) return TR_NOT_CONVERGED;
  if ((theta * fabs(P)) > 3.14159265358979323846 / 2) return TR_THETA_OUT_OF_BOUNDS;
  tr_v3 rp;
  if (theta < 1e-8) {
    rp = p_c;
  } else {
    const double linth = P * theta;
    double chi;
    if (P < -1e-15) chi = sin(linth) / P;
    else if (P > 1e-15) chi = tan(linth) / P;
    else chi = theta;
    const double chi2 = chi * chi;
    double mu = R.z;
    mu = R.y + chi2 * mu;
    mu = R.x + chi2 * mu;
    const double lc = lambda / chi, m1 = 1 + mu;
    rp = tr_v3{lc * O.x + m1 * lambda3.x, lc * O.y + m1 * lambda3.y, lc * O.z + m1 * lambda3.z};
  }
  const double alpha = tr_dot(rp, tr_load3(c.A));
  pix = tr_v2{tr_dot(rp, tr_load3(c.H)) / alpha, tr_dot(rp, tr_load3(c.V)) / alpha};
  return TR_OK;
}

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

// tr_ray for every kind; anything but TR_OK where CAHVOREModel::pixel_to_vector throws PixelToRayErr
template <int CAM>
__device__ inline int tr_ray_status(const vwgpu_camera& c, const tr_v2& pix, bool flip, tr_v3& vec) {
  if (CAM == TR_CAM_CAHVORE) return tr_cahvore_ray(c, pix, vec);
  if (CAM == TR_CAM_CAHVOR) {
    vec = tr_cahvor_ray(c, pix, flip);
    return TR_OK;
  }
  vec = tr_ray<CAM>(c, pix, flip);
  return TR_OK;
}

}  // namespace
