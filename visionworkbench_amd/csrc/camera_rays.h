// camera_rays.h — the camera models, both directions, and what the two camera engines share.  The small fp64 vector
// helpers in the reference's expression order; pixel_to_vector of PinholeModel (src/vw/Camera/PinholeModel.cc:422-434)
// and of CAHVModel (src/vw/Camera/CAHVModel.cc:173-189); undistorted_coordinates and distorted_coordinates of the seven
// lenses (src/vw/Camera/LensDistortion.cc, over src/vw/Math/NewtonRaphson.cc:58-119 and
// src/vw/Math/LevenbergMarquardt.h:389-561); both directions of CAHVORModel (src/vw/Camera/CAHVORModel.cc:297-348,
// :431-448) and CAHVOREModel (src/vw/Camera/CAHVOREModel.cc:167-301).  Then what the host side of both engines shares: the
// camera check, the code a kernel carries for a camera, the handedness test of the CAHV family and the grid of row bands.
// Used by triangulate.hip and camera_transform.hip, and by camera_host.hip, which runs the model functions on the host;
// internal linkage, so every translation unit compiles its own copy.
#pragma once
#include <cmath>
#include <cstddef>

#include "vwgpu_internal.h"

namespace {

// which code a kernel carries for one camera: a pinhole without lens distortion, a pinhole whose distortion kind is read
// at run time (null or Tsai), CAHV, CAHVOR, CAHVORE, and a pinhole with any of the seven lenses: the code of every pinhole
// of a pair in which one carries a lens other than null and Tsai
enum { TR_CAM_PINHOLE_NULL = 0, TR_CAM_PINHOLE = 1, TR_CAM_CAHV = 2, TR_CAM_CAHVOR = 3, TR_CAM_CAHVORE = 4, TR_CAM_PINHOLE_LENS = 5 };
// how a CAHVORE function or a projection left: its result, one of the reference's two CAHVORE throws, or the throw of
// LensDistortion::distorted_coordinates
enum { TR_OK = 0, TR_NOT_CONVERGED = 1, TR_THETA_OUT_OF_BOUNDS = 2, TR_LENS_NOT_CONVERGED = 3 };

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

// the lens words L[0..13] of a pinhole: distortion[0..4], A, H, V are contiguous, and a pinhole uses none of A, H, V
static_assert(offsetof(vwgpu_camera, distortion) == 144 && offsetof(vwgpu_camera, V) + sizeof(double[3]) == 256, "lens words");
__host__ __device__ inline const double* tr_lens_words(const vwgpu_camera& c) { return reinterpret_cast<const double*>(&c) + 18; }
inline bool tr_lens_known(int kind) {
  return kind == VWGPU_DISTORTION_NULL || kind == VWGPU_DISTORTION_TSAI || kind == VWGPU_DISTORTION_FOV || kind == VWGPU_DISTORTION_FISHEYE ||
         kind == VWGPU_DISTORTION_BROWN_CONRADY || kind == VWGPU_DISTORTION_ADJUSTABLE_TSAI || kind == VWGPU_DISTORTION_PHOTOMETRIX;
}
// a lens kind the kernels know, and for the adjustable Tsai a coefficient count the lens words can hold (it indexes them)
inline bool tr_lens_valid(const vwgpu_camera& c) {
  if (!tr_lens_known(c.distortion_kind)) return false;
  if (c.distortion_kind != VWGPU_DISTORTION_ADJUSTABLE_TSAI) return true;
  const double n = tr_lens_words(c)[13];
  return n >= 4 && n <= 13 && n == (double)(int)n;
}
// a pinhole whose lens the null / Tsai instantiations do not carry
inline bool tr_lens_pinhole(const vwgpu_camera& c) {
  return c.kind == VWGPU_CAMERA_PINHOLE && c.distortion_kind != VWGPU_DISTORTION_NULL && c.distortion_kind != VWGPU_DISTORTION_TSAI;
}

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
__host__ __device__ inline tr_v2 tr_tsai_norm(const tr_v2& P, const double* distortion) {
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
__host__ __device__ inline void tr_tsai_jacobian(const tr_v2& P, const double* distortion, double* jacobian) {
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

// what NewtonRaphson::solve iterates on: the distortion of a normalised pixel and its Jacobian {J00, J01, J10, J11}
struct tr_tsai_model {
  const double* distortion;
  __host__ __device__ tr_v2 norm(const tr_v2& P) const { return tr_tsai_norm(P, distortion); }
  __host__ __device__ void jacobian(const tr_v2& P, double* J) const { tr_tsai_jacobian(P, distortion, J); }
};

// numericalJacobian::operator() (NewtonRaphson.cc:27-47): central differences with step 1e-6, a column per coordinate
template <class MODEL>
__host__ __device__ inline void tr_numerical_jacobian(const MODEL& m, const tr_v2& P, double* J) {
  const double step = 1e-6;
  const tr_v2 xp = m.norm(tr_v2{P.x + step, P.y + 0.0}), xm = m.norm(tr_v2{P.x - step, P.y - 0.0});
  const tr_v2 JX{(xp.x - xm.x) / (2 * step), (xp.y - xm.y) / (2 * step)};
  const tr_v2 yp = m.norm(tr_v2{P.x + 0.0, P.y + step}), ym = m.norm(tr_v2{P.x - 0.0, P.y - step});
  const tr_v2 JY{(yp.x - ym.x) / (2 * step), (yp.y - ym.y) / (2 * step)};
  J[0] = JX.x;
  J[1] = JY.x;
  J[2] = JX.y;
  J[3] = JY.y;
}

// NewtonRaphson::solve (NewtonRaphson.cc:58-119) with guessX = outY = the normalised distorted pixel, tol = 1e-9
template <class MODEL>
__host__ __device__ inline tr_v2 tr_newton(const tr_v2& outY, const MODEL& model) {
  tr_v2 X = outY;
  tr_v2 bestX = X;
  double best_err = 1.7976931348623157e308;   // std::numeric_limits<double>::max()
  int count = 1;
  const int maxTries = 20;
  while (count < maxTries) {
    const tr_v2 FX = model.norm(X);
    const tr_v2 F{FX.x - outY.x, FX.y - outY.y};
    const double nF = tr_norm(F);
    if (nF != nF) return bestX;
    if (nF < best_err) {
      best_err = nF;
      bestX = X;
    }
    double J[4];
    model.jacobian(X, J);
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
__host__ __device__ inline tr_v2 tr_tsai_undistort(const vwgpu_camera& c, const tr_v2& p) {
  if (c.fu < 1e-300 || c.fv < 1e-300) return tr_v2{HUGE_VAL, HUGE_VAL};
  const tr_v2 p0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const tr_v2 U = tr_newton(p0, tr_tsai_model{c.distortion});
  double ux = U.x, uy = U.y;
  ux = ux * c.fu + c.cu;
  uy = uy * c.fv + c.cv;
  return tr_v2{ux, uy};
}

// FovLensDistortion::undistorted_coordinates (LensDistortion.cc:490-515); L = {k1, 1 / k1, 2 tan(k1 / 2)}
__host__ __device__ inline tr_v2 tr_fov_undistort(const vwgpu_camera& c, const tr_v2& p) {
  const double* L = tr_lens_words(c);
  if (c.fu < 1e-300 || c.fv < 1e-300) return tr_v2{HUGE_VAL, HUGE_VAL};
  const tr_v2 p0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const double rd = tr_norm(p0);
  const double ru = tan(rd * L[0]) / L[2];
  double conv = 1.0;
  if (rd > 1e-8) conv = ru / rd;
  return tr_v2{conv * p0.x * c.fu + c.cu, conv * p0.y * c.fv + c.cv};
}

// fishEyeDistortionNorm (LensDistortion.cc:573-598)
__host__ __device__ inline tr_v2 tr_fisheye_norm(const tr_v2& P, const double* dist) {
  double k1 = dist[0];
  double k2 = dist[1];
  double k3 = dist[2];
  double k4 = dist[3];
  double x = P.x;
  double y = P.y;
  double r2 = x * x + y * y;
  double r = sqrt(r2);
  double theta = atan(r);
  double theta1 = theta * theta;
  double theta2 = theta1 * theta1;
  double theta3 = theta2 * theta1;
  double theta4 = theta2 * theta2;
  double theta_d = theta * (1 + k1 * theta1 + k2 * theta2 + k3 * theta3 + k4 * theta4);
  double scale = 1.0;
  if (r > 1e-8) scale = theta_d / r;
  return tr_v2{x * scale, y * scale};
}

// AdjTsaiDistortionNorm (LensDistortion.cc:799-824): n - 3 radial coefficients, two tangential ones and alpha; n = L[13]
// is between 4 and 13 (vwgpu_camera_set_lens), so the radial loop makes at most 10 passes
__host__ __device__ inline tr_v2 tr_adjustable_tsai_norm(const tr_v2& p_0, const double* distortion) {
  const int n = (int)distortion[13];
  const double r2 = 0.0 + p_0.x * p_0.x + p_0.y * p_0.y;
  double r_n = 1, radial = 0;
  for (int i = 0; i < 10 && i < n - 3; i++) {
    r_n *= r2;
    radial += distortion[i] * r_n;
  }
  tr_v2 tangent{0.0, 0.0};
  const tr_v2 swap_coeff{distortion[n - 2], distortion[n - 3]};
  tangent.x += swap_coeff.x * (r2 + 2 * (p_0.x * p_0.x));
  tangent.y += swap_coeff.y * (r2 + 2 * (p_0.y * p_0.y));
  tangent.x += 2 * (p_0.x * p_0.y) * distortion[n - 3];
  tangent.y += 2 * (p_0.x * p_0.y) * distortion[n - 2];
  tr_v2 result{p_0.x + tangent.x + radial * p_0.x, p_0.y + tangent.y + radial * p_0.y};
  result.x += distortion[n - 1] * result.y;
  result.y += 0.0;
  return result;
}

// the two lenses NewtonRaphson::solve inverts with the numerical Jacobian
struct tr_fisheye_model {
  const double* L;
  __host__ __device__ tr_v2 norm(const tr_v2& P) const { return tr_fisheye_norm(P, L); }
  __host__ __device__ void jacobian(const tr_v2& P, double* J) const { tr_numerical_jacobian(*this, P, J); }
};
struct tr_adjustable_tsai_model {
  const double* L;
  __host__ __device__ tr_v2 norm(const tr_v2& P) const { return tr_adjustable_tsai_norm(P, L); }
  __host__ __device__ void jacobian(const tr_v2& P, double* J) const { tr_numerical_jacobian(*this, P, J); }
};

// FisheyeLensDistortion::undistorted_coordinates (LensDistortion.cc:634-658) and
// AdjustableTsaiLensDistortion::undistorted_coordinates (:851-880)
template <class MODEL>
__host__ __device__ inline tr_v2 tr_numeric_undistort(const vwgpu_camera& c, const tr_v2& p) {
  if (c.fu < 1e-300 || c.fv < 1e-300) return tr_v2{HUGE_VAL, HUGE_VAL};
  const tr_v2 p0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const tr_v2 U = tr_newton(p0, MODEL{tr_lens_words(c)});
  return tr_v2{U.x * c.fu + c.cu, U.y * c.fv + c.cv};
}

// BrownConradyDistortion::undistorted_coordinates (LensDistortion.cc:731-744); L = {xp, yp, k1, k2, k3, p1, p2, phi, sin(phi),
// cos(phi)}
__host__ __device__ inline tr_v2 tr_brown_conrady_undistort(const vwgpu_camera& c, const tr_v2& p) {
  const double* L = tr_lens_words(c);
  tr_v2 intermediate{p.x - L[0] - c.cu, p.y - L[1] - c.cv};
  const double r2 = 0.0 + intermediate.x * intermediate.x + intermediate.y * intermediate.y;
  const double radial = 1 + L[2] * r2 + L[3] * r2 * r2 + L[4] * r2 * r2 * r2;
  const double tangential = L[5] * r2 + L[6] * r2 * r2;
  intermediate.x *= radial;
  intermediate.y *= radial;
  intermediate.x -= tangential * L[8];
  intermediate.y += tangential * L[9];
  return tr_v2{intermediate.x + c.cu, intermediate.y + c.cv};
}

// PhotometrixLensDistortion::undistorted_coordinates (LensDistortion.cc:961-999); L = {xp, yp, k1, k2, k3, p1, p2, b1, b2},
// b1 and b2 unused as in the reference
__host__ __device__ inline tr_v2 tr_photometrix_undistort(const vwgpu_camera& c, const tr_v2& p) {
  const double* L = tr_lens_words(c);
  double x_meas = p.x;
  double y_meas = p.y;
  double xp = L[0] + c.cu;
  double yp = L[1] + c.cv;
  double x = x_meas - xp;
  double y = y_meas - yp;
  double x2 = x * x;
  double y2 = y * y;
  double r2 = x2 + y2;
  double K1 = L[2];
  double K2 = L[3];
  double K3 = L[4];
  double P1 = L[5];
  double P2 = L[6];
  double drr = K1 * r2 + K2 * r2 * r2 + K3 * r2 * r2 * r2;
  double x_corr = x_meas + x * drr + P1 * (r2 + 2.0 * x2) + 2.0 * P2 * x * y;
  double y_corr = y_meas + y * drr + P2 * (r2 + 2.0 * y2) + 2.0 * P1 * x * y;
  return tr_v2{x_corr, y_corr};
}

// undistorted_coordinates of a pinhole's lens, whichever it is (the kinds are checked on the host)
__host__ __device__ inline tr_v2 tr_lens_undistort(const vwgpu_camera& c, const tr_v2& p) {
  switch (c.distortion_kind) {
    case VWGPU_DISTORTION_TSAI: return tr_tsai_undistort(c, p);
    case VWGPU_DISTORTION_FOV: return tr_fov_undistort(c, p);
    case VWGPU_DISTORTION_FISHEYE: return tr_numeric_undistort<tr_fisheye_model>(c, p);
    case VWGPU_DISTORTION_BROWN_CONRADY: return tr_brown_conrady_undistort(c, p);
    case VWGPU_DISTORTION_ADJUSTABLE_TSAI: return tr_numeric_undistort<tr_adjustable_tsai_model>(c, p);
    case VWGPU_DISTORTION_PHOTOMETRIX: return tr_photometrix_undistort(c, p);
    default: return p;
  }
}

// TsaiLensDistortion::distorted_coordinates (LensDistortion.cc:345-369)
__host__ __device__ inline tr_v2 tr_tsai_distort(const vwgpu_camera& c, const tr_v2& p) {
  if (c.fu < 1e-300 || c.fv < 1e-300) return tr_v2{HUGE_VAL, HUGE_VAL};
  const tr_v2 p0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const tr_v2 d = tr_tsai_norm(p0, c.distortion);
  double dx = d.x, dy = d.y;
  dx = dx * c.fu + c.cu;
  dy = dy * c.fv + c.cv;
  return tr_v2{dx, dy};
}

// FovLensDistortion::distorted_coordinates (LensDistortion.cc:462-488); L = {k1, 1 / k1, 2 tan(k1 / 2)}
__host__ __device__ inline tr_v2 tr_fov_distort(const vwgpu_camera& c, const tr_v2& p) {
  const double* L = tr_lens_words(c);
  if (c.fu < 1e-300 || c.fv < 1e-300) return tr_v2{HUGE_VAL, HUGE_VAL};
  const tr_v2 p0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const double ru = tr_norm(p0);
  const double rd = atan(ru * L[2]) * L[1];
  double conv = 1.0;
  if (ru > 1e-8) conv = rd / ru;
  return tr_v2{conv * p0.x * c.fu + c.cu, conv * p0.y * c.fv + c.cv};
}

// FisheyeLensDistortion::distorted_coordinates (:612-632) and AdjustableTsaiLensDistortion::distorted_coordinates (:832-849)
template <class MODEL>
__host__ __device__ inline tr_v2 tr_norm_distort(const vwgpu_camera& c, const tr_v2& p) {
  if (c.fu < 1e-300 || c.fv < 1e-300) return tr_v2{HUGE_VAL, HUGE_VAL};
  const tr_v2 p0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const tr_v2 d = MODEL{tr_lens_words(c)}.norm(p0);
  return tr_v2{d.x * c.fu + c.cu, d.y * c.fv + c.cv};
}

// DistortOptimizeFunctor (LensDistortion.cc:29-41) for the two lenses that have no distorted_coordinates of their own
__host__ __device__ inline tr_v2 tr_solver_model(const vwgpu_camera& c, const tr_v2& x) {
  return c.distortion_kind == VWGPU_DISTORTION_PHOTOMETRIX ? tr_photometrix_undistort(c, x) : tr_brown_conrady_undistort(c, x);
}

// LensDistortion::distorted_coordinates (LensDistortion.cc:175-195): levenberg_marquardtFixed(model, v, v, status, 1e-16,
// 1e-16, 100) (Math/LevenbergMarquardt.h:389-561) for two unknowns, with the forward-difference Jacobian of
// LeastSquaresModelBaseFixed::jacobian (:344-377) and inverse() of Math/Matrix.h:2209-2216, then the 1e-10 test.  At most
// 100 outer passes of at most 6 inner ones.  false where the reference throws "LensDistortion: Did not converge.", and
// where det(hessian_lm) > 0.0 does not hold (NaN, overflow), for which the reference leaves for LAPACK.
__host__ __device__ inline bool tr_solver_distort(const vwgpu_camera& c, const tr_v2& v, tr_v2& solution) {
  const double abs_tolerance = 1e-16, rel_tolerance = 1e-16;
  const int max_iterations = 100;
  bool done = false;
  const double Rinv = 10;
  double lambda = 0.1;
  tr_v2 x_try{0.0, 0.0}, x = v;
  tr_v2 h = tr_solver_model(c, x);
  tr_v2 error{v.x - h.x, v.y - h.y};
  double norm_start = tr_norm(error);
  if (norm_start < abs_tolerance) done = true;
  for (int outer_iter = 1; outer_iter <= max_iterations && !done; ++outer_iter) {
    bool shortCircuit = false;
    h = tr_solver_model(c, x);
    error = tr_v2{v.x - h.x, v.y - h.y};
    norm_start = tr_norm(error);
    // the Jacobian, J[row][column]
    const tr_v2 h0 = tr_solver_model(c, x);
    const double eps0 = 1e-7 + fabs(x.x * 1e-7), eps1 = 1e-7 + fabs(x.y * 1e-7);
    const tr_v2 h_0 = tr_solver_model(c, tr_v2{x.x + eps0, x.y}), h_1 = tr_solver_model(c, tr_v2{x.x, x.y + eps1});
    const double J00 = (h_0.x - h0.x) / eps0, J10 = (h_0.y - h0.y) / eps0;
    const double J01 = (h_1.x - h0.x) / eps1, J11 = (h_1.y - h0.y) / eps1;
    const double del_J0 = -1.0 * Rinv * (0.0 + J00 * error.x + J10 * error.y);
    const double del_J1 = -1.0 * Rinv * (0.0 + J01 * error.x + J11 * error.y);
    const double H00 = Rinv * (0.0 + J00 * J00 + J10 * J10), H01 = Rinv * (0.0 + J00 * J01 + J10 * J11);
    const double H10 = Rinv * (0.0 + J01 * J00 + J11 * J10), H11 = Rinv * (0.0 + J01 * J01 + J11 * J11);
    int iterations = 0;
    double norm_try = norm_start + 1.0;
    while (norm_try > norm_start && iterations < 6) {
      double d0 = H00, d3 = H11;
      const double d1 = H01, d2 = H10;
      d0 += d0 * lambda + lambda;
      d3 += d3 * lambda + lambda;
      const double det = d0 * d3 - d1 * d2;
      if (!(det > 0.0)) return false;
      const double i0 = d3 / det, i1 = -d1 / det, i2 = -d2 / det, i3 = d0 / det;
      const tr_v2 delta_x{0.0 + i0 * del_J0 + i1 * del_J1, 0.0 + i2 * del_J0 + i3 * del_J1};
      x_try = tr_v2{x.x - delta_x.x, x.y - delta_x.y};
      const tr_v2 h_try = tr_solver_model(c, x_try);
      const tr_v2 error_try{v.x - h_try.x, v.y - h_try.y};
      norm_try = tr_norm(error_try);
      if (norm_try > norm_start) lambda *= 10;
      ++iterations;
      if (iterations > 5) {
        shortCircuit = true;
        norm_try = norm_start;
      }
    }
    if (!shortCircuit && ((norm_start - norm_try) / norm_start) < rel_tolerance) done = true;
    if (norm_try < abs_tolerance) done = true;
    if (!shortCircuit) x = x_try;
    norm_start = norm_try;
    lambda /= 10;
  }
  solution = x;
  const tr_v2 undist = tr_solver_model(c, solution);
  const double nv = tr_norm(v);
  const double err = tr_norm(tr_v2{undist.x - v.x, undist.y - v.y}) / (nv > 0.1 ? nv : 0.1);
  return !(err > 1e-10);
}

// distorted_coordinates of a pinhole's lens, whichever it is; false where the reference throws
__host__ __device__ inline bool tr_lens_distort(const vwgpu_camera& c, const tr_v2& p, tr_v2& out) {
  switch (c.distortion_kind) {
    case VWGPU_DISTORTION_TSAI: out = tr_tsai_distort(c, p); return true;
    case VWGPU_DISTORTION_FOV: out = tr_fov_distort(c, p); return true;
    case VWGPU_DISTORTION_FISHEYE: out = tr_norm_distort<tr_fisheye_model>(c, p); return true;
    case VWGPU_DISTORTION_ADJUSTABLE_TSAI: out = tr_norm_distort<tr_adjustable_tsai_model>(c, p); return true;
    case VWGPU_DISTORTION_BROWN_CONRADY:
    case VWGPU_DISTORTION_PHOTOMETRIX: return tr_solver_distort(c, p, out);
    default: out = p; return true;
  }
}

// pixel_to_vector of the camera kinds a kernel carries
// `flip`: the handedness test of CAHVModel::pixel_to_vector, dot(cross(V, H), A) < 0 — the same for every pixel, so the
// host evaluates it once (tr_cahv_flip)
template <int CAM>
__host__ __device__ inline tr_v3 tr_ray(const vwgpu_camera& c, const tr_v2& pix, bool flip) {
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
  if (CAM == TR_CAM_PINHOLE_LENS) u = tr_lens_undistort(c, u);
  else if (CAM != TR_CAM_PINHOLE_NULL && c.distortion_kind == VWGPU_DISTORTION_TSAI) u = tr_tsai_undistort(c, u);
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

// ---- what the host side of both engines shares -------------------------------------------------------------------------

inline int tr_cahv_flip(const vwgpu_camera& c) {   // CAHVORModel.cc:306 is the same test
  return (c.kind == VWGPU_CAMERA_CAHV || c.kind == VWGPU_CAMERA_CAHVOR) && tr_dot(tr_cross(tr_load3(c.V), tr_load3(c.H)), tr_load3(c.A)) < 0.0;   // CAHVModel.cc:182
}

// a camera of a kind and with a lens the kernels know; `which` ("source", "destination") names it in the null message, or is null
inline int tr_camera_check(vwgpu_ctx* ctx, const char* name, const char* which, const vwgpu_camera* c) {
  if (!c) return which ? vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: null %s camera", name, which) : vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: null camera", name);
  if (c->kind != VWGPU_CAMERA_PINHOLE && c->kind != VWGPU_CAMERA_CAHV && !tr_new_kind(*c))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: unknown camera kind %d", name, c->kind);
  if (c->kind == VWGPU_CAMERA_PINHOLE && !tr_lens_valid(*c))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: unknown lens distortion kind %d", name, c->distortion_kind);
  return VWGPU_OK;
}

// the code a kernel carries for the camera whose rays it forms.  `lens_pair`: one camera of the pair is a pinhole with a
// lens other than null and Tsai, and every pinhole of the pair takes the any-lens code.
inline int tr_camera_code(const vwgpu_camera& c, bool lens_pair) {
  if (tr_new_kind(c)) return c.kind == VWGPU_CAMERA_CAHVOR ? TR_CAM_CAHVOR : TR_CAM_CAHVORE;
  if (lens_pair && c.kind == VWGPU_CAMERA_PINHOLE) return TR_CAM_PINHOLE_LENS;
  return c.kind == VWGPU_CAMERA_CAHV ? TR_CAM_CAHV : c.distortion_kind == VWGPU_DISTORTION_NULL ? TR_CAM_PINHOLE_NULL : TR_CAM_PINHOLE;
}

// Every band of BY rows has a workgroup of BX x BY lanes of its own, numbered through grid y and then z: a row loop would
// keep both cameras and every argument live across its iterations, in more scalar registers than there are.
template <int BX, int BY>
inline dim3 tr_band_grid(int w, int h) {
  const long long bands = ((long long)h + BY - 1) / BY, gy = bands < 65535 ? bands : 65535;
  return dim3((unsigned)((w + BX - 1) / BX), (unsigned)gy, (unsigned)((bands + gy - 1) / gy));
}
template <int BX, int BY>
__device__ inline bool tr_band_position(int w, int h, int& x, int& y, long long& band) {
  x = blockIdx.x * BX + threadIdx.x;
  band = (long long)blockIdx.z * gridDim.y + blockIdx.y;
  const long long row = band * BY + threadIdx.y;
  y = (int)row;
  return x < w && row < h;
}

}  // namespace
