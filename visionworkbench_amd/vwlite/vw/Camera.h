// vw/Camera.h — the part of vw::camera that triangulation and epipolar rectification need: PinholeModel with the null, Tsai,
// FOV, fisheye, Brown-Conrady, adjustable Tsai or Photometrix lens distortion (src/vw/Camera/PinholeModel.{h,cc},
// LensDistortion.{h,cc}; the lens arithmetic is the engine's, vwgpu_lens_coordinates), CAHVModel
// (src/vw/Camera/CAHVModel.{h,cc}) and epipolar() for both, CAHVORModel and CAHVOREModel (src/vw/Camera/CAHVORModel.{h,cc},
// CAHVOREModel.{h,cc}) and linearize_camera() for those.  Each model carries the flat camera descriptor of the C ABI
// (struct vwgpu_camera, include/vwgpu.h) and, for a pinhole, the 3 x 4 camera matrix beside it, which is what the engine's
// kernels read; pixel_to_vector, camera_center and point_to_pixel are host code for single pixels, with the reference's
// expressions (whole images are computed on the device: vw/Stereo.h, vw/CameraTransform.h).
#ifndef VWLITE_CAMERA_H
#define VWLITE_CAMERA_H

#include <cmath>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "Core.h"
#include "Math.h"
#include "vwgpu.h"

namespace vw {
namespace camera {

namespace detail {
inline double dot3(const double* a, Vector3 const& b) { return 0.0 + a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline double dot3(Vector3 const& a, Vector3 const& b) { return 0.0 + a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline Vector3 cross3(Vector3 const& a, Vector3 const& b) {
  return Vector3(a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]);
}
inline Vector3 normalize3(Vector3 const& v) {
  const double n = std::sqrt(dot3(v, v));
  return Vector3(v[0] / n, v[1] / n, v[2] / n);
}
}  // namespace detail

/// What StereoModel needs of a camera (src/vw/Camera/CameraModel.h).
class CameraModel {
public:
  virtual ~CameraModel() {}
  virtual Vector2 point_to_pixel(Vector3 const& point) const = 0;
  virtual Vector3 pixel_to_vector(Vector2 const& pix) const = 0;
  virtual Vector3 camera_center(Vector2 const& pix = Vector2()) const = 0;
  /// the descriptor the engine reads
  vwgpu_camera const& descriptor() const { return m_desc; }
  /// m_camera_matrix (row-major 3 x 4) of a pinhole, which travels beside the descriptor; NULL for other models
  virtual const double* camera_matrix() const { return NULL; }
  /// PinholeModel::set_do_point_to_pixel_check (on by default, as in the reference); other models have no check
  virtual bool do_point_to_pixel_check() const { return true; }
  static Vector2 invalid_pixel() { return Vector2(-1e8, -1e8); }
protected:
  vwgpu_camera m_desc;
};

/// What the lens solvers throw (src/vw/Camera/CameraModel.h).
VWLITE_EXCEPTION(PixelToRayErr, Exception);
VWLITE_EXCEPTION(PointToPixelErr, Exception);

class PinholeModel;

/// LensDistortion (LensDistortion.h): the name and the parameters of a lens (the reference's Vector<double> of any length is
/// a std::vector<double> here).  The two coordinate functions take a point in
/// focal-plane units (pixel * pixel_pitch) and run the functions of the engine's kernels on the host
/// (vwgpu_lens_coordinates) on the descriptor of `cam`, which must carry this lens.
class LensDistortion {
protected:
  std::vector<double> m_distortion;
  LensDistortion(const double* p, size_t n) : m_distortion(p, p + n) {}
  explicit LensDistortion(std::vector<double> const& v) : m_distortion(v) {}
public:
  virtual ~LensDistortion() {}
  virtual std::string name() const = 0;
  virtual int kind() const = 0;   ///< vwgpu_distortion_kind
  virtual LensDistortion* copy() const = 0;
  std::vector<double> distortion_parameters() const { return m_distortion; }
  const double* parameter_data() const { return m_distortion.data(); }
  int parameter_count() const { return (int)m_distortion.size(); }
  inline Vector2 distorted_coordinates(PinholeModel const& cam, Vector2 const& p) const;
  inline Vector2 undistorted_coordinates(PinholeModel const& cam, Vector2 const& p) const;
};

/// TsaiLensDistortion (LensDistortion.cc:225-400): parameters k1, k2, p1, p2, k3.
class TsaiLensDistortion : public LensDistortion {
  static std::vector<double> five(double k1, double k2, double p1, double p2, double k3) { return std::vector<double>{k1, k2, p1, p2, k3}; }
public:
  TsaiLensDistortion(double k1, double k2, double p1, double p2, double k3 = 0) : LensDistortion(five(k1, k2, p1, p2, k3).data(), 5) {}
  std::string name() const { return "TSAI"; }
  int kind() const { return VWGPU_DISTORTION_TSAI; }
  LensDistortion* copy() const { return new TsaiLensDistortion(*this); }
  const double* distortion_parameters() const { return m_distortion.data(); }
  /// TsaiDistortionNorm (:260-276)
  Vector2 distort_norm(Vector2 const& P) const {
    const double* m_p = m_distortion.data();
    const double x = P[0], y = P[1], k1 = m_p[0], k2 = m_p[1], p1 = m_p[2], p2 = m_p[3], k3 = m_p[4];
    const double r2 = x * x + y * y;
    const double rdist = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
    return Vector2(x * rdist + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)), y * rdist + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y));
  }
};

/// FovLensDistortion (LensDistortion.cc:418-530): k1 > 0, or IOErr.
class FovLensDistortion : public LensDistortion {
public:
  explicit FovLensDistortion(std::vector<double> const& params) : LensDistortion(params) {
    VW_ASSERT(params.size() == 1, IOErr() << "FovLensDistortion: Incorrect number of parameters was passed in.");
    VW_ASSERT(params[0] > 0, IOErr() << "FovLensDistortion: The distortion coefficient must be positive.\n");
  }
  std::string name() const { return "FOV"; }
  int kind() const { return VWGPU_DISTORTION_FOV; }
  LensDistortion* copy() const { return new FovLensDistortion(*this); }
};

/// FisheyeLensDistortion (LensDistortion.cc:532-673): k1, k2, k3, k4.
class FisheyeLensDistortion : public LensDistortion {
public:
  explicit FisheyeLensDistortion(std::vector<double> const& params) : LensDistortion(params) {
    VW_ASSERT(params.size() == 4, IOErr() << "FisheyeLensDistortion: Incorrect number of parameters was passed in.");
  }
  std::string name() const { return "FISHEYE"; }
  int kind() const { return VWGPU_DISTORTION_FISHEYE; }
  LensDistortion* copy() const { return new FisheyeLensDistortion(*this); }
};

/// BrownConradyDistortion (LensDistortion.cc:675-775): xp, yp, k1, k2, k3, p1, p2, phi, or the four groups.
class BrownConradyDistortion : public LensDistortion {
  static std::vector<double> join(Vector2 const& principal, Vector3 const& radial, Vector2 const& centering, double angle) {
    return std::vector<double>{principal[0], principal[1], radial[0], radial[1], radial[2], centering[0], centering[1], angle};
  }
public:
  explicit BrownConradyDistortion(std::vector<double> const& params) : LensDistortion(params) {
    VW_ASSERT(params.size() == 8, ArgumentErr() << "BrownConradyDistortion: requires constructor input of size 8.");
  }
  BrownConradyDistortion(Vector2 const& principal, Vector3 const& radial, Vector2 const& centering, double const& angle)
      : LensDistortion(join(principal, radial, centering, angle)) {}
  std::string name() const { return "BrownConrady"; }
  int kind() const { return VWGPU_DISTORTION_BROWN_CONRADY; }
  LensDistortion* copy() const { return new BrownConradyDistortion(*this); }
};

/// AdjustableTsaiLensDistortion (LensDistortion.cc:777-917): n - 3 radial coefficients, two tangential ones and alpha; the
/// camera descriptor holds up to 13.
class AdjustableTsaiLensDistortion : public LensDistortion {
public:
  explicit AdjustableTsaiLensDistortion(std::vector<double> params) : LensDistortion(params) {
    VW_ASSERT(params.size() > 3, ArgumentErr() << "Requires at least 4 coefficients for distortion. Last 3 are always the distortion coefficients and alpha. All leading elements are even radial distortion coefficients.");
    VW_ASSERT(params.size() <= 13, NoImplErr() << "AdjustableTsaiLensDistortion: more than 13 coefficients do not fit the camera descriptor.");
  }
  std::string name() const { return "AdjustableTSAI"; }
  int kind() const { return VWGPU_DISTORTION_ADJUSTABLE_TSAI; }
  LensDistortion* copy() const { return new AdjustableTsaiLensDistortion(*this); }
};

/// PhotometrixLensDistortion (LensDistortion.cc:919-1013): xp, yp, k1, k2, k3, p1, p2, b1, b2.
class PhotometrixLensDistortion : public LensDistortion {
public:
  explicit PhotometrixLensDistortion(std::vector<double> const& params) : LensDistortion(params) {
    VW_ASSERT(params.size() == 9, IOErr() << "PhotometrixLensDistortion: Incorrect number of parameters was passed in.");
  }
  std::string name() const { return "Photometrix"; }
  int kind() const { return VWGPU_DISTORTION_PHOTOMETRIX; }
  LensDistortion* copy() const { return new PhotometrixLensDistortion(*this); }
};

/// PinholeModel(center, rotation, fu, fv, cu, cv[, u, v, w][, distortion][, pixel_pitch]) (PinholeModel.h).
class PinholeModel : public CameraModel {
  Vector3 m_center;
  Matrix3x3 m_rotation;
  Vector3 m_u, m_v, m_w;
  std::shared_ptr<LensDistortion> m_distortion;   // null: NullLensDistortion
  double m_matrix[12];
  bool m_check = true;
  void rebuild() {
    const double c[3] = {m_center[0], m_center[1], m_center[2]}, u[3] = {m_u[0], m_u[1], m_u[2]}, v[3] = {m_v[0], m_v[1], m_v[2]},
                 w[3] = {m_w[0], m_w[1], m_w[2]};
    const double fu = m_desc.fu, fv = m_desc.fv, cu = m_desc.cu, cv = m_desc.cv, pitch = m_desc.pixel_pitch;
    const int rc = vwgpu_pinhole_camera(c, m_rotation.data(), fu, fv, cu, cv, u, v, w, pitch, VWGPU_DISTORTION_NULL, NULL, &m_desc);
    VW_ASSERT(rc == VWGPU_OK, ArgumentErr() << "PinholeModel: the coordinate frame u, v, w must be orthonormal.");
    if (m_distortion) {
      const int lens_rc = vwgpu_camera_set_lens(&m_desc, m_distortion->kind(), m_distortion->parameter_data(), m_distortion->parameter_count());
      VW_ASSERT(lens_rc == VWGPU_OK, ArgumentErr() << "PinholeModel: the parameters of the " << m_distortion->name() << " lens are refused.");
    }
    vwgpu_pinhole_camera_matrix(c, m_rotation.data(), fu, fv, cu, cv, u, v, w, pitch, VWGPU_DISTORTION_NULL, NULL, m_matrix);
  }
  static Matrix3x3 identity() { Matrix3x3 r; r.set_identity(); return r; }
public:
  PinholeModel() : PinholeModel(Vector3(0, 0, 0), identity(), 1, 1, 0, 0) {}
  PinholeModel(Vector3 const& center, Matrix3x3 const& rotation, double fu, double fv, double cu, double cv,
               Vector3 const& u = Vector3(1, 0, 0), Vector3 const& v = Vector3(0, 1, 0), Vector3 const& w = Vector3(0, 0, 1),
               LensDistortion const* distortion = NULL, double pixel_pitch = 1.0)
      : m_center(center), m_rotation(rotation), m_u(u), m_v(v), m_w(w) {
    if (distortion) m_distortion.reset(distortion->copy());
    m_desc.fu = fu; m_desc.fv = fv; m_desc.cu = cu; m_desc.cv = cv; m_desc.pixel_pitch = pixel_pitch;
    rebuild();
  }
  PinholeModel(Vector3 const& center, Matrix3x3 const& rotation, double fu, double fv, double cu, double cv,
               LensDistortion const* distortion, double pixel_pitch = 1.0)
      : PinholeModel(center, rotation, fu, fv, cu, cv, Vector3(1, 0, 0), Vector3(0, 1, 0), Vector3(0, 0, 1), distortion, pixel_pitch) {}

  Vector3 camera_center(Vector2 const& = Vector2()) const { return m_center; }
  const double* camera_matrix() const { return m_matrix; }
  Matrix3x3 const& get_rotation_matrix() const { return m_rotation; }
  Vector2 focal_length() const { return Vector2(m_desc.fu, m_desc.fv); }
  Vector2 point_offset() const { return Vector2(m_desc.cu, m_desc.cv); }
  double pixel_pitch() const { return m_desc.pixel_pitch; }
  void set_point_offset(Vector2 const& offset) { m_desc.cu = offset[0]; m_desc.cv = offset[1]; rebuild(); }
  void set_do_point_to_pixel_check(bool value) { m_check = value; }
  bool do_point_to_pixel_check() const { return m_check; }

  LensDistortion const* lens_distortion() const { return m_distortion.get(); }

  /// PinholeModel::pixel_to_vector (PinholeModel.cc:422-430); the lens is undone by the engine's functions on the host
  Vector3 pixel_to_vector(Vector2 const& pix) const {
    Vector2 u(pix[0] * m_desc.pixel_pitch, pix[1] * m_desc.pixel_pitch);
    if (m_distortion) u = m_distortion->undistorted_coordinates(*this, u);
    const Vector3 p(u[0], u[1], 1);
    const double* m = m_desc.inv_camera_transform;
    return detail::normalize3(Vector3(detail::dot3(m, p), detail::dot3(m + 3, p), detail::dot3(m + 6, p)));
  }

  /// PinholeModel::point_to_pixel without its round-trip check (PinholeModel.cc:370-413): K [uvw R^T | -uvw R^T C]
  Vector2 point_to_pixel(Vector3 const& point) const {
    double q[3];
    const Vector3 uvw[3] = {m_u, m_v, m_w};
    for (int i = 0; i < 3; ++i) {
      q[i] = 0;
      for (int j = 0; j < 3; ++j) {
        double e = 0;   // (uvw R^T)(i, j)
        for (int k = 0; k < 3; ++k) e += uvw[i][k] * m_rotation(j, k);
        q[i] += e * (point[j] - m_center[j]);
      }
    }
    Vector2 pix(q[0] / q[2], q[1] / q[2]);   // normalised; the intrinsics follow
    if (m_distortion && m_distortion->kind() != VWGPU_DISTORTION_TSAI) {
      // distorted_coordinates of the undistorted position in focal-plane units; PointToPixelErr where it does not converge
      const Vector2 d = m_distortion->distorted_coordinates(*this, Vector2(pix[0] * m_desc.fu + m_desc.cu, pix[1] * m_desc.fv + m_desc.cv));
      return Vector2(d[0] / m_desc.pixel_pitch, d[1] / m_desc.pixel_pitch);
    }
    if (m_distortion) pix = static_cast<TsaiLensDistortion const*>(m_distortion.get())->distort_norm(pix);
    return Vector2((pix[0] * m_desc.fu + m_desc.cu) / m_desc.pixel_pitch, (pix[1] * m_desc.fv + m_desc.cv) / m_desc.pixel_pitch);
  }
};

namespace detail {
inline Vector2 lens_coordinates(PinholeModel const& cam, LensDistortion const* lens, int direction, Vector2 const& p) {
  VW_ASSERT(cam.lens_distortion() && cam.lens_distortion()->kind() == lens->kind(), ArgumentErr() << "LensDistortion: the camera carries another lens.");
  const double in[2] = {p[0], p[1]};
  double out[2];
  const int rc = vwgpu_lens_coordinates(&cam.descriptor(), direction, in, 1, out, NULL);
  if (rc == VWGPU_ERR_LOGIC) vw_throw(PointToPixelErr() << "LensDistortion: Did not converge.\n");
  VW_ASSERT(rc == VWGPU_OK, ArgumentErr() << "LensDistortion: bad arguments.");
  return Vector2(out[0], out[1]);
}
}  // namespace detail
inline Vector2 LensDistortion::distorted_coordinates(PinholeModel const& cam, Vector2 const& p) const { return detail::lens_coordinates(cam, this, 0, p); }
inline Vector2 LensDistortion::undistorted_coordinates(PinholeModel const& cam, Vector2 const& p) const { return detail::lens_coordinates(cam, this, 1, p); }

/// CAHVModel(C, A, H, V) (CAHVModel.h).
class CAHVModel : public CameraModel {
public:
  Vector3 C, A, H, V;
  CAHVModel() : CAHVModel(Vector3(0, 0, 0), Vector3(0, 0, 1), Vector3(1, 0, 0), Vector3(0, 1, 0)) {}
  explicit CAHVModel(vwgpu_camera const& d)
      : CAHVModel(Vector3(d.center[0], d.center[1], d.center[2]), Vector3(d.A[0], d.A[1], d.A[2]), Vector3(d.H[0], d.H[1], d.H[2]),
                  Vector3(d.V[0], d.V[1], d.V[2])) {}
  CAHVModel(Vector3 const& c, Vector3 const& a, Vector3 const& h, Vector3 const& v) : C(c), A(a), H(h), V(v) {
    m_desc = vwgpu_camera();
    m_desc.kind = VWGPU_CAMERA_CAHV;
    for (int i = 0; i < 3; ++i) { m_desc.center[i] = C[i]; m_desc.A[i] = A[i]; m_desc.H[i] = H[i]; m_desc.V[i] = V[i]; }
  }
  /// CAHVModel::point_to_pixel (CAHVModel.cc:167-171)
  Vector2 point_to_pixel(Vector3 const& point) const {
    const Vector3 p = point - C;
    const double dDot = detail::dot3(p, A);
    return Vector2(detail::dot3(p, H) / dDot, detail::dot3(p, V) / dDot);
  }
  /// CAHVModel::pixel_to_vector (CAHVModel.cc:173-185)
  Vector3 pixel_to_vector(Vector2 const& pix) const {
    Vector3 vec = detail::normalize3(detail::cross3(Vector3(V[0] - pix[1] * A[0], V[1] - pix[1] * A[1], V[2] - pix[1] * A[2]),
                                                    Vector3(H[0] - pix[0] * A[0], H[1] - pix[0] * A[1], H[2] - pix[0] * A[2])));
    if (detail::dot3(detail::cross3(V, H), A) < 0.0) vec = Vector3(vec[0] * -1.0, vec[1] * -1.0, vec[2] * -1.0);
    return vec;
  }
  Vector3 camera_center(Vector2 const& = Vector2()) const { return C; }
};

/// CAHVORModel(C, A, H, V, O, R) (CAHVORModel.h): CAHV with radial distortion about the axis O.  The single-pixel functions
/// are host code in the reference's expressions (CAHVORModel.cc:297-348, :431-448); images and arrays of points go through
/// the engine (vw/CameraTransform.h, vw/Stereo.h).
class CAHVORModel : public CameraModel {
public:
  typedef CAHVModel linearized_type;
  Vector3 C, A, H, V, O, R;
  CAHVORModel() : CAHVORModel(Vector3(0, 0, 0), Vector3(0, 0, 1), Vector3(1, 0, 0), Vector3(0, 1, 0), Vector3(0, 0, 1), Vector3(0, 0, 0)) {}
  CAHVORModel(Vector3 const& c, Vector3 const& a, Vector3 const& h, Vector3 const& v, Vector3 const& o, Vector3 const& r)
      : C(c), A(a), H(h), V(v), O(o), R(r) {
    const int rc = vwgpu_cahvor_camera(&C[0], &A[0], &H[0], &V[0], &O[0], &R[0], &m_desc);
    VW_ASSERT(rc == VWGPU_OK, ArgumentErr() << "CAHVORModel: bad arguments.");
  }
  std::string type() const { return "CAHVOR"; }
  Vector3 pixel_to_vector(Vector2 const& pix) const {
    Vector3 rr = detail::normalize3(detail::cross3(V - pix[1] * A, H - pix[0] * A));
    if (detail::dot3(detail::cross3(V, H), A) < 0) rr = -1.0 * rr;
    const double omega = detail::dot3(rr, O);
    const Vector3 lambda = rr - omega * O;
    const double tau = detail::dot3(lambda, lambda) / (omega * omega);
    const double k1 = 1 + R[0], k3 = R[1] * tau, k5 = R[2] * tau * tau;
    double u = 1.0 - (R[0] + k3 + k5);
    for (int i = 0; i < 20; ++i) {
      const double u_2 = u * u;
      const double poly = ((k5 * u_2 + k3) * u_2 + k1) * u - 1;
      const double deriv = (5 * k5 * u_2 + 3 * k3) * u_2 + k1;
      if (deriv <= 0) break;
      const double du = poly / deriv;
      u -= du;
      if (std::fabs(du) < 1.0e-6) break;
    }
    return detail::normalize3(rr - (1 - u) * lambda);
  }
  Vector2 point_to_pixel(Vector3 const& point) const {
    const Vector3 vec = point - C;
    const double omega = detail::dot3(vec, O);
    const Vector3 lambda = vec - omega * O;
    const double tau = detail::dot3(lambda, lambda) / (omega * omega);
    const double mu = R[0] + (R[1] * tau) + (R[2] * tau * tau);
    const Vector3 pp_c = vec + mu * lambda;
    const double alpha = detail::dot3(pp_c, A);
    return Vector2(detail::dot3(pp_c, H) / alpha, detail::dot3(pp_c, V) / alpha);
  }
  Vector3 camera_center(Vector2 const& = Vector2()) const { return C; }
};

/// CAHVOREModel(C, A, H, V, O, R, E[, T, P | P]) (CAHVOREModel.h, CAHVOREModel.cc:105-132): the fisheye member of the family.
/// T = 1 sets P = 1, T = 2 sets P = 0, T = 3 takes P in [0, 1]; anything else throws ArgumentErr.
class CAHVOREModel : public CameraModel {
  void fill(int type) {
    const int rc = vwgpu_cahvore_camera(&C[0], &A[0], &H[0], &V[0], &O[0], &R[0], &E[0], type, P, &m_desc);
    VW_ASSERT(rc == VWGPU_OK, ArgumentErr() << (type >= 1 && type <= 3 ? "Invalid P value: " : "Unknown CAHVORE type: ") << (type >= 1 && type <= 3 ? P : (double)type));
    P = m_desc.distortion[0];
  }
public:
  typedef CAHVModel linearized_type;
  Vector3 C, A, H, V, O, R, E;
  double P;
  CAHVOREModel() : CAHVOREModel(Vector3(0, 0, 0), Vector3(0, 0, 1), Vector3(1, 0, 0), Vector3(0, 1, 0), Vector3(0, 0, 1), Vector3(0, 0, 0), Vector3(0, 0, 0)) {}
  CAHVOREModel(Vector3 const& c, Vector3 const& a, Vector3 const& h, Vector3 const& v, Vector3 const& o, Vector3 const& r, Vector3 const& e)
      : C(c), A(a), H(h), V(v), O(o), R(r), E(e), P(1.0) { fill(3); }
  CAHVOREModel(Vector3 const& c, Vector3 const& a, Vector3 const& h, Vector3 const& v, Vector3 const& o, Vector3 const& r, Vector3 const& e,
               int T, double P_v)
      : C(c), A(a), H(h), V(v), O(o), R(r), E(e), P(P_v) { fill(T); }
  CAHVOREModel(Vector3 const& c, Vector3 const& a, Vector3 const& h, Vector3 const& v, Vector3 const& o, Vector3 const& r, Vector3 const& e,
               double P_v)
      : C(c), A(a), H(h), V(v), O(o), R(r), E(e), P(P_v) { fill(3); }
  std::string type() const { return "CAHVORE"; }
  /// CAHVOREModel::pixel_to_vector (CAHVOREModel.cc:167-228)
  Vector3 pixel_to_vector(Vector2 const& pix) const {
    const Vector3 w3 = detail::cross3(V - pix[1] * A, H - pix[0] * A);
    const Vector3 rp = (1 / detail::dot3(A, detail::cross3(V, H))) * w3;
    const double zetap = detail::dot3(rp, O);
    const Vector3 lambdap3 = rp - zetap * O;
    const double lambdap = std::sqrt(detail::dot3(lambdap3, lambdap3));
    const double chip = lambdap / zetap;
    if (chip < 1e-8) return O;
    double chi = chip, dchi = 1;
    for (int32 n = 0;; ++n) {
      if (n > 100) vw_throw(PixelToRayErr() << "CAHVOREModel: Did not converge.\n");
      if (std::fabs(dchi) < 1e-8) break;
      const double chi2 = chi * chi, chi3 = chi * chi2, chi4 = chi * chi3, chi5 = chi * chi4;
      const double deriv = (1 + R[0]) + 3 * R[1] * chi2 + 5 * R[2] * chi4;
      dchi = ((1 + R[0]) * chi + R[1] * chi3 + R[2] * chi5 - chip) / deriv;
      chi -= dchi;
    }
    const double linchi = P * chi;
    double theta;
    if (P < -1e-15) theta = std::asin(linchi) / P;
    else if (P > 1e-15) theta = std::atan(linchi) / P;
    else theta = chi;
    return std::sin(theta) * detail::normalize3(lambdap3) + std::cos(theta) * O;
  }
  /// CAHVOREModel::point_to_pixel (CAHVOREModel.cc:232-301)
  Vector2 point_to_pixel(Vector3 const& point) const {
    const Vector3 p_c = point - C;
    const double zeta = detail::dot3(p_c, O);
    const Vector3 lambda3 = p_c - zeta * O;
    const double lambda = std::sqrt(detail::dot3(lambda3, lambda3));
    double theta = std::atan2(lambda, zeta), dtheta = 1;
    for (int32 n = 0;; ++n) {
      if (n > 100) vw_throw(PointToPixelErr() << "CAHVOREModel: Did not converge.\n");
      if (std::fabs(dtheta) < 1e-8) break;
      const double costh = std::cos(theta), sinth = std::sin(theta);
      const double theta2 = theta * theta, theta3 = theta * theta2, theta4 = theta * theta3;
      const double upsilon = zeta * costh + lambda * sinth - (1 - costh) * (E[0] + E[1] * theta2 + E[2] * theta4) -
                             (theta - sinth) * (2 * E[1] * theta + 4 * E[2] * theta3);
      dtheta = (zeta * sinth - lambda * costh - (theta - sinth) * (E[0] + E[1] * theta2 + E[2] * theta4)) / upsilon;
      theta -= dtheta;
    }
    if ((theta * std::fabs(P)) > 3.14159265358979323846 / 2) vw_throw(PointToPixelErr() << "CAHVOREModel: Theta out of bounds.\n");
    Vector3 rp;
    if (theta < 1e-8) {
      rp = p_c;
    } else {
      const double linth = P * theta;
      double chi;
      if (P < -1e-15) chi = std::sin(linth) / P;
      else if (P > 1e-15) chi = std::tan(linth) / P;
      else chi = theta;
      const double chi2 = chi * chi;
      double mu = R[2];
      mu = R[1] + chi2 * mu;
      mu = R[0] + chi2 * mu;
      rp = (lambda / chi) * O + (1 + mu) * lambda3;
    }
    const double alpha = detail::dot3(rp, A);
    return Vector2(detail::dot3(rp, H) / alpha, detail::dot3(rp, V) / alpha);
  }
  Vector3 camera_center(Vector2 const& = Vector2()) const { return C; }
};

/// linearize_camera(model, input size, output size) for a CAHVORModel (CAHVORModel.cc:460-547) or a CAHVOREModel
/// (CAHVOREModel.cc:303-381): host arithmetic in the engine (vwgpu_linearize_camera).  A CAHVORE landmark ray that does not
/// converge throws PixelToRayErr.
namespace detail {
inline CAHVModel linearize(CameraModel const& camera_model, int32 ix, int32 iy, int32 ox, int32 oy) {
  vwgpu_camera d;
  const int rc = vwgpu_linearize_camera(&camera_model.descriptor(), ix, iy, ox, oy, &d);
  if (rc == VWGPU_ERR_LOGIC) vw_throw(PixelToRayErr() << "CAHVOREModel: Did not converge.\n");
  VW_ASSERT(rc == VWGPU_OK, ArgumentErr() << "linearize_camera: the image sizes must be positive.");
  return CAHVModel(d);
}
}  // namespace detail
inline CAHVModel linearize_camera(CAHVORModel const& camera_model, Vector2i const& cahvor_image_size, Vector2i const& cahv_image_size) {
  return detail::linearize(camera_model, cahvor_image_size[0], cahvor_image_size[1], cahv_image_size[0], cahv_image_size[1]);
}
inline CAHVModel linearize_camera(CAHVORModel const& camera_model, int32 ix, int32 iy, int32 ox, int32 oy) {
  return detail::linearize(camera_model, ix, iy, ox, oy);
}
inline CAHVModel linearize_camera(CAHVOREModel const& camera_model, Vector2i const& cahvore_image_size, Vector2i const& cahv_image_size) {
  return detail::linearize(camera_model, cahvore_image_size[0], cahvore_image_size[1], cahv_image_size[0], cahv_image_size[1]);
}
inline CAHVModel linearize_camera(CAHVOREModel const& camera_model, int32 ix, int32 iy, int32 ox, int32 oy) {
  return detail::linearize(camera_model, ix, iy, ox, oy);
}

/// epipolar(src0, src1, dst0, dst1) for two pinholes (PinholeModel.cc:679-732): host arithmetic in the engine
/// (vwgpu_epipolar_pinhole); cameras without a baseline throw ArgumentErr.
inline void epipolar(PinholeModel const& src_camera0, PinholeModel const& src_camera1, PinholeModel& dst_camera0, PinholeModel& dst_camera1) {
  const Vector3 c0 = src_camera0.camera_center(), c1 = src_camera1.camera_center();
  const Vector2 f0 = src_camera0.focal_length(), f1 = src_camera1.focal_length(), o0 = src_camera0.point_offset(), o1 = src_camera1.point_offset();
  const double center0[3] = {c0[0], c0[1], c0[2]}, center1[3] = {c1[0], c1[1], c1[2]};
  const double focal0[2] = {f0[0], f0[1]}, focal1[2] = {f1[0], f1[1]}, offset0[2] = {o0[0], o0[1]}, offset1[2] = {o1[0], o1[1]};
  double rot[9], focal[2], offset[2], pitch;
  const int rc = vwgpu_epipolar_pinhole(center0, src_camera0.get_rotation_matrix().data(), focal0, offset0, src_camera0.pixel_pitch(), center1,
                                        src_camera1.get_rotation_matrix().data(), focal1, offset1, src_camera1.pixel_pitch(), rot, focal,
                                        offset, &pitch);
  VW_ASSERT(rc == VWGPU_OK, ArgumentErr() << "epipolar: the two cameras have the same centre.");
  Matrix3x3 new_rot;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) new_rot(i, j) = rot[i * 3 + j];
  dst_camera0 = PinholeModel(c0, new_rot, focal[0], focal[1], offset[0], offset[1], NULL, pitch);
  dst_camera1 = PinholeModel(c1, new_rot, focal[0], focal[1], offset[0], offset[1], NULL, pitch);
}

/// epipolar(src0, src1, dst0, dst1) for two CAHV models (CAHVModel.cc:297-337).
inline void epipolar(CAHVModel const& src_camera0, CAHVModel const& src_camera1, CAHVModel& dst_camera0, CAHVModel& dst_camera1) {
  vwgpu_camera d0, d1;
  const int rc = vwgpu_epipolar_cahv(&src_camera0.descriptor(), &src_camera1.descriptor(), &d0, &d1);
  VW_ASSERT(rc == VWGPU_OK, ArgumentErr() << "epipolar: the two cameras have the same centre.");
  dst_camera0 = CAHVModel(d0);
  dst_camera1 = CAHVModel(d1);
}

}  // namespace camera
}  // namespace vw
#endif
