// triangulate_ref.cc — CPU restatement of two-camera triangulation as the reference computes it (test infrastructure
// only; dependency-free): StereoModel for two cameras (src/vw/Stereo/StereoModel.cc), StereoView::operator()
// (src/vw/Stereo/StereoView.h:91-99), UniverseRadiusFunc (:139-222) and the rays of PinholeModel with the null and the
// Tsai lens distortion and of CAHVModel.  Plain scalar loops in raster order, double everywhere, every expression in the
// reference's order; built with -O2 -ffp-contract=off.  The camera is the flat descriptor of the C ABI (vwgpu_camera,
// include/vwgpu.h), declared again here so that this file stands alone.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

namespace {

struct Camera {   // = vwgpu_camera
  int kind, distortion_kind;
  double center[3];
  double inv_camera_transform[9];
  double pixel_pitch, fu, fv, cu, cv;
  double distortion[5];
  double A[3], H[3], V[3];
};
enum { PINHOLE = 0, CAHV = 1, DIST_NULL = 0, DIST_TSAI = 1 };
enum { VIEW = 0, MODEL = 1, LAYOUT_MASK = 0x300, DXDYV = 0, DXDY = 0x100, DV = 0x200, D = 0x300 };
// how NewtonRaphson::solve left: converged on the step, bad determinant, NaN residual, 19 passes used up
enum { EXIT_NONE = 0, EXIT_STEP = 1, EXIT_DET = 2, EXIT_NAN = 3, EXIT_PASSES = 4 };
// what became of a pixel
enum { PX_INVALID = 0, PX_NAN = 1, PX_INVALID_PIXEL = 2, PX_PARALLEL = 3, PX_REFLECTED = 4, PX_POINT = 5 };

struct V3 { double x, y, z; };
struct V2 { double x, y; };

// dot_prod (src/vw/Math/Vector.h:1719-1726): the accumulator starts from zero
double dot(V3 const& a, V3 const& b) {
  double result = 0.0;
  result += a.x * b.x;
  result += a.y * b.y;
  result += a.z * b.z;
  return result;
}
// cross_prod (Vector.h:1738-1743)
V3 cross(V3 const& v1, V3 const& v2) {
  return V3{v1.y * v2.z - v1.z * v2.y, v1.z * v2.x - v1.x * v2.z, v1.x * v2.y - v1.y * v2.x};
}
V3 sub(V3 const& a, V3 const& b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
// norm_2 (Vector.h:1593-1604)
double norm_2(V3 const& v) {
  double result = 0.0;
  result += v.x * v.x;
  result += v.y * v.y;
  result += v.z * v.z;
  return std::sqrt(result);
}
double norm_2(V2 const& v) {
  double result = 0.0;
  result += v.x * v.x;
  result += v.y * v.y;
  return std::sqrt(result);
}
// normalize (Vector.h:1694-1696): every element divided by the norm
V3 normalize(V3 const& v) {
  const double n = norm_2(v);
  return V3{v.x / n, v.y / n, v.z / n};
}
V3 v3(const double* p) { return V3{p[0], p[1], p[2]}; }

// TsaiDistortionNorm (src/vw/Camera/LensDistortion.cc:260-276)
V2 TsaiDistortionNorm(V2 const& P, const double* distortion) {
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
  return V2{x_out, y_out};
}

// TsaiDistortionJacobian (LensDistortion.cc:286-324)
void TsaiDistortionJacobian(V2 const& P, const double* distortion, double* jacobian) {
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

// NewtonRaphson::solve (src/vw/Math/NewtonRaphson.cc:58-119) for the Tsai model and its analytic Jacobian
V2 newton_solve(V2 const& guessX, V2 const& outY, const double* distortion, double tol, int* how) {
  V2 X = guessX;
  V2 bestX = X;
  double best_err = std::numeric_limits<double>::max();
  int count = 1, maxTries = 20;
  while (count < maxTries) {
    const V2 FX = TsaiDistortionNorm(X, distortion);
    V2 F{FX.x - outY.x, FX.y - outY.y};
    if (std::isnan(norm_2(F))) { *how = EXIT_NAN; return bestX; }
    if (norm_2(F) < best_err) {
      best_err = norm_2(F);
      bestX = X;
    }
    double J[4];
    TsaiDistortionJacobian(X, distortion, J);
    double det = J[0] * J[3] - J[1] * J[2];
    if (std::abs(det) < 1e-6 || std::isnan(det)) { *how = EXIT_DET; return bestX; }
    V2 DX;
    DX.x = (J[3] * F.x - J[1] * F.y) / det;
    DX.y = (J[0] * F.y - J[2] * F.x) / det;
    X.x -= DX.x;
    X.y -= DX.y;
    if (norm_2(DX) < tol) { *how = EXIT_STEP; return X; }
    count++;
  }
  *how = EXIT_PASSES;
  return bestX;
}

// TsaiLensDistortion::distorted_coordinates (LensDistortion.cc:345-369)
V2 tsai_distorted(Camera const& c, V2 const& p) {
  if (c.fu < 1e-300 || c.fv < 1e-300) return V2{HUGE_VAL, HUGE_VAL};
  const V2 p_0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const V2 d = TsaiDistortionNorm(p_0, c.distortion);
  double dx = d.x, dy = d.y;
  dx = dx * c.fu + c.cu;
  dy = dy * c.fv + c.cv;
  return V2{dx, dy};
}

// TsaiLensDistortion::undistorted_coordinates (LensDistortion.cc:371-400)
V2 tsai_undistorted(Camera const& c, V2 const& p, int* how) {
  *how = EXIT_NONE;
  if (c.fu < 1e-300 || c.fv < 1e-300) return V2{HUGE_VAL, HUGE_VAL};
  const V2 p_0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  double tol = 1e-9;
  const V2 U = newton_solve(p_0, p_0, c.distortion, tol, how);
  double ux = U.x, uy = U.y;
  ux = ux * c.fu + c.cu;
  uy = uy * c.fv + c.cv;
  return V2{ux, uy};
}

// PinholeModel::pixel_to_vector (src/vw/Camera/PinholeModel.cc:422-430), CAHVModel::pixel_to_vector
// (src/vw/Camera/CAHVModel.cc:173-185)
V3 pixel_to_vector(Camera const& c, V2 const& pix, int* how) {
  *how = EXIT_NONE;
  if (c.kind == CAHV) {
    const V3 A = v3(c.A), H = v3(c.H), V = v3(c.V);
    V3 vec = normalize(cross(V3{V.x - pix.y * A.x, V.y - pix.y * A.y, V.z - pix.y * A.z},
                             V3{H.x - pix.x * A.x, H.y - pix.x * A.y, H.z - pix.x * A.z}));
    if (dot(cross(V, H), A) < 0.0) {
      vec.x *= -1.0;
      vec.y *= -1.0;
      vec.z *= -1.0;
    }
    return vec;
  }
  V2 undistorted_pix{pix.x * c.pixel_pitch, pix.y * c.pixel_pitch};
  if (c.distortion_kind == DIST_TSAI) undistorted_pix = tsai_undistorted(c, undistorted_pix, how);
  const V3 p{undistorted_pix.x, undistorted_pix.y, 1};
  const double* m = c.inv_camera_transform;   // MatrixVectorProduct (src/vw/Math/Matrix.h:1977-1980): a dot_prod per row
  return normalize(V3{dot(v3(m), p), dot(v3(m + 3), p), dot(v3(m + 6), p)});
}

// triangulate_pair (src/vw/Stereo/StereoModel.cc:35-48)
V3 triangulate_pair(V3 const& dir0, V3 const& ctr0, V3 const& dir1, V3 const& ctr1, V3& errorVec) {
  V3 v12 = cross(dir0, dir1);
  V3 v1 = cross(v12, dir0);
  V3 v2 = cross(v12, dir1);
  const double s1 = dot(v2, sub(ctr1, ctr0)) / dot(v2, dir0), s2 = dot(v1, sub(ctr0, ctr1)) / dot(v1, dir1);
  V3 closestPoint1{ctr0.x + s1 * dir0.x, ctr0.y + s1 * dir0.y, ctr0.z + s1 * dir0.z};
  V3 closestPoint2{ctr1.x + s2 * dir1.x, ctr1.y + s2 * dir1.y, ctr1.z + s2 * dir1.z};
  errorVec = sub(closestPoint1, closestPoint2);
  return V3{0.5 * (closestPoint1.x + closestPoint2.x), 0.5 * (closestPoint1.y + closestPoint2.y),
            0.5 * (closestPoint1.z + closestPoint2.z)};
}

bool skipped(V2 const& pix) { return pix.x != pix.x || pix.y != pix.y; }
bool is_invalid_pixel(V2 const& pix) { return pix.x == -1e8 && pix.y == -1e8; }   // CameraModel::invalid_pixel()

// StereoModel::operator()(pixVec, errorVec) for two cameras (StereoModel.cc:97-147) with are_nearly_parallel (:68-91)
V3 stereo_model(Camera const& cam1, Camera const& cam2, double angle_tol, V2 const& pix1, V2 const& pix2, V3& errorVec, int* cls,
                int* how1, int* how2) {
  errorVec = V3{0, 0, 0};
  *how1 = *how2 = EXIT_NONE;
  if (skipped(pix1) || skipped(pix2)) { *cls = PX_NAN; return V3{0, 0, 0}; }
  if (is_invalid_pixel(pix1) || is_invalid_pixel(pix2)) { *cls = PX_INVALID_PIXEL; return V3{0, 0, 0}; }
  const V3 dir0 = pixel_to_vector(cam1, pix1, how1), dir1 = pixel_to_vector(cam2, pix2, how2);
  const V3 ctr0 = v3(cam1.center), ctr1 = v3(cam2.center);
  double tol = 1e-4;
  if (angle_tol > 0) tol = angle_tol;
  bool are_par = true;
  if (1 - dot(dir0, dir1) >= tol) are_par = false;
  if (are_par) { *cls = PX_PARALLEL; return V3{0, 0, 0}; }
  V3 result = triangulate_pair(dir0, ctr0, dir1, ctr1, errorVec);
  bool reflect = false;
  if (dot(sub(result, ctr0), dir0) < 0) reflect = true;
  if (dot(sub(result, ctr1), dir1) < 0) reflect = true;
  if (reflect) result = V3{-result.x + 2 * ctr0.x, -result.y + 2 * ctr0.y, -result.z + 2 * ctr0.z};
  *cls = reflect ? PX_REFLECTED : PX_POINT;
  return result;
}

// one disparity pixel in the layouts of DispHelper (StereoView.h:37-53)
template <class T>
bool load_disp(const T* disp, int layout, long long i, T& dx, T& dy) {
  switch (layout) {
    case DXDYV: dx = disp[3 * i]; dy = disp[3 * i + 1]; return disp[3 * i + 2] != 0;
    case DXDY: dx = disp[2 * i]; dy = disp[2 * i + 1]; return true;
    case DV: dx = disp[2 * i]; dy = 0; return disp[2 * i + 1] != 0;
    default: dx = disp[i]; dy = 0; return true;
  }
}

// the pixel pair: StereoView.h:94-95 (a double add) or StereoModel.cc:278-280 (int32 + channel in the channel's
// arithmetic type, then widened)
void pixel_pair(int model, int x, int y, float dx, float dy, V2& pix1, V2& pix2) {
  pix1 = V2{(double)x, (double)y};
  if (model) {
    const float fx = x + dx, fy = y + dy;
    pix2 = V2{fx, fy};
  } else {
    pix2 = V2{pix1.x + (double)dx, pix1.y + (double)dy};
  }
}
void pixel_pair(int model, int x, int y, int32_t dx, int32_t dy, V2& pix1, V2& pix2) {
  pix1 = V2{(double)x, (double)y};
  if (model) {
    const int32_t ix = (int32_t)((uint32_t)x + (uint32_t)dx), iy = (int32_t)((uint32_t)y + (uint32_t)dy);
    pix2 = V2{(double)ix, (double)iy};
  } else {
    pix2 = V2{pix1.x + (double)dx, pix1.y + (double)dy};
  }
}

struct Stats {
  long long point_count;
  double max_error, sum_error;
};

template <class T>
void triangulate_image(const T* disp, int w, int h, int x0, int y0, Camera const& cam1, Camera const& cam2, double angle_tol,
                       int semantics, double* xyz, double* error, double* errvec, Stats* stats, int32_t* classes) {
  const int layout = semantics & LAYOUT_MASK, model = (semantics & ~LAYOUT_MASK) == MODEL;
  // StereoModel.cc:258-261, :283-293
  double mean_error = 0.0, max_error = 0.0;
  long long point_count = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const long long i = (long long)y * w + x;
      T dx, dy;
      V3 p{0, 0, 0}, ev{0, 0, 0};
      double err = 0;
      int cls = PX_INVALID, how1 = EXIT_NONE, how2 = EXIT_NONE;
      if (load_disp(disp, layout, i, dx, dy)) {
        V2 pix1, pix2;
        pixel_pair(model, x0 + x, y0 + y, dx, dy, pix1, pix2);
        p = stereo_model(cam1, cam2, angle_tol, pix1, pix2, ev, &cls, &how1, &how2);
        err = norm_2(ev);
        if (err >= 0) {
          if (err > max_error) max_error = err;
          mean_error += err;
          ++point_count;
        } else if (model) {
          p = V3{0, 0, 0};
        }
      }
      xyz[3 * i] = p.x; xyz[3 * i + 1] = p.y; xyz[3 * i + 2] = p.z;
      if (error) error[i] = err;
      if (errvec) { errvec[3 * i] = ev.x; errvec[3 * i + 1] = ev.y; errvec[3 * i + 2] = ev.z; }
      if (classes) { classes[3 * i] = cls; classes[3 * i + 1] = how1; classes[3 * i + 2] = how2; }
    }
  if (stats) {
    stats->point_count = point_count;
    stats->max_error = max_error;
    stats->sum_error = mean_error;
  }
}

template <class T>
void angle_image(const T* disp, int w, int h, int x0, int y0, Camera const& cam1, Camera const& cam2, int semantics, double* out) {
  const int layout = semantics & LAYOUT_MASK, model = (semantics & ~LAYOUT_MASK) == MODEL;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const long long i = (long long)y * w + x;
      T dx, dy;
      double ang = 0;
      if (load_disp(disp, layout, i, dx, dy)) {
        V2 pix1, pix2;
        int how;
        pixel_pair(model, x0 + x, y0 + y, dx, dy, pix1, pix2);
        // StereoModel::convergence_angle (StereoModel.cc:174-177)
        ang = std::acos(dot(pixel_to_vector(cam1, pix1, &how), pixel_to_vector(cam2, pix2, &how)));
      }
      out[i] = ang;
    }
}

void mat_mul(const double* a, const double* b, double* out) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[k * 3 + j];
      out[i * 3 + j] = s;
    }
}
void mat_inverse(const double* m, double* out) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  out[0] = c00 / det; out[1] = (m[2] * m[7] - m[1] * m[8]) / det; out[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  out[3] = c01 / det; out[4] = (m[0] * m[8] - m[2] * m[6]) / det; out[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  out[6] = c02 / det; out[7] = (m[1] * m[6] - m[0] * m[7]) / det; out[8] = (m[0] * m[4] - m[1] * m[3]) / det;
}

}  // namespace

extern "C" {

int trr_camera_size() { return (int)sizeof(Camera); }

// PinholeModel::rebuild_camera_matrix (src/vw/Camera/PinholeModel.cc:553-605) into the flat descriptor; the inverses are
// plain adjugates
int trr_pinhole_camera(const double* center, const double* rotation, double fu, double fv, double cu, double cv, const double* u,
                       const double* v, const double* w, double pixel_pitch, int distortion_kind, const double* distortion, void* out) {
  if (!(dot(v3(u), v3(v)) == 0) || !(dot(v3(u), v3(w)) == 0) || !(dot(v3(v), v3(w)) == 0)) return -1;
  if (!(std::fabs(norm_2(v3(u)) - 1) < 0.001) || !(std::fabs(norm_2(v3(v)) - 1) < 0.001) || !(std::fabs(norm_2(v3(w)) - 1) < 0.001)) return -1;
  Camera c;
  std::memset(&c, 0, sizeof(c));
  c.kind = PINHOLE;
  c.distortion_kind = distortion_kind;
  std::memcpy(c.center, center, sizeof(c.center));
  c.pixel_pitch = pixel_pitch;
  c.fu = fu; c.fv = fv; c.cu = cu; c.cv = cv;
  if (distortion) std::memcpy(c.distortion, distortion, sizeof(c.distortion));
  const double uvw[9] = {u[0], u[1], u[2], v[0], v[1], v[2], w[0], w[1], w[2]};
  const double rt[9] = {rotation[0], rotation[3], rotation[6], rotation[1], rotation[4], rotation[7], rotation[2], rotation[5], rotation[8]};
  const double k[9] = {fu, 0, cu, 0, fv, cv, 0, 0, 1};
  double ext[9], ext_inv[9], k_inv[9];
  mat_mul(uvw, rt, ext);
  mat_inverse(ext, ext_inv);
  mat_inverse(k, k_inv);
  mat_mul(ext_inv, k_inv, c.inv_camera_transform);
  std::memcpy(out, &c, sizeof(c));
  return 0;
}

// type 0 = int32, 1 = float pixels; dense images; classes (optional) int32[3] per pixel: {what became of the pixel,
// how the Tsai solver of camera 1 left, of camera 2}
int trr_stereo_triangulate(int type, const void* disp, int w, int h, int x0, int y0, const void* cam1, const void* cam2, double angle_tol,
                           int semantics, double* xyz, double* error, double* errvec, void* stats, int32_t* classes) {
  if (!disp || !xyz || !cam1 || !cam2 || w <= 0 || h <= 0) return -1;
  Camera c1, c2;
  std::memcpy(&c1, cam1, sizeof(c1));
  std::memcpy(&c2, cam2, sizeof(c2));
  if (type == 0)
    triangulate_image(static_cast<const int32_t*>(disp), w, h, x0, y0, c1, c2, angle_tol, semantics, xyz, error, errvec,
                      static_cast<Stats*>(stats), classes);
  else
    triangulate_image(static_cast<const float*>(disp), w, h, x0, y0, c1, c2, angle_tol, semantics, xyz, error, errvec,
                      static_cast<Stats*>(stats), classes);
  return 0;
}

int trr_convergence_angle(int type, const void* disp, int w, int h, int x0, int y0, const void* cam1, const void* cam2, int semantics,
                          double* out) {
  if (!disp || !out || !cam1 || !cam2 || w <= 0 || h <= 0) return -1;
  Camera c1, c2;
  std::memcpy(&c1, cam1, sizeof(c1));
  std::memcpy(&c2, cam2, sizeof(c2));
  if (type == 0) angle_image(static_cast<const int32_t*>(disp), w, h, x0, y0, c1, c2, semantics, out);
  else angle_image(static_cast<const float*>(disp), w, h, x0, y0, c1, c2, semantics, out);
  return 0;
}

// UniverseRadiusFunc::operator() (src/vw/Stereo/StereoView.h:172-220); counts = {total_points, rejected_points}
int trr_universe_radius(const double* points, int channels, int w, int h, const double* origin, double near_radius, double far_radius,
                        double* out, long long* counts) {
  if (!(near_radius >= 0 && far_radius >= 0) || !(near_radius <= far_radius)) return -1;   // the constructor's asserts (:160-163)
  long long total = 0, rejected = 0;
  for (long long i = 0; i < (long long)w * h; ++i) {
    const double* pix = points + i * channels;
    double* o = out + i * channels;
    total++;
    bool keep = false;
    if (pix[0] != 0 || pix[1] != 0 || pix[2] != 0) {
      const double dist = norm_2(V3{pix[0] - origin[0], pix[1] - origin[1], pix[2] - origin[2]});
      if ((near_radius != 0 && dist < near_radius) || (far_radius != 0 && dist > far_radius)) rejected++;
      else keep = true;
    }
    double tmp[6];
    for (int k = 0; k < channels; ++k) tmp[k] = keep ? pix[k] : 0.0;
    for (int k = 0; k < channels; ++k) o[k] = tmp[k];
  }
  if (counts) { counts[0] = total; counts[1] = rejected; }
  return 0;
}

void trr_pixel_to_vector(const void* cam, double x, double y, double* out3, int* how) {
  Camera c;
  std::memcpy(&c, cam, sizeof(c));
  const V3 d = pixel_to_vector(c, V2{x, y}, how);
  out3[0] = d.x; out3[1] = d.y; out3[2] = d.z;
}
void trr_tsai_distorted(const void* cam, double x, double y, double* out2) {
  Camera c;
  std::memcpy(&c, cam, sizeof(c));
  const V2 d = tsai_distorted(c, V2{x, y});
  out2[0] = d.x; out2[1] = d.y;
}
void trr_tsai_undistorted(const void* cam, double x, double y, double* out2, int* how) {
  Camera c;
  std::memcpy(&c, cam, sizeof(c));
  const V2 d = tsai_undistorted(c, V2{x, y}, how);
  out2[0] = d.x; out2[1] = d.y;
}

}  // extern "C"
