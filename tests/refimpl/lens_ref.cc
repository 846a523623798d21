// lens_ref.cc — CPU restatement of five lens distortion models of the reference and of the pinhole camera around them (test
// infrastructure only; dependency-free): FovLensDistortion (src/vw/Camera/LensDistortion.cc:462-515), FisheyeLensDistortion
// (:573-658), BrownConradyDistortion (:731-744), AdjustableTsaiLensDistortion (:799-880), PhotometrixLensDistortion
// (:961-999), the base class's LensDistortion::distorted_coordinates (:175-195) over levenberg_marquardtFixed
// (src/vw/Math/LevenbergMarquardt.h:336-561), NewtonRaphson::solve with numericalJacobian (src/vw/Math/NewtonRaphson.cc:27-119),
// PinholeModel::pixel_to_vector and point_to_pixel around a lens (src/vw/Camera/PinholeModel.cc:351-430), and the
// compositions the library offers: camera_transform, CameraTransform and StereoModel.  Written from the reference's text.
// A lens is its kind and the plain parameter vector of distortion_parameters(), not the packed words of the C ABI; what a
// class precomputes (FOV) is computed here.  The geometry of the pinhole (centre, inverse camera transform, camera matrix)
// and everything after the lens (CAHV, the bilinear tap, the disparity layouts, triangulate_pair) are those of
// triangulate_ref.cc and epipolar_ref.cc, included below.  Built with -O2 -ffp-contract=off.
#include "epipolar_ref.cc"

namespace {

enum { L_NULL = 0, L_TSAI = 1, L_FOV = 2, L_FISHEYE = 3, L_BROWN_CONRADY = 4, L_ADJUSTABLE_TSAI = 6, L_PHOTOMETRIX = 7 };
enum { LS_OK = 0, LS_INACCURATE = 1, LS_LENS = 3 };   // a projection: fine, the failed round trip, "LensDistortion: Did not converge."

// the parameters of a lens, and what PinholeModel hands a lens of itself
struct Lens {
  int kind, n;
  double p[13];
};
struct Intrinsics {
  double fu, fv, cu, cv;
};

// ---- Vector2 arithmetic as the expression templates evaluate it: element by element ------------------------------------
V2 vsub(V2 const& a, V2 const& b) { return V2{a.x - b.x, a.y - b.y}; }
V2 vadd(V2 const& a, V2 const& b) { return V2{a.x + b.x, a.y + b.y}; }
V2 vscale(double s, V2 const& a) { return V2{s * a.x, s * a.y}; }
V2 vdiv(V2 const& a, double s) { return V2{a.x / s, a.y / s}; }
V2 elem_prod(V2 const& a, V2 const& b) { return V2{a.x * b.x, a.y * b.y}; }
V2 elem_quot(V2 const& a, V2 const& b) { return V2{a.x / b.x, a.y / b.y}; }
double norm_2_sqr(V2 const& v) {
  double result = 0.0;
  result += v.x * v.x;
  result += v.y * v.y;
  return result;
}
V2 huge() { return V2{HUGE_VAL, HUGE_VAL}; }

// ---- the normalised models ---------------------------------------------------------------------------------------------
// fishEyeDistortionNorm (LensDistortion.cc:573-598)
V2 fishEyeDistortionNorm(V2 const& P, Lens const& l) {
  double k1 = l.p[0], k2 = l.p[1], k3 = l.p[2], k4 = l.p[3];
  double x = P.x;
  double y = P.y;
  double r2 = x * x + y * y;
  double r = std::sqrt(r2);
  double theta = std::atan(r);
  double theta1 = theta * theta;
  double theta2 = theta1 * theta1;
  double theta3 = theta2 * theta1;
  double theta4 = theta2 * theta2;
  double theta_d = theta * (1 + k1 * theta1 + k2 * theta2 + k3 * theta3 + k4 * theta4);
  double scale = 1.0;
  if (r > 1e-8) scale = theta_d / r;
  return V2{x * scale, y * scale};
}

// AdjTsaiDistortionNorm (LensDistortion.cc:799-824)
V2 AdjTsaiDistortionNorm(V2 const& p_0, Lens const& l) {
  const double* distortion = l.p;
  const int size = l.n;
  double r2 = norm_2_sqr(p_0);
  double r_n = 1, radial = 0;
  for (int i = 0; i < size - 3; i++) {
    r_n *= r2;
    radial += distortion[i] * r_n;
  }
  V2 tangent{0, 0};
  V2 swap_coeff{distortion[size - 2], distortion[size - 3]};
  V2 twice_sq = vscale(2, elem_prod(p_0, p_0));
  tangent = vadd(tangent, elem_prod(swap_coeff, V2{r2 + twice_sq.x, r2 + twice_sq.y}));
  double two_prod = 2 * (p_0.x * p_0.y);
  tangent = vadd(tangent, V2{two_prod * distortion[size - 3], two_prod * distortion[size - 2]});
  V2 result = vadd(vadd(p_0, tangent), vscale(radial, p_0));
  result = vadd(result, V2{distortion[size - 1] * result.y, 0});
  return result;
}

V2 norm_model(Lens const& l, V2 const& P) { return l.kind == L_FISHEYE ? fishEyeDistortionNorm(P, l) : AdjTsaiDistortionNorm(P, l); }

// numericalJacobian::operator() (NewtonRaphson.cc:27-47)
void numericalJacobian(Lens const& l, V2 const& P, double step, double* jacobian) {
  V2 dx{step, 0};
  V2 JX = vdiv(vsub(norm_model(l, vadd(P, dx)), norm_model(l, vsub(P, dx))), 2 * step);
  V2 dy{0, step};
  V2 JY = vdiv(vsub(norm_model(l, vadd(P, dy)), norm_model(l, vsub(P, dy))), 2 * step);
  jacobian[0] = JX.x;
  jacobian[1] = JY.x;
  jacobian[2] = JX.y;
  jacobian[3] = JY.y;
}

// NewtonRaphson::solve (NewtonRaphson.cc:58-119) with the numerical Jacobian; *how: an EXIT_ value of triangulate_ref.cc
V2 newton_numeric(Lens const& l, V2 const& guessX, V2 const& outY, double step_size, double tol, int* how) {
  V2 X = guessX;
  V2 bestX = X;
  double best_err = std::numeric_limits<double>::max();
  int count = 1, maxTries = 20;
  while (count < maxTries) {
    V2 F = vsub(norm_model(l, X), outY);
    if (std::isnan(norm_2(F))) { *how = EXIT_NAN; return bestX; }
    if (norm_2(F) < best_err) {
      best_err = norm_2(F);
      bestX = X;
    }
    double J[4];
    numericalJacobian(l, X, step_size, J);
    double det = J[0] * J[3] - J[1] * J[2];
    if (std::abs(det) < 1e-6 || std::isnan(det)) { *how = EXIT_DET; return bestX; }
    V2 DX;
    DX.x = (J[3] * F.x - J[1] * F.y) / det;
    DX.y = (J[0] * F.y - J[2] * F.x) / det;
    X = vsub(X, DX);
    if (norm_2(DX) < tol) { *how = EXIT_STEP; return X; }
    count++;
  }
  *how = EXIT_PASSES;
  return bestX;
}

// ---- undistorted_coordinates -------------------------------------------------------------------------------------------
V2 fov_undistorted(Intrinsics const& k, Lens const& l, V2 const& p) {   // :490-515
  V2 focal{k.fu, k.fv}, offset{k.cu, k.cv};
  if (focal.x < 1e-300 || focal.y < 1e-300) return huge();
  const double precalc2 = 2 * std::tan(l.p[0] / 2);
  V2 p_0 = elem_quot(vsub(p, offset), focal);
  double rd = norm_2(p_0);
  double ru = std::tan(rd * l.p[0]) / precalc2;
  double conv = 1.0;
  if (rd > 1e-8) conv = ru / rd;
  return vadd(elem_prod(vscale(conv, p_0), focal), offset);
}

V2 newton_undistorted(Intrinsics const& k, Lens const& l, V2 const& p, int* how) {   // :634-658, :851-880
  V2 focal{k.fu, k.fv}, offset{k.cu, k.cv};
  if (focal.x < 1e-300 || focal.y < 1e-300) return huge();
  V2 p_0 = elem_quot(vsub(p, offset), focal);
  double step = 1e-6, tol = 1e-9;
  V2 U = newton_numeric(l, p_0, p_0, step, tol, how);
  return vadd(elem_prod(U, focal), offset);
}

V2 brown_conrady_undistorted(Intrinsics const& k, Lens const& l, V2 const& p) {   // :731-744
  V2 offset{k.cu, k.cv}, principal{l.p[0], l.p[1]};
  const double* radial_d = l.p + 2;
  const double* centering = l.p + 5;
  const double angle = l.p[7];
  V2 intermediate = vsub(vsub(p, principal), offset);
  double r2 = norm_2_sqr(intermediate);
  double radial = 1 + radial_d[0] * r2 + radial_d[1] * r2 * r2 + radial_d[2] * r2 * r2 * r2;
  double tangential = centering[0] * r2 + centering[1] * r2 * r2;
  intermediate = vscale(radial, intermediate);
  intermediate.x -= tangential * std::sin(angle);
  intermediate.y += tangential * std::cos(angle);
  return vadd(intermediate, offset);
}

V2 photometrix_undistorted(Intrinsics const& k, Lens const& l, V2 const& p) {   // :961-999
  double x_meas = p.x;
  double y_meas = p.y;
  double xp = l.p[0] + k.cu;
  double yp = l.p[1] + k.cv;
  double x = x_meas - xp;
  double y = y_meas - yp;
  double x2 = x * x;
  double y2 = y * y;
  double r2 = x2 + y2;
  double K1 = l.p[2], K2 = l.p[3], K3 = l.p[4], P1 = l.p[5], P2 = l.p[6];
  double drr = K1 * r2 + K2 * r2 * r2 + K3 * r2 * r2 * r2;
  double x_corr = x_meas + x * drr + P1 * (r2 + 2.0 * x2) + 2.0 * P2 * x * y;
  double y_corr = y_meas + y * drr + P2 * (r2 + 2.0 * y2) + 2.0 * P1 * x * y;
  return V2{x_corr, y_corr};
}

Camera tsai_camera(Intrinsics const& k, Lens const& l) {
  Camera c{};
  c.distortion_kind = DIST_TSAI;
  c.fu = k.fu; c.fv = k.fv; c.cu = k.cu; c.cv = k.cv;
  for (int i = 0; i < 5; ++i) c.distortion[i] = i < l.n ? l.p[i] : 0.0;
  return c;
}

V2 lens_undistorted(Intrinsics const& k, Lens const& l, V2 const& p, int* how) {
  *how = EXIT_NONE;
  switch (l.kind) {
    case L_TSAI: return tsai_undistorted(tsai_camera(k, l), p, how);
    case L_FOV: return fov_undistorted(k, l, p);
    case L_FISHEYE:
    case L_ADJUSTABLE_TSAI: return newton_undistorted(k, l, p, how);
    case L_BROWN_CONRADY: return brown_conrady_undistorted(k, l, p);
    case L_PHOTOMETRIX: return photometrix_undistorted(k, l, p);
    default: return p;
  }
}

// ---- distorted_coordinates ---------------------------------------------------------------------------------------------
V2 fov_distorted(Intrinsics const& k, Lens const& l, V2 const& p) {   // :462-488
  V2 focal{k.fu, k.fv}, offset{k.cu, k.cv};
  if (focal.x < 1e-300 || focal.y < 1e-300) return huge();
  const double precalc1 = 1 / l.p[0], precalc2 = 2 * std::tan(l.p[0] / 2);
  V2 p_0 = elem_quot(vsub(p, offset), focal);
  double ru = norm_2(p_0);
  double rd = std::atan(ru * precalc2) * precalc1;
  double conv = 1.0;
  if (ru > 1e-8) conv = rd / ru;
  return vadd(elem_prod(vscale(conv, p_0), focal), offset);
}

V2 norm_distorted(Intrinsics const& k, Lens const& l, V2 const& p) {   // :612-632, :832-849
  V2 focal{k.fu, k.fv}, offset{k.cu, k.cv};
  if (focal.x < 1e-300 || focal.y < 1e-300) return huge();
  V2 p_0 = elem_quot(vsub(p, offset), focal);
  return vadd(elem_prod(norm_model(l, p_0), focal), offset);
}

// DistortOptimizeFunctor (:29-41) with LeastSquaresModelBaseFixed<., 2, 2> (LevenbergMarquardt.h:336-383)
struct DistortOptimizeFunctor {
  Intrinsics const& k;
  Lens const& l;
  V2 operator()(V2 const& x) const { int how; return lens_undistorted(k, l, x, &how); }
  V2 difference(V2 const& a, V2 const& b) const { return vsub(a, b); }
  // H(row, col): row-major 2 x 2
  void jacobian(V2 const& x, double H[2][2]) const {
    V2 h0 = (*this)(x);
    for (int i = 0; i < 2; ++i) {
      double xi[2] = {x.x, x.y};
      double epsilon = 1e-7 + std::fabs(xi[i] * 1e-7);
      xi[i] += epsilon;
      V2 hi = (*this)(V2{xi[0], xi[1]});
      V2 col = vdiv(difference(hi, h0), epsilon);
      H[0][i] = col.x;
      H[1][i] = col.y;
    }
  }
};

// levenberg_marquardtFixed (LevenbergMarquardt.h:389-561) for NI = NO = 2; *lapack: the branch that leaves for LAPACK was
// reached (det(hessian_lm) > 0.0 did not hold), which this restatement does not follow
V2 levenberg_marquardtFixed(DistortOptimizeFunctor const& model, V2 const& seed, V2 const& observation, double abs_tolerance,
                            double rel_tolerance, double max_iterations, bool* lapack) {
  *lapack = false;
  bool done = false;
  double Rinv = 10;
  double lambda = 0.1;
  V2 x_try{0, 0}, x = seed;
  V2 h = model(x);
  V2 error = model.difference(observation, h);
  double norm_start = norm_2(error);
  if (norm_start < abs_tolerance) done = true;
  double J[2][2], J_trans[2][2], J_trans_J[2][2], hessian[2][2], hessian_lm[2][2], hessian_lm_inv[2][2];
  double del_J[2];
  int outer_iter = 0;
  while (!done) {
    bool shortCircuit = false;
    outer_iter++;
    h = model(x);
    error = model.difference(observation, h);
    norm_start = norm_2(error);
    model.jacobian(x, J);
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j) J_trans[i][j] = J[j][i];
    const double e[2] = {error.x, error.y};
    for (int i = 0; i < 2; ++i) {   // -1.0 * Rinv * (J_trans * error): a dot_prod per row
      double s = 0.0;
      for (int q = 0; q < 2; ++q) s += J_trans[i][q] * e[q];
      del_J[i] = -1.0 * Rinv * s;
    }
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j) {
        double s = 0.0;
        for (int q = 0; q < 2; ++q) s += J_trans[i][q] * J[q][j];
        J_trans_J[i][j] = s;
        hessian[i][j] = Rinv * J_trans_J[i][j];
      }
    int iterations = 0;
    double norm_try = norm_start + 1.0;
    while (norm_try > norm_start) {
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) hessian_lm[i][j] = hessian[i][j];
      for (int i = 0; i < 2; ++i) hessian_lm[i][i] += hessian_lm[i][i] * lambda + lambda;
      const double* d = &hessian_lm[0][0];
      double det = d[0] * d[3] - d[1] * d[2];
      if (!(det > 0.0)) {
        *lapack = true;
        return x;
      }
      // inverse(Matrix<T, 2, 2>) (Math/Matrix.h:2209-2216)
      hessian_lm_inv[0][0] = d[3] / det;
      hessian_lm_inv[0][1] = -d[1] / det;
      hessian_lm_inv[1][0] = -d[2] / det;
      hessian_lm_inv[1][1] = d[0] / det;
      double delta_x[2];
      for (int i = 0; i < 2; ++i) {
        double s = 0.0;
        for (int q = 0; q < 2; ++q) s += hessian_lm_inv[i][q] * del_J[q];
        delta_x[i] = s;
      }
      x_try = V2{x.x - delta_x[0], x.y - delta_x[1]};
      V2 h_try = model(x_try);
      V2 error_try = model.difference(observation, h_try);
      norm_try = norm_2(error_try);
      if (norm_try > norm_start) lambda *= 10;
      ++iterations;
      if (iterations > 5) {
        shortCircuit = true;
        norm_try = norm_start;
      }
    }
    if (!shortCircuit && ((norm_start - norm_try) / norm_start) < rel_tolerance) done = true;
    if (norm_try < abs_tolerance) done = true;
    if (outer_iter >= max_iterations) done = true;
    if (!shortCircuit) x = x_try;
    norm_start = norm_try;
    lambda /= 10;
  }
  return x;
}

// LensDistortion::distorted_coordinates (:175-195); false where it throws PointToPixelErr (or would go to LAPACK)
bool solver_distorted(Intrinsics const& k, Lens const& l, V2 const& v, V2& solution) {
  DistortOptimizeFunctor model{k, l};
  bool lapack;
  solution = levenberg_marquardtFixed(model, v, v, 1e-16, 1e-16, 100, &lapack);
  if (lapack) return false;
  V2 undist = model(solution);
  double err = norm_2(vsub(undist, v)) / std::max(norm_2(v), 0.1);
  double tol = 1e-10;
  if (err > tol) return false;
  return true;
}

bool lens_distorted(Intrinsics const& k, Lens const& l, V2 const& p, V2& out) {
  switch (l.kind) {
    case L_TSAI: out = tsai_distorted(tsai_camera(k, l), p); return true;
    case L_FOV: out = fov_distorted(k, l, p); return true;
    case L_FISHEYE:
    case L_ADJUSTABLE_TSAI: out = norm_distorted(k, l, p); return true;
    case L_BROWN_CONRADY:
    case L_PHOTOMETRIX: return solver_distorted(k, l, p, out);
    default: out = p; return true;
  }
}

// ---- the pinhole around the lens ---------------------------------------------------------------------------------------
// geometry: the descriptor of the pinhole without its lens (or a CAHV camera, whose lens is ignored), and its camera matrix
struct LensCamera {
  Camera geo;
  const double* matrix;
  Lens lens;
  Intrinsics intrinsics() const { return Intrinsics{geo.fu, geo.fv, geo.cu, geo.cv}; }
};

// PinholeModel::pixel_to_vector (PinholeModel.cc:422-430)
V3 lens_pixel_to_vector(LensCamera const& c, V2 const& pix, int* how) {
  if (c.geo.kind == CAHV) return pixel_to_vector(c.geo, pix, how);
  V2 undistorted_pix = lens_undistorted(c.intrinsics(), c.lens, V2{pix.x * c.geo.pixel_pitch, pix.y * c.geo.pixel_pitch}, how);
  const V3 p{undistorted_pix.x, undistorted_pix.y, 1};
  const double* m = c.geo.inv_camera_transform;
  return normalize(V3{dot(v3(m), p), dot(v3(m + 3), p), dot(v3(m + 6), p)});
}

// PinholeModel::point_to_pixel (PinholeModel.cc:351-397)
int lens_point_to_pixel(LensCamera const& c, V3 const& point, int check, V2& final_pixel) {
  if (c.geo.kind == CAHV) {
    point_to_pixel(c.geo, nullptr, point, check, final_pixel);
    return LS_OK;
  }
  const double* m = c.matrix;
  double den = m[8] * point.x + m[9] * point.y + m[10] * point.z + m[11];
  V2 pixel{(m[0] * point.x + m[1] * point.y + m[2] * point.z + m[3]) / den, (m[4] * point.x + m[5] * point.y + m[6] * point.z + m[7]) / den};
  V2 distorted;
  if (!lens_distorted(c.intrinsics(), c.lens, pixel, distorted)) return LS_LENS;
  final_pixel = V2{distorted.x / c.geo.pixel_pitch, distorted.y / c.geo.pixel_pitch};
  if (!check) return LS_OK;
  const double ERROR_THRESHOLD = 0.01;
  int how;
  V3 pixel_vector = lens_pixel_to_vector(c, final_pixel, &how);
  V3 phys_vector = normalize(sub(point, v3(c.geo.center)));
  double diff = norm_2(sub(pixel_vector, phys_vector));
  if (diff >= ERROR_THRESHOLD) diff = norm_2(add(pixel_vector, phys_vector));
  if (diff >= ERROR_THRESHOLD || diff != diff) return LS_INACCURATE;
  return LS_OK;
}

int lens_transform(LensCamera const& from, LensCamera const& to, int check, V2 const& p, V2& q) {
  int how;
  V3 vec = lens_pixel_to_vector(from, p, &how);
  return lens_point_to_pixel(to, add(vec, v3(from.geo.center)), check, q);
}

LensCamera make_camera(const void* cam, const double* matrix, int kind, const double* params, int n) {
  LensCamera c{};
  std::memcpy(&c.geo, cam, sizeof(c.geo));
  c.geo.distortion_kind = DIST_NULL;
  c.matrix = matrix;
  c.lens.kind = kind;
  c.lens.n = n;
  for (int i = 0; i < n && i < 13; ++i) c.lens.p[i] = params[i];
  return c;
}

const double NaN = std::numeric_limits<double>::quiet_NaN();

}  // namespace

extern "C" {

// direction 0: distorted_coordinates, 1: undistorted_coordinates, of n points; intrinsics = {fu, fv, cu, cv}.  how (optional)
// receives per point the exit of the Newton solver (undistort: an EXIT_ value) or 1 where the solve failed (distort).
// Returns the number of failed points, which are NaN pairs.
long long lnr_coordinates(const double* intrinsics, int kind, const double* params, int np, int direction, const double* points,
                          long long n, double* out, int* how) {
  Intrinsics k{intrinsics[0], intrinsics[1], intrinsics[2], intrinsics[3]};
  Lens l{};
  l.kind = kind;
  l.n = np;
  for (int i = 0; i < np && i < 13; ++i) l.p[i] = params[i];
  long long failed = 0;
  for (long long i = 0; i < n; ++i) {
    V2 p{points[2 * i], points[2 * i + 1]}, q{0, 0};
    int h = 0;
    if (direction == 1) {
      q = lens_undistorted(k, l, p, &h);
    } else if (!lens_distorted(k, l, p, q)) {
      q = V2{NaN, NaN};
      h = 1;
      ++failed;
    }
    out[2 * i] = q.x;
    out[2 * i + 1] = q.y;
    if (how) how[i] = h;
  }
  return failed;
}

void lnr_pixel_to_vector(const void* cam, int kind, const double* params, int np, double x, double y, double* out3) {
  LensCamera c = make_camera(cam, nullptr, kind, params, np);
  int how;
  V3 v = lens_pixel_to_vector(c, V2{x, y}, &how);
  out3[0] = v.x; out3[1] = v.y; out3[2] = v.z;
}

int lnr_point_to_pixel(const void* cam, const double* matrix, int kind, const double* params, int np, const double* point, int check,
                       double* out2) {
  LensCamera c = make_camera(cam, matrix, kind, params, np);
  V2 q{NaN, NaN};
  int st = lens_point_to_pixel(c, v3(point), check, q);
  out2[0] = q.x; out2[1] = q.y;
  return st;
}

// camera_transform rasterised as epr_camera_transform does; q (optional) the source positions, status (optional) an LS_
// value per pixel; counts = {failed, failed by the lens solver}
int lnr_camera_transform(const float* src, int sw, int sh, const unsigned char* src_mask, const void* src_cam, const double* src_matrix,
                         int src_kind, const double* src_params, int src_np, const void* dst_cam, const double* dst_matrix, int dst_kind,
                         const double* dst_params, int dst_np, int w, int h, int x0, int y0, float edge_value, int edge_valid, int check,
                         float* out, unsigned char* out_mask, double* q_out, int* status, long long* counts) {
  LensCamera sc = make_camera(src_cam, src_matrix, src_kind, src_params, src_np), dc = make_camera(dst_cam, dst_matrix, dst_kind, dst_params, dst_np);
  if (!same(v3(sc.geo.center), v3(dc.geo.center))) return RC_LOGIC;
  Source s{src, src_mask, sw, sh, edge_value, edge_valid};
  long long nfailed = 0, nlens = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      V2 p{(double)((long long)x0 + x), (double)((long long)y0 + y)}, q{NaN, NaN};
      Px r{edge_value, edge_valid != 0};
      int cls;
      const int st = lens_transform(dc, sc, check, p, q);
      if (st == LS_OK) r = bilinear(s, q.x, q.y, &cls);
      else {
        ++nfailed;
        if (st == LS_LENS) ++nlens;
      }
      const long long i = (long long)y * w + x;
      out[i] = r.v;
      if (out_mask) out_mask[i] = r.valid ? 255 : 0;
      if (q_out) { q_out[2 * i] = q.x; q_out[2 * i + 1] = q.y; }
      if (status) status[i] = st;
    }
  if (counts) { counts[0] = nfailed; counts[1] = nlens; }
  return RC_OK;
}

int lnr_transform_points(const void* src_cam, const double* src_matrix, int src_kind, const double* src_params, int src_np,
                         const void* dst_cam, const double* dst_matrix, int dst_kind, const double* dst_params, int dst_np, int direction,
                         int check, const double* points, long long n, double* out, long long* counts) {
  LensCamera sc = make_camera(src_cam, src_matrix, src_kind, src_params, src_np), dc = make_camera(dst_cam, dst_matrix, dst_kind, dst_params, dst_np);
  if (!same(v3(sc.geo.center), v3(dc.geo.center))) return RC_LOGIC;
  long long nfailed = 0, nlens = 0;
  for (long long i = 0; i < n; ++i) {
    V2 p{points[2 * i], points[2 * i + 1]}, q{NaN, NaN};
    const int st = direction == FORWARD ? lens_transform(sc, dc, check, p, q) : lens_transform(dc, sc, check, p, q);
    if (st != LS_OK) {
      ++nfailed;
      if (st == LS_LENS) ++nlens;
      q = V2{NaN, NaN};
    }
    out[2 * i] = q.x;
    out[2 * i + 1] = q.y;
  }
  if (counts) { counts[0] = nfailed; counts[1] = nlens; }
  return RC_OK;
}

// StereoModel::operator()(pixVec, errorVec) (StereoModel.cc:97-147) and the image overload with its statistics (:254-309)
// over lens_pixel_to_vector, for float {dx, dy, valid} disparities; angle (optional) the convergence angle (:174-177)
int lnr_stereo_triangulate(const float* disp, int w, int h, int x0, int y0, const void* cam1, int kind1, const double* params1, int np1,
                           const void* cam2, int kind2, const double* params2, int np2, double angle_tol, int semantics, double* xyz,
                           double* error, double* errvec, void* stats, double* angle) {
  LensCamera c1 = make_camera(cam1, nullptr, kind1, params1, np1), c2 = make_camera(cam2, nullptr, kind2, params2, np2);
  const int layout = semantics & LAYOUT_MASK, model = (semantics & ~LAYOUT_MASK) == MODEL;
  double mean_error = 0.0, max_error = 0.0;
  long long point_count = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const long long i = (long long)y * w + x;
      float dx, dy;
      V3 p{0, 0, 0}, ev{0, 0, 0};
      double err = 0, ang = 0;
      if (load_disp(disp, layout, i, dx, dy)) {
        V2 pix1, pix2;
        pixel_pair(model, x0 + x, y0 + y, dx, dy, pix1, pix2);
        int how;
        const bool skip = pix1.x != pix1.x || pix1.y != pix1.y || pix2.x != pix2.x || pix2.y != pix2.y ||
                          (pix1.x == -1e8 && pix1.y == -1e8) || (pix2.x == -1e8 && pix2.y == -1e8);
        if (!skip) {
          const V3 dir0 = lens_pixel_to_vector(c1, pix1, &how), dir1 = lens_pixel_to_vector(c2, pix2, &how);
          const V3 ctr0 = v3(c1.geo.center), ctr1 = v3(c2.geo.center);
          double tol = 1e-4;
          if (angle_tol > 0) tol = angle_tol;
          if (1 - dot(dir0, dir1) >= tol) {
            p = triangulate_pair(dir0, ctr0, dir1, ctr1, ev);
            bool reflect = false;
            if (dot(sub(p, ctr0), dir0) < 0) reflect = true;
            if (dot(sub(p, ctr1), dir1) < 0) reflect = true;
            if (reflect) p = V3{-p.x + 2 * ctr0.x, -p.y + 2 * ctr0.y, -p.z + 2 * ctr0.z};
          }
        }
        err = norm_2(ev);
        if (err >= 0) {
          if (err > max_error) max_error = err;
          mean_error += err;
          ++point_count;
        } else if (model) {
          p = V3{0, 0, 0};
        }
        ang = std::acos(dot(lens_pixel_to_vector(c1, pix1, &how), lens_pixel_to_vector(c2, pix2, &how)));
      }
      xyz[3 * i] = p.x; xyz[3 * i + 1] = p.y; xyz[3 * i + 2] = p.z;
      if (error) error[i] = err;
      if (errvec) { errvec[3 * i] = ev.x; errvec[3 * i + 1] = ev.y; errvec[3 * i + 2] = ev.z; }
      if (angle) angle[i] = ang;
    }
  if (stats) {
    Stats* s = static_cast<Stats*>(stats);
    s->point_count = point_count;
    s->max_error = max_error;
    s->sum_error = mean_error;
  }
  return RC_OK;
}

}  // extern "C"
