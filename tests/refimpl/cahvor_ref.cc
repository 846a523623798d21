// cahvor_ref.cc — CPU restatement of the CAHVOR and CAHVORE camera models as the reference computes them (test
// infrastructure only; dependency-free): CAHVORModel::pixel_to_vector and point_to_pixel without partials
// (src/vw/Camera/CAHVORModel.cc:297-348, :431-448), CAHVOREModel::pixel_to_vector and point_to_pixel
// (src/vw/Camera/CAHVOREModel.cc:167-301), both linearize_camera overloads (CAHVORModel.cc:460-547, CAHVOREModel.cc:303-381),
// and the compositions the library offers for them: CameraTransform / camera_transform against a CAHV camera
// (src/vw/Camera/CameraTransform.h:43-183) and StereoModel for two cameras of one kind (src/vw/Stereo/StereoModel.cc:97-177).
// Plain scalar loops in raster order, every expression in the reference's order; built with -O2 -ffp-contract=off.
// The vector helpers, the CAHV model, the bilinear tap and the disparity layouts are those of epipolar_ref.cc and
// triangulate_ref.cc, included below.  The camera is the flat descriptor of the C ABI: O, R, E live in
// inv_camera_transform[0..8] and P in distortion[0] (include/vwgpu.h).
#include "epipolar_ref.cc"

namespace {

enum { CAHVOR = 3, CAHVORE = 4 };
enum { ST_OK = 0, ST_NOT_CONVERGED = 1, ST_THETA = 2 };

V3 O_of(Camera const& c) { return v3(c.inv_camera_transform); }
V3 R_of(Camera const& c) { return v3(c.inv_camera_transform + 3); }
V3 E_of(Camera const& c) { return v3(c.inv_camera_transform + 6); }
double P_of(Camera const& c) { return c.distortion[0]; }

// CAHVORModel::pixel_to_vector (CAHVORModel.cc:297-348); *passes receives the loop index at which the Newton loop left
V3 cahvor_pixel_to_vector(Camera const& c, V2 const& pix, int* passes) {
  const V3 A = v3(c.A), H = v3(c.H), V = v3(c.V), O = O_of(c), R = R_of(c);
  V3 rr = normalize(cross(sub(V, mul(A, pix.y)), sub(H, mul(A, pix.x))));
  if (dot(cross(V, H), A) < 0) rr = mul(rr, -1.0);
  double omega = dot(rr, O);
  V3 lambda = sub(rr, mul(O, omega));
  const double tau = dot(lambda, lambda) / (omega * omega);
  const double k1 = 1 + R.x;
  const double k3 = R.y * tau;
  const double k5 = R.z * tau * tau;
  double u = 1.0 - (R.x + k3 + k5);
  double du, poly, deriv;
  int i = 0;
  for (;; i++) {
    if (i >= 20) break;
    double u_2 = u * u;
    poly = ((k5 * u_2 + k3) * u_2 + k1) * u - 1;
    deriv = (5 * k5 * u_2 + 3 * k3) * u_2 + k1;
    if (deriv <= 0) {
      break;
    } else {
      du = poly / deriv;
      u -= du;
      if (std::fabs(du) < 1.0e-6) break;
    }
  }
  if (passes) *passes = i;   // the passes completed before the one that left the loop
  return normalize(sub(rr, mul(lambda, 1 - u)));
}

// CAHVORModel::point_to_pixel (CAHVORModel.cc:431-448)
V2 cahvor_point_to_pixel(Camera const& c, V3 const& point) {
  const V3 O = O_of(c), R = R_of(c);
  V3 vec = sub(point, v3(c.center));
  double omega = dot(vec, O);
  V3 lambda = sub(vec, mul(O, omega));
  double tau = dot(lambda, lambda) / (omega * omega);
  double mu = R.x + (R.y * tau) + (R.z * tau * tau);
  V3 pp_c = add(vec, mul(lambda, mu));
  double alpha = dot(pp_c, v3(c.A));
  return V2{dot(pp_c, v3(c.H)) / alpha, dot(pp_c, v3(c.V)) / alpha};
}

// CAHVOREModel::pixel_to_vector (CAHVOREModel.cc:167-228); ST_NOT_CONVERGED where it throws PixelToRayErr
int cahvore_pixel_to_vector(Camera const& c, V2 const& pix, V3& result, int* passes) {
  const V3 A = v3(c.A), H = v3(c.H), V = v3(c.V), O = O_of(c), R = R_of(c);
  const double P = P_of(c);
  if (passes) *passes = 0;
  V3 w3 = cross(sub(V, mul(A, pix.y)), sub(H, mul(A, pix.x)));
  V3 rp = mul(w3, 1 / dot(A, cross(V, H)));
  double zetap = dot(rp, O);
  V3 lambdap3 = sub(rp, mul(O, zetap));
  double lambdap = norm_2(lambdap3);
  double chip = lambdap / zetap;
  if (chip < 1e-8) {
    result = O;
    return ST_OK;
  }
  double chi = chip;
  double dchi = 1;
  for (int n = 0;; ++n) {
    if (n > 100) return ST_NOT_CONVERGED;
    if (std::fabs(dchi) < 1e-8) break;
    double chi2 = chi * chi;
    double chi3 = chi * chi2;
    double chi4 = chi * chi3;
    double chi5 = chi * chi4;
    double deriv = (1 + R.x) + 3 * R.y * chi2 + 5 * R.z * chi4;
    dchi = ((1 + R.x) * chi + R.y * chi3 + R.z * chi5 - chip) / deriv;
    chi -= dchi;
    if (passes) ++*passes;
  }
  double linchi, theta;
  linchi = P * chi;
  if (P < -1e-15) theta = std::asin(linchi) / P;
  else if (P > 1e-15) theta = std::atan(linchi) / P;
  else theta = chi;
  result = add(mul(normalize(lambdap3), std::sin(theta)), mul(O, std::cos(theta)));
  return ST_OK;
}

// CAHVOREModel::point_to_pixel (CAHVOREModel.cc:232-301); where it throws PointToPixelErr, which of the two
int cahvore_point_to_pixel(Camera const& c, V3 const& point, V2& pix) {
  const V3 O = O_of(c), R = R_of(c), E = E_of(c);
  const double P = P_of(c);
  V3 p_c = sub(point, v3(c.center));
  double zeta = dot(p_c, O);
  V3 lambda3 = sub(p_c, mul(O, zeta));
  double lambda = norm_2(lambda3);
  double theta = std::atan2(lambda, zeta);
  double dtheta = 1;
  for (int n = 0;; ++n) {
    if (n > 100) return ST_NOT_CONVERGED;
    if (std::fabs(dtheta) < 1e-8) break;
    double costh = std::cos(theta);
    double sinth = std::sin(theta);
    double theta2 = theta * theta;
    double theta3 = theta * theta2;
    double theta4 = theta * theta3;
    double upsilon = zeta * costh + lambda * sinth
      - (1 - costh) * (E.x + E.y * theta2 + E.z * theta4)
      - (theta - sinth) * (2 * E.y * theta + 4 * E.z * theta3);
    dtheta = (zeta * sinth - lambda * costh
              - (theta - sinth) * (E.x + E.y * theta2 + E.z * theta4)) / upsilon;
    theta -= dtheta;
  }
  if ((theta * std::fabs(P)) > M_PI / 2) return ST_THETA;
  V3 rp;
  if (theta < 1e-8) {
    rp = p_c;
  } else {
    double linth, chi;
    linth = P * theta;
    if (P < -1e-15) chi = std::sin(linth) / P;
    else if (P > 1e-15) chi = std::tan(linth) / P;
    else chi = theta;
    double chi2 = chi * chi;
    double mu = R.z;
    mu = R.y + chi2 * mu;
    mu = R.x + chi2 * mu;
    rp = add(mul(O, lambda / chi), mul(lambda3, 1 + mu));
  }
  double alpha = dot(rp, v3(c.A));
  pix = V2{dot(rp, v3(c.H)) / alpha, dot(rp, v3(c.V)) / alpha};
  return ST_OK;
}

// pixel_to_vector / point_to_pixel of every kind
int any_pixel_to_vector(Camera const& c, V2 const& pix, V3& vec, int* passes) {
  if (passes) *passes = 0;
  if (c.kind == CAHVORE) return cahvore_pixel_to_vector(c, pix, vec, passes);
  if (c.kind == CAHVOR) {
    vec = cahvor_pixel_to_vector(c, pix, passes);
    return ST_OK;
  }
  int how;
  vec = pixel_to_vector(c, pix, &how);
  return ST_OK;
}
int any_point_to_pixel(Camera const& c, const double* matrix, V3 const& point, int check, V2& pix) {
  if (c.kind == CAHVORE) return cahvore_point_to_pixel(c, point, pix);
  if (c.kind == CAHVOR) {
    pix = cahvor_point_to_pixel(c, point);
    return ST_OK;
  }
  return point_to_pixel(c, matrix, point, check, pix) ? ST_OK : ST_NOT_CONVERGED;
}
int any_transform(Camera const& from, Camera const& to, const double* to_matrix, int check, V2 const& p, V2& q, int* passes) {
  V3 vec;
  int st = any_pixel_to_vector(from, p, vec, passes);
  if (st != ST_OK) return st;
  return any_point_to_pixel(to, to_matrix, add(vec, v3(from.center)), check, q);
}

// linearize_camera for a CAHVOR or CAHVORE camera
int linearize(Camera const& cam, int iw, int ih, int ow, int oh, Camera& out) {
  const bool e = cam.kind == CAHVORE;
  V2 hpts[6], vpts[6];
  hpts[0] = V2{0, 0};
  hpts[1] = e ? V2{0, (double)((ih - 1) / 2)} : V2{0, (ih - 1) / 2.0};
  hpts[2] = V2{0, (double)(ih - 1)};
  hpts[3] = V2{(double)(iw - 1), 0};
  hpts[4] = e ? V2{(double)(iw - 1), (double)((ih - 1) / 2)} : V2{(double)(iw - 1), (ih - 1) / 2.0};
  hpts[5] = V2{(double)iw - 1, (double)ih - 1};
  vpts[0] = V2{0, 0};
  vpts[1] = e ? V2{(double)((iw - 1) / 2), 0} : V2{(iw - 1) / 2.0, 0};
  vpts[2] = V2{(double)(iw - 1), 0};
  vpts[3] = V2{0, (double)(ih - 1)};
  vpts[4] = V2{(double)((iw - 1) / 2), (double)(ih - 1)};
  vpts[5] = V2{(double)iw - 1, (double)ih - 1};

  V3 A{0, 0, 0}, ray;
  if (e) {
    if (any_pixel_to_vector(cam, V2{(iw - 1) / 2.0, (ih - 1) / 2.0}, A, nullptr) != ST_OK) return RC_LOGIC;
  } else {
    for (V2 const& local : vpts) {
      any_pixel_to_vector(cam, local, ray, nullptr);
      A = add(A, ray);
    }
    for (V2 const& local : hpts) {
      any_pixel_to_vector(cam, local, ray, nullptr);
      A = add(A, ray);
    }
    A = normalize(A);
  }
  V3 dn = cross(v3(cam.A), v3(cam.H));
  V3 rt = normalize(cross(dn, v3(cam.A)));
  dn = normalize(dn);
  rt = cross(dn, A);
  dn = normalize(cross(A, rt));
  rt = normalize(rt);

  double hmin = 1, hmax = -1;
  for (V2 const& loop : hpts) {
    V3 u3;
    if (any_pixel_to_vector(cam, loop, u3, nullptr) != ST_OK) return RC_LOGIC;
    V3 n = normalize(sub(u3, mul(dn, dot(dn, u3))));
    double v = e ? dot(A, n) : norm_2(cross(A, n));
    if (hmin > v) hmin = v;
    if (hmax < v) hmax = v;
  }
  double vmin = 1, vmax = -1;
  for (V2 const& loop : vpts) {
    V3 u3;
    if (any_pixel_to_vector(cam, loop, u3, nullptr) != ST_OK) return RC_LOGIC;
    V3 n = normalize(sub(u3, mul(rt, dot(rt, u3))));
    double v = e ? dot(A, n) : norm_2(cross(A, n));
    if (vmin > v) vmin = v;
    if (vmax < v) vmax = v;
  }
  double s0, s1, c0, c1;
  if (e) {
    const double limfov = M_PI * 3 / 4;
    double cos0 = hmax, cos1 = vmax;
    if (std::acos(cos0) > limfov) cos0 = std::cos(limfov);
    if (std::acos(cos1) > limfov) cos1 = std::cos(limfov);
    s0 = (ow / 2.0 * cos0) / std::sqrt(1 - cos0 * cos0);
    s1 = (oh / 2.0 * cos1) / std::sqrt(1 - cos1 * cos1);
    c0 = (ow - 1) / 2.0;
    c1 = (oh - 1) / 2.0;
  } else {
    c0 = (ow - 1) / 2.0;
    c1 = (oh - 1) / 2.0;
    const double c0_2 = c0 * c0, c1_2 = c1 * c1;
    s0 = std::sqrt(c0_2 / (hmin * hmin) - c0_2);
    s1 = std::sqrt(c1_2 / (vmin * vmin) - c1_2);
  }
  std::memset(&out, 0, sizeof(out));
  out.kind = CAHV;
  std::memcpy(out.center, cam.center, sizeof(out.center));
  put(A, out.A);
  put(add(mul(rt, s0), mul(A, c0)), out.H);
  put(add(mul(dn, s1), mul(A, c1)), out.V);
  return RC_OK;
}

// StereoModel::operator()(pixVec, errorVec) (StereoModel.cc:97-147) over any_pixel_to_vector; a throwing ray gives zero
V3 stereo_model_any(Camera const& cam1, Camera const& cam2, double angle_tol, V2 const& pix1, V2 const& pix2, V3& errorVec) {
  errorVec = V3{0, 0, 0};
  if (skipped(pix1) || skipped(pix2) || is_invalid_pixel(pix1) || is_invalid_pixel(pix2)) return V3{0, 0, 0};
  V3 dir0, dir1;
  if (any_pixel_to_vector(cam1, pix1, dir0, nullptr) != ST_OK) return V3{0, 0, 0};
  if (any_pixel_to_vector(cam2, pix2, dir1, nullptr) != ST_OK) return V3{0, 0, 0};
  const V3 ctr0 = v3(cam1.center), ctr1 = v3(cam2.center);
  double tol = 1e-4;
  if (angle_tol > 0) tol = angle_tol;
  if (!(1 - dot(dir0, dir1) >= tol)) return V3{0, 0, 0};
  V3 result = triangulate_pair(dir0, ctr0, dir1, ctr1, errorVec);
  bool reflect = false;
  if (dot(sub(result, ctr0), dir0) < 0) reflect = true;
  if (dot(sub(result, ctr1), dir1) < 0) reflect = true;
  if (reflect) result = V3{-result.x + 2 * ctr0.x, -result.y + 2 * ctr0.y, -result.z + 2 * ctr0.z};
  return result;
}

}  // namespace

extern "C" {

// status; out3 the ray, *passes the Newton loop's index at its exit (CAHVOR) or its steps (CAHVORE)
int cvr_pixel_to_vector(const void* cam, double x, double y, double* out3, int* passes) {
  Camera c;
  std::memcpy(&c, cam, sizeof(c));
  V3 vec{0, 0, 0};
  int st = any_pixel_to_vector(c, V2{x, y}, vec, passes);
  put(vec, out3);
  return st;
}

int cvr_point_to_pixel(const void* cam, const double* point, double* out2) {
  Camera c;
  std::memcpy(&c, cam, sizeof(c));
  V2 pix{0, 0};
  int st = any_point_to_pixel(c, nullptr, v3(point), 0, pix);
  out2[0] = pix.x; out2[1] = pix.y;
  return st;
}

int cvr_linearize(const void* cam, int iw, int ih, int ow, int oh, void* out) {
  Camera c, o;
  std::memcpy(&c, cam, sizeof(c));
  if ((c.kind != CAHVOR && c.kind != CAHVORE) || iw <= 0 || ih <= 0 || ow <= 0 || oh <= 0) return RC_ARGUMENT;
  int rc = linearize(c, iw, ih, ow, oh, o);
  if (rc == RC_OK) std::memcpy(out, &o, sizeof(o));
  return rc;
}

// camera_transform rasterised as epr_camera_transform does, for any pair of kinds without a pinhole.  q (optional)
// receives the source position of every pixel (2 doubles), status (optional) an ST_ value, passes (optional) the Newton
// steps of the dst ray; counts = {failed, theta out of bounds}.
int cvr_camera_transform(const float* src, int sw, int sh, const unsigned char* src_mask, const void* src_cam, const void* dst_cam, int w,
                         int h, int x0, int y0, float edge_value, int edge_valid, float* out, unsigned char* out_mask, double* q_out,
                         int* status, int* passes, long long* counts) {
  Camera sc, dc;
  std::memcpy(&sc, src_cam, sizeof(sc));
  std::memcpy(&dc, dst_cam, sizeof(dc));
  if (!same(v3(sc.center), v3(dc.center))) return RC_LOGIC;
  Source s{src, src_mask, sw, sh, edge_value, edge_valid};
  long long nfailed = 0, ntheta = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      V2 p{(double)((long long)x0 + x), (double)((long long)y0 + y)}, q{0, 0};
      Px r{edge_value, edge_valid != 0};
      int cls, np = 0;
      const int st = any_transform(dc, sc, nullptr, 0, p, q, &np);
      if (st == ST_OK) r = bilinear(s, q.x, q.y, &cls);
      else {
        ++nfailed;
        if (st == ST_THETA) ++ntheta;
      }
      const long long i = (long long)y * w + x;
      out[i] = r.v;
      if (out_mask) out_mask[i] = r.valid ? 255 : 0;
      if (q_out) { q_out[2 * i] = q.x; q_out[2 * i + 1] = q.y; }
      if (status) status[i] = st;
      if (passes) passes[i] = np;
    }
  if (counts) { counts[0] = nfailed; counts[1] = ntheta; }
  return RC_OK;
}

int cvr_transform_points(const void* src_cam, const void* dst_cam, int direction, const double* points, long long n, double* out,
                         long long* counts) {
  Camera sc, dc;
  std::memcpy(&sc, src_cam, sizeof(sc));
  std::memcpy(&dc, dst_cam, sizeof(dc));
  if (!same(v3(sc.center), v3(dc.center))) return RC_LOGIC;
  long long nfailed = 0, ntheta = 0;
  for (long long i = 0; i < n; ++i) {
    V2 p{points[2 * i], points[2 * i + 1]}, q;
    const int st = direction == FORWARD ? any_transform(sc, dc, nullptr, 0, p, q, nullptr) : any_transform(dc, sc, nullptr, 0, p, q, nullptr);
    if (st != ST_OK) {
      ++nfailed;
      if (st == ST_THETA) ++ntheta;
      q = V2{std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::quiet_NaN()};
    }
    out[2 * i] = q.x;
    out[2 * i + 1] = q.y;
  }
  if (counts) { counts[0] = nfailed; counts[1] = ntheta; }
  return RC_OK;
}

// float {dx, dy, valid} disparities; stats as trr_stereo_triangulate; angle (optional) the convergence angle, NaN where a
// ray throws
int cvr_stereo_triangulate(const float* disp, int w, int h, int x0, int y0, const void* cam1, const void* cam2, double angle_tol,
                           int semantics, double* xyz, double* error, double* errvec, void* stats, double* angle) {
  Camera c1, c2;
  std::memcpy(&c1, cam1, sizeof(c1));
  std::memcpy(&c2, cam2, sizeof(c2));
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
        p = stereo_model_any(c1, c2, angle_tol, pix1, pix2, ev);
        err = norm_2(ev);
        if (err >= 0) {
          if (err > max_error) max_error = err;
          mean_error += err;
          ++point_count;
        } else if (model) {
          p = V3{0, 0, 0};
        }
        V3 d0, d1;
        if (any_pixel_to_vector(c1, pix1, d0, nullptr) == ST_OK && any_pixel_to_vector(c2, pix2, d1, nullptr) == ST_OK)
          ang = std::acos(dot(d0, d1));
        else
          ang = std::numeric_limits<double>::quiet_NaN();
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
