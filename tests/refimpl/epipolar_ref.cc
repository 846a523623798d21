// epipolar_ref.cc — CPU restatement of epipolar rectification as the reference computes it (test infrastructure only;
// dependency-free): epipolar() for two pinholes (src/vw/Camera/PinholeModel.cc:679-732, with camera_pose().rotation_matrix(),
// src/vw/Math/Quaternion.h:211-340) and two CAHV models (src/vw/Camera/CAHVModel.cc:297-337), m_camera_matrix of
// rebuild_camera_matrix (PinholeModel.cc:593-603), CameraTransform::forward / reverse (src/vw/Camera/CameraTransform.h:52-74)
// over PinholeModel::point_to_pixel with its round-trip check (PinholeModel.cc:351-397) and CAHVModel::point_to_pixel
// (CAHVModel.cc:167-171), and camera_transform rasterised with BilinearInterpolation over a ValueEdgeExtension
// (src/vw/Image/Interpolation.h:76-110) for float and PixelMask<float> images (src/vw/Image/PixelMask.h:321-345, :424-433).
// Plain scalar loops in raster order, every expression in the reference's order; built with -O2 -ffp-contract=off.
// The rays (pixel_to_vector, the Tsai model and its Newton solver) are those of triangulate_ref.cc, included below.
#include "triangulate_ref.cc"

namespace {

enum { FORWARD = 0, REVERSE = 1 };
// what became of an output pixel
enum { CL_INTEGER = 0, CL_INSIDE = 1, CL_STRADDLE = 2, CL_OUTSIDE = 3, CL_NAN_HUGE = 4, CL_CHECK_FAILED = 5 };
enum { RC_OK = 0, RC_ARGUMENT = -1, RC_LOGIC = -5 };

V3 add(V3 const& a, V3 const& b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
V3 mul(V3 const& a, double s) { return V3{a.x * s, a.y * s, a.z * s}; }
V3 quot(V3 const& a, double s) { return V3{a.x / s, a.y / s, a.z / s}; }
V3 neg(V3 const& a) { return V3{-a.x, -a.y, -a.z}; }
void put(V3 const& a, double* p) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }
bool same(V3 const& a, V3 const& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// Quaternion<double>(rot).rotation_matrix() (Quaternion.h:211-252, :314-329); rot and out are row-major 3 x 3
void pose_rotation_matrix(const double* r, double* out) {
#define ROT(i, j) r[(i) * 3 + (j)]
  double d0 = ROT(0, 0), d1 = ROT(1, 1), d2 = ROT(2, 2);
  double ww = 1.0 + d0 + d1 + d2;
  double xx = 1.0 + d0 - d1 - d2;
  double yy = 1.0 - d0 + d1 - d2;
  double zz = 1.0 - d0 - d1 + d2;
  double max = ww;
  if (xx > max) max = xx;
  if (yy > max) max = yy;
  if (zz > max) max = zz;
  double c[4];
  if (ww == max) {
    double w4 = std::sqrt(ww * 4.0);
    c[0] = w4 / 4;
    c[1] = (ROT(2, 1) - ROT(1, 2)) / w4;
    c[2] = (ROT(0, 2) - ROT(2, 0)) / w4;
    c[3] = (ROT(1, 0) - ROT(0, 1)) / w4;
  } else if (xx == max) {
    double x4 = std::sqrt(xx * 4.0);
    c[0] = (ROT(2, 1) - ROT(1, 2)) / x4;
    c[1] = x4 / 4;
    c[2] = (ROT(0, 1) + ROT(1, 0)) / x4;
    c[3] = (ROT(0, 2) + ROT(2, 0)) / x4;
  } else if (yy == max) {
    double y4 = std::sqrt(yy * 4.0);
    c[0] = (ROT(0, 2) - ROT(2, 0)) / y4;
    c[1] = (ROT(0, 1) + ROT(1, 0)) / y4;
    c[2] = y4 / 4;
    c[3] = (ROT(1, 2) + ROT(2, 1)) / y4;
  } else {
    double z4 = std::sqrt(zz * 4.0);
    c[0] = (ROT(1, 0) - ROT(0, 1)) / z4;
    c[1] = (ROT(0, 2) + ROT(2, 0)) / z4;
    c[2] = (ROT(1, 2) + ROT(2, 1)) / z4;
    c[3] = z4 / 4;
  }
#undef ROT
  double w = c[0], x = c[1], y = c[2], z = c[3];
  double w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
  double wx = w * x, wy = w * y, wz = w * z;
  double xy = x * y, yz = y * z, zx = z * x;
#define OUT(i, j) out[(i) * 3 + (j)]
  OUT(0, 0) = w2 + x2 - y2 - z2;
  OUT(1, 1) = w2 - x2 + y2 - z2;
  OUT(2, 2) = w2 - x2 - y2 + z2;
  OUT(0, 1) = 2 * (xy - wz);
  OUT(0, 2) = 2 * (zx + wy);
  OUT(1, 2) = 2 * (yz - wx);
  OUT(1, 0) = 2 * (xy + wz);
  OUT(2, 0) = 2 * (zx - wy);
  OUT(2, 1) = 2 * (yz + wx);
#undef OUT
}

// PinholeModel::point_to_pixel (PinholeModel.cc:351-397) on m_camera_matrix `m` (row-major 3 x 4); false where it throws
bool pinhole_point_to_pixel(Camera const& c, const double* m, V3 const& point, int check, V2& final_pixel) {
  double den = m[8] * point.x + m[9] * point.y + m[10] * point.z + m[11];
  V2 pixel{(m[0] * point.x + m[1] * point.y + m[2] * point.z + m[3]) / den,
           (m[4] * point.x + m[5] * point.y + m[6] * point.z + m[7]) / den};
  V2 distorted = c.distortion_kind == DIST_TSAI ? tsai_distorted(c, pixel) : pixel;
  final_pixel = V2{distorted.x / c.pixel_pitch, distorted.y / c.pixel_pitch};
  if (!check) return true;
  const double ERROR_THRESHOLD = 0.01;
  int how;
  V3 pixel_vector = pixel_to_vector(c, final_pixel, &how);
  V3 phys_vector = normalize(sub(point, v3(c.center)));
  double diff = norm_2(sub(pixel_vector, phys_vector));
  if (diff >= ERROR_THRESHOLD) diff = norm_2(add(pixel_vector, phys_vector));
  if (diff >= ERROR_THRESHOLD || diff != diff) return false;
  return true;
}

bool point_to_pixel(Camera const& c, const double* m, V3 const& point, int check, V2& pix) {
  if (c.kind == CAHV) {   // CAHVModel.cc:167-171
    double dDot = dot(sub(point, v3(c.center)), v3(c.A));
    pix = V2{dot(sub(point, v3(c.center)), v3(c.H)) / dDot, dot(sub(point, v3(c.center)), v3(c.V)) / dDot};
    return true;
  }
  return pinhole_point_to_pixel(c, m, point, check, pix);
}

// CameraTransform::forward / reverse with (from, to) = (src, dst) / (dst, src)
bool transform(Camera const& from, Camera const& to, const double* to_matrix, int check, V2 const& p, V2& q) {
  int how;
  V3 vec = pixel_to_vector(from, p, &how);
  return point_to_pixel(to, to_matrix, add(vec, v3(from.center)), check, q);
}

struct Source {
  const float* img;
  const unsigned char* mask;
  int w, h;
  float edge_value;
  int edge_valid;
};
struct Px { float v; bool valid; };
bool inside(Source const& s, int x, int y) { return x >= 0 && y >= 0 && x < s.w && y < s.h; }
Px edge_extended(Source const& s, int x, int y) {
  if (inside(s, x, y)) return Px{s.img[(long long)y * s.w + x], s.mask ? s.mask[(long long)y * s.w + x] != 0 : true};
  return Px{s.edge_value, s.edge_valid != 0};
}
// PixelMask<float> * float, and += (PixelMask.h:424-433: the value whatever the validity, invalid if either side is)
Px times(Px a, float s) { return Px{a.v * s, a.valid}; }
void accumulate(Px& a, Px b) { a.v += b.v; if (!b.valid) a.valid = false; }

// BilinearInterpolationImpl::operator() (Interpolation.h:77-109)
Px bilinear(Source const& s, double i, double j, int* cls) {
  const double lim = 1073741824.0;   // beyond 2^30 (or NaN) the conversion of _floor is undefined: {0, invalid} by definition
  if (!(i >= -lim && i <= lim && j >= -lim && j <= lim)) {
    *cls = CL_NAN_HUGE;
    return Px{0.0f, false};
  }
  int x = (int)std::floor(i), y = (int)std::floor(j);
  if (x == i && y == j) {
    *cls = inside(s, x, y) ? CL_INTEGER : CL_OUTSIDE;
    return edge_extended(s, x, y);
  }
  int n_in = inside(s, x, y) + inside(s, x + 1, y) + inside(s, x, y + 1) + inside(s, x + 1, y + 1);
  *cls = n_in == 4 ? CL_INSIDE : n_in == 0 ? CL_OUTSIDE : CL_STRADDLE;
  float normx = float(i) - float(x), normy = float(j) - float(y), norm1mx = 1 - normx, norm1my = 1 - normy;
  Px result = times(edge_extended(s, x, y), norm1mx);
  accumulate(result, times(edge_extended(s, x + 1, y), normx));
  result = times(result, norm1my);
  Px row = times(edge_extended(s, x, y + 1), norm1mx);
  accumulate(row, times(edge_extended(s, x + 1, y + 1), normx));
  accumulate(result, times(row, normy));
  return result;
}

}  // namespace

extern "C" {

int epr_camera_matrix(const double* center, const double* rotation, double fu, double fv, double cu, double cv, const double* u,
                      const double* v, const double* w, double* out) {
  if (!(dot(v3(u), v3(v)) == 0) || !(dot(v3(u), v3(w)) == 0) || !(dot(v3(v), v3(w)) == 0)) return RC_ARGUMENT;
  if (!(std::fabs(norm_2(v3(u)) - 1) < 0.001) || !(std::fabs(norm_2(v3(v)) - 1) < 0.001) || !(std::fabs(norm_2(v3(w)) - 1) < 0.001))
    return RC_ARGUMENT;
  double uvw[9] = {u[0], u[1], u[2], v[0], v[1], v[2], w[0], w[1], w[2]};
  double rotation_inverse[9], neg_inverse[9], a[9], b[9], extrinsics[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      rotation_inverse[i * 3 + j] = rotation[j * 3 + i];
      neg_inverse[i * 3 + j] = -rotation[j * 3 + i];
    }
  mat_mul(uvw, rotation_inverse, a);
  mat_mul(uvw, neg_inverse, b);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) extrinsics[i * 4 + j] = a[i * 3 + j];
    extrinsics[i * 4 + 3] = dot(v3(b + 3 * i), v3(center));
  }
  double intrinsics[9] = {fu, 0, cu, 0, fv, cv, 0, 0, 1};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double result = 0.0;
      for (int k = 0; k < 3; ++k) result += intrinsics[i * 3 + k] * extrinsics[k * 4 + j];
      out[i * 4 + j] = result;
    }
  return RC_OK;
}

int epr_epipolar_pinhole(const double* center0, const double* rotation0, const double* focal0, const double* offset0, double pitch0,
                         const double* center1, const double* rotation1, const double* focal1, const double* offset1, double pitch1,
                         double* new_rot, double* focal_length, double* point_offset, double* pixel_pitch) {
  if (same(v3(center0), v3(center1))) return RC_ARGUMENT;
  double rot0[9], rot1[9];
  pose_rotation_matrix(rotation0, rot0);
  pose_rotation_matrix(rotation1, rot1);
  V3 c0 = v3(center0), c1 = v3(center1);
  V3 look0 = mul(V3{rot0[2], rot0[5], rot0[8]}, -1), look1 = mul(V3{rot1[2], rot1[5], rot1[8]}, -1);
  V3 u = quot(sub(c1, c0), norm_2(sub(c1, c0)));
  V3 mean_look = quot(add(look0, look1), 2.0);
  V3 temp = cross(u, cross(mean_look, u));
  V3 w = quot(temp, norm_2(temp));
  V3 v = cross(w, u);
  double r[9] = {u.x, -v.x, -w.x, u.y, -v.y, -w.y, u.z, -v.z, -w.z};
  std::memcpy(new_rot, r, sizeof(r));
  for (int k = 0; k < 2; ++k) {
    focal_length[k] = (focal0[k] + focal1[k]) / 2.0;
    point_offset[k] = (offset0[k] + offset1[k]) / 2.0;
  }
  *pixel_pitch = (pitch0 + pitch1) / 2.0;
  return RC_OK;
}

int epr_epipolar_cahv(const void* src0, const void* src1, void* dst0, void* dst1) {
  Camera const& s0 = *static_cast<const Camera*>(src0);
  Camera const& s1 = *static_cast<const Camera*>(src1);
  if (s0.kind != CAHV || s1.kind != CAHV || same(v3(s0.center), v3(s1.center))) return RC_ARGUMENT;
  double hc = dot(v3(s0.H), v3(s0.A)) / 2.0 + dot(v3(s1.H), v3(s1.A)) / 2.0;
  double vc = dot(v3(s0.V), v3(s0.A)) / 2.0 + dot(v3(s1.V), v3(s1.A)) / 2.0;
  double hs = norm_2(cross(v3(s0.A), v3(s0.H))) / 2.0 + norm_2(cross(v3(s1.A), v3(s1.H))) / 2.0;
  double vs = norm_2(cross(v3(s0.A), v3(s0.V))) / 2.0 + norm_2(cross(v3(s1.A), v3(s1.V))) / 2.0;
  V3 app = add(v3(s0.A), v3(s1.A));
  V3 f = cross(cross(app, sub(v3(s1.center), v3(s0.center))), app);
  V3 hp;
  if (dot(f, v3(s0.H)) > 0) hp = quot(mul(f, hs), norm_2(f));
  else hp = quot(mul(neg(f), hs), norm_2(f));
  app = mul(app, 0.5);
  V3 g = quot(mul(hp, dot(app, hp)), hs * hs);
  V3 a = normalize(sub(app, g));
  V3 vp = quot(mul(cross(a, hp), vs), hs);
  Camera d;
  std::memset(&d, 0, sizeof(d));
  d.kind = CAHV;
  put(a, d.A);
  put(add(hp, mul(a, hc)), d.H);
  put(add(vp, mul(a, vc)), d.V);
  Camera d0 = d, d1 = d;
  std::memcpy(d0.center, s0.center, sizeof(d0.center));
  std::memcpy(d1.center, s1.center, sizeof(d1.center));
  *static_cast<Camera*>(dst0) = d0;
  *static_cast<Camera*>(dst1) = d1;
  return RC_OK;
}

// camera_transform(image, src, dst, Vector2i(w, h), ValueEdgeExtension(edge), BilinearInterpolation()) rasterised at
// (x0 + x, y0 + y); src_mask / out_mask may be null.  classes (optional) receives a CL_ value per pixel; *failed the
// number of pixels where point_to_pixel threw (they hold the edge pixel).
int epr_camera_transform(const float* src, int sw, int sh, const unsigned char* src_mask, const void* src_cam, const double* src_matrix,
                         const void* dst_cam, int w, int h, int x0, int y0, float edge_value, int edge_valid, int check, float* out,
                         unsigned char* out_mask, int* classes, long long* failed) {
  Camera const& sc = *static_cast<const Camera*>(src_cam);
  Camera const& dc = *static_cast<const Camera*>(dst_cam);
  if (!same(v3(sc.center), v3(dc.center))) return RC_LOGIC;
  Source s{src, src_mask, sw, sh, edge_value, edge_valid};
  long long nfailed = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      V2 p{(double)((long long)x0 + x), (double)((long long)y0 + y)}, q;
      Px r{edge_value, edge_valid != 0};
      int cls = CL_CHECK_FAILED;
      if (transform(dc, sc, src_matrix, check, p, q)) r = bilinear(s, q.x, q.y, &cls);
      else ++nfailed;
      const long long i = (long long)y * w + x;
      out[i] = r.v;
      if (out_mask) out_mask[i] = r.valid ? 255 : 0;
      if (classes) classes[i] = cls;
    }
  if (failed) *failed = nfailed;
  return RC_OK;
}

int epr_transform_points(const void* src_cam, const double* src_matrix, const void* dst_cam, const double* dst_matrix, int direction,
                         int check, const double* points, long long n, double* out, long long* failed) {
  Camera const& sc = *static_cast<const Camera*>(src_cam);
  Camera const& dc = *static_cast<const Camera*>(dst_cam);
  if (!same(v3(sc.center), v3(dc.center))) return RC_LOGIC;
  long long nfailed = 0;
  for (long long i = 0; i < n; ++i) {
    V2 p{points[2 * i], points[2 * i + 1]}, q;
    const bool ok = direction == FORWARD ? transform(sc, dc, dst_matrix, check, p, q) : transform(dc, sc, src_matrix, check, p, q);
    if (!ok) {
      ++nfailed;
      q = V2{std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::quiet_NaN()};
    }
    out[2 * i] = q.x;
    out[2 * i + 1] = q.y;
  }
  if (failed) *failed = nfailed;
  return RC_OK;
}

}  // extern "C"
