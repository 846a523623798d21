// camera_host.hip — the host arithmetic of the camera entry points; no kernel.  The pinhole descriptor and its 3 x 4
// camera matrix (rebuild_camera_matrix, src/vw/Camera/PinholeModel.cc:586-604), the lens words of a descriptor and
// distorted / undistorted_coordinates on the host (src/vw/Camera/LensDistortion.cc, through camera_rays.h), epipolar() for
// two pinholes (PinholeModel.cc:679-732, with the quaternion round trip of camera_pose().rotation_matrix(),
// src/vw/Math/Quaternion.h:211-340) and two CAHV models (src/vw/Camera/CAHVModel.cc:297-337), the CAHVOR and CAHVORE
// descriptors (src/vw/Camera/CAHVOREModel.cc:111-124) and linearize_camera (src/vw/Camera/CAHVORModel.cc:460-547,
// CAHVOREModel.cc:303-381), which runs the model functions of the kernels (camera_rays.h).  tests/refimpl/epipolar_ref.cc,
// cahvor_ref.cc, lens_ref.cc and triangulate_ref.cc restate them; DESIGN §4.18 and §4.19 list what is reproduced.
//
// Everything is double in the reference's expression order (-ffp-contract=off).
#include <cmath>
#include <cstring>

#include "camera_rays.h"
#include "vwgpu_internal.h"

namespace {

// MatrixMatrixProduct (src/vw/Math/Matrix.h:2081-2086): a dot_prod per element, the accumulator starting from zero
void ct_mat_mul3(const double* a, const double* b, double* out) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[k * 3 + j];
      out[i * 3 + j] = s;
    }
}

// Quaternion(rotation).rotation_matrix() (Math/Quaternion.h:211-252, :314-329): what camera_pose().rotation_matrix() returns
void ct_pose_round_trip(const double* rot, double* out) {
  const double d0 = rot[0], d1 = rot[4], d2 = rot[8];
  const double ww = 1.0 + d0 + d1 + d2;
  const double xx = 1.0 + d0 - d1 - d2;
  const double yy = 1.0 - d0 + d1 - d2;
  const double zz = 1.0 - d0 - d1 + d2;
  double max = ww;
  if (xx > max) max = xx;
  if (yy > max) max = yy;
  if (zz > max) max = zz;
  double c[4];
  if (ww == max) {
    const double w4 = sqrt(ww * 4.0);
    c[0] = w4 / 4;
    c[1] = (rot[7] - rot[5]) / w4;
    c[2] = (rot[2] - rot[6]) / w4;
    c[3] = (rot[3] - rot[1]) / w4;
  } else if (xx == max) {
    const double x4 = sqrt(xx * 4.0);
    c[0] = (rot[7] - rot[5]) / x4;
    c[1] = x4 / 4;
    c[2] = (rot[1] + rot[3]) / x4;
    c[3] = (rot[2] + rot[6]) / x4;
  } else if (yy == max) {
    const double y4 = sqrt(yy * 4.0);
    c[0] = (rot[2] - rot[6]) / y4;
    c[1] = (rot[1] + rot[3]) / y4;
    c[2] = y4 / 4;
    c[3] = (rot[5] + rot[7]) / y4;
  } else {
    const double z4 = sqrt(zz * 4.0);
    c[0] = (rot[3] - rot[1]) / z4;
    c[1] = (rot[2] + rot[6]) / z4;
    c[2] = (rot[5] + rot[7]) / z4;
    c[3] = z4 / 4;
  }
  const double w = c[0], x = c[1], y = c[2], z = c[3];
  const double w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
  const double wx = w * x, wy = w * y, wz = w * z;
  const double xy = x * y, yz = y * z, zx = z * x;
  out[0] = w2 + x2 - y2 - z2;
  out[4] = w2 - x2 + y2 - z2;
  out[8] = w2 - x2 - y2 + z2;
  out[1] = 2 * (xy - wz);
  out[2] = 2 * (zx + wy);
  out[5] = 2 * (yz - wx);
  out[3] = 2 * (xy + wz);
  out[6] = 2 * (zx - wy);
  out[7] = 2 * (yz + wx);
}

tr_v3 ct_scale(const tr_v3& a, double s) { return tr_v3{a.x * s, a.y * s, a.z * s}; }
tr_v3 ct_div(const tr_v3& a, double s) { return tr_v3{a.x / s, a.y / s, a.z / s}; }
tr_v3 ct_add(const tr_v3& a, const tr_v3& b) { return tr_v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
void ct_store3(const tr_v3& a, double* p) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }

// pixel_to_vector of a CAHVOR or CAHVORE descriptor on the host: the text the kernels run
int ct_host_ray(const vwgpu_camera& c, double x, double y, tr_v3& vec) {
  if (c.kind == VWGPU_CAMERA_CAHVORE) return tr_cahvore_ray(c, tr_v2{x, y}, vec);
  vec = tr_cahvor_ray(c, tr_v2{x, y}, tr_cahv_flip(c) != 0);
  return TR_OK;
}

// the six landmarks on the left and right edge (hpts) and on the top and bottom edge (vpts) of linearize_camera.  The
// midpoints are the reference's: CAHVOR halves in double but for vpts[4] (CAHVORModel.cc:472-484), CAHVORE divides the
// integers everywhere (CAHVOREModel.cc:314-326).
void ct_landmarks(bool cahvore, int w, int h, tr_v2* hpts, tr_v2* vpts) {
  const double xe = w - 1, ye = h - 1;
  const double ymid = cahvore ? (double)((h - 1) / 2) : (h - 1) / 2.0;
  const double xmid1 = cahvore ? (double)((w - 1) / 2) : (w - 1) / 2.0;
  const double xmid4 = (double)((w - 1) / 2);
  hpts[0] = tr_v2{0, 0}; hpts[1] = tr_v2{0, ymid}; hpts[2] = tr_v2{0, ye};
  hpts[3] = tr_v2{xe, 0}; hpts[4] = tr_v2{xe, ymid}; hpts[5] = tr_v2{xe, ye};
  vpts[0] = tr_v2{0, 0}; vpts[1] = tr_v2{xmid1, 0}; vpts[2] = tr_v2{xe, 0};
  vpts[3] = tr_v2{0, ye}; vpts[4] = tr_v2{xmid4, ye}; vpts[5] = tr_v2{xe, ye};
}

// u3 - dot(d, u3) * d, normalised
tr_v3 ct_reject(const tr_v3& u3, const tr_v3& d) {
  const double s = tr_dot(d, u3);
  return tr_normalize(tr_v3{u3.x - s * d.x, u3.y - s * d.y, u3.z - s * d.z});
}

// the inverse of a 3 x 3 matrix by cofactors (row-major)
void tr_mat_inverse(const double* m, double* out) {
  const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
  const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
  out[0] = c00 / det; out[1] = (m[2] * m[7] - m[1] * m[8]) / det; out[2] = (m[1] * m[5] - m[2] * m[4]) / det;
  out[3] = c01 / det; out[4] = (m[0] * m[8] - m[2] * m[6]) / det; out[5] = (m[2] * m[3] - m[0] * m[5]) / det;
  out[6] = c02 / det; out[7] = (m[1] * m[6] - m[0] * m[7]) / det; out[8] = (m[0] * m[4] - m[1] * m[3]) / det;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------------

extern "C" {

int vwgpu_pinhole_camera(const double* center, const double* rotation, double fu, double fv, double cu, double cv, const double* u_dir,
                         const double* v_dir, const double* w_dir, double pixel_pitch, int distortion_kind, const double* distortion,
                         vwgpu_camera* out) {
  if (!center || !rotation || !u_dir || !v_dir || !w_dir || !out) return VWGPU_ERR_ARGUMENT;
  if (distortion_kind != VWGPU_DISTORTION_NULL && distortion_kind != VWGPU_DISTORTION_TSAI) return VWGPU_ERR_ARGUMENT;
  if (distortion_kind == VWGPU_DISTORTION_TSAI && !distortion) return VWGPU_ERR_ARGUMENT;
  // the asserts of rebuild_camera_matrix (PinholeModel.cc:586-591)
  const tr_v3 u = tr_load3(u_dir), v = tr_load3(v_dir), w = tr_load3(w_dir);
  if (!(tr_dot(u, v) == 0) || !(tr_dot(u, w) == 0) || !(tr_dot(v, w) == 0)) return VWGPU_ERR_ARGUMENT;
  if (!(fabs(tr_norm(u) - 1) < 0.001) || !(fabs(tr_norm(v) - 1) < 0.001) || !(fabs(tr_norm(w) - 1) < 0.001)) return VWGPU_ERR_ARGUMENT;
  std::memset(out, 0, sizeof(*out));
  out->kind = VWGPU_CAMERA_PINHOLE;
  out->distortion_kind = distortion_kind;
  std::memcpy(out->center, center, sizeof(out->center));
  out->pixel_pitch = pixel_pitch;
  out->fu = fu; out->fv = fv; out->cu = cu; out->cv = cv;
  if (distortion) std::memcpy(out->distortion, distortion, sizeof(out->distortion));
  const double uvw[9] = {u.x, u.y, u.z, v.x, v.y, v.z, w.x, w.y, w.z};
  const double rt[9] = {rotation[0], rotation[3], rotation[6], rotation[1], rotation[4], rotation[7], rotation[2], rotation[5], rotation[8]};
  const double k[9] = {fu, 0, cu, 0, fv, cv, 0, 0, 1};
  double ext[9], ext_inv[9], k_inv[9];
  ct_mat_mul3(uvw, rt, ext);
  tr_mat_inverse(ext, ext_inv);
  tr_mat_inverse(k, k_inv);
  ct_mat_mul3(ext_inv, k_inv, out->inv_camera_transform);   // :604
  return VWGPU_OK;
}

int vwgpu_pinhole_camera_matrix(const double* center, const double* rotation, double fu, double fv, double cu, double cv,
                                const double* u_dir, const double* v_dir, const double* w_dir, double pixel_pitch, int distortion_kind,
                                const double* distortion, double* out) {
  (void)pixel_pitch; (void)distortion;
  if (!center || !rotation || !u_dir || !v_dir || !w_dir || !out) return VWGPU_ERR_ARGUMENT;
  if (distortion_kind != VWGPU_DISTORTION_NULL && distortion_kind != VWGPU_DISTORTION_TSAI) return VWGPU_ERR_ARGUMENT;
  // the asserts of rebuild_camera_matrix (PinholeModel.cc:586-591)
  const tr_v3 u = tr_load3(u_dir), v = tr_load3(v_dir), w = tr_load3(w_dir);
  if (!(tr_dot(u, v) == 0) || !(tr_dot(u, w) == 0) || !(tr_dot(v, w) == 0)) return VWGPU_ERR_ARGUMENT;
  if (!(fabs(tr_norm(u) - 1) < 0.001) || !(fabs(tr_norm(v) - 1) < 0.001) || !(fabs(tr_norm(w) - 1) < 0.001)) return VWGPU_ERR_ARGUMENT;
  const double uvw[9] = {u.x, u.y, u.z, v.x, v.y, v.z, w.x, w.y, w.z};
  const double rt[9] = {rotation[0], rotation[3], rotation[6], rotation[1], rotation[4], rotation[7], rotation[2], rotation[5], rotation[8]};
  double neg_rt[9], r33[9], t33[9], ext[12];
  for (int k = 0; k < 9; ++k) neg_rt[k] = -rt[k];
  ct_mat_mul3(uvw, rt, r33);       // :600
  ct_mat_mul3(uvw, neg_rt, t33);   // :601, (uvwRotation * (-rotation_inverse)) * m_camera_center
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) ext[i * 4 + j] = r33[i * 3 + j];
    ext[i * 4 + 3] = tr_dot(tr_load3(t33 + 3 * i), tr_load3(center));
  }
  const double k[9] = {fu, 0, cu, 0, fv, cv, 0, 0, 1};
  for (int i = 0; i < 3; ++i)      // :603
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      for (int q = 0; q < 3; ++q) s += k[i * 3 + q] * ext[q * 4 + j];
      out[i * 4 + j] = s;
    }
  return VWGPU_OK;
}

int vwgpu_camera_set_lens(vwgpu_camera* cam, int distortion_kind, const double* params, int n) {
  if (!cam || cam->kind != VWGPU_CAMERA_PINHOLE || !tr_lens_known(distortion_kind) || n < 0 || (n > 0 && !params)) return VWGPU_ERR_ARGUMENT;
  bool n_ok = false;
  switch (distortion_kind) {
    case VWGPU_DISTORTION_NULL: n_ok = n == 0; break;
    case VWGPU_DISTORTION_TSAI: n_ok = n == 4 || n == 5; break;
    case VWGPU_DISTORTION_FOV: n_ok = n == 1; break;
    case VWGPU_DISTORTION_FISHEYE: n_ok = n == 4; break;
    case VWGPU_DISTORTION_BROWN_CONRADY: n_ok = n == 8; break;
    case VWGPU_DISTORTION_ADJUSTABLE_TSAI: n_ok = n >= 4 && n <= 13; break;
    default: n_ok = n == 9; break;   // Photometrix
  }
  if (!n_ok) return VWGPU_ERR_ARGUMENT;
  double L[14] = {0};
  for (int k = 0; k < n; ++k) {
    if (!std::isfinite(params[k])) return VWGPU_ERR_ARGUMENT;
    L[k] = params[k];
  }
  if (distortion_kind == VWGPU_DISTORTION_FOV) {
    // FovLensDistortion::set_distortion_parameters (LensDistortion.cc:441-455)
    if (L[0] <= 0) return VWGPU_ERR_ARGUMENT;
    L[1] = 1 / L[0];
    L[2] = 2 * tan(L[0] / 2);
  } else if (distortion_kind == VWGPU_DISTORTION_BROWN_CONRADY) {
    L[8] = sin(L[7]);
    L[9] = cos(L[7]);
  } else if (distortion_kind == VWGPU_DISTORTION_ADJUSTABLE_TSAI) {
    L[13] = (double)n;
  }
  cam->distortion_kind = distortion_kind;
  std::memcpy(cam->distortion, L, 5 * sizeof(double));
  std::memcpy(cam->A, L + 5, 3 * sizeof(double));
  std::memcpy(cam->H, L + 8, 3 * sizeof(double));
  std::memcpy(cam->V, L + 11, 3 * sizeof(double));
  return VWGPU_OK;
}

int vwgpu_lens_coordinates(const vwgpu_camera* cam, int direction, const double* points, long long n, double* out, long long* failed) {
  if (failed) *failed = 0;
  if (!cam || cam->kind != VWGPU_CAMERA_PINHOLE || !tr_lens_valid(*cam) || (direction != 0 && direction != 1) || n < 0 ||
      (n > 0 && (!points || !out)))
    return VWGPU_ERR_ARGUMENT;
  const vwgpu_camera c = *cam;
  long long count = 0;
  for (long long i = 0; i < n; ++i) {
    const tr_v2 p{points[2 * i], points[2 * i + 1]};
    tr_v2 q;
    if (direction == 1) {
      q = tr_lens_undistort(c, p);
    } else if (!tr_lens_distort(c, p, q)) {
      q = tr_v2{std::nan(""), std::nan("")};
      ++count;
    }
    out[2 * i] = q.x;
    out[2 * i + 1] = q.y;
  }
  if (failed) *failed = count;
  return count != 0 ? VWGPU_ERR_LOGIC : VWGPU_OK;
}

int vwgpu_epipolar_pinhole(const double* center0, const double* rotation0, const double* focal0, const double* offset0, double pitch0,
                           const double* center1, const double* rotation1, const double* focal1, const double* offset1, double pitch1,
                           double* rotation, double* focal, double* offset, double* pitch) {
  if (!center0 || !rotation0 || !focal0 || !offset0 || !center1 || !rotation1 || !focal1 || !offset1 || !rotation || !focal || !offset ||
      !pitch)
    return VWGPU_ERR_ARGUMENT;
  const tr_v3 c0 = tr_load3(center0), c1 = tr_load3(center1);
  if (c0.x == c1.x && c0.y == c1.y && c0.z == c1.z) return VWGPU_ERR_ARGUMENT;   // no baseline
  double rot0[9], rot1[9];
  ct_pose_round_trip(rotation0, rot0);
  ct_pose_round_trip(rotation1, rot1);
  const tr_v3 look0{-1 * rot0[2], -1 * rot0[5], -1 * rot0[8]}, look1{-1 * rot1[2], -1 * rot1[5], -1 * rot1[8]};
  const tr_v3 u = ct_div(tr_sub(c1, c0), tr_norm(tr_sub(c1, c0)));
  const tr_v3 mean_look = ct_div(ct_add(look0, look1), 2.0);
  const tr_v3 temp = tr_cross(u, tr_cross(mean_look, u));
  const tr_v3 w = ct_div(temp, tr_norm(temp));
  const tr_v3 v = tr_cross(w, u);
  const double new_rot[9] = {u.x, -v.x, -w.x, u.y, -v.y, -w.y, u.z, -v.z, -w.z};
  std::memcpy(rotation, new_rot, sizeof(new_rot));
  focal[0] = (focal0[0] + focal1[0]) / 2.0;
  focal[1] = (focal0[1] + focal1[1]) / 2.0;
  offset[0] = (offset0[0] + offset1[0]) / 2.0;
  offset[1] = (offset0[1] + offset1[1]) / 2.0;
  *pitch = (pitch0 + pitch1) / 2.0;
  return VWGPU_OK;
}

int vwgpu_epipolar_cahv(const vwgpu_camera* src0, const vwgpu_camera* src1, vwgpu_camera* dst0, vwgpu_camera* dst1) {
  if (!src0 || !src1 || !dst0 || !dst1) return VWGPU_ERR_ARGUMENT;
  if (src0->kind != VWGPU_CAMERA_CAHV || src1->kind != VWGPU_CAMERA_CAHV) return VWGPU_ERR_ARGUMENT;
  const tr_v3 C0 = tr_load3(src0->center), C1 = tr_load3(src1->center);
  if (C0.x == C1.x && C0.y == C1.y && C0.z == C1.z) return VWGPU_ERR_ARGUMENT;
  const tr_v3 A0 = tr_load3(src0->A), H0 = tr_load3(src0->H), V0 = tr_load3(src0->V);
  const tr_v3 A1 = tr_load3(src1->A), H1 = tr_load3(src1->H), V1 = tr_load3(src1->V);
  const double hc = tr_dot(H0, A0) / 2.0 + tr_dot(H1, A1) / 2.0;
  const double vc = tr_dot(V0, A0) / 2.0 + tr_dot(V1, A1) / 2.0;
  const double hs = tr_norm(tr_cross(A0, H0)) / 2.0 + tr_norm(tr_cross(A1, H1)) / 2.0;
  const double vs = tr_norm(tr_cross(A0, V0)) / 2.0 + tr_norm(tr_cross(A1, V1)) / 2.0;
  tr_v3 app = ct_add(A0, A1);
  const tr_v3 f = tr_cross(tr_cross(app, tr_sub(C1, C0)), app);
  tr_v3 hp;
  if (tr_dot(f, H0) > 0) hp = ct_div(ct_scale(f, hs), tr_norm(f));
  else hp = ct_div(ct_scale(tr_v3{-f.x, -f.y, -f.z}, hs), tr_norm(f));
  app = ct_scale(app, 0.5);
  const tr_v3 g = ct_div(ct_scale(hp, tr_dot(app, hp)), hs * hs);
  const tr_v3 a = tr_normalize(tr_sub(app, g));
  const tr_v3 vp = ct_div(ct_scale(tr_cross(a, hp), vs), hs);
  vwgpu_camera out{};
  out.kind = VWGPU_CAMERA_CAHV;
  ct_store3(a, out.A);
  ct_store3(ct_add(hp, ct_scale(a, hc)), out.H);
  ct_store3(ct_add(vp, ct_scale(a, vc)), out.V);
  ct_store3(C1, out.center);
  const vwgpu_camera second = out;
  ct_store3(C0, out.center);
  *dst0 = out;
  *dst1 = second;
  return VWGPU_OK;
}

int vwgpu_cahvor_camera(const double* C, const double* A, const double* H, const double* V, const double* O, const double* R,
                        vwgpu_camera* out) {
  if (!C || !A || !H || !V || !O || !R || !out) return VWGPU_ERR_ARGUMENT;
  std::memset(out, 0, sizeof(*out));
  out->kind = VWGPU_CAMERA_CAHVOR;
  std::memcpy(out->center, C, sizeof(out->center));
  std::memcpy(out->A, A, sizeof(out->A));
  std::memcpy(out->H, H, sizeof(out->H));
  std::memcpy(out->V, V, sizeof(out->V));
  std::memcpy(out->inv_camera_transform, O, 3 * sizeof(double));
  std::memcpy(out->inv_camera_transform + 3, R, 3 * sizeof(double));
  return VWGPU_OK;
}

int vwgpu_cahvore_camera(const double* C, const double* A, const double* H, const double* V, const double* O, const double* R,
                         const double* E, int type, double P, vwgpu_camera* out) {
  if (!E) return VWGPU_ERR_ARGUMENT;
  // CAHVOREModel(C, A, H, V, O, R, E, T, P) (CAHVOREModel.cc:111-124)
  switch (type) {
    case 1: P = 1.0; break;
    case 2: P = 0.0; break;
    case 3:
      if (P < 0 || P > 1 || P != P) return VWGPU_ERR_ARGUMENT;
      break;
    default: return VWGPU_ERR_ARGUMENT;
  }
  int rc = vwgpu_cahvor_camera(C, A, H, V, O, R, out);
  if (rc) return rc;
  out->kind = VWGPU_CAMERA_CAHVORE;
  std::memcpy(out->inv_camera_transform + 6, E, 3 * sizeof(double));
  out->distortion[0] = P;
  return VWGPU_OK;
}

int vwgpu_linearize_camera(const vwgpu_camera* src, int in_w, int in_h, int out_w, int out_h, vwgpu_camera* dst) {
  if (!src || !dst || !tr_new_kind(*src) || in_w <= 0 || in_h <= 0 || out_w <= 0 || out_h <= 0) return VWGPU_ERR_ARGUMENT;
  const vwgpu_camera cam = *src;   // dst may be src
  const bool cahvore = cam.kind == VWGPU_CAMERA_CAHVORE;
  tr_v2 hpts[6], vpts[6];
  ct_landmarks(cahvore, in_w, in_h, hpts, vpts);
  tr_v3 hray[6], vray[6];
  for (int k = 0; k < 6; ++k)
    if (ct_host_ray(cam, hpts[k].x, hpts[k].y, hray[k]) != TR_OK || ct_host_ray(cam, vpts[k].x, vpts[k].y, vray[k]) != TR_OK) return VWGPU_ERR_LOGIC;
  tr_v3 A{0.0, 0.0, 0.0};
  if (cahvore) {
    // the ray of the real-valued centre (CAHVOREModel.cc:329-330)
    if (ct_host_ray(cam, (in_w - 1) / 2.0, (in_h - 1) / 2.0, A) != TR_OK) return VWGPU_ERR_LOGIC;
  } else {
    // the normalised sum over vpts, then hpts (CAHVORModel.cc:486-492)
    for (int k = 0; k < 6; ++k) A = ct_add(A, vray[k]);
    for (int k = 0; k < 6; ++k) A = ct_add(A, hray[k]);
    A = tr_normalize(A);
  }
  // the original right and down vectors, made orthogonal to the new axis
  const tr_v3 srcA = tr_load3(cam.A), srcH = tr_load3(cam.H);
  tr_v3 dn = tr_cross(srcA, srcH);
  tr_v3 rt = tr_normalize(tr_cross(dn, srcA));
  dn = tr_normalize(dn);
  rt = tr_cross(dn, A);
  dn = tr_normalize(tr_cross(A, rt));
  rt = tr_normalize(rt);
  double hmin = 1, hmax = -1, vmin = 1, vmax = -1;
  for (int k = 0; k < 6; ++k) {
    const tr_v3 n = ct_reject(hray[k], dn);
    const double v = cahvore ? tr_dot(A, n) : tr_norm(tr_cross(A, n));
    if (hmin > v) hmin = v;
    if (hmax < v) hmax = v;
  }
  for (int k = 0; k < 6; ++k) {
    const tr_v3 n = ct_reject(vray[k], rt);
    const double v = cahvore ? tr_dot(A, n) : tr_norm(tr_cross(A, n));
    if (vmin > v) vmin = v;
    if (vmax < v) vmax = v;
  }
  double scale[2], centre[2] = {(out_w - 1) / 2.0, (out_h - 1) / 2.0};
  if (cahvore) {
    // minfov: the larger cosines, limited to a field of view of 135 degrees (CAHVOREModel.cc:359-371)
    const double limfov = 3.14159265358979323846 * 3 / 4;
    double cosines[2] = {hmax, vmax};
    if (acos(cosines[0]) > limfov) cosines[0] = cos(limfov);
    if (acos(cosines[1]) > limfov) cosines[1] = cos(limfov);
    scale[0] = (out_w / 2.0 * cosines[0]) / sqrt(1 - cosines[0] * cosines[0]);
    scale[1] = (out_h / 2.0 * cosines[1]) / sqrt(1 - cosines[1] * cosines[1]);
  } else {
    // minfov: the smaller sines (CAHVORModel.cc:527-534)
    const double c2[2] = {centre[0] * centre[0], centre[1] * centre[1]};
    scale[0] = sqrt(c2[0] / (hmin * hmin) - c2[0]);
    scale[1] = sqrt(c2[1] / (vmin * vmin) - c2[1]);
  }
  vwgpu_camera out{};
  out.kind = VWGPU_CAMERA_CAHV;
  std::memcpy(out.center, cam.center, sizeof(out.center));
  ct_store3(A, out.A);
  ct_store3(ct_add(ct_scale(rt, scale[0]), ct_scale(A, centre[0])), out.H);
  ct_store3(ct_add(ct_scale(dn, scale[1]), ct_scale(A, centre[1])), out.V);
  *dst = out;
  return VWGPU_OK;
}

}  // extern "C"
