// image_sample.h — what vw::transform is built from, as __host__ __device__ functions: the closed-form 2-D maps of
// src/vw/Math/Transform.h:231-443 as steps of a chain, the edge extensions of src/vw/Image/EdgeExtension.tcc:47-272 and the
// three interpolations of src/vw/Image/Interpolation.h:75-225 on float pixels with an optional validity mask
// (PixelMask<float>, src/vw/Image/PixelMask.h:321-345, :424-433).  transform.hip runs them per output pixel, and its host
// point entry runs the same map steps.  tests/refimpl/transform_ref.cc restates all of it on its own.
//
// The maps are double in the reference's expression order, the bilinear tap is float and the bicubic one double, every
// product and sum rounded on its own (-ffp-contract=off).
#pragma once
#include <cmath>
#include <cstdint>

#include "vwgpu.h"

#define IS_HD __host__ __device__ inline

// IS_SCALAR_TAPS: the interior bicubic rows as four dword loads each instead of one 16-byte load (tools build, csrc/Makefile,
// which also turns the compiler's load-store vectoriser off: it fuses four adjacent dword loads into the 16-byte one).

// ---- the maps ------------------------------------------------------------------------------------------------------------
// One direction of one vwgpu_transform, as the host resolves it (transform.hip, tf_resolve): the arithmetic and its words.
enum {
  IS_OP_IDENTITY = 0,
  IS_OP_ADD,          // TranslateTransform::forward: p + (w0, w1)
  IS_OP_SUB,          // TranslateTransform::reverse: p - (w0, w1)
  IS_OP_MUL,          // ResampleTransform::forward: p * (w0, w1)
  IS_OP_DIV,          // ResampleTransform::reverse: p / (w0, w1)
  IS_OP_AFFINE_POST,  // AffineTransform::forward: (w0 x + w1 y + w4, w2 x + w3 y + w5)
  IS_OP_AFFINE_PRE,   // AffineTransform::reverse: the matrix w0..w3 applied to p - (w4, w5)
  IS_OP_HOMOGRAPHY    // HomographyTransform::forward / reverse: w first, then each numerator divided by it
};
struct is_v2 { double x, y; };
struct is_step { int op, pad; double w[9]; };
struct is_chain { int n, pad; is_step s[4]; };   // applied in array order

IS_HD is_v2 is_step_apply(const is_step& s, const is_v2& p) {
  const double* w = s.w;
  switch (s.op) {
    case IS_OP_ADD: return is_v2{p.x + w[0], p.y + w[1]};
    case IS_OP_SUB: return is_v2{p.x - w[0], p.y - w[1]};
    case IS_OP_MUL: return is_v2{p.x * w[0], p.y * w[1]};
    case IS_OP_DIV: return is_v2{p.x / w[0], p.y / w[1]};
    case IS_OP_AFFINE_POST: return is_v2{w[0] * p.x + w[1] * p.y + w[4], w[2] * p.x + w[3] * p.y + w[5]};
    case IS_OP_AFFINE_PRE: {
      const double px = p.x - w[4], py = p.y - w[5];
      return is_v2{w[0] * px + w[1] * py, w[2] * px + w[3] * py};
    }
    case IS_OP_HOMOGRAPHY: {
      const double d = w[6] * p.x + w[7] * p.y + w[8];
      return is_v2{(w[0] * p.x + w[1] * p.y + w[2]) / d, (w[3] * p.x + w[4] * p.y + w[5]) / d};
    }
    default: return p;
  }
}
IS_HD is_v2 is_chain_apply(const is_chain& c, is_v2 p) {
  for (int k = 0; k < c.n; ++k) p = is_step_apply(c.s[k], p);
  return p;
}

// ---- the edge-extended source ----------------------------------------------------------------------------------------------
struct is_src {
  const float* px;
  long long stride;
  int w, h;
  const uint8_t* mask;   // nullptr: every pixel valid
  long long mstride;
  int edge;              // vwgpu_transform_edge
  float edge_value;      // VWGPU_TRANSFORM_EDGE_VALUE; 0 and invalid for VWGPU_TRANSFORM_EDGE_ZERO
  int edge_valid;
};

template <bool MASKED>
IS_HD float is_at(const is_src& s, int x, int y, bool& valid) {
  if (MASKED && s.mask && s.mask[(long long)y * s.mstride + x] == 0) valid = false;
  return s.px[(long long)y * s.stride + x];
}
IS_HD float is_at(const is_src& s, int x, int y) { return s.px[(long long)y * s.stride + x]; }

IS_HD int is_clamp(int i, int n) { return i < 0 ? 0 : i >= n ? n - 1 : i; }
// PeriodicEdgeExtension (EdgeExtension.tcc:113-120)
IS_HD int is_periodic(int i, int n) {
  int d = i % n;
  if (d < 0) d += n;
  return d;
}
// ReflectEdgeExtension (:190-200); n >= 2
IS_HD int is_reflect(int i, int n) {
  int d = i;
  if (d < 0) d = -d;
  const int nm1 = n - 1;
  d %= 2 * nm1;
  if (d > nm1) d = 2 * nm1 - d;
  return d;
}
// LinearEdgeExtension (:254-272) on float pixels: the int32 offsets are converted to float, left to right; w, h >= 2
IS_HD float is_linear(const is_src& s, int i, int j) {
  const int vcm1 = s.w - 1, vrm1 = s.h - 1;
  if (i < 0) {
    if (j < 0) return is_at(s, 0, 0) - i * (is_at(s, 0, 0) - is_at(s, 1, 0)) - j * (is_at(s, 0, 0) - is_at(s, 0, 1));
    else if (j > vrm1)
      return is_at(s, 0, vrm1) - i * (is_at(s, 0, vrm1) - is_at(s, 1, vrm1)) + (j - vrm1) * (is_at(s, 0, vrm1) - is_at(s, 0, vrm1 - 1));
    else return is_at(s, 0, j) - i * (is_at(s, 0, j) - is_at(s, 1, j));
  } else if (i > vcm1) {
    if (j < 0)
      return is_at(s, vcm1, 0) + (i - vcm1) * (is_at(s, vcm1, 0) - is_at(s, vcm1 - 1, 0)) - j * (is_at(s, vcm1, 0) - is_at(s, vcm1, 1));
    else if (j > vrm1)
      return is_at(s, vcm1, vrm1) + (i - vcm1) * (is_at(s, vcm1, vrm1) - is_at(s, vcm1 - 1, vrm1)) +
             (j - vrm1) * (is_at(s, vcm1, vrm1) - is_at(s, vcm1, vrm1 - 1));
    else return is_at(s, vcm1, j) + (i - vcm1) * (is_at(s, vcm1, j) - is_at(s, vcm1 - 1, j));
  } else {
    if (j < 0) return is_at(s, i, 0) - j * (is_at(s, i, 0) - is_at(s, i, 1));
    else if (j > vrm1) return is_at(s, i, vrm1) + (j - vrm1) * (is_at(s, i, vrm1) - is_at(s, i, vrm1 - 1));
    else return is_at(s, i, j);
  }
}

// pixel (i, j) of the edge-extended source, anywhere
template <bool MASKED>
IS_HD float is_tap(const is_src& s, int i, int j, bool& valid) {
  int di = i, dj = j;
  switch (s.edge) {
    case VWGPU_TRANSFORM_EDGE_CONSTANT: di = is_clamp(i, s.w); dj = is_clamp(j, s.h); break;
    case VWGPU_TRANSFORM_EDGE_PERIODIC: di = is_periodic(i, s.w); dj = is_periodic(j, s.h); break;
    case VWGPU_TRANSFORM_EDGE_CYLINDRICAL: di = is_periodic(i, s.w); dj = is_clamp(j, s.h); break;
    case VWGPU_TRANSFORM_EDGE_REFLECT: di = is_reflect(i, s.w); dj = is_reflect(j, s.h); break;
    case VWGPU_TRANSFORM_EDGE_LINEAR: return is_linear(s, i, j);   // never masked
    default:   // ZeroEdgeExtension, ValueEdgeExtension (:49-54, :71-76)
      if (!(i >= 0 && j >= 0 && i < s.w && j < s.h)) {
        if (MASKED && !s.edge_valid) valid = false;
        return s.edge_value;
      }
  }
  return is_at<MASKED>(s, di, dj, valid);
}

IS_HD bool is_inside(const is_src& s, int xa, int ya, int xb, int yb) { return xa >= 0 && ya >= 0 && xb < s.w && yb < s.h; }

// the four floats of an interior bicubic row
struct is_row4 { float v[4]; };
IS_HD is_row4 is_load_row4(const float* p) {
  is_row4 r;
#if defined(IS_SCALAR_TAPS)
  r.v[0] = p[0]; r.v[1] = p[1]; r.v[2] = p[2]; r.v[3] = p[3];
#else
  typedef float is_f4u __attribute__((ext_vector_type(4), aligned(4)));   // one 16-byte load at 4-byte alignment
  const is_f4u q = *reinterpret_cast<const is_f4u*>(p);
  r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
#endif
  return r;
}

// BilinearInterpolationImpl (:94-105) on its four taps; mosaic.hip runs it per channel of an interleaved pixel
IS_HD float is_bilinear_mix(float t00, float t10, float t01, float t11, float normx, float normy) {
  const float norm1mx = 1.0f - normx, norm1my = 1.0f - normy;
  float res = t00 * norm1mx;
  res += t10 * normx;
  res *= norm1my;
  float row = t01 * norm1mx;
  row += t11 * normx;
  res += row * normy;
  return res;
}

// ---- the interpolations ------------------------------------------------------------------------------------------------
// The value of the interpolation at (qx, qy); `valid` is set: false where a tap that was used is invalid.  A coordinate
// that is NaN or beyond +-2^30 has an undefined int32 conversion in the reference: 0 and invalid here.  Every pixel
// takes one of two paths: all its taps inside the source (plain loads, no edge logic) or through is_tap.
template <int INTERP, bool MASKED>
IS_HD float is_sample(const is_src& s, double qx, double qy, bool& valid) {
  const double lim = 1073741824.0;
  valid = false;
  if (!(qx >= -lim && qx <= lim && qy >= -lim && qy <= lim)) return 0.0f;
  valid = true;
  int xi, yi;
  bool single = true;
  if (INTERP == VWGPU_TRANSFORM_INTERP_NEAREST) {
    // NearestPixelInterpolation (Interpolation.h:221-224) over _round (Math/Functions.h:48-51)
    xi = qx < 0 ? (int)(qx - 0.5) : (int)(qx + 0.5);
    yi = qy < 0 ? (int)(qy - 0.5) : (int)(qy + 0.5);
  } else {
    xi = (int)floor(qx);
    yi = (int)floor(qy);
    single = (double)xi == qx && (double)yi == qy;   // the integer-position shortcut (:88-92, :148-151)
  }
  if (single) return is_inside(s, xi, yi, xi, yi) ? is_at<MASKED>(s, xi, yi, valid) : is_tap<MASKED>(s, xi, yi, valid);
  if (INTERP == VWGPU_TRANSFORM_INTERP_BILINEAR) {
    // BilinearInterpolationImpl (:94-105)
    const float normx = (float)qx - (float)xi, normy = (float)qy - (float)yi;
    float t00, t10, t01, t11;
    if (is_inside(s, xi, yi, xi + 1, yi + 1)) {
      t00 = is_at<MASKED>(s, xi, yi, valid);
      t10 = is_at<MASKED>(s, xi + 1, yi, valid);
      t01 = is_at<MASKED>(s, xi, yi + 1, valid);
      t11 = is_at<MASKED>(s, xi + 1, yi + 1, valid);
    } else {
      t00 = is_tap<MASKED>(s, xi, yi, valid);
      t10 = is_tap<MASKED>(s, xi + 1, yi, valid);
      t01 = is_tap<MASKED>(s, xi, yi + 1, valid);
      t11 = is_tap<MASKED>(s, xi + 1, yi + 1, valid);
    }
    return is_bilinear_mix(t00, t10, t01, t11, normx, normy);
  }
  // BicubicInterpolationImpl (:153-184)
  const double normx = qx - xi, normy = qy - yi;
  const double s0 = ((2 - normx) * normx - 1) * normx, t0 = ((2 - normy) * normy - 1) * normy;
  const double s1 = (3 * normx - 5) * normx * normx + 2, t1 = (3 * normy - 5) * normy * normy + 2;
  const double s2 = ((4 - 3 * normx) * normx + 1) * normx, t2 = ((4 - 3 * normy) * normy + 1) * normy;
  const double s3 = (normx - 1) * normx * normx, t3 = (normy - 1) * normy * normy;
  const double t[4] = {t0, t1, t2, t3};
  double result = 0.0;
  const bool inside = is_inside(s, xi - 1, yi - 1, xi + 2, yi + 2);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int y = yi - 1 + r;
    is_row4 v;
    if (inside) {
      v = is_load_row4(s.px + (long long)y * s.stride + (xi - 1));
      if (MASKED && s.mask) {
        const uint8_t* m = s.mask + (long long)y * s.mstride + (xi - 1);
        if (m[0] == 0 || m[1] == 0 || m[2] == 0 || m[3] == 0) valid = false;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) v.v[c] = is_tap<MASKED>(s, xi - 1 + c, y, valid);
    }
    double row = s0 * v.v[0];
    row += s1 * v.v[1];
    row += s2 * v.v[2];
    row += s3 * v.v[3];
    if (r == 0) result = t[0] * row;
    else result += t[r] * row;
  }
  result *= 0.25;
  return (float)result;
}

// TransformViewNoData::operator() (src/vw/Image/Transform.h:430-437): the comparisons are in double, a NaN passes none
IS_HD bool is_nodata(const is_v2& q, int b, int cols, int rows) {
  return q.x < b - 1 || q.x >= cols - b || q.y < b - 1 || q.y >= rows - b;
}
