// disparity_map_ref.cc — CPU restatement (test infrastructure) of the operators of src/vw/Stereo/DisparityMap.h that
// work on a finished disparity map: get_disparity_range (:48-66 with Image/Statistics.h:193-224, :283-290),
// missing_pixel_image (:68-87), disparity_range_mask (:255-300), transform_disparities (:1016-1057 and :1190-1224),
// transform(right, DisparityTransform(d)) (:1164-1187, Image/Interpolation.h:76-110), intersect_mask_and_data
// (:1226-1249), disparity_subsample and disparity_upsample (:1251-1358).  Written from that header as plain sequential
// loops in raster order; dependency-free; built with -ffp-contract=off.
// Layouts: disparity (rows, cols, 3) int32 (type 0) or float32 (type 1) {dx, dy, valid != 0}, packed; images (rows, cols)
// float32; missing_pixel_image (rows, cols, 3) uint8.
// Where the reference leaves the result open the project's definitions (include/vwgpu.h) are used: a warp position that
// is NaN or beyond +-2^30 gives 0; an int32 product of a subsample tap wraps.
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {

struct I32 {
  typedef int32_t chan;
  typedef int64_t acc;   // AccumulatorType<int32> (Core/FundamentalTypes.h:118)
  static chan from_double(double d) { return (chan)d; }
  static chan twice(chan a) { return (chan)((uint32_t)a * 2u); }
  static chan times(int wt, chan a) { return (chan)((uint32_t)wt * (uint32_t)a); }
  static chan one() { return INT32_MAX; }   // validate(): ChannelRange<int32>::max()
  static chan max_minus_one(double mx) { return (chan)mx - 1; }
};
struct F32 {
  typedef float chan;
  typedef double acc;    // AccumulatorType<float32> (Core/FundamentalTypes.h:121)
  static chan from_double(double d) { return (chan)d; }
  static chan twice(chan a) { return a * 2; }
  static chan times(int wt, chan a) { return (float)wt * a; }
  static chan one() { return 1.0f; }
  static chan max_minus_one(double mx) { return (chan)mx - 1; }
};

// PixelAccumulator<EWMinMaxAccumulator<Vector2>> over the image in raster order
template <class T>
void disparity_range(const typename T::chan* d, int w, int h, float* out) {
  typedef typename T::chan C;
  C mn[2] = {0, 0}, mx[2] = {0, 0};
  bool any = false;
  for (long long i = 0; i < (long long)w * h; ++i) {
    const C* p = d + i * 3;
    if (p[2] == 0) continue;   // Statistics.h:287
    if (!any) {
      mn[0] = mx[0] = p[0];
      mn[1] = mx[1] = p[1];
      any = true;
      continue;
    }
    for (int k = 0; k < 2; ++k) {
      if (p[k] < mn[k]) mn[k] = p[k];
      else if (p[k] > mx[k]) mx[k] = p[k];
    }
  }
  out[0] = any ? (float)mn[0] : 0.f;
  out[1] = any ? (float)mn[1] : 0.f;
  out[2] = any ? (float)mx[0] : 0.f;
  out[3] = any ? (float)mx[1] : 0.f;
}

template <class T>
long long range_mask(const typename T::chan* d, int w, int h, int x0, int y0, const double* mn_, const double* mx_, int fixed,
                     typename T::chan* out) {
  typedef typename T::chan C;
  const C mn[2] = {(C)mn_[0], (C)mn_[1]};
  const C mx1[2] = {T::max_minus_one(mx_[0]), T::max_minus_one(mx_[1])};
  const C ylow = fixed ? mn[1] : mn[0];   // DisparityMap.h:279 compares with m_min[0]
  long long masked = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const C* p = d + ((long long)y * w + x) * 3;
      C* o = out + ((long long)y * w + x) * 3;
      const double loc[2] = {(double)((long long)x0 + x), (double)((long long)y0 + y)};
      const C px = p[0], py = p[1], pv = p[2];
      if (pv != 0 && (loc[0] + px < mn[0] || loc[0] + px >= mx1[0] || loc[1] + py < ylow || loc[1] + py >= mx1[1])) {
        o[0] = o[1] = o[2] = 0;
        ++masked;
      } else {
        o[0] = px; o[1] = py; o[2] = pv;
      }
    }
  return masked;
}

// HomographyTransform::forward (Math/Transform.h:383-387)
void homography(const double* m, const double* p, double* q) {
  const double w = m[6] * p[0] + m[7] * p[1] + m[8];
  q[0] = (m[0] * p[0] + m[1] * p[1] + m[2]) / w;
  q[1] = (m[3] * p[0] + m[4] * p[1] + m[5]) / w;
}

// mode 0: TransformDisparitiesFunc with the applied matrix; 1, 2: the subregion overload without / with round()
template <class T>
void transform(const typename T::chan* d, int w, int h, int x0, int y0, const double* m, int mode, typename T::chan* out) {
  typedef typename T::chan C;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const C* p = d + ((long long)y * w + x) * 3;
      C* o = out + ((long long)y * w + x) * 3;
      const C px = p[0], py = p[1], pv = p[2];
      if (mode != 0 && pv == 0) {
        o[0] = o[1] = o[2] = 0;
        continue;
      }
      const double loc[2] = {(double)((long long)x0 + x), (double)((long long)y0 + y)};
      const double old_point[2] = {loc[0] + px, loc[1] + py};
      double new_point[2];
      homography(m, old_point, new_point);
      double diff[2] = {new_point[0] - loc[0], new_point[1] - loc[1]};
      if (mode == 2) {
        diff[0] = std::round(diff[0]);
        diff[1] = std::round(diff[1]);
      }
      o[0] = T::from_double(diff[0]);
      o[1] = T::from_double(diff[1]);
      o[2] = pv;
    }
}

template <class T>
void subsample(const typename T::chan* d, int w, int h, typename T::chan* out) {
  typedef typename T::chan C;
  typedef typename T::acc A;
  const int ow = 1 + (w - 1) / 2, oh = 1 + (h - 1) / 2;
  auto child = [&](int x, int y) {   // ConstantEdgeExtension
    x = x < 0 ? 0 : (x >= w ? w - 1 : x);
    y = y < 0 ? 0 : (y >= h ? h - 1 : y);
    return d + ((long long)y * w + x) * 3;
  };
  for (int j = 0; j < oh; ++j)
    for (int i = 0; i < ow; ++i) {
      const int ci = i << 1, cj = j << 1;
      A buffer[2] = {0, 0}, count = 0;
      const C* p;
      // the accumulator-typed taps (:1273-1281)
      p = child(ci, cj);         if (p[2] != 0) { count += 10; buffer[0] += 10 * (A)p[0]; buffer[1] += 10 * (A)p[1]; }
      p = child(ci + 1, cj);     if (p[2] != 0) { count += 5;  buffer[0] += 5 * (A)p[0];  buffer[1] += 5 * (A)p[1]; }
      p = child(ci, cj + 1);     if (p[2] != 0) { count += 5;  buffer[0] += 5 * (A)p[0];  buffer[1] += 5 * (A)p[1]; }
      // the pixel-typed taps (:1282-1299)
      p = child(ci - 1, cj);     if (p[2] != 0) { count += 5;  buffer[0] += T::times(5, p[0]); buffer[1] += T::times(5, p[1]); }
      p = child(ci, cj - 1);     if (p[2] != 0) { count += 5;  buffer[0] += T::times(5, p[0]); buffer[1] += T::times(5, p[1]); }
      p = child(ci + 1, cj + 1); if (p[2] != 0) { count += 2;  buffer[0] += T::times(2, p[0]); buffer[1] += T::times(2, p[1]); }
      p = child(ci - 1, cj - 1); if (p[2] != 0) { count += 2;  buffer[0] += T::times(2, p[0]); buffer[1] += T::times(2, p[1]); }
      p = child(ci - 1, cj + 1); if (p[2] != 0) { count += 2;  buffer[0] += T::times(2, p[0]); buffer[1] += T::times(2, p[1]); }
      p = child(ci + 1, cj - 1); if (p[2] != 0) { count += 2;  buffer[0] += T::times(2, p[0]); buffer[1] += T::times(2, p[1]); }
      C* o = out + ((long long)j * ow + i) * 3;
      if (count > 0) {
        o[0] = (C)(buffer[0] / (count * 2));
        o[1] = (C)(buffer[1] / (count * 2));
        o[2] = T::one();
      } else {
        o[0] = o[1] = o[2] = 0;
      }
    }
}

template <class T>
void upsample(const typename T::chan* d, int w, int h, typename T::chan* out) {
  typedef typename T::chan C;
  for (int j = 0; j < 2 * h; ++j)
    for (int i = 0; i < 2 * w; ++i) {
      const C* p = d + ((long long)(j >> 1) * w + (i >> 1)) * 3;
      C* o = out + ((long long)j * 2 * w + i) * 3;
      o[0] = T::twice(p[0]);
      o[1] = T::twice(p[1]);
      o[2] = p[2];
    }
}

template <class T>
void missing(const typename T::chan* d, int w, int h, uint8_t* out) {
  for (long long i = 0; i < (long long)w * h; ++i) {
    const bool ok = d[i * 3 + 2] != 0;
    out[i * 3] = ok ? 200 : 255;
    out[i * 3 + 1] = out[i * 3 + 2] = ok ? 200 : 0;
  }
}

template <class T>
void intersect(const typename T::chan* data, const typename T::chan* mask, int w, int h, typename T::chan* out) {
  for (long long i = 0; i < (long long)w * h; ++i) {
    const typename T::chan* src = data + i * 3;
    if (data[i * 3 + 2] == 0 && mask[i * 3 + 2] != 0) src = mask + i * 3;
    const typename T::chan a = src[0], b = src[1], c = src[2];
    out[i * 3] = a; out[i * 3 + 1] = b; out[i * 3 + 2] = c;
  }
}

struct RightImage {
  const float* px;
  int w, h;
  float at(int x, int y) const { return (x < 0 || y < 0 || x >= w || y >= h) ? 0.0f : px[(long long)y * w + x]; }   // ZeroEdgeExtension
};

// BilinearInterpolationImpl::operator() (Image/Interpolation.h:77-109) on a float image
float bilinear(const RightImage& view, double i, double j) {
  if (!(std::fabs(i) <= 1073741824.0) || !(std::fabs(j) <= 1073741824.0)) return 0.0f;   // the project's definition
  const int32_t x = (int32_t)std::floor(i), y = (int32_t)std::floor(j);
  if (x == i && y == j) return view.at(x, y);
  const float normx = float(i) - float(x), normy = float(j) - float(y), norm1mx = 1 - normx, norm1my = 1 - normy;
  float result = view.at(x, y) * norm1mx;
  result += view.at(x + 1, y) * normx;
  result *= norm1my;
  float row = view.at(x, y + 1) * norm1mx;
  row += view.at(x + 1, y + 1) * normx;
  result += row * normy;
  return result;
}

}  // namespace

extern "C" {

int dmr_get_disparity_range(int type, const void* d, int w, int h, float* out) {
  if (w <= 0 || h <= 0) return 1;
  if (type == 0) disparity_range<I32>(static_cast<const int32_t*>(d), w, h, out);
  else disparity_range<F32>(static_cast<const float*>(d), w, h, out);
  return 0;
}

int dmr_disparity_range_mask(int type, const void* d, int w, int h, int x0, int y0, const double* mn, const double* mx, int fixed,
                             void* out, long long* masked) {
  if (w <= 0 || h <= 0) return 1;
  *masked = type == 0 ? range_mask<I32>(static_cast<const int32_t*>(d), w, h, x0, y0, mn, mx, fixed, static_cast<int32_t*>(out))
                      : range_mask<F32>(static_cast<const float*>(d), w, h, x0, y0, mn, mx, fixed, static_cast<float*>(out));
  return 0;
}

int dmr_transform_disparities(int type, const void* d, int w, int h, int x0, int y0, const double* m, int mode, void* out) {
  if (w <= 0 || h <= 0 || mode < 0 || mode > 2) return 1;
  if (type == 0) transform<I32>(static_cast<const int32_t*>(d), w, h, x0, y0, m, mode, static_cast<int32_t*>(out));
  else transform<F32>(static_cast<const float*>(d), w, h, x0, y0, m, mode, static_cast<float*>(out));
  return 0;
}

int dmr_disparity_subsample(int type, const void* d, int w, int h, void* out) {
  if (w <= 0 || h <= 0) return 1;
  if (type == 0) subsample<I32>(static_cast<const int32_t*>(d), w, h, static_cast<int32_t*>(out));
  else subsample<F32>(static_cast<const float*>(d), w, h, static_cast<float*>(out));
  return 0;
}

int dmr_disparity_upsample(int type, const void* d, int w, int h, void* out) {
  if (w <= 0 || h <= 0) return 1;
  if (type == 0) upsample<I32>(static_cast<const int32_t*>(d), w, h, static_cast<int32_t*>(out));
  else upsample<F32>(static_cast<const float*>(d), w, h, static_cast<float*>(out));
  return 0;
}

int dmr_missing_pixel_image(int type, const void* d, int w, int h, uint8_t* out) {
  if (w <= 0 || h <= 0) return 1;
  if (type == 0) missing<I32>(static_cast<const int32_t*>(d), w, h, out);
  else missing<F32>(static_cast<const float*>(d), w, h, out);
  return 0;
}

int dmr_intersect_mask_and_data(int type, const void* data, const void* mask, int w, int h, void* out) {
  if (w <= 0 || h <= 0) return 1;
  if (type == 0) intersect<I32>(static_cast<const int32_t*>(data), static_cast<const int32_t*>(mask), w, h, static_cast<int32_t*>(out));
  else intersect<F32>(static_cast<const float*>(data), static_cast<const float*>(mask), w, h, static_cast<float*>(out));
  return 0;
}

// DisparityTransform::reverse (DisparityMap.h:1181-1186) at one position: the offset image is read at the nearest pixel
// over ZeroEdgeExtension
void dmr_disparity_transform_reverse(const float* disp, int dw, int dh, double px, double py, double* out) {
  // NearestPixelInterpolation (Image/Interpolation.h:221-224) with _round (Math/Functions.h:48-51)
  const int32_t x = px < 0 ? (int32_t)(px - 0.5) : (int32_t)(px + 0.5), y = py < 0 ? (int32_t)(py - 0.5) : (int32_t)(py + 0.5);
  const bool inside = x >= 0 && y >= 0 && x < dw && y < dh;
  const float* d = inside ? disp + ((long long)y * dw + x) * 3 : nullptr;
  if (!d || d[2] == 0) {
    out[0] = -1;
    out[1] = py;
    return;
  }
  out[0] = px + d[0];
  out[1] = py + d[1];
}

int dmr_disparity_warp(const float* right, int rw, int rh, const float* disp, int dw, int dh, float* out) {
  if (rw <= 0 || rh <= 0 || dw <= 0 || dh <= 0) return 1;
  const RightImage view{right, rw, rh};
  for (int y = 0; y < rh; ++y)
    for (int x = 0; x < rw; ++x) {
      double p[2];
      dmr_disparity_transform_reverse(disp, dw, dh, (double)x, (double)y, p);
      out[(long long)y * rw + x] = bilinear(view, p[0], p[1]);
    }
  return 0;
}

}  // extern "C"
