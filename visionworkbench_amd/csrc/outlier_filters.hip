// outlier_filters.hip — the local outlier filters of src/vw/Stereo/DisparityMap.h that the pyramid does not use:
// rm_outliers_using_mean (DisparityMap.h:444-578), rm_outliers_using_stddev (:600-748), rm_outliers_using_plane
// (:769-927, DisparityMap.cc:37-118), their clean-up compositions disparity_cleanup_using_mean / _stddev and
// disparity_clean_using_plane (:580-598, :750-767, :929-947), and std_dev_image (:949-1014, DisparityMap.cc:24-34).
// tests/refimpl/outlier_filters_ref.cc restates them and DESIGN §4.16 lists what is reproduced.
//
// Every filter is a per-pixel functor over edge_extend(disparity, ConstantEdgeExtension()): a window of
// (2 half_h + 1) x (2 half_v + 1) pixels, rows outer and columns inner, every coordinate clamped to the image on its own,
// always read from the unmodified input.  of_kernel<METHOD, TYPE>: one workgroup per 16 x 16 output positions, the
// positions' clamped windows staged in LDS once, one lane per position running the reference's loops in its order in
// double.  An invalid centre is copied, a rejected pixel becomes {0, 0, 0}.
//
// A clean-up composition applies RmOutliersUsingThreshFunc(1, 1, 3.0, 0.2) (DisparityMap.h:357-385) to the INNER VIEW,
// which is also defined one pixel outside the image (the inner functor runs there on clamped reads): the first pass
// writes (w + 2) x (h + 2) positions from (-1, -1) into a padded intermediate, of_thresh_kernel reads it.
//
// rm_outliers_using_stddev / _plane size their value buffers (2 half_v + 1)^2 (DisparityMap.h:656, :829): with
// half_h > half_v the reference writes past them, which is outside what it defines.  The values are only written and
// read back in order, so the kernels compute the evident result for every half_h, half_v.
#include <cmath>
#include <cstring>

#include "vwgpu_internal.h"

namespace {

constexpr int OF_TX = 16, OF_TY = 16, OF_THREADS = OF_TX * OF_TY;
constexpr int OF_MAX_HALF = 15, OF_MAX_STDDEV = 31;   // include/vwgpu.h states these limits

struct of_args {
  const uint32_t* in;      // {dx, dy, valid} per pixel, float or int32 words
  long long istride;       // pixels
  int w, h;
  uint32_t* out;           // position (ox + i, oy + j) is written to pixel j * ostride + i
  long long ostride;
  int ox, oy, ow, oh;
  int hh, hv;
  double p0, p1;           // mean: max_mean_diff^2; stddev, plane: pixel_threshold, rejection_threshold
  int skip;                // mean: VWGPU_OUTLIER_SKIP
  unsigned long long* counter;   // pixels rejected at positions inside the image
};

// PixelMask<Vector2i> / PixelMask<Vector2f> as three 32-bit words
template <int TYPE>
struct of_px;
template <>
struct of_px<VWGPU_DISPARITY_I32> {
  static constexpr uint32_t TOP_BIT = 0x80000000u;
  static __device__ bool valid(uint32_t v) { return v != 0; }
  static __device__ double val(uint32_t a) { return (double)(int32_t)a; }
  // |dx| + |dy|, an int add in the reference; sums that do not fit an int are outside its contract (taken modulo 2^32)
  static __device__ uint32_t key(uint32_t a, uint32_t b) {
    const uint32_t ua = (int32_t)a < 0 ? 0u - a : a, ub = (int32_t)b < 0 ? 0u - b : b;
    return ua + ub;
  }
  static __device__ double mag(uint32_t k) { return (double)k; }
  static __device__ bool key_nan(uint32_t) { return false; }
  static __device__ double absdiff(uint32_t a, uint32_t b) { return fabs((double)(int32_t)(a - b)); }
};
template <>
struct of_px<VWGPU_DISPARITY_F32> {
  static constexpr uint32_t TOP_BIT = 0x40000000u;   // keys are bits of non-negative floats
  static __device__ bool valid(uint32_t v) { return __uint_as_float(v) != 0.f; }
  static __device__ double val(uint32_t a) { return (double)__uint_as_float(a); }
  // |dx| + |dy| as a float add; non-negative floats order as their bits; every NaN becomes one pattern above +inf
  static __device__ uint32_t key(uint32_t a, uint32_t b) {
    const float m = __fadd_rn(fabsf(__uint_as_float(a)), fabsf(__uint_as_float(b)));
    return isnan(m) ? 0x7fc00000u : __float_as_uint(m);
  }
  static __device__ double mag(uint32_t k) { return (double)__uint_as_float(k); }
  static __device__ bool key_nan(uint32_t k) { return k > 0x7f800000u; }
  static __device__ double absdiff(uint32_t a, uint32_t b) {
    return (double)fabsf(__fsub_rn(__uint_as_float(a), __uint_as_float(b)));
  }
};

// RmOutliersUsingMeanFunc (DisparityMap.h:485-553).  win: the window's first pixel in the staged tile, keys: |dx| + |dy|
// of the same pixels.  cutoff = 2.0 * sorted(len)[(int)(0.75 n)]: a selection, by bisection over the keys (the largest v
// with #(keys < v) <= rank).  The mean is taken over the valid pixels with magnitude <= cutoff; in reference semantics a
// window row ends at its first valid pixel above the cutoff (the `continue` at :525 skips next_col()).
template <int TYPE>
__device__ bool of_mean_keep(const uint32_t* win, const uint32_t* keys, int pw, int kw, int kh, double max_diff_sq, int skip,
                             uint32_t cx, uint32_t cy) {
  using P = of_px<TYPE>;
  int n = 0;
  bool nan = false;
  for (int rr = 0; rr < kh; ++rr)
    for (int cc = 0; cc < kw; ++cc) {
      if (!P::valid(win[(rr * pw + cc) * 3 + 2])) continue;
      n += 1;
      nan = nan || P::key_nan(keys[rr * pw + cc]);
    }
  if (nan) return true;   // std::sort over NaN is undefined in the reference: the pixel is left as it is
  const int rank = (int)(0.75 * (double)n);
  uint32_t sel = 0;
  for (uint32_t bit = P::TOP_BIT; bit; bit >>= 1) {
    const uint32_t c = sel | bit;
    int below = 0;
    for (int rr = 0; rr < kh; ++rr)
      for (int cc = 0; cc < kw; ++cc)
        below += (P::valid(win[(rr * pw + cc) * 3 + 2]) && keys[rr * pw + cc] < c) ? 1 : 0;
    if (below <= rank) sel = c;
  }
  const double cutoff = n > 0 ? 2.0 * P::mag(sel) : 0.0;
  double mx = 0.0, my = 0.0;
  int matched = 0;
  for (int rr = 0; rr < kh; ++rr)
    for (int cc = 0; cc < kw; ++cc) {
      const uint32_t* p = win + (rr * pw + cc) * 3;
      if (!P::valid(p[2])) continue;
      if (P::mag(keys[rr * pw + cc]) > cutoff) {
        if (skip) continue;
        break;
      }
      mx += P::val(p[0]);
      my += P::val(p[1]);
      matched += 1;
    }
  double err = max_diff_sq + 1.0;   // :536, no pixel matched
  if (matched > 0) {
    mx = mx / (double)matched;
    my = my / (double)matched;
    const double tx = P::val(cx), ty = P::val(cy);
    err = (tx - mx) * (tx - mx) + (ty - my) * (ty - my);
  }
  return !(err > max_diff_sq);
}

// RmOutliersUsingStdDev (DisparityMap.h:647-723)
template <int TYPE>
__device__ bool of_stddev_keep(const uint32_t* win, int pw, int kw, int kh, double pixel_thr, double reject_thr, uint32_t cx,
                               uint32_t cy) {
  using P = of_px<TYPE>;
  double mx = 0.0, my = 0.0;
  int n = 0;
  for (int rr = 0; rr < kh; ++rr)
    for (int cc = 0; cc < kw; ++cc) {
      const uint32_t* p = win + (rr * pw + cc) * 3;
      if (!P::valid(p[2])) continue;
      mx += P::val(p[0]);
      my += P::val(p[1]);
      n += 1;
    }
  if (n == 0) return false;
  mx = mx / (double)n;
  my = my / (double)n;
  double sx = 0.0, sy = 0.0;
  for (int rr = 0; rr < kh; ++rr)
    for (int cc = 0; cc < kw; ++cc) {
      const uint32_t* p = win + (rr * pw + cc) * 3;
      if (!P::valid(p[2])) continue;
      const double dx = P::val(p[0]) - mx, dy = P::val(p[1]) - my;
      sx += dx * dx;
      sy += dy * dy;
    }
  double sdx = sqrt(sx / (double)n), sdy = sqrt(sy / (double)n);
  if (sdx < reject_thr) sdx = reject_thr;
  if (sdy < reject_thr) sdy = reject_thr;
  const double ex = fabs(P::val(cx) - mx), ey = fabs(P::val(cy) - my);
  return !((ex > pixel_thr * sdx) || (ey > pixel_thr * sdy));
}

// pointToPlaneDist (DisparityMap.cc:76-89) of (x, y, z) from z = a x + b y + c
__device__ inline double of_plane_dist(double a, double b, double c, double x, double y, double z) {
  const double num = fabs(a * x + b * y + -1.0 * z + c);
  const double den = sqrt(a * a + b * b + -1.0 * -1.0);
  return num / den;
}

__device__ inline void of_swap(double& a, double& b) {
  const double t = a;
  a = b;
  b = t;
}

// RmOutliersUsingPlane (DisparityMap.h:820-902).  The normal equations of fitPlaneToPoints (DisparityMap.cc:40-73) in window
// order; the 3 x 3 matrix holds window offsets only and is the same for dx and dy.  The solve is the restatement's
// elimination, operation for operation: unblocked LU with partial pivoting (column-wise search, the first largest |a|
// wins), multipliers by the reciprocal of the pivot, rank-1 update, then the two triangular solves; an exactly zero pivot
// is the reference's "failed to solve" and keeps the pixel (:866-875).
template <int TYPE>
__device__ bool of_plane_keep(const uint32_t* win, int pw, int hh, int hv, double pixel_thr, double reject_thr, uint32_t cx,
                              uint32_t cy) {
  using P = of_px<TYPE>;
  double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0;
  double bx0 = 0.0, bx1 = 0.0, bx2 = 0.0, by0 = 0.0, by1 = 0.0, by2 = 0.0;
  int n = 0;
  for (int yk = -hv; yk <= hv; ++yk)
    for (int xk = -hh; xk <= hh; ++xk) {
      const uint32_t* p = win + ((yk + hv) * pw + xk + hh) * 3;
      if (!P::valid(p[2])) continue;
      const double x = (double)xk, y = (double)yk, zx = P::val(p[0]), zy = P::val(p[1]);
      m00 += x * x;
      m01 += x * y;
      m02 += x;
      m11 += y * y;
      m12 += y;
      bx0 += x * zx;
      bx1 += y * zx;
      bx2 += zx;
      by0 += x * zy;
      by1 += y * zy;
      by2 += zy;
      n += 1;
    }
  if (n == 0) return false;
  double m10 = m01, m20 = m02, m21 = m12, m22 = (double)n;
  // column 0
  {
    int p = 0;
    double big = fabs(m00);
    if (fabs(m10) > big) { big = fabs(m10); p = 1; }
    if (fabs(m20) > big) p = 2;
    if (p == 1) { of_swap(m00, m10); of_swap(m01, m11); of_swap(m02, m12); of_swap(bx0, bx1); of_swap(by0, by1); }
    if (p == 2) { of_swap(m00, m20); of_swap(m01, m21); of_swap(m02, m22); of_swap(bx0, bx2); of_swap(by0, by2); }
    if (m00 == 0.0) return true;
    const double r = 1.0 / m00;
    m10 = m10 * r;
    m20 = m20 * r;
    m11 = m11 - m10 * m01;
    m21 = m21 - m20 * m01;
    m12 = m12 - m10 * m02;
    m22 = m22 - m20 * m02;
  }
  // column 1
  {
    if (fabs(m21) > fabs(m11)) { of_swap(m10, m20); of_swap(m11, m21); of_swap(m12, m22); of_swap(bx1, bx2); of_swap(by1, by2); }
    if (m11 == 0.0) return true;
    const double r = 1.0 / m11;
    m21 = m21 * r;
    m22 = m22 - m21 * m12;
  }
  if (m22 == 0.0) return true;
  // L y = P b, then U x = y, for both right-hand sides
  bx1 = bx1 - bx0 * m10;
  bx2 = bx2 - bx0 * m20;
  bx2 = bx2 - bx1 * m21;
  bx2 = bx2 / m22;
  bx0 = bx0 - bx2 * m02;
  bx1 = bx1 - bx2 * m12;
  bx1 = bx1 / m11;
  bx0 = bx0 - bx1 * m01;
  bx0 = bx0 / m00;
  by1 = by1 - by0 * m10;
  by2 = by2 - by0 * m20;
  by2 = by2 - by1 * m21;
  by2 = by2 / m22;
  by0 = by0 - by2 * m02;
  by1 = by1 - by2 * m12;
  by1 = by1 / m11;
  by0 = by0 - by1 * m01;
  by0 = by0 / m00;
  // checkPointToPlaneFit (DisparityMap.cc:92-118): sqrt(sum dist^2 / n)
  double sx = 0.0, sy = 0.0;
  for (int yk = -hv; yk <= hv; ++yk)
    for (int xk = -hh; xk <= hh; ++xk) {
      const uint32_t* p = win + ((yk + hv) * pw + xk + hh) * 3;
      if (!P::valid(p[2])) continue;
      const double dx = of_plane_dist(bx0, bx1, bx2, (double)xk, (double)yk, P::val(p[0]));
      const double dy = of_plane_dist(by0, by1, by2, (double)xk, (double)yk, P::val(p[1]));
      sx += dx * dx;
      sy += dy * dy;
    }
  double sdx = sqrt(sx / (double)n), sdy = sqrt(sy / (double)n);
  if (sdx < reject_thr) sdx = reject_thr;
  if (sdy < reject_thr) sdy = reject_thr;
  const double ex = of_plane_dist(bx0, bx1, bx2, 0.0, 0.0, P::val(cx));
  const double ey = of_plane_dist(by0, by1, by2, 0.0, 0.0, P::val(cy));
  return !((ex > pixel_thr * sdx) || (ey > pixel_thr * sdy));
}

template <int METHOD, int TYPE>
__global__ __launch_bounds__(OF_THREADS) void of_kernel(of_args a) {
  using P = of_px<TYPE>;
  extern __shared__ uint32_t of_tile[];
  const int pw = OF_TX + 2 * a.hh, ph = OF_TY + 2 * a.hv;
  const int x0 = a.ox + (int)blockIdx.x * OF_TX, y0 = a.oy + (int)blockIdx.y * OF_TY;
  uint32_t* keys = of_tile + pw * ph * 3;   // mean only
  for (int o = threadIdx.x; o < pw * ph; o += OF_THREADS) {
    const int c = min(max(x0 - a.hh + o % pw, 0), a.w - 1), r = min(max(y0 - a.hv + o / pw, 0), a.h - 1);
    const uint32_t* p = a.in + ((long long)r * a.istride + c) * 3;
    const uint32_t dx = p[0], dy = p[1], v = p[2];
    of_tile[o * 3] = dx;
    of_tile[o * 3 + 1] = dy;
    of_tile[o * 3 + 2] = v;
    if (METHOD == VWGPU_OUTLIER_MEAN) keys[o] = P::key(dx, dy);
  }
  __syncthreads();
  const int tx = threadIdx.x % OF_TX, ty = threadIdx.x / OF_TX;
  const int x = x0 + tx, y = y0 + ty;
  int rejected = 0;
  if (x < a.ox + a.ow && y < a.oy + a.oh) {
    const uint32_t* win = of_tile + (ty * pw + tx) * 3;
    const uint32_t* ctr = win + (a.hv * pw + a.hh) * 3;
    uint32_t cx = ctr[0], cy = ctr[1], cv = ctr[2];
    if (P::valid(cv)) {
      bool keep;
      if (METHOD == VWGPU_OUTLIER_MEAN)
        keep = of_mean_keep<TYPE>(win, keys + ty * pw + tx, pw, 2 * a.hh + 1, 2 * a.hv + 1, a.p0, a.skip, cx, cy);
      else if (METHOD == VWGPU_OUTLIER_STDDEV)
        keep = of_stddev_keep<TYPE>(win, pw, 2 * a.hh + 1, 2 * a.hv + 1, a.p0, a.p1, cx, cy);
      else
        keep = of_plane_keep<TYPE>(win, pw, a.hh, a.hv, a.p0, a.p1, cx, cy);
      if (!keep) {
        cx = cy = cv = 0;
        rejected = (x >= 0 && y >= 0 && x < a.w && y < a.h) ? 1 : 0;
      }
    }
    uint32_t* o = a.out + ((long long)(y - a.oy) * a.ostride + (x - a.ox)) * 3;
    o[0] = cx;
    o[1] = cy;
    o[2] = cv;
  }
  const int nr = __syncthreads_count(rejected);
  if (threadIdx.x == 0 && nr) atomicAdd(a.counter, (unsigned long long)nr);
}

// RmOutliersUsingThreshFunc(1, 1, pixel_thr, reject_thr) (DisparityMap.h:357-385) on the padded inner view `pad` of
// (w + 2) x (h + 2) pixels whose pixel (1, 1) is image position (0, 0): no read leaves it
template <int TYPE>
__global__ __launch_bounds__(OF_THREADS) void of_thresh_kernel(const uint32_t* pad, int w, int h, double pixel_thr,
                                                               double reject_thr, uint32_t* out, long long ostride,
                                                               unsigned long long* counter) {
  using P = of_px<TYPE>;
  const int x = (int)blockIdx.x * OF_TX + (int)threadIdx.x % OF_TX, y = (int)blockIdx.y * OF_TY + (int)threadIdx.x / OF_TX;
  int rejected = 0;
  if (x < w && y < h) {
    const long long pw = (long long)w + 2;
    const uint32_t* c = pad + ((long long)(y + 1) * pw + x + 1) * 3;
    uint32_t cx = c[0], cy = c[1], cv = c[2];
    if (P::valid(cv)) {
      int matched = 0, total = 0;
      for (int yk = -1; yk <= 1; ++yk)
        for (int xk = -1; xk <= 1; ++xk) {
          const uint32_t* q = c + (yk * pw + xk) * 3;
          if (P::valid(q[2]) && P::absdiff(cx, q[0]) <= pixel_thr && P::absdiff(cy, q[1]) <= pixel_thr) matched += 1;
          total += 1;
        }
      if ((double)matched / (double)total < reject_thr) {
        cx = cy = cv = 0;
        rejected = 1;
      }
    }
    uint32_t* o = out + ((long long)y * ostride + x) * 3;
    o[0] = cx;
    o[1] = cy;
    o[2] = cv;
  }
  const int nr = __syncthreads_count(rejected);
  if (threadIdx.x == 0 && nr) atomicAdd(counter, (unsigned long long)nr);
}

struct of_sd_args {
  const float* img;
  long long stride;
  int w, h;
  float* out;
  long long ostride;
  int kw, kh, zero_edge;
};

// StdDevImageFunc (DisparityMap.h:963-995) on a plain float image: float accumulators in the reference's order, loops
// from -k/2 to k/2 (an even size reads k + 1 samples), mean = sum / (kw kh), result = sum of squares / (kw kh - 1)
__global__ __launch_bounds__(OF_THREADS) void of_std_dev_kernel(of_sd_args a) {
  extern __shared__ float of_sd_tile[];
  const int hx = a.kw / 2, hy = a.kh / 2;
  const int pw = OF_TX + 2 * hx, ph = OF_TY + 2 * hy;
  const int x0 = (int)blockIdx.x * OF_TX, y0 = (int)blockIdx.y * OF_TY;
  for (int o = threadIdx.x; o < pw * ph; o += OF_THREADS) {
    const int c = x0 - hx + o % pw, r = y0 - hy + o / pw;
    const bool inside = c >= 0 && r >= 0 && c < a.w && r < a.h;
    float v = 0.0f;
    if (inside || !a.zero_edge) v = a.img[(long long)min(max(r, 0), a.h - 1) * a.stride + min(max(c, 0), a.w - 1)];
    of_sd_tile[o] = v;
  }
  __syncthreads();
  const int tx = threadIdx.x % OF_TX, ty = threadIdx.x / OF_TX;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= a.w || y >= a.h) return;
  const float* win = of_sd_tile + ty * pw + tx;
  float sum = 0.0f;
  for (int rr = 0; rr <= 2 * hy; ++rr)
    for (int cc = 0; cc <= 2 * hx; ++cc) sum = __fadd_rn(sum, win[rr * pw + cc]);
  const float mean = __fdiv_rn(sum, (float)(a.kw * a.kh));
  sum = 0.0f;
  for (int rr = 0; rr <= 2 * hy; ++rr)
    for (int cc = 0; cc <= 2 * hx; ++cc) {
      const float diff = __fsub_rn(win[rr * pw + cc], mean);
      sum = __fadd_rn(sum, __fmul_rn(diff, diff));
    }
  a.out[(long long)y * a.ostride + x] = __fdiv_rn(sum, (float)(a.kw * a.kh - 1));
}

// ---- host side ---------------------------------------------------------------------------------------------------

const char* of_name(int method, int cleanup) {
  if (method == VWGPU_OUTLIER_MEAN) return cleanup ? "disparity_cleanup_using_mean" : "rm_outliers_using_mean";
  if (method == VWGPU_OUTLIER_STDDEV) return cleanup ? "disparity_cleanup_using_stddev" : "rm_outliers_using_stddev";
  return cleanup ? "disparity_clean_using_plane" : "rm_outliers_using_plane";
}

int of_check(vwgpu_ctx* ctx, int method, int type, const void* in, int w, int h, ptrdiff_t& istride, int half_h, int half_v,
             double p0, double p1, int semantics, const void* out, ptrdiff_t& ostride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (method != VWGPU_OUTLIER_MEAN && method != VWGPU_OUTLIER_STDDEV && method != VWGPU_OUTLIER_PLANE)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "rm_outliers: unknown method %d", method);
  const char* name = of_name(method, 0);
  if (type != VWGPU_DISPARITY_I32 && type != VWGPU_DISPARITY_F32)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: disparity type %d is neither int32 nor float", name, type);
  if (!in || !out || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: empty image or null pointer", name);
  if (in == out) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: input and output must be different images", name);
  if (semantics != VWGPU_OUTLIER_REFERENCE && semantics != VWGPU_OUTLIER_SKIP)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: semantics %d is neither reference nor skip", name, semantics);
  if (half_h <= 0 || half_v <= 0)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: half kernel sizes must be non-zero.",
                      method == VWGPU_OUTLIER_MEAN ? "RmOutliersUsingMeanFunc" : "RmOutliersFunc");
  if (half_h > OF_MAX_HALF || half_v > OF_MAX_HALF)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: half kernel sizes %d, %d are larger than %d", name, half_h, half_v, OF_MAX_HALF);
  if (std::isnan(p0) || (method != VWGPU_OUTLIER_MEAN && std::isnan(p1)))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: a threshold is NaN", name);
  if (istride == 0) istride = w;
  if (ostride == 0) ostride = w;
  if (istride < w || ostride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
  return VWGPU_OK;
}

template <int METHOD>
void of_launch(vwgpu_ctx* ctx, int type, const of_args& a) {
  const int pw = OF_TX + 2 * a.hh, ph = OF_TY + 2 * a.hv;
  const size_t lds = (size_t)pw * ph * (METHOD == VWGPU_OUTLIER_MEAN ? 16 : 12);
  const dim3 grid((unsigned)((a.ow + OF_TX - 1) / OF_TX), (unsigned)((a.oh + OF_TY - 1) / OF_TY));
  if (type == VWGPU_DISPARITY_I32)
    hipLaunchKernelGGL((of_kernel<METHOD, VWGPU_DISPARITY_I32>), grid, dim3(OF_THREADS), lds, ctx->stream, a);
  else
    hipLaunchKernelGGL((of_kernel<METHOD, VWGPU_DISPARITY_F32>), grid, dim3(OF_THREADS), lds, ctx->stream, a);
}

// device images, arguments checked
int of_run(vwgpu_ctx* ctx, int method, int type, const uint32_t* d_in, int w, int h, ptrdiff_t istride, int half_h, int half_v,
           double p0, double p1, int cleanup, int semantics, uint32_t* d_out, ptrdiff_t ostride, long long* stats) {
  if (stats) stats[0] = stats[1] = 0;
  const size_t pad_bytes = cleanup ? vwgpu_align_up((size_t)(w + 2) * (size_t)(h + 2) * 12, 256) : 0;
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, 256 + pad_bytes);
  if (rc) return rc;
  char* base = static_cast<char*>(ctx->scratch.base);
  unsigned long long* d_counters = reinterpret_cast<unsigned long long*>(base);
  uint32_t* d_pad = reinterpret_cast<uint32_t*>(base + 256);
  VWGPU_HIP(ctx, hipMemsetAsync(d_counters, 0, 256, ctx->stream));
  of_args a{};
  a.in = d_in; a.istride = istride; a.w = w; a.h = h;
  a.hh = half_h; a.hv = half_v;
  a.p0 = method == VWGPU_OUTLIER_MEAN ? p0 * p0 : p0;   // m_max_mean_diffSq (DisparityMap.h:466)
  a.p1 = p1;
  a.skip = semantics == VWGPU_OUTLIER_SKIP;
  a.counter = d_counters;
  if (cleanup) {
    a.out = d_pad; a.ostride = (long long)w + 2; a.ox = a.oy = -1; a.ow = w + 2; a.oh = h + 2;
  } else {
    a.out = d_out; a.ostride = ostride; a.ox = a.oy = 0; a.ow = w; a.oh = h;
  }
  {
    vwgpu_prof_scope ps(ctx, of_name(method, 0));
    if (method == VWGPU_OUTLIER_MEAN) of_launch<VWGPU_OUTLIER_MEAN>(ctx, type, a);
    else if (method == VWGPU_OUTLIER_STDDEV) of_launch<VWGPU_OUTLIER_STDDEV>(ctx, type, a);
    else of_launch<VWGPU_OUTLIER_PLANE>(ctx, type, a);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (cleanup) {
    vwgpu_prof_scope ps(ctx, "outlier_cleanup_thresh");
    const dim3 grid((unsigned)((w + OF_TX - 1) / OF_TX), (unsigned)((h + OF_TY - 1) / OF_TY));
    if (type == VWGPU_DISPARITY_I32)
      hipLaunchKernelGGL((of_thresh_kernel<VWGPU_DISPARITY_I32>), grid, dim3(OF_THREADS), 0, ctx->stream, d_pad, w, h, 3.0, 0.2,
                         d_out, (long long)ostride, d_counters + 1);
    else
      hipLaunchKernelGGL((of_thresh_kernel<VWGPU_DISPARITY_F32>), grid, dim3(OF_THREADS), 0, ctx->stream, d_pad, w, h, 3.0, 0.2,
                         d_out, (long long)ostride, d_counters + 1);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (stats) {
    unsigned long long cnt[2] = {0, 0};
    VWGPU_HIP(ctx, hipMemcpyAsync(cnt, d_counters, 16, hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    stats[0] = (long long)cnt[0];
    stats[1] = (long long)cnt[1];
  }
  return VWGPU_OK;
}

int sd_check(vwgpu_ctx* ctx, const void* img, int w, int h, ptrdiff_t& stride, int kw, int kh, int edge, const void* out,
             ptrdiff_t& ostride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!img || !out || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "std_dev_image: empty image or null pointer");
  if (img == out) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "std_dev_image: input and output must be different images");
  if (kw <= 0 || kh <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "StdDevImageFunc: kernel sizes must be non-zero.");
  if (kw > OF_MAX_STDDEV || kh > OF_MAX_STDDEV)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "std_dev_image: kernel size %d x %d is larger than %d", kw, kh, OF_MAX_STDDEV);
  if (edge != VWGPU_EDGE_ZERO && edge != VWGPU_EDGE_CONSTANT)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "std_dev_image: edge extension %d is neither constant nor zero", edge);
  if (stride == 0) stride = w;
  if (ostride == 0) ostride = w;
  if (stride < w || ostride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "std_dev_image: row stride smaller than row width");
  return VWGPU_OK;
}

int sd_run(vwgpu_ctx* ctx, const float* d_img, int w, int h, ptrdiff_t stride, int kw, int kh, int edge, float* d_out,
           ptrdiff_t ostride) {
  of_sd_args a{d_img, (long long)stride, w, h, d_out, (long long)ostride, kw, kh, edge == VWGPU_EDGE_ZERO ? 1 : 0};
  vwgpu_prof_scope ps(ctx, "std_dev_image");
  const size_t lds = (size_t)(OF_TX + 2 * (kw / 2)) * (OF_TY + 2 * (kh / 2)) * 4;
  const dim3 grid((unsigned)((w + OF_TX - 1) / OF_TX), (unsigned)((h + OF_TY - 1) / OF_TY));
  hipLaunchKernelGGL(of_std_dev_kernel, grid, dim3(OF_THREADS), lds, ctx->stream, a);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------

extern "C" {

int vwgpu_rm_outliers_dev(vwgpu_ctx* ctx, int method, int type, const void* d_in, int w, int h, ptrdiff_t istride, int half_h,
                          int half_v, double p0, double p1, int cleanup, int semantics, void* d_out, ptrdiff_t ostride,
                          long long* stats) {
  int rc = of_check(ctx, method, type, d_in, w, h, istride, half_h, half_v, p0, p1, semantics, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return of_run(ctx, method, type, static_cast<const uint32_t*>(d_in), w, h, istride, half_h, half_v, p0, p1, cleanup, semantics,
                static_cast<uint32_t*>(d_out), ostride, stats);
}

int vwgpu_rm_outliers(vwgpu_ctx* ctx, int method, int type, const void* in, int w, int h, ptrdiff_t istride, int half_h,
                      int half_v, double p0, double p1, int cleanup, int semantics, void* out, ptrdiff_t ostride,
                      long long* stats) {
  int rc = of_check(ctx, method, type, in, w, h, istride, half_h, half_v, p0, p1, semantics, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 12, istride, VWGPU_STAGE_IN), po = st.add(out, w, h, 12, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = of_run(ctx, method, type, st.dev<uint32_t>(pi), w, h, w, half_h, half_v, p0, p1, cleanup, semantics, st.dev<uint32_t>(po), w,
              stats);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_std_dev_image_dev(vwgpu_ctx* ctx, const float* d_image, int w, int h, ptrdiff_t stride, int kernel_width,
                            int kernel_height, int edge, float* d_out, ptrdiff_t ostride) {
  int rc = sd_check(ctx, d_image, w, h, stride, kernel_width, kernel_height, edge, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return sd_run(ctx, d_image, w, h, stride, kernel_width, kernel_height, edge, d_out, ostride);
}

int vwgpu_std_dev_image(vwgpu_ctx* ctx, const float* image, int w, int h, ptrdiff_t stride, int kernel_width, int kernel_height,
                        int edge, float* out, ptrdiff_t ostride) {
  int rc = sd_check(ctx, image, w, h, stride, kernel_width, kernel_height, edge, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(image, w, h, 4, stride, VWGPU_STAGE_IN), po = st.add(out, w, h, 4, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = sd_run(ctx, st.dev<float>(pi), w, h, w, kernel_width, kernel_height, edge, st.dev<float>(po), w);
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
