// affine_subpixel.hip — pyramid sub-pixel refinement: vw::stereo::PyramidSubpixelView::prerasterize
// (src/vw/Stereo/SubpixelView.cc:33-224) with SUBPIXEL_FAST_AFFINE (subpixel_optimized_affine_2d,
// src/vw/Stereo/Correlate.cc:848-1200), SUBPIXEL_LUCAS_KANADE (subpixel_optimized_LK_2d, :1203-1391) and SUBPIXEL_BAYES_EM
// (subpixel_optimized_affine_2d_EM, :500-845), tile by tile, bit-identical to the reference's sequential order.  The
// algorithms share everything but the refinement kernel launched in the fixpoint loop.
//
// Per call: one kernel reduces the disparity range of every tile, one readback sizes the tile patches.  Per tile:
// prefiltered crops (the prefilter of the edge-extended image, as vwgpu_parabola_subpixel), the zero-extended
// disparity patch minus the range minimum, the subsample chain of images and disparities, derivative images, then
// coarse to fine: the refinement fixpoint on the level's ROI plus a 1-pixel ring, the upsample-crop to the next level,
// and the final write of the tile's box.
//
// The reference updates the disparity map in place, in raster order: a pixel it invalidates is missing from the
// weight window (adjust_weight_image, Correlate.cc:1393-1440) of every later pixel.  the refinement kernel evaluates
// the pixels of one level in parallel, each with the window validity "earlier pixels as of the previous round, the
// pixel itself and later pixels as on entry"; a round re-evaluates only pixels whose causal window (rows above, and
// the same row to the left) holds a pixel whose state changed in the previous round, and the rounds stop when none
// changes.  The dependency graph is acyclic (raster order), so that fixpoint is the sequential result.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "em_exp.h"
#include "vwgpu_internal.h"

namespace {

constexpr int AFF_BX = 16, AFF_BY = 16;

// ---- per-tile disparity range (get_disparity_range, DisparityMap.h:48-66) ---------------------------------------------
// PixelAccumulator<EWMinMaxAccumulator> takes the VALID pixels only (Image/Statistics.h:283-290): what an invalid pixel
// stores never reaches the range.  A tile without a valid pixel leaves its keys at the initial values (range 0, 0, 0, 0).

__device__ inline int aff_float_key(float f) {   // order-preserving float -> int map for atomicMin / atomicMax
  const int b = __float_as_int(f);
  return b >= 0 ? b : b ^ 0x7fffffff;
}

__global__ void __launch_bounds__(256)
affine_range_kernel(const float* __restrict__ d, ptrdiff_t stride_px, const int* __restrict__ tiles, int* __restrict__ keys, int t0) {
  const int t = t0 + blockIdx.y;
  const int bx = tiles[4 * t], by = tiles[4 * t + 1], bw = tiles[4 * t + 2], bh = tiles[4 * t + 3];
  int mnx = INT_MAX, mny = INT_MAX, mxx = INT_MIN, mxy = INT_MIN;
  const long long n = (long long)bw * bh;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int y = by + (int)(i / bw), x = bx + (int)(i % bw);
    const float* q = d + ((ptrdiff_t)y * stride_px + x) * 3;
    if (q[2] == 0.0f) continue;
    const int kx = aff_float_key(q[0]), ky = aff_float_key(q[1]);
    mnx = min(mnx, kx); mxx = max(mxx, kx);
    mny = min(mny, ky); mxy = max(mxy, ky);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mnx = min(mnx, __shfl_xor(mnx, o)); mxx = max(mxx, __shfl_xor(mxx, o));
    mny = min(mny, __shfl_xor(mny, o)); mxy = max(mxy, __shfl_xor(mxy, o));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(keys + 4 * t, mnx); atomicMin(keys + 4 * t + 1, mny);
    atomicMax(keys + 4 * t + 2, mxx); atomicMax(keys + 4 * t + 3, mxy);
  }
}

__global__ void affine_range_init_kernel(int* keys, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = (i & 3) < 2 ? INT_MAX : INT_MIN;
}

// ---- patches -----------------------------------------------------------------------------------------------------

// crop(edge_extend(disparity, ZeroEdgeExtension()), left_crop_bbox) - range.min (SubpixelView.cc:88-95)
__global__ void affine_disp_patch_kernel(const float* __restrict__ d, int w, int h, ptrdiff_t stride_px, int x0, int y0,
                                         int pw, int ph, float sminx, float sminy,
                                         float* __restrict__ dx, float* __restrict__ dy, uint8_t* __restrict__ v) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= pw || y >= ph) return;
  const int sx = x0 + x, sy = y0 + y;
  float vx = 0.f, vy = 0.f;
  uint8_t vv = 0;
  if (sx >= 0 && sy >= 0 && sx < w && sy < h) {
    const float* q = d + ((ptrdiff_t)sy * stride_px + sx) * 3;
    vx = q[0]; vy = q[1]; vv = q[2] != 0.0f;
  }
  const size_t o = (size_t)y * pw + x;
  dx[o] = vx - sminx;
  dy[o] = vy - sminy;
  v[o] = vv;
}

// subsample(img, 2) (Manipulation.h:214-293), no smoothing
__global__ void affine_subsample_kernel(const float* __restrict__ s, int sw, float* __restrict__ d, int dw, int dh) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= dw || y >= dh) return;
  d[(size_t)y * dw + x] = s[(size_t)(2 * y) * sw + 2 * x];
}

// disparity_subsample (DisparityMap.h:1253-1324), ConstantEdgeExtension child, double accumulator; the first three
// terms convert the pixel to double before the product, the other six multiply in float.
__global__ void affine_disp_subsample_kernel(const float* __restrict__ sx_, const float* __restrict__ sy_, const uint8_t* __restrict__ sv,
                                             int sw, int sh, float* __restrict__ dx, float* __restrict__ dy, uint8_t* __restrict__ dv,
                                             int dw, int dh) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= dw || j >= dh) return;
  const int ci = i << 1, cj = j << 1;
  double bx = 0, by = 0, count = 0;
  const int ox[9] = {0, 1, 0, -1, 0, 1, -1, -1, 1}, oy[9] = {0, 0, 1, 0, -1, 1, -1, 1, -1}, wt[9] = {10, 5, 5, 5, 5, 2, 2, 2, 2};
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int x = min(max(ci + ox[k], 0), sw - 1), y = min(max(cj + oy[k], 0), sh - 1);
    const size_t q = (size_t)y * sw + x;
    if (!sv[q]) continue;
    count += wt[k];
    if (k < 3) {
      bx += wt[k] * (double)sx_[q];
      by += wt[k] * (double)sy_[q];
    } else {
      bx += (double)__fmul_rn((float)wt[k], sx_[q]);
      by += (double)__fmul_rn((float)wt[k], sy_[q]);
    }
  }
  const size_t o = (size_t)j * dw + i;
  if (count > 0) {
    dx[o] = (float)__ddiv_rn(bx, count * 2);
    dy[o] = (float)__ddiv_rn(by, count * 2);
    dv[o] = 1;
  } else {
    dx[o] = 0.f; dy[o] = 0.f; dv[o] = 0;
  }
}

// crop(disparity_upsample(edge_extend(d)), BBox2i(0, 0, W, H)) (SubpixelView.cc:183-189, DisparityMap.h:1326-1358)
__global__ void affine_upsample_kernel(const float* __restrict__ sx_, const float* __restrict__ sy_, const uint8_t* __restrict__ sv,
                                       int sw, int sh, float* __restrict__ dx, float* __restrict__ dy, uint8_t* __restrict__ dv,
                                       int dw, int dh) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= dw || y >= dh) return;
  const int cx = min(x >> 1, sw - 1), cy = min(y >> 1, sh - 1);
  const size_t q = (size_t)cy * sw + cx, o = (size_t)y * dw + x;
  dx[o] = sx_[q] * 2.0f;
  dy[o] = sy_[q] * 2.0f;
  dv[o] = sv[q];
}

// derivative_filter(img, 1, 0) and (img, 0, 1) (Filter.h:275-308): kernel {0.5, 0, -0.5}, ConstantEdgeExtension on the
// patch; correlate_1d_at_point sums k[2] * s(-1) + k[1] * s(0) + k[0] * s(+1) from 0 in float (Convolution.h:53-65).
__global__ void affine_deriv_kernel(const float* __restrict__ s, int w, int h, float* __restrict__ ix, float* __restrict__ iy) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  const float c = s[(size_t)y * w + x];
  {
    const float a = s[(size_t)y * w + max(x - 1, 0)], b = s[(size_t)y * w + min(x + 1, w - 1)];
    float r = 0.0f;
    r = __fadd_rn(r, __fmul_rn(-0.5f, a));
    r = __fadd_rn(r, __fmul_rn(0.0f, c));
    r = __fadd_rn(r, __fmul_rn(0.5f, b));
    ix[(size_t)y * w + x] = r;
  }
  {
    const float a = s[(size_t)max(y - 1, 0) * w + x], b = s[(size_t)min(y + 1, h - 1) * w + x];
    float r = 0.0f;
    r = __fadd_rn(r, __fmul_rn(-0.5f, a));
    r = __fadd_rn(r, __fmul_rn(0.0f, c));
    r = __fadd_rn(r, __fmul_rn(0.5f, b));
    iy[(size_t)y * w + x] = r;
  }
}

// ---- the 6 x 6 solve: LAPACK reference SPOSV('L') = SPOTRF2 (recursive) + SPOTRS, float, in registers -------------
// A(i, j) = a[i * 6 + j], i >= j.  Template recursion keeps every index a compile-time constant (no scratch).

// Correctly rounded float sqrt (SPOTRF2's SQRT).  The compiler lowers sqrtf / __fsqrt_rn to v_sqrt_f32 (1 ulp) here, so
// the square root of the nearest float is corrected with exact double arithmetic: a float sqrt never lies on a midpoint,
// and a midpoint of two floats has 25 significant bits, so its square is exact in double.
__device__ inline float aff_sqrt_rn(float x) {
  float r = (float)__dsqrt_rn((double)x);
  const float up = nextafterf(r, INFINITY), dn = nextafterf(r, 0.0f);
  const double mu = ((double)r + (double)up) * 0.5, md = ((double)r + (double)dn) * 0.5;
  if (mu * mu < (double)x) r = up;
  else if (md * md > (double)x) r = dn;
  return r;
}

template <int O, int N>
struct aff_potrf2 {
  __device__ static inline int run(float* a) {
    constexpr int N1 = N / 2, N2 = N - N1;
    int info = aff_potrf2<O, N1>::run(a);
    if (info) return info;
#pragma unroll
    for (int k = 0; k < N1; ++k) {                                   // STRSM('R', 'L', 'T', 'N', N2, N1, 1, A11, A21)
      const float t = __fdiv_rn(1.0f, a[(O + k) * 6 + O + k]);
#pragma unroll
      for (int i = 0; i < N2; ++i) a[(O + N1 + i) * 6 + O + k] = __fmul_rn(t, a[(O + N1 + i) * 6 + O + k]);
#pragma unroll
      for (int j = k + 1; j < N1; ++j)
        if (a[(O + j) * 6 + O + k] != 0.0f) {
          const float t2 = a[(O + j) * 6 + O + k];
#pragma unroll
          for (int i = 0; i < N2; ++i)
            a[(O + N1 + i) * 6 + O + j] = __fsub_rn(a[(O + N1 + i) * 6 + O + j], __fmul_rn(t2, a[(O + N1 + i) * 6 + O + k]));
        }
    }
#pragma unroll
    for (int j = 0; j < N2; ++j)                                     // SSYRK('L', 'N', N2, N1, -1, A21, 1, A22)
#pragma unroll
      for (int l = 0; l < N1; ++l)
        if (a[(O + N1 + j) * 6 + O + l] != 0.0f) {
          const float t = -a[(O + N1 + j) * 6 + O + l];
#pragma unroll
          for (int i = j; i < N2; ++i)
            a[(O + N1 + i) * 6 + O + N1 + j] = __fadd_rn(a[(O + N1 + i) * 6 + O + N1 + j], __fmul_rn(t, a[(O + N1 + i) * 6 + O + l]));
        }
    info = aff_potrf2<O + N1, N2>::run(a);
    return info ? info + N1 : 0;
  }
};
template <int O>
struct aff_potrf2<O, 1> {
  __device__ static inline int run(float* a) {
    const float v = a[O * 6 + O];
    if (!(v > 0.0f)) return 1;                                       // A(1,1) <= 0 or NaN: info > 0
    a[O * 6 + O] = aff_sqrt_rn(v);
    return 0;
  }
};

__device__ inline void aff_posv6(float* a, float* b) {               // b untouched when the factorisation fails
  if (aff_potrf2<0, 6>::run(a)) return;
#pragma unroll
  for (int k = 0; k < 6; ++k)                                        // STRSM('L', 'L', 'N', 'N')
    if (b[k] != 0.0f) {
      b[k] = __fdiv_rn(b[k], a[k * 6 + k]);
#pragma unroll
      for (int i = k + 1; i < 6; ++i) b[i] = __fsub_rn(b[i], __fmul_rn(b[k], a[i * 6 + k]));
    }
#pragma unroll
  for (int i = 5; i >= 0; --i) {                                     // STRSM('L', 'L', 'T', 'N')
    float t = b[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) t = __fsub_rn(t, __fmul_rn(a[k * 6 + i], b[k]));
    b[i] = __fdiv_rn(t, a[i * 6 + i]);
  }
}

// norm_2 (Vector.h:1593-1604): float squares summed in double, the sum stored as float, sqrt in double
__device__ inline double aff_norm2_2(float a, float b) {
  double r = 0.0;
  r = __dadd_rn(r, (double)__fmul_rn(a, a));
  r = __dadd_rn(r, (double)__fmul_rn(b, b));
  return __dsqrt_rn((double)(float)r);
}

// BilinearInterpolation over ZeroEdgeExtension (Interpolation.h:76-106), with the integer-pixel shortcut
__device__ inline float aff_zero(const float* __restrict__ r, int w, int h, int x, int y) {
  return (x < 0 || y < 0 || x >= w || y >= h) ? 0.0f : r[(size_t)y * w + x];
}
__device__ inline float aff_bilinear(const float* __restrict__ r, int w, int h, float xx, float yy) {
  const float fx = floorf(xx), fy = floorf(yy);
  const int x = (int)fx, y = (int)fy;
  if (fx == xx && fy == yy) return aff_zero(r, w, h, x, y);
  const float nx = __fsub_rn(xx, (float)x), ny = __fsub_rn(yy, (float)y);
  const float n1mx = __fsub_rn(1.0f, nx), n1my = __fsub_rn(1.0f, ny);
  float res = __fmul_rn(aff_zero(r, w, h, x, y), n1mx);
  res = __fadd_rn(res, __fmul_rn(aff_zero(r, w, h, x + 1, y), nx));
  res = __fmul_rn(res, n1my);
  float row = __fmul_rn(aff_zero(r, w, h, x, y + 1), n1mx);
  row = __fadd_rn(row, __fmul_rn(aff_zero(r, w, h, x + 1, y + 1), nx));
  return __fadd_rn(res, __fmul_rn(row, ny));
}

struct aff_level_args {
  const float *L, *R, *Ix, *Iy, *tmpl;
  const float *dx, *dy;        // the map on entry to the level
  const uint8_t* v0;           // validity on entry
  const uint8_t* sprev;        // state after the previous round (= v0 outside the ROI)
  const uint8_t* cprev;        // changed in the previous round
  uint8_t *scur, *ccur;
  float *rdx, *rdy;            // refined values of the pixels evaluated
  int* changes;                // number of state changes of this round
  unsigned long long* iters;   // optional: window-loop iterations run
  int w, h, kx, ky, x0, y0, x1, y1, round;
};

// One lane per pixel of the level's ROI plus the 1-pixel ring (Correlate.cc:898-905 loop bounds).
__global__ void __launch_bounds__(AFF_BX * AFF_BY)
affine_refine_kernel(aff_level_args a) {
  const int x = a.x0 + blockIdx.x * AFF_BX + threadIdx.x, y = a.y0 + blockIdx.y * AFF_BY + threadIdx.y;
  if (x >= a.x1 || y >= a.y1) return;
  const int w = a.w;
  const size_t p = (size_t)y * w + x;
  if (!a.v0[p]) return;                                              // skipped by the reference, never changes
  const int khw = a.kx / 2, khh = a.ky / 2;
  if (a.round > 0) {                                                 // dirty: a state in the causal window changed last round
    bool dirty = false;
    for (int jj = -khh; jj <= 0 && !dirty; ++jj) {
      const int iend = jj < 0 ? khw : -1;
      const uint8_t* c = a.cprev + (size_t)(y + jj) * w + x;
      for (int ii = -khw; ii <= iend; ++ii)
        if (c[ii]) { dirty = true; break; }
    }
    if (!dirty) {
      a.scur[p] = a.sprev[p];
      a.ccur[p] = 0;
      return;
    }
  }
  // adjust_weight_image (Correlate.cc:1393-1440): earlier pixels with their current state, the rest as on entry
  float sum = 0.0f;
  int good = 0;
  for (int jj = -khh; jj <= khh; ++jj) {
    const size_t r = (size_t)(y + jj) * w + x;
    for (int ii = -khw; ii <= khw; ++ii) {
      const bool earlier = jj < 0 || (jj == 0 && ii < 0);
      if (earlier ? a.sprev[r + ii] : a.v0[r + ii]) {
        sum = __fadd_rn(sum, a.tmpl[(jj + khh) * a.kx + ii + khw]);
        ++good;
      }
    }
  }
  uint8_t ns = 1;
  float d0 = 1.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f, d4 = 1.0f, d5 = 0.0f;
  unsigned iters = 0;
  if (good < (a.kx * a.ky) / 2) {
    ns = 0;
  } else {
    const float max_translation = (float)(a.kx / 2);
    const float x_base = __fadd_rn((float)x, a.dx[p]), y_base = __fadd_rn((float)y, a.dy[p]);
    const int kqw = khw / 2, kqh = khh / 2;
    // The reference reads the weight through w_ptr = w_row = w.origin() and never advances either accessor
    // (Correlate.cc:1002-1046): every window pixel gets w(0, 0) = the top-left pixel's weight after adjust_weight_image
    // (its template weight / sum if that pixel is valid, else 0 / sum).  The top-left pixel precedes the centre unless
    // the window is 1 x 1.
    const bool tl_valid = (khh > 0 || khw > 0) ? a.sprev[(size_t)(y - khh) * w + x - khw] : a.v0[p];
    const float wt = tl_valid ? __fdiv_rn(a.tmpl[0], sum) : __fdiv_rn(0.0f, sum);
    for (unsigned iter = 0; iter < 10; ++iter) {
      if (aff_norm2_2(d2, d5) > (double)max_translation) break;
      ++iters;
      float rhs[36];
      float lhs[6];
#pragma unroll
      for (int k = 0; k < 36; ++k) rhs[k] = 0.0f;
#pragma unroll
      for (int k = 0; k < 6; ++k) lhs[k] = 0.0f;
      for (int jj = -khh; jj <= khh; ++jj) {
        const float fj = (float)jj;
        const float xx_partial = __fadd_rn(__fadd_rn(x_base, __fmul_rn(d1, fj)), d2);
        const float yy_partial = __fadd_rn(__fadd_rn(y_base, __fmul_rn(d4, fj)), d5);
        const size_t r = (size_t)(y + jj) * w + x;
        for (int ii = -khw; ii <= khw; ++ii) {
          const float fi = (float)ii;
          const float xx = __fadd_rn(__fmul_rn(d0, fi), xx_partial);
          const float yy = __fadd_rn(__fmul_rn(d3, fi), yy_partial);
          const float I_e = __fsub_rn(aff_bilinear(a.R, w, a.h, xx, yy), a.L[r + ii]);
          const float ix = a.Ix[r + ii], iy = a.Iy[r + ii];
          const float Ixv = __fmul_rn(wt, ix), Iyv = __fmul_rn(wt, iy);
          const float Ixx = __fmul_rn(Ixv, ix), Iyy = __fmul_rn(Iyv, iy), Ixy = __fmul_rn(Ixv, iy);
          const float IxIe = __fmul_rn(Ixv, I_e), IyIe = __fmul_rn(Iyv, I_e);
          lhs[0] = __fsub_rn(lhs[0], __fmul_rn(fi, IxIe));
          lhs[1] = __fsub_rn(lhs[1], __fmul_rn(fj, IxIe));
          lhs[2] = __fsub_rn(lhs[2], IxIe);
          lhs[3] = __fsub_rn(lhs[3], __fmul_rn(fi, IyIe));
          lhs[4] = __fsub_rn(lhs[4], __fmul_rn(fj, IyIe));
          lhs[5] = __fsub_rn(lhs[5], IyIe);
          const float m0 = (float)(ii * ii), m1 = (float)(ii * jj), m2 = (float)(jj * jj);
          rhs[0] = __fadd_rn(rhs[0], __fmul_rn(m0, Ixx));
          rhs[1] = __fadd_rn(rhs[1], __fmul_rn(m1, Ixx));
          rhs[2] = __fadd_rn(rhs[2], __fmul_rn(fi, Ixx));
          rhs[7] = __fadd_rn(rhs[7], __fmul_rn(m2, Ixx));
          rhs[8] = __fadd_rn(rhs[8], __fmul_rn(fj, Ixx));
          rhs[14] = __fadd_rn(rhs[14], Ixx);
          rhs[3] = __fadd_rn(rhs[3], __fmul_rn(m0, Ixy));
          rhs[4] = __fadd_rn(rhs[4], __fmul_rn(m1, Ixy));
          rhs[5] = __fadd_rn(rhs[5], __fmul_rn(fi, Ixy));
          rhs[10] = __fadd_rn(rhs[10], __fmul_rn(m2, Ixy));
          rhs[11] = __fadd_rn(rhs[11], __fmul_rn(fj, Ixy));
          rhs[17] = __fadd_rn(rhs[17], Ixy);
          rhs[21] = __fadd_rn(rhs[21], __fmul_rn(m0, Iyy));
          rhs[22] = __fadd_rn(rhs[22], __fmul_rn(m1, Iyy));
          rhs[23] = __fadd_rn(rhs[23], __fmul_rn(fi, Iyy));
          rhs[28] = __fadd_rn(rhs[28], __fmul_rn(m2, Iyy));
          rhs[29] = __fadd_rn(rhs[29], __fmul_rn(fj, Iyy));
          rhs[35] = __fadd_rn(rhs[35], Iyy);
        }
      }
      // symmetric fill (Correlate.cc:1133-1145); the solve reads the lower triangle only
      rhs[9] = rhs[4]; rhs[15] = rhs[5]; rhs[16] = rhs[11];
#pragma unroll
      for (int r = 1; r < 6; ++r)
#pragma unroll
        for (int c = 0; c < r; ++c) rhs[r * 6 + c] = rhs[c * 6 + r];
      aff_posv6(rhs, lhs);
      d0 = __fadd_rn(d0, lhs[0]); d1 = __fadd_rn(d1, lhs[1]); d2 = __fadd_rn(d2, lhs[2]);
      d3 = __fadd_rn(d3, lhs[3]); d4 = __fadd_rn(d4, lhs[4]); d5 = __fadd_rn(d5, lhs[5]);
      const float wl[6] = {__fmul_rn(lhs[0], (float)kqw), __fmul_rn(lhs[1], (float)kqh), lhs[2],
                           __fmul_rn(lhs[3], (float)kqw), __fmul_rn(lhs[4], (float)kqh), lhs[5]};
      double s2 = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) s2 = __dadd_rn(s2, (double)__fmul_rn(wl[k], wl[k]));
      if (__dsqrt_rn((double)(float)s2) < 0.05) break;
    }
    if (aff_norm2_2(d2, d5) > (double)max_translation || isnan(d2) || isnan(d5)) ns = 0;
  }
  a.rdx[p] = __fadd_rn(a.dx[p], d2);
  a.rdy[p] = __fadd_rn(a.dy[p], d5);
  const uint8_t old = a.round > 0 ? a.sprev[p] : a.v0[p];
  a.scur[p] = ns;
  a.ccur[p] = ns != old;
  if (ns != old) atomicAdd(a.changes, 1);
  if (a.iters) atomicAdd(a.iters, (unsigned long long)iters);
}

// ---- SUBPIXEL_LUCAS_KANADE and SUBPIXEL_BAYES_EM: the same launch shape, rounds and commit ---------

// The part before the window loop shared by lk_refine_kernel and em_refine_kernel (as in affine_refine_kernel): the
// dirty test of rounds > 0 and adjust_weight_image.  Returns false when the lane is done.
__device__ inline bool pyr_prologue(const aff_level_args& a, int x, int y, size_t p, float& sum, int& good) {
  if (!a.v0[p]) return false;
  const int w = a.w, khw = a.kx / 2, khh = a.ky / 2;
  if (a.round > 0) {
    bool dirty = false;
    for (int jj = -khh; jj <= 0 && !dirty; ++jj) {
      const int iend = jj < 0 ? khw : -1;
      const uint8_t* c = a.cprev + (size_t)(y + jj) * w + x;
      for (int ii = -khw; ii <= iend; ++ii)
        if (c[ii]) { dirty = true; break; }
    }
    if (!dirty) {
      a.scur[p] = a.sprev[p];
      a.ccur[p] = 0;
      return false;
    }
  }
  sum = 0.0f;
  good = 0;
  for (int jj = -khh; jj <= khh; ++jj) {
    const size_t r = (size_t)(y + jj) * w + x;
    for (int ii = -khw; ii <= khw; ++ii) {
      const bool earlier = jj < 0 || (jj == 0 && ii < 0);
      if (earlier ? a.sprev[r + ii] : a.v0[r + ii]) {
        sum = __fadd_rn(sum, a.tmpl[(jj + khh) * a.kx + ii + khw]);
        ++good;
      }
    }
  }
  return true;
}

// w(0, 0) after adjust_weight_image: the weight every window pixel gets (the accessor is never advanced)
__device__ inline float pyr_top_left_weight(const aff_level_args& a, int x, int y, size_t p, float sum) {
  const int khw = a.kx / 2, khh = a.ky / 2;
  const bool tl_valid = (khh > 0 || khw > 0) ? a.sprev[(size_t)(y - khh) * a.w + x - khw] : a.v0[p];
  return tl_valid ? __fdiv_rn(a.tmpl[0], sum) : __fdiv_rn(0.0f, sum);
}

__device__ inline void pyr_epilogue(const aff_level_args& a, size_t p, uint8_t ns, float ux, float uy, unsigned iters) {
  a.rdx[p] = __fadd_rn(a.dx[p], ux);
  a.rdy[p] = __fadd_rn(a.dy[p], uy);
  const uint8_t old = a.round > 0 ? a.sprev[p] : a.v0[p];
  a.scur[p] = ns;
  a.ccur[p] = ns != old;
  if (ns != old) atomicAdd(a.changes, 1);
  if (a.iters) atomicAdd(a.iters, (unsigned long long)iters);
}

// SPOSV('L', 2, 1) = SPOTRF2 (n1 = n2 = 1) + SPOTRS; b untouched when the factorisation fails
__device__ inline void pyr_posv2(float a00, float a10, float a11, float& b0, float& b1) {
  if (!(a00 > 0.0f)) return;
  a00 = aff_sqrt_rn(a00);
  a10 = __fmul_rn(__fdiv_rn(1.0f, a00), a10);                        // STRSM('R', 'L', 'T', 'N')
  if (a10 != 0.0f) a11 = __fadd_rn(a11, __fmul_rn(-a10, a10));       // SSYRK
  if (!(a11 > 0.0f)) return;
  a11 = aff_sqrt_rn(a11);
  if (b0 != 0.0f) {                                                  // STRSM('L', 'L', 'N', 'N')
    b0 = __fdiv_rn(b0, a00);
    b1 = __fsub_rn(b1, __fmul_rn(b0, a10));
  }
  if (b1 != 0.0f) b1 = __fdiv_rn(b1, a11);
  b1 = __fdiv_rn(b1, a11);                                           // STRSM('L', 'L', 'T', 'N')
  b0 = __fdiv_rn(__fsub_rn(b0, __fmul_rn(a10, b1)), a00);
}

// subpixel_optimized_LK_2d (Correlate.cc:1203-1391): a translation, at most 10 Gauss-Newton steps, a 2 x 2 solve.
__global__ void __launch_bounds__(AFF_BX * AFF_BY)
lk_refine_kernel(aff_level_args a) {
  const int x = a.x0 + blockIdx.x * AFF_BX + threadIdx.x, y = a.y0 + blockIdx.y * AFF_BY + threadIdx.y;
  if (x >= a.x1 || y >= a.y1) return;
  const int w = a.w;
  const size_t p = (size_t)y * w + x;
  float sum;
  int good;
  if (!pyr_prologue(a, x, y, p, sum, good)) return;
  const int khw = a.kx / 2, khh = a.ky / 2;
  uint8_t ns = 1;
  float d0 = 0.0f, d1 = 0.0f;
  unsigned iters = 0;
  if (good < (a.kx * a.ky) / 2) {
    ns = 0;
  } else {
    const float max_translation = (float)(a.kx / 2);
    const float x_base = __fadd_rn((float)x, a.dx[p]), y_base = __fadd_rn((float)y, a.dy[p]);
    const float wt = pyr_top_left_weight(a, x, y, p, sum);          // robust_weight (1) * w(0, 0)
    for (unsigned iter = 0; iter < 10; ++iter) {
      if (aff_norm2_2(d0, d1) > (double)max_translation) break;
      ++iters;
      float r00 = 0.0f, r01 = 0.0f, r11 = 0.0f, l0 = 0.0f, l1 = 0.0f;
      const float xx_partial = __fadd_rn(x_base, d0);
      for (int jj = -khh; jj <= khh; ++jj) {
        const float yy = __fadd_rn(__fadd_rn(y_base, (float)jj), d1);
        const size_t r = (size_t)(y + jj) * w + x;
        for (int ii = -khw; ii <= khw; ++ii) {
          const float xx = __fadd_rn((float)ii, xx_partial);
          const float I_e = __fsub_rn(aff_bilinear(a.R, w, a.h, xx, yy), a.L[r + ii]);
          const float ix = a.Ix[r + ii], iy = a.Iy[r + ii];
          const float Ixv = __fmul_rn(wt, ix), Iyv = __fmul_rn(wt, iy);
          l0 = __fsub_rn(l0, __fmul_rn(Ixv, I_e));
          l1 = __fsub_rn(l1, __fmul_rn(Iyv, I_e));
          r00 = __fadd_rn(r00, __fmul_rn(Ixv, ix));
          r01 = __fadd_rn(r01, __fmul_rn(Ixv, iy));
          r11 = __fadd_rn(r11, __fmul_rn(Iyv, iy));
        }
      }
      pyr_posv2(r00, r01, r11, l0, l1);
      d0 = __fadd_rn(d0, l0);
      d1 = __fadd_rn(d1, l1);
      if (aff_norm2_2(l0, l1) < 0.05) break;
    }
    if (aff_norm2_2(d0, d1) > (double)max_translation || isnan(d0) || isnan(d1)) ns = 0;
  }
  pyr_epilogue(a, p, ns, d0, d1, iters);
}

// subpixel_optimized_affine_2d_EM (Correlate.cc:500-845): up to 10 outer steps of up to 2 EM passes, each a 6 x 6 solve.
// plane_nf / noise_nf are plane_norm_factor / noise_norm_factor (constant: the variances are never updated).
__global__ void __launch_bounds__(AFF_BX * AFF_BY)
em_refine_kernel(aff_level_args a, float plane_nf, float noise_nf) {
  const int x = a.x0 + blockIdx.x * AFF_BX + threadIdx.x, y = a.y0 + blockIdx.y * AFF_BY + threadIdx.y;
  if (x >= a.x1 || y >= a.y1) return;
  const int w = a.w;
  const size_t p = (size_t)y * w + x;
  float sum;
  int good;
  if (!pyr_prologue(a, x, y, p, sum, good)) return;
  const int khw = a.kx / 2, khh = a.ky / 2, kern_pixels = a.kx * a.ky;
  constexpr float two_var2_plane = 2 * 1e-3f, two_var2_noise = 2 * 1e-2f;
  uint8_t ns = 1;
  float d[6] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
  unsigned iters = 0;
  if (good < kern_pixels / 2) {
    ns = 0;
  } else {
    const float max_translation = (float)(a.kx / 2);
    const float x_base = __fadd_rn((float)x, a.dx[p]), y_base = __fadd_rn((float)y, a.dy[p]);
    const float wt = pyr_top_left_weight(a, x, y, p, sum);
    float curr_sum_I_e = 0.0f, prev_sum_I_e = 0.0f;
    for (unsigned iter = 0; iter < 10; ++iter) {
      if (aff_norm2_2(d[2], d[5]) > (double)max_translation) break;
      float lhs[6], prev_lhs[6], d_em[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) { lhs[k] = 0.0f; prev_lhs[k] = 0.0f; d_em[k] = d[k]; }
      float mean_noise = 0.0f, w_plane = 0.8f, w_noise = 0.2f;
      for (unsigned em_iter = 0; em_iter < 2; ++em_iter) {
        ++iters;
        float rhs[36];
#pragma unroll
        for (int k = 0; k < 36; ++k) rhs[k] = 0.0f;
#pragma unroll
        for (int k = 0; k < 6; ++k) lhs[k] = 0.0f;
        float in_curr_sum_I_e = 0.0f, mean_noise_tmp = 0.0f, sum_gamma_noise = 0.0f, sum_gamma_plane = 0.0f;
        int skip = 0;
        for (int jj = -khh; jj <= khh; ++jj) {
          const float fj = (float)jj;
          const float xx_partial = __fadd_rn(__fadd_rn(x_base, __fmul_rn(d[1], fj)), d[2]);
          const float yy_partial = __fadd_rn(__fadd_rn(y_base, __fmul_rn(d[4], fj)), d[5]);
          const float delta_x_partial = __fadd_rn(__fmul_rn(d_em[1], fj), d_em[2]);
          const float delta_y_partial = __fadd_rn(__fmul_rn(d_em[4], fj), d_em[5]);
          const size_t r = (size_t)(y + jj) * w + x;
          for (int ii = -khw; ii <= khw; ++ii) {
            const float fi = (float)ii;
            const float xx = __fadd_rn(__fmul_rn(d[0], fi), xx_partial);
            const float yy = __fadd_rn(__fmul_rn(d[3], fi), yy_partial);
            const float delta_x = __fadd_rn(__fmul_rn(d_em[0], fi), delta_x_partial);
            const float delta_y = __fadd_rn(__fmul_rn(d_em[3], fi), delta_y_partial);
            const float px = aff_bilinear(a.R, w, a.h, xx, yy);
            const float I_e = __fsub_rn(px, a.L[r + ii]);
            in_curr_sum_I_e = __fadd_rn(in_curr_sum_I_e, I_e);
            const float ix = a.Ix[r + ii], iy = a.Iy[r + ii];
            const float temp_plane = __fsub_rn(__fsub_rn(I_e, __fmul_rn(delta_x, ix)), __fmul_rn(delta_y, iy));
            const float temp_noise = __fsub_rn(px, mean_noise);
            const float plane_e = __fdiv_rn(-__fmul_rn(temp_plane, temp_plane), two_var2_plane);
            const float plane_prob = plane_e < -75.0f ? 0.0f : em_scaled_exp(plane_nf, plane_e);
            const float noise_e = __fdiv_rn(-__fmul_rn(temp_noise, temp_noise), two_var2_noise);
            const float noise_prob = noise_e < -75.0f ? 0.0f : em_scaled_exp(noise_nf, noise_e);
            const float pw = __fmul_rn(plane_prob, w_plane), nw = __fmul_rn(noise_prob, w_noise);
            const float psum = __fadd_rn(pw, nw);
            const float gamma_plane = __fdiv_rn(pw, psum), gamma_noise = __fdiv_rn(nw, psum);
            mean_noise_tmp = __fadd_rn(mean_noise_tmp, __fmul_rn(px, gamma_noise));
            sum_gamma_plane = __fadd_rn(sum_gamma_plane, gamma_plane);
            sum_gamma_noise = __fadd_rn(sum_gamma_noise, gamma_noise);
            const float weight = __fmul_rn(gamma_plane, wt);
            if ((double)weight < 1e-26) {                            // NaN is not: it enters the sums
              ++skip;
              continue;
            }
            const float Ixv = __fmul_rn(weight, ix), Iyv = __fmul_rn(weight, iy);
            const float Ixx = __fmul_rn(Ixv, ix), Iyy = __fmul_rn(Iyv, iy), Ixy = __fmul_rn(Ixv, iy);
            lhs[0] = __fsub_rn(lhs[0], __fmul_rn(__fmul_rn(fi, Ixv), I_e));
            lhs[1] = __fsub_rn(lhs[1], __fmul_rn(__fmul_rn(fj, Ixv), I_e));
            lhs[2] = __fsub_rn(lhs[2], __fmul_rn(Ixv, I_e));
            lhs[3] = __fsub_rn(lhs[3], __fmul_rn(__fmul_rn(fi, Iyv), I_e));
            lhs[4] = __fsub_rn(lhs[4], __fmul_rn(__fmul_rn(fj, Iyv), I_e));
            lhs[5] = __fsub_rn(lhs[5], __fmul_rn(Iyv, I_e));
            const float m0 = (float)(ii * ii), m1 = (float)(ii * jj), m2 = (float)(jj * jj);
            rhs[0] = __fadd_rn(rhs[0], __fmul_rn(m0, Ixx));
            rhs[1] = __fadd_rn(rhs[1], __fmul_rn(m1, Ixx));
            rhs[2] = __fadd_rn(rhs[2], __fmul_rn(fi, Ixx));
            rhs[7] = __fadd_rn(rhs[7], __fmul_rn(m2, Ixx));
            rhs[8] = __fadd_rn(rhs[8], __fmul_rn(fj, Ixx));
            rhs[14] = __fadd_rn(rhs[14], Ixx);
            rhs[3] = __fadd_rn(rhs[3], __fmul_rn(m0, Ixy));
            rhs[4] = __fadd_rn(rhs[4], __fmul_rn(m1, Ixy));
            rhs[5] = __fadd_rn(rhs[5], __fmul_rn(fi, Ixy));
            rhs[10] = __fadd_rn(rhs[10], __fmul_rn(m2, Ixy));
            rhs[11] = __fadd_rn(rhs[11], __fmul_rn(fj, Ixy));
            rhs[17] = __fadd_rn(rhs[17], Ixy);
            rhs[21] = __fadd_rn(rhs[21], __fmul_rn(m0, Iyy));
            rhs[22] = __fadd_rn(rhs[22], __fmul_rn(m1, Iyy));
            rhs[23] = __fadd_rn(rhs[23], __fmul_rn(fi, Iyy));
            rhs[28] = __fadd_rn(rhs[28], __fmul_rn(m2, Iyy));
            rhs[29] = __fadd_rn(rhs[29], __fmul_rn(fj, Iyy));
            rhs[35] = __fadd_rn(rhs[35], Iyy);
          }
        }
        if (skip == kern_pixels) break;                              // before the solve: lhs stays zero
        rhs[9] = rhs[4]; rhs[15] = rhs[5]; rhs[16] = rhs[11];
#pragma unroll
        for (int rr = 1; rr < 6; ++rr)
#pragma unroll
          for (int c = 0; c < rr; ++c) rhs[rr * 6 + c] = rhs[c * 6 + rr];
        aff_posv6(rhs, lhs);
        mean_noise = __fdiv_rn(mean_noise_tmp, sum_gamma_noise);
        w_plane = __fdiv_rn(sum_gamma_plane, (float)kern_pixels);
        w_noise = __fdiv_rn(sum_gamma_noise, (float)kern_pixels);
        double s2 = 0.0;                                             // norm_2(prev_lhs - lhs), stored as float
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const float t = __fsub_rn(prev_lhs[k], lhs[k]);
          s2 = __dadd_rn(s2, (double)__fmul_rn(t, t));
        }
        const float conv_error = (float)__dsqrt_rn((double)(float)s2);
#pragma unroll
        for (int k = 0; k < 6; ++k) { d_em[k] = __fadd_rn(d[k], lhs[k]); prev_lhs[k] = lhs[k]; }
        if (in_curr_sum_I_e < 0.0f) in_curr_sum_I_e = -in_curr_sum_I_e;
        curr_sum_I_e = in_curr_sum_I_e;
        if ((double)conv_error < 1e-3 && em_iter > 0) break;
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) d[k] = __fadd_rn(d[k], lhs[k]);
      if (curr_sum_I_e < 0.0f) curr_sum_I_e = -curr_sum_I_e;
      if (prev_sum_I_e < curr_sum_I_e && iter > 0) break;
      prev_sum_I_e = curr_sum_I_e;
    }
    if (aff_norm2_2(d[2], d[5]) > (double)max_translation || isnan(d[2]) || isnan(d[5])) ns = 0;
  }
  pyr_epilogue(a, p, ns, d[2], d[5], iters);
}

// the converged state back into the level's map (ROI + ring only)
__global__ void affine_commit_kernel(float* __restrict__ dx, float* __restrict__ dy, uint8_t* __restrict__ v,
                                     const uint8_t* __restrict__ s, const float* __restrict__ rdx, const float* __restrict__ rdy,
                                     int w, int x0, int y0, int x1, int y1) {
  const int x = x0 + blockIdx.x * blockDim.x + threadIdx.x, y = y0 + blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= x1 || y >= y1) return;
  const size_t p = (size_t)y * w + x;
  if (!v[p]) return;
  v[p] = s[p];
  if (s[p]) { dx[p] = rdx[p]; dy[p] = rdy[p]; }
}

// disparity_map_patch + range.min, cropped to the tile's box (SubpixelView.cc:208-220); invalid -> {0, 0, 0}
__global__ void affine_write_kernel(const float* __restrict__ dx, const float* __restrict__ dy, const uint8_t* __restrict__ v,
                                    int pw, int kx, int ky, int bx, int by, int bw, int bh, float sminx, float sminy,
                                    float* __restrict__ out, ptrdiff_t ostride_px) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= bw || y >= bh) return;
  const size_t q = (size_t)(y + ky) * pw + x + kx;
  float* o = out + ((ptrdiff_t)(by + y) * ostride_px + bx + x) * 3;
  if (v[q]) {
    o[0] = __fadd_rn(dx[q], sminx);
    o[1] = __fadd_rn(dy[q], sminy);
    o[2] = 1.0f;
  } else {
    o[0] = 0.0f; o[1] = 0.0f; o[2] = 0.0f;
  }
}

dim3 aff_grid(int w, int h) { return dim3((w + AFF_BX - 1) / AFF_BX, (h + AFF_BY - 1) / AFF_BY); }

// compute_spatial_weight_image (Correlate.cc:36-55) on the host: two_sigma_sqr formed in double and stored as float,
// a float exponent, exp in double stored as float, the sum in float, then weight /= sum.
void aff_weight_template(int kw, int kh, std::vector<float>& w) {
  const float two_sigma_sqr = 2.0 * std::pow(float(kw) / 5.0, 2.0);
  const int cx = kw / 2, cy = kh / 2;
  w.assign((size_t)kw * kh, 0.0f);
  float sum = 0.0f;
  for (int j = 0; j < kh; ++j)
    for (int i = 0; i < kw; ++i) {
      const float e = -1 * ((i - cx) * (i - cx) + (j - cy) * (j - cy)) / two_sigma_sqr;
      w[(size_t)j * kw + i] = (float)std::exp((double)e);
      sum += w[(size_t)j * kw + i];
    }
  for (auto& v : w) v /= sum;
}

struct aff_level {
  int w, h;
  float *L, *R, *Ix, *Iy, *dx, *dy;
  uint8_t* v;
};

}  // namespace

// The tile loop of vwgpu_pyramid_subpixel_dev (include/vwgpu.h) and vwgpu_phase_subpixel_dev (phase_subpixel.hip, through
// `refiner`); arguments are checked by the caller.
int vwgpu_pyramid_subpixel_tiles(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride,
                                 const float* d_left, ptrdiff_t lstride, const float* d_right, int rw, int rh, ptrdiff_t rstride,
                                 int mode, float width, int kx, int ky, int levels, int algorithm, const vwgpu_pyr_refiner* refiner,
                                 const int* tiles, int ntiles, float* d_out, ptrdiff_t ostride, long long* stats) {
  if (refiner) stats = nullptr;
  // ranges of all tiles: one launch, one readback
  const size_t tb = vwgpu_align_up((size_t)ntiles * 16, 256);
  int rc = vwgpu_arena_reserve(ctx, &ctx->misc, 2 * tb + 256 + vwgpu_align_up((size_t)kx * ky * 4, 256));
  if (rc) return rc;
  char* mb = static_cast<char*>(ctx->misc.base);
  int* d_tiles = reinterpret_cast<int*>(mb);
  int* d_keys = reinterpret_cast<int*>(mb + tb);
  int* d_changes = reinterpret_cast<int*>(mb + 2 * tb);
  unsigned long long* d_iters = reinterpret_cast<unsigned long long*>(mb + 2 * tb + 64);
  float* d_tmpl = reinterpret_cast<float*>(mb + 2 * tb + 256);
  std::vector<float> tmpl;
  aff_weight_template(kx, ky, tmpl);
  VWGPU_HIP(ctx, hipMemcpyAsync(d_tiles, tiles, (size_t)ntiles * 16, hipMemcpyHostToDevice, ctx->stream));
  VWGPU_HIP(ctx, hipMemcpyAsync(d_tmpl, tmpl.data(), tmpl.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  VWGPU_HIP(ctx, hipMemsetAsync(d_iters, 0, 8, ctx->stream));
  {
    vwgpu_prof_scope ps(ctx, "affine_range");
    hipLaunchKernelGGL(affine_range_init_kernel, dim3((4 * ntiles + 255) / 256), dim3(256), 0, ctx->stream, d_keys, 4 * ntiles);
    for (int t0 = 0; t0 < ntiles; t0 += 65535)   // gridDim.y <= 65535 tiles per launch
      hipLaunchKernelGGL(affine_range_kernel, dim3(16, std::min(65535, ntiles - t0)), dim3(256), 0, ctx->stream, d_disp, dstride,
                         d_tiles, d_keys, t0);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  std::vector<int> keys((size_t)4 * ntiles);
  VWGPU_HIP(ctx, hipMemcpyAsync(keys.data(), d_keys, keys.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
  auto key_float = [](int k) { const int b = k >= 0 ? k : k ^ 0x7fffffff; float f; std::memcpy(&f, &b, 4); return f; };

  // PREFILTER_LOG: the Gaussian of each whole image once per call; every tile crops the Laplacian of it
  float taps[1024];
  int nt = 0;
  if (mode == VWGPU_PREFILTER_LOG || mode == VWGPU_PREFILTER_MEANSUB) {
    nt = vwgpu_generate_gaussian_kernel((double)width, 0, taps, 1024);
    if (nt < 0) return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "prefilter width %g too large", (double)width);
  }
  float *gl = nullptr, *gr = nullptr;
  const int c = nt ? (nt - 1) / 2 : 0;
  if (mode == VWGPU_PREFILTER_LOG) {
    const size_t gb = vwgpu_align_up((size_t)w * h * 4, 256), grb = vwgpu_align_up((size_t)rw * rh * 4, 256);
    rc = vwgpu_arena_reserve(ctx, &ctx->filt, gb + grb);
    if (rc) return rc;
    gl = static_cast<float*>(ctx->filt.base);
    gr = reinterpret_cast<float*>(static_cast<char*>(ctx->filt.base) + gb);
    if ((rc = vwgpu_launch_sepconv(ctx, d_left, w, h, lstride, taps, nt, c, taps, nt, c, 0, 1, gl, w))) return rc;
    if ((rc = vwgpu_launch_sepconv(ctx, d_right, rw, rh, rstride, taps, nt, c, taps, nt, c, 0, 1, gr, rw))) return rc;
  }
  const float lap[9] = {0, 1, 0, 1, -4, 1, 0, 1, 0};
  int total_rounds = 0, max_rounds = 0;
  // BAYES_EM: plane_norm_factor / noise_norm_factor as the reference forms them (Correlate.cc:634-635), 1.0 / sqrt(2 pi
  // var2) in double stored to float; var2_plane = 1e-3 and var2_noise = 1e-2 are never updated.
  const float var2_plane = 1e-3f, var2_noise = 1e-2f;
  const float plane_nf = 1.0 / std::sqrt(2 * M_PI * var2_plane), noise_nf = 1.0 / std::sqrt(2 * M_PI * var2_noise);

  // BBox2f -> BBox2i: a C cast of each corner (BBox.tcc:49-50).  Every tile is checked before the first one is written.
  std::vector<int> rng((size_t)4 * ntiles, 0);
  for (int t = 0; t < ntiles; ++t) {
    const int bw = tiles[4 * t + 2], bh = tiles[4 * t + 3];
    if (!(keys[4 * t] == INT_MAX && keys[4 * t + 2] == INT_MIN)) {     // min > max: the initial keys, no valid pixel
      const float fmnx = key_float(keys[4 * t]), fmny = key_float(keys[4 * t + 1]);
      const float fmxx = key_float(keys[4 * t + 2]), fmxy = key_float(keys[4 * t + 3]);
      if (!(std::isfinite(fmnx) && std::isfinite(fmny) && std::isfinite(fmxx) && std::isfinite(fmxy)))
        return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_subpixel: tile %d holds a non-finite disparity in a valid pixel", t);
      // the patch spans the range: a range this wide cannot be held (and would overflow the int conversion below)
      if (!(std::fabs(fmnx) < 1e9f && std::fabs(fmny) < 1e9f && std::fabs(fmxx) < 1e9f && std::fabs(fmxy) < 1e9f))
        return vwgpu_fail(ctx, VWGPU_ERR_NOMEM, "pyramid_subpixel: the disparity range of tile %d needs a patch that cannot be held", t);
      rng[4 * t] = (int)fmnx; rng[4 * t + 1] = (int)fmny; rng[4 * t + 2] = (int)fmxx; rng[4 * t + 3] = (int)fmxy;
    }
    const long long pwl = (long long)bw + (rng[4 * t + 2] - rng[4 * t]) + 2LL * kx, phl = (long long)bh + (rng[4 * t + 3] - rng[4 * t + 1]) + 2LL * ky;
    if (pwl > 32768 || phl > 32768 || pwl * phl > (1LL << 28))
      return vwgpu_fail(ctx, VWGPU_ERR_NOMEM, "pyramid_subpixel: tile %d needs a %lld x %lld patch", t, pwl, phl);
  }

  for (int t = 0; t < ntiles; ++t) {
    const int bx = tiles[4 * t], by = tiles[4 * t + 1], bw = tiles[4 * t + 2], bh = tiles[4 * t + 3];
    const int sminx = rng[4 * t], sminy = rng[4 * t + 1], smaxx = rng[4 * t + 2], smaxy = rng[4 * t + 3];
    const long long pwl = (long long)bw + (smaxx - sminx) + 2LL * kx, phl = (long long)bh + (smaxy - sminy) + 2LL * ky;
    const int pw = (int)pwl, ph = (int)phl;
    const int lx0 = bx - kx, ly0 = by - ky, rx0 = bx + sminx - kx, ry0 = by + sminy - ky;

    // arena layout: per level L, R, Ix, Iy, dx, dy (float), v (u8); then the fixpoint buffers of level 0's size
    std::vector<aff_level> lv(levels + 1);
    std::vector<size_t> off(levels + 1);
    size_t bytes = 0;
    int lw = pw, lh = ph;
    for (int i = 0; i <= levels; ++i) {
      if (i > 0) { lw = 1 + (lw - 1) / 2; lh = 1 + (lh - 1) / 2; }
      lv[i].w = lw; lv[i].h = lh;
      off[i] = bytes;
      bytes += 6 * vwgpu_align_up((size_t)lw * lh * 4, 256) + vwgpu_align_up((size_t)lw * lh, 256);
    }
    const size_t n0 = (size_t)pw * ph;
    const size_t fix_off = bytes;
    bytes += 2 * vwgpu_align_up(n0 * 4, 256) + 4 * vwgpu_align_up(n0, 256) + vwgpu_align_up(n0 * 4, 256);   // + prefilter scratch
    rc = vwgpu_arena_reserve(ctx, &ctx->pyr, bytes);
    if (rc) return rc;
    char* base = static_cast<char*>(ctx->pyr.base);
    for (int i = 0; i <= levels; ++i) {
      const size_t fb = vwgpu_align_up((size_t)lv[i].w * lv[i].h * 4, 256);
      char* q = base + off[i];
      lv[i].L = reinterpret_cast<float*>(q);
      lv[i].R = reinterpret_cast<float*>(q + fb);
      lv[i].Ix = reinterpret_cast<float*>(q + 2 * fb);
      lv[i].Iy = reinterpret_cast<float*>(q + 3 * fb);
      lv[i].dx = reinterpret_cast<float*>(q + 4 * fb);
      lv[i].dy = reinterpret_cast<float*>(q + 5 * fb);
      lv[i].v = reinterpret_cast<uint8_t*>(q + 6 * fb);
    }
    char* fq = base + fix_off;
    const size_t f4 = vwgpu_align_up(n0 * 4, 256), f1 = vwgpu_align_up(n0, 256);
    float* rdx = reinterpret_cast<float*>(fq);
    float* rdy = reinterpret_cast<float*>(fq + f4);
    uint8_t* sA = reinterpret_cast<uint8_t*>(fq + 2 * f4);
    uint8_t* sB = sA + f1;
    uint8_t* cA = sB + f1;
    uint8_t* cB = cA + f1;
    float* pscratch = reinterpret_cast<float*>(cB + f1);

    // prefiltered crops (SubpixelView.cc:65-86)
    if (mode == VWGPU_PREFILTER_LOG) {
      if ((rc = vwgpu_launch_conv2d_region(ctx, gl, w, h, w, lap, 3, 3, 1, 1, 0, lv[0].L, pw, pw, ph, lx0, ly0))) return rc;
      if ((rc = vwgpu_launch_conv2d_region(ctx, gr, rw, rh, rw, lap, 3, 3, 1, 1, 0, lv[0].R, pw, pw, ph, rx0, ry0))) return rc;
    } else {
      if ((rc = vwgpu_prefilter_region(ctx, d_left, w, h, lstride, mode, width, lx0, ly0, pw, ph, lv[0].L, pscratch))) return rc;
      if ((rc = vwgpu_prefilter_region(ctx, d_right, rw, rh, rstride, mode, width, rx0, ry0, pw, ph, lv[0].R, pscratch))) return rc;
    }
    vwgpu_prof_scope ps(ctx, "affine_subpixel_tile");
    hipLaunchKernelGGL(affine_disp_patch_kernel, aff_grid(pw, ph), dim3(AFF_BX, AFF_BY), 0, ctx->stream, d_disp, w, h, dstride,
                       lx0, ly0, pw, ph, (float)sminx, (float)sminy, lv[0].dx, lv[0].dy, lv[0].v);
    // pyramid (:108-129)
    for (int i = 1; i <= levels; ++i) {
      const aff_level &s = lv[i - 1], &d = lv[i];
      hipLaunchKernelGGL(affine_subsample_kernel, aff_grid(d.w, d.h), dim3(AFF_BX, AFF_BY), 0, ctx->stream, s.L, s.w, d.L, d.w, d.h);
      hipLaunchKernelGGL(affine_subsample_kernel, aff_grid(d.w, d.h), dim3(AFF_BX, AFF_BY), 0, ctx->stream, s.R, s.w, d.R, d.w, d.h);
      hipLaunchKernelGGL(affine_disp_subsample_kernel, aff_grid(d.w, d.h), dim3(AFF_BX, AFF_BY), 0, ctx->stream,
                         s.dx, s.dy, s.v, s.w, s.h, d.dx, d.dy, d.v, d.w, d.h);
    }
    // coarse to fine (:133-190), then the final pass at full resolution (:195-222)
    for (int i = levels; i >= 0; --i) {
      aff_level& L = lv[i];
      const int div = 1 << i;
      int x0 = kx, y0 = ky, x1 = kx + bw, y1 = ky + bh;
      for (int k = 0; k < i; ++k) { x0 /= 2; y0 /= 2; x1 /= 2; y1 /= 2; }
      (void)div;
      x0 = std::max(x0 - 1, kx / 2); y0 = std::max(y0 - 1, ky / 2);
      x1 = std::min(L.w - kx / 2, x1 + 1); y1 = std::min(L.h - ky / 2, y1 + 1);
      if (x1 > x0 && y1 > y0 && refiner) {
        const vwgpu_pyr_level_view view{L.w, L.h, L.L, L.R, L.dx, L.dy, L.v};
        if ((rc = refiner->refine(ctx, view, kx, ky, x0, y0, x1, y1, refiner->user))) return rc;
      } else if (x1 > x0 && y1 > y0) {
        hipLaunchKernelGGL(affine_deriv_kernel, aff_grid(L.w, L.h), dim3(AFF_BX, AFF_BY), 0, ctx->stream, L.L, L.w, L.h, L.Ix, L.Iy);
        const size_t n = (size_t)L.w * L.h;
        VWGPU_HIP(ctx, hipMemcpyAsync(sA, L.v, n, hipMemcpyDeviceToDevice, ctx->stream));
        VWGPU_HIP(ctx, hipMemcpyAsync(sB, L.v, n, hipMemcpyDeviceToDevice, ctx->stream));
        VWGPU_HIP(ctx, hipMemsetAsync(cA, 0, n, ctx->stream));
        VWGPU_HIP(ctx, hipMemsetAsync(cB, 0, n, ctx->stream));
        aff_level_args a;
        a.L = L.L; a.R = L.R; a.Ix = L.Ix; a.Iy = L.Iy; a.tmpl = d_tmpl;
        a.dx = L.dx; a.dy = L.dy; a.v0 = L.v;
        a.rdx = rdx; a.rdy = rdy; a.changes = d_changes; a.iters = stats ? d_iters : nullptr;
        a.w = L.w; a.h = L.h; a.kx = kx; a.ky = ky; a.x0 = x0; a.y0 = y0; a.x1 = x1; a.y1 = y1;
        const long long cap = (long long)(x1 - x0) * (y1 - y0) + 1;
        uint8_t *sp = sA, *sc = sB, *cp = cA, *cc = cB;
        for (int round = 0;; ++round) {
          if (round > cap) return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "pyramid_subpixel: invalidation fixpoint did not converge");
          a.round = round; a.sprev = sp; a.cprev = cp; a.scur = sc; a.ccur = cc;
          VWGPU_HIP(ctx, hipMemsetAsync(d_changes, 0, 4, ctx->stream));
          if (algorithm == VWGPU_SUBPIXEL_FAST_AFFINE)
            hipLaunchKernelGGL(affine_refine_kernel, aff_grid(x1 - x0, y1 - y0), dim3(AFF_BX, AFF_BY), 0, ctx->stream, a);
          else if (algorithm == VWGPU_SUBPIXEL_LUCAS_KANADE)
            hipLaunchKernelGGL(lk_refine_kernel, aff_grid(x1 - x0, y1 - y0), dim3(AFF_BX, AFF_BY), 0, ctx->stream, a);
          else
            hipLaunchKernelGGL(em_refine_kernel, aff_grid(x1 - x0, y1 - y0), dim3(AFF_BX, AFF_BY), 0, ctx->stream, a, plane_nf,
                               noise_nf);
          int changes = 0;
          VWGPU_HIP(ctx, hipMemcpyAsync(&changes, d_changes, 4, hipMemcpyDeviceToHost, ctx->stream));
          VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
          std::swap(sp, sc);
          std::swap(cp, cc);
          if (changes == 0) {
            total_rounds += round + 1;
            max_rounds = std::max(max_rounds, round + 1);
            break;
          }
        }
        hipLaunchKernelGGL(affine_commit_kernel, aff_grid(x1 - x0, y1 - y0), dim3(AFF_BX, AFF_BY), 0, ctx->stream,
                           L.dx, L.dy, L.v, sp, rdx, rdy, L.w, x0, y0, x1, y1);
      }
      if (i > 0) {
        const aff_level& U = lv[i - 1];
        hipLaunchKernelGGL(affine_upsample_kernel, aff_grid(U.w, U.h), dim3(AFF_BX, AFF_BY), 0, ctx->stream,
                           L.dx, L.dy, L.v, L.w, L.h, U.dx, U.dy, U.v, U.w, U.h);
      }
    }
    hipLaunchKernelGGL(affine_write_kernel, aff_grid(bw, bh), dim3(AFF_BX, AFF_BY), 0, ctx->stream, lv[0].dx, lv[0].dy, lv[0].v,
                       pw, kx, ky, bx, by, bw, bh, (float)sminx, (float)sminy, d_out, ostride);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (stats) {
    unsigned long long it = 0;
    VWGPU_HIP(ctx, hipMemcpyAsync(&it, d_iters, 8, hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    stats[0] = total_rounds;
    stats[1] = max_rounds;
    stats[2] = (long long)it;
  }
  return VWGPU_OK;
}

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------

namespace {

int aff_check(vwgpu_ctx* ctx, const void* disp, int w, int h, ptrdiff_t& dstride, const void* left, ptrdiff_t& lstride,
              const void* right, int rw, int rh, ptrdiff_t& rstride, int mode, int kx, int ky, int algorithm,
              const int* tiles, int ntiles, const void* out, ptrdiff_t& ostride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!disp || !left || !right || !out || w <= 0 || h <= 0 || rw <= 0 || rh <= 0 || ntiles < 0 || (ntiles > 0 && !tiles))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_subpixel: empty image or null pointer");
  if (kx < 1 || ky < 1 || kx % 2 != 1 || ky % 2 != 1)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_subpixel: Kernel input not sized with odd values.");
  if (mode != VWGPU_PREFILTER_NONE && mode != VWGPU_PREFILTER_MEANSUB && mode != VWGPU_PREFILTER_LOG)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_subpixel: unknown prefilter mode %d", mode);
  if (algorithm < VWGPU_SUBPIXEL_LUCAS_KANADE || algorithm > VWGPU_SUBPIXEL_PHASE)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_subpixel: unknown algorithm %d", algorithm);
  if (algorithm == VWGPU_SUBPIXEL_PHASE)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "pyramid_subpixel: algorithm %d (PHASE) is not implemented", algorithm);
  if (dstride == 0) dstride = w;
  if (ostride == 0) ostride = w;
  if (lstride == 0) lstride = w;
  if (rstride == 0) rstride = rw;
  if (dstride < w || ostride < w || lstride < w || rstride < rw)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_subpixel: row stride smaller than row width");
  for (int t = 0; t < ntiles; ++t) {
    const int* b = tiles + 4 * t;
    if (b[2] <= 0 || b[3] <= 0 || b[0] < 0 || b[1] < 0 || b[0] > w - b[2] || b[1] > h - b[3])
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_subpixel: tile %d {%d, %d, %d, %d} is not inside the %d x %d image",
                        t, b[0], b[1], b[2], b[3], w, h);
  }
  return VWGPU_OK;
}

}  // namespace

extern "C" {

int vwgpu_pyramid_subpixel_dev(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride,
                               const float* d_left, ptrdiff_t lstride, const float* d_right, int rw, int rh, ptrdiff_t rstride,
                               int mode, float width, int kx, int ky, int levels, int algorithm, const int* tiles, int ntiles,
                               float* d_out, ptrdiff_t ostride, long long* stats) {
  int rc = aff_check(ctx, d_disp, w, h, dstride, d_left, lstride, d_right, rw, rh, rstride, mode, kx, ky, algorithm, tiles, ntiles,
                     d_out, ostride);
  if (rc) return rc;
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  if (ntiles == 0) return VWGPU_OK;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return vwgpu_pyramid_subpixel_tiles(ctx, d_disp, w, h, dstride, d_left, lstride, d_right, rw, rh, rstride, mode, width, kx, ky,
                                      levels < 0 ? 0 : levels, algorithm, nullptr, tiles, ntiles, d_out, ostride, stats);
}

int vwgpu_pyramid_subpixel(vwgpu_ctx* ctx, const float* disp, int w, int h, ptrdiff_t dstride,
                           const float* left, ptrdiff_t lstride, const float* right, int rw, int rh, ptrdiff_t rstride,
                           int mode, float width, int kx, int ky, int levels, int algorithm, const int* tiles, int ntiles,
                           float* out, ptrdiff_t ostride, long long* stats) {
  int rc = aff_check(ctx, disp, w, h, dstride, left, lstride, right, rw, rh, rstride, mode, kx, ky, algorithm, tiles, ntiles,
                     out, ostride);
  if (rc) return rc;
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  if (ntiles == 0) return VWGPU_OK;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pd = st.add(disp, w, h, 12, dstride, VWGPU_STAGE_IN), po = st.add(out, w, h, 12, ostride, VWGPU_STAGE_INOUT);
  const int pl = st.add(left, w, h, 4, lstride, VWGPU_STAGE_IN), pr = st.add(right, rw, rh, 4, rstride, VWGPU_STAGE_IN);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_pyramid_subpixel_tiles(ctx, st.dev<float>(pd), w, h, w, st.dev<float>(pl), w, st.dev<float>(pr), rw, rh, rw, mode, width, kx, ky,
                                    levels < 0 ? 0 : levels, algorithm, nullptr, tiles, ntiles, st.dev<float>(po), w, stats);
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
