// phase_subpixel.hip — vw::stereo::phase_subpixel (src/vw/Stereo/SubpixelView.h:136-144, SubpixelView.cc:275-289):
// PyramidSubpixelView with SUBPIXEL_PHASE, whose refiner is subpixel_phase_2d (src/vw/Stereo/PhaseSubpixelView.cc:231-326)
// calling phase_correlation_subpixel (:103-229) twice per pixel.  The tile loop (ranges, crops, pyramids, subsample and
// upsample, the final write) is affine_subpixel.hip's, reached through a vwgpu_pyr_refiner; this file adds the refiner.
//
// The reference's pixels do not depend on each other (a pixel reads and writes only its own disparity), so a level is one
// launch, in place: one workgroup per pixel of the ROI plus its 1-pixel ring.  The reference's transforms are OpenCV DFTs
// whose internal order cannot be reproduced; the project defines the arithmetic instead, and the CPU
// restatement tests/refimpl/phase_ref.cc follows the same definition:
//   - every DFT is a direct sum, one __fmaf_rn chain per output in ascending k, from host-built float twiddles (double
//     cos / sin of 2 pi k / n rounded to float); a complex step (a + ib)(c + is) accumulates re: a c, then -b s and
//     im: a s, then b c (a forward twiddle is c - is);
//   - the inverse DFT with real output is the real part of the complex inverse of the padded spectrum, rows first (over
//     the padded columns), then the real part over the padded rows; the padded spectrum is zero outside the N x M
//     entries pad_fourier_transform places, and the sums run over those entries only (a zero term can change only the
//     sign of a zero, which no maximum sees).  For odd windows the padded spectrum is Hermitian, so this is what a c2r
//     transform computes mathematically;
//   - the partial_upsample_dft kernels are host tables of the reference's own form: the host libm's
//     std::exp(complex<float>(m, 0) * (complex<float>(0, -1) * float(2 pi) / float(N * pad))) for every integer m used;
//   - a maximum is the first element, in row-major order, strictly greater than a running maximum that starts at -inf
//     (index 0 when none is), so NaN never wins;
//   - the magnitude is the correctly rounded sqrt of fl(re * re) + fl(im * im).
// The second right crop is translate(right, d) with BicubicInterpolation (Interpolation.h:138-185) in FP64 over a zero
// edge extension, sampled at p - d (Math/Transform.h:281).
// get_dft (Fourier.cc:36-75) transforms every patch after percentile_scale_convert(patch, 0.02, 0.98) (ImageThresh.h:
// 244-268): the 8-bit image of the patch, values 0..255 (ph_to_u8).
#include <cfloat>
#include <climits>
#include <cmath>
#include <complex>
#include <vector>

#include "vwgpu_internal.h"

namespace {

constexpr int PH_THREADS = 256;
constexpr int PH_MAX_KERNEL = 41, PH_MAX_ACCURACY = 64;   // include/vwgpu.h states these limits

struct ph_call {             // one phase_correlation_subpixel call at pad factor `pad`
  int pad, up;               // up = ceil(1.5 pad) (upsampled_width / upsampled_height)
  float dft_shift;           // floor(ceil(1.5 pad) / 2)
  int mxc, mxr;              // the kernel tables hold m in [-mx, mx]
  const float2 *ec, *er;     // column kernel exp(m * -2 pi i / (C pad)) and row kernel exp(m * -2 pi i / (R pad)), at m + mx
};

struct ph_args {
  const float *L, *R;
  float *dx, *dy;
  uint8_t* v;
  int w, h, kx, ky;
  int x0, y0, rw;            // the pixels: [x0, x0 + rw) x [y0, ...), one per workgroup in raster order
  const float* tw;           // cos then sin of 2 pi k / n for n = C, R, 2C, 2R
  float invs;                // DFT_SCALE of the padded inverse: float(1 / (4 R C))
  ph_call c1, c2;            // accuracy / 2 and accuracy
  unsigned long long* counters;   // [0] pixels refined, [1] pixels invalidated
};

// Correctly rounded float sqrt (cv::magnitude's sqrt): v_sqrt_f32 is 1 ulp, so the nearest float to the double root is
// corrected with exact double arithmetic (as aff_sqrt_rn in affine_subpixel.hip).
__device__ inline float ph_sqrt_rn(float x) {
  float r = (float)__dsqrt_rn((double)x);
  const float up = nextafterf(r, INFINITY), dn = nextafterf(r, 0.0f);
  const double mu = ((double)r + (double)up) * 0.5, md = ((double)r + (double)dn) * 0.5;
  if (mu * mu < (double)x) r = up;
  else if (md * md > (double)x) r = dn;
  return r;
}

// (av, ai) precedes (bv, bi) as the first maximum: a qualifies (ai >= 0) and b does not, or a is larger, or equal and earlier
__device__ inline bool ph_wins(float av, int ai, float bv, int bi) {
  return ai >= 0 && (bi < 0 || av > bv || (av == bv && ai < bi));
}

// Workgroup reduction of every thread's first maximum (over its own indices, scanned in ascending order); index 0 when no
// element qualified.  The result is the first strict maximum of the whole row-major scan.
__device__ int ph_argmax(float bv, int bi, float* red_v, int* red_i) {
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (ph_wins(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = bv; red_i[threadIdx.x >> 6] = bi; }
  __syncthreads();
  float rv = red_v[0];
  int ri = red_i[0];
  for (int k = 1; k < PH_THREADS / 64; ++k)
    if (ph_wins(red_v[k], red_i[k], rv, ri)) { rv = red_v[k]; ri = red_i[k]; }
  __syncthreads();
  return ri < 0 ? 0 : ri;
}

// get_dft of a real R x C patch (row transforms, then column transforms).  With lspec != nullptr the column pass writes
// mulSpectrums(lspec, F, conj) = lspec * conj(F) instead of F: re = fl(lr fr) + fl(li fi), im = fl(li fr) - fl(lr fi).
// Complex arrays interleave re, im.  T: 2 R C floats of scratch.
__device__ void ph_forward(const float* pat, float* T, const float* twc, const float* twr, int R, int C, const float* lspec,
                           float* out) {
  const int n = R * C;
  for (int o = threadIdx.x; o < n; o += PH_THREADS) {
    const int y = o / C, v = o - y * C;
    const float* row = pat + y * C;
    float re = 0.0f, im = 0.0f;
    int t = 0;
    for (int x = 0; x < C; ++x) {
      re = __fmaf_rn(row[x], twc[t], re);
      im = __fmaf_rn(row[x], -twc[C + t], im);
      t += v;
      if (t >= C) t -= C;
    }
    T[2 * o] = re;
    T[2 * o + 1] = im;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < n; o += PH_THREADS) {
    const int u = o / C, v = o - u * C;
    float re = 0.0f, im = 0.0f;
    int t = 0;
    for (int y = 0; y < R; ++y) {
      const float a = T[2 * (y * C + v)], b = T[2 * (y * C + v) + 1], c = twr[t], s = twr[R + t];
      re = __fmaf_rn(a, c, re);
      re = __fmaf_rn(b, s, re);
      im = __fmaf_rn(a, -s, im);
      im = __fmaf_rn(b, c, im);
      t += u;
      if (t >= R) t -= R;
    }
    if (lspec) {
      const float lr = lspec[2 * o], li = lspec[2 * o + 1];
      out[2 * o] = __fadd_rn(__fmul_rn(lr, re), __fmul_rn(li, im));
      out[2 * o + 1] = __fsub_rn(__fmul_rn(li, re), __fmul_rn(lr, im));
    } else {
      out[2 * o] = re;
      out[2 * o + 1] = im;
    }
  }
  __syncthreads();
}

__device__ inline float2 ph_tab(const float2* tab, int mx, int m) {
  const int k = min(max(m + mx, 0), 2 * mx);   // m never leaves [-mx, mx] (host bound); the clamp keeps loads inside
  return tab[k];
}

// phase_correlation_subpixel (PhaseSubpixelView.cc:103-229) of the left spectrum FL and the cross spectrum X = FL conj(FR).
// S: scratch of max(4 R C, 2 up C) floats.  Returns the offset {x, y}.
__device__ float2 ph_correlate(const float* X, float* S, const float* tw2c, const float* tw2r, int R, int C, float invs,
                               const ph_call& k, float* red_v, int* red_i) {
  const int C2 = 2 * C, R2 = 2 * R, mc = C / 2, mr = R / 2;
  // pad_fourier_transform to 2R x 2C (scale 4) and the scaled inverse DFT with real output: G[u][x] over the padded
  // columns of source row u (column v sits at v for v <= C / 2, at v + C above), then the real part over the padded rows
  for (int o = threadIdx.x; o < R * C2; o += PH_THREADS) {
    const int u = o / C2, x = o - u * C2;
    const int hi = (x & 1) ? C : 0;          // (v + C) x = v x + C x (mod 2C)
    float re = 0.0f, im = 0.0f;
    int t = 0;                               // v x mod 2C
    for (int v = 0; v < C; ++v) {
      int tt = v <= mc ? t : t + hi;
      if (tt >= C2) tt -= C2;
      const float a = __fmul_rn(4.0f, X[2 * (u * C + v)]), b = __fmul_rn(4.0f, X[2 * (u * C + v) + 1]);
      const float c = tw2c[tt], s = tw2c[C2 + tt];
      re = __fmaf_rn(a, c, re);
      re = __fmaf_rn(-b, s, re);
      im = __fmaf_rn(a, s, im);
      im = __fmaf_rn(b, c, im);
      t += x;
      if (t >= C2) t -= C2;
    }
    S[2 * o] = re;
    S[2 * o + 1] = im;
  }
  __syncthreads();
  float bv = -INFINITY;
  int bi = -1;
  for (int o = threadIdx.x; o < R2 * C2; o += PH_THREADS) {
    const int y = o / C2, x = o - y * C2;
    const int hi = (y & 1) ? R : 0;
    float acc = 0.0f;
    int t = 0;
    for (int u = 0; u < R; ++u) {
      int tt = u <= mr ? t : t + hi;
      if (tt >= R2) tt -= R2;
      const float c = tw2r[tt], s = tw2r[R2 + tt];
      acc = __fmaf_rn(S[2 * (u * C2 + x)], c, acc);
      acc = __fmaf_rn(-S[2 * (u * C2 + x) + 1], s, acc);
      t += y;
      if (t >= R2) t -= R2;
    }
    const float val = __fmul_rn(acc, invs);
    if (val > bv) { bv = val; bi = o; }
  }
  const int loc = ph_argmax(bv, bi, red_v, red_i);
  const int ly = loc / C2, lx = loc - ly * C2;
  float sx = __fdiv_rn((float)(lx < C ? lx : lx - C2), 2.0f);
  float sy = __fdiv_rn((float)(ly < R ? ly : ly - R2), 2.0f);
  if (k.pad <= 2) return make_float2(sx, sy);

  // second pass: partial_upsample_dft (:42-101) of R conj(L) = conj(X) around the rounded shift
  const float fpad = (float)k.pad;
  sx = (float)__ddiv_rn(round((double)__fmul_rn(sx, fpad)), (double)k.pad);
  sy = (float)__ddiv_rn(round((double)__fmul_rn(sy, fpad)), (double)k.pad);
  const int roff = (int)__fsub_rn(k.dft_shift, __fmul_rn(sy, fpad));
  const int coff = (int)__fsub_rn(k.dft_shift, __fmul_rn(sx, fpad));
  const int up = k.up;
  for (int o = threadIdx.x; o < up * C; o += PH_THREADS) {      // o1 = row_kernel * conj(X), up x C
    const int i = o / C, c = o - i * C;
    float re = 0.0f, im = 0.0f;
    for (int r = 0; r < R; ++r) {
      const float2 e = ph_tab(k.er, k.mxr, (i - roff) * (r <= mr ? r : r - R));
      const float p = X[2 * (r * C + c)], q = -X[2 * (r * C + c) + 1];
      re = __fmaf_rn(e.x, p, re);
      re = __fmaf_rn(-e.y, q, re);
      im = __fmaf_rn(e.x, q, im);
      im = __fmaf_rn(e.y, p, im);
    }
    S[2 * o] = re;
    S[2 * o + 1] = im;
  }
  __syncthreads();
  bv = -INFINITY;
  bi = -1;
  for (int o = threadIdx.x; o < up * up; o += PH_THREADS) {     // out = o1 * col_kernel, up x up, and its magnitude
    const int i = o / up, j = o - i * up;
    float re = 0.0f, im = 0.0f;
    for (int c = 0; c < C; ++c) {
      const float2 e = ph_tab(k.ec, k.mxc, (c <= mc ? c : c - C) * (j - coff));
      const float a = S[2 * (i * C + c)], b = S[2 * (i * C + c) + 1];
      re = __fmaf_rn(a, e.x, re);
      re = __fmaf_rn(-b, e.y, re);
      im = __fmaf_rn(a, e.y, im);
      im = __fmaf_rn(b, e.x, im);
    }
    const float mag = ph_sqrt_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)));
    if (mag > bv) { bv = mag; bi = o; }
  }
  const int l2 = ph_argmax(bv, bi, red_v, red_i);
  const int ds = (int)k.dft_shift;
  sy = __fadd_rn(sy, __fdiv_rn((float)(l2 / up - ds), fpad));
  sx = __fadd_rn(sx, __fdiv_rn((float)(l2 % up - ds), fpad));
  return make_float2(sx, sy);
}

__device__ inline float ph_zero(const float* __restrict__ r, int w, int h, int x, int y) {
  return (x < 0 || y < 0 || x >= w || y >= h) ? 0.0f : r[(size_t)y * w + x];
}

__device__ inline int ph_floor(double v) {   // math::impl::_floor
  const int iv = (int)v;
  return (v < 0 && (double)iv != v) ? iv - 1 : iv;
}

// BicubicInterpolation over ZeroEdgeExtension at (i, j), in double, with the integer-pixel shortcut
__device__ float ph_bicubic(const float* __restrict__ r, int w, int h, double i, double j) {
  const int x = ph_floor(i), y = ph_floor(j);
  if ((double)x == i && (double)y == j) return ph_zero(r, w, h, x, y);
  const double nx = __dsub_rn(i, (double)x), ny = __dsub_rn(j, (double)y);
  const double s[4] = {__dmul_rn(__dsub_rn(__dmul_rn(__dsub_rn(2.0, nx), nx), 1.0), nx),
                       __dadd_rn(__dmul_rn(__dmul_rn(__dsub_rn(__dmul_rn(3.0, nx), 5.0), nx), nx), 2.0),
                       __dmul_rn(__dadd_rn(__dmul_rn(__dsub_rn(4.0, __dmul_rn(3.0, nx)), nx), 1.0), nx),
                       __dmul_rn(__dmul_rn(__dsub_rn(nx, 1.0), nx), nx)};
  const double t[4] = {__dmul_rn(__dsub_rn(__dmul_rn(__dsub_rn(2.0, ny), ny), 1.0), ny),
                       __dadd_rn(__dmul_rn(__dmul_rn(__dsub_rn(__dmul_rn(3.0, ny), 5.0), ny), ny), 2.0),
                       __dmul_rn(__dadd_rn(__dmul_rn(__dsub_rn(4.0, __dmul_rn(3.0, ny)), ny), 1.0), ny),
                       __dmul_rn(__dmul_rn(__dsub_rn(ny, 1.0), ny), ny)};
  double result = 0.0;
  for (int b = 0; b < 4; ++b) {
    double row = __dmul_rn(s[0], (double)ph_zero(r, w, h, x - 1, y - 1 + b));
    row = __dadd_rn(row, __dmul_rn(s[1], (double)ph_zero(r, w, h, x, y - 1 + b)));
    row = __dadd_rn(row, __dmul_rn(s[2], (double)ph_zero(r, w, h, x + 1, y - 1 + b)));
    row = __dadd_rn(row, __dmul_rn(s[3], (double)ph_zero(r, w, h, x + 2, y - 1 + b)));
    result = b == 0 ? __dmul_rn(t[0], row) : __dadd_rn(result, __dmul_rn(t[b], row));
  }
  return (float)__dmul_rn(result, 0.25);
}

// A double -> int32 conversion as x86's cvttsd2si does it (the reference's static_cast<int> on its platform): truncation,
// and INT_MIN for NaN and for values outside the int32 range.
__device__ inline int ph_toint(double x) {
  return (x >= -2147483648.0 && x < 2147483648.0) ? (int)x : INT_MIN;
}

// percentile_scale_convert(patch, 0.02, 0.98, 256 bins) (ImageThresh.h:244-268) of the n floats of pat, in place, as the
// floats 0..255 of the uint8 image get_dft transforms:
//   find_image_min_max: min / max in double, NaN skipped (Image/Statistics.h:114-128);
//   histogram: max = min + 1 when they are equal; bin = int(round(255 ((v - min) / range))), clamped to [0, 255], every
//   value counted (NaN: bin 0) (ImageThresh.h:52-70, Math/Statistics.cc:34-76);
//   get_percentile: the first bin whose running sum of count / n reaches the percentile (Statistics.cc:85-104);
//   low / high = (bin + 1) * bin_width + min; clamp to the floats of low / high, normalize to 0..255 with the double ratio
//   255 / float(high - low) (0 when equal), then the uint8 cast (truncation; NaN: 0) (Image/Algorithms.h).
__device__ void ph_to_u8(float* pat, int n, unsigned* hist, double* terms, double* red_d) {
  double mn = DBL_MAX, mx = -DBL_MAX;
  for (int i = threadIdx.x; i < n; i += PH_THREADS) {
    const double v = (double)pat[i];
    if (v < mn) mn = v;
    if (v > mx) mx = v;
  }
  for (int i = threadIdx.x; i < 256; i += PH_THREADS) hist[i] = 0;
  for (int o = 32; o > 0; o >>= 1) {
    mn = fmin(mn, __shfl_xor(mn, o));
    mx = fmax(mx, __shfl_xor(mx, o));
  }
  if ((threadIdx.x & 63) == 0) { red_d[threadIdx.x >> 6] = mn; red_d[4 + (threadIdx.x >> 6)] = mx; }
  __syncthreads();
  mn = red_d[0];
  mx = red_d[4];
  for (int k = 1; k < PH_THREADS / 64; ++k) { mn = fmin(mn, red_d[k]); mx = fmax(mx, red_d[4 + k]); }
  const double range = __dsub_rn(mx == mn ? __dadd_rn(mn, 1.0) : mx, mn);
  for (int i = threadIdx.x; i < n; i += PH_THREADS) {
    int bin = ph_toint(round(__dmul_rn(255.0, __ddiv_rn(__dsub_rn((double)pat[i], mn), range))));
    bin = bin < 0 ? 0 : (bin > 255 ? 255 : bin);
    atomicAdd(hist + bin, 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 256; i += PH_THREADS) terms[i] = __ddiv_rn((double)hist[i], (double)n);   // count / n
  __syncthreads();
  if (threadIdx.x == 0) {                    // the running sum is sequential, as get_percentile adds it
    const double bw = __ddiv_rn(range, 256.0);
    double running = 0.0;
    int lo_bin = -1, hi_bin = 255;
    for (int i = 0; i < 256; ++i) {
      running = __dadd_rn(running, terms[i]);
      if (lo_bin < 0 && running >= 0.02) lo_bin = i;
      if (running >= 0.98) { hi_bin = i; break; }
    }
    if (lo_bin < 0) lo_bin = hi_bin;
    const float lo = (float)__dadd_rn(__dmul_rn((double)(lo_bin + 1), bw), mn);
    const float hi = (float)__dadd_rn(__dmul_rn((double)(hi_bin + 1), bw), mn);
    red_d[8] = (double)lo;
    red_d[9] = (double)hi;
    red_d[10] = hi == lo ? 0.0 : __ddiv_rn(255.0, (double)__fsub_rn(hi, lo));
  }
  __syncthreads();
  const float lo = (float)red_d[8], hi = (float)red_d[9];
  const double ratio = red_d[10];
  for (int i = threadIdx.x; i < n; i += PH_THREADS) {
    const float v = pat[i];
    const float c = v > hi ? hi : (v < lo ? lo : v);
    const float o = (float)__dadd_rn(__dmul_rn((double)__fsub_rn(c, lo), ratio), 0.0);
    pat[i] = (float)(ph_toint((double)o) & 0xff);
  }
  __syncthreads();
}

// subpixel_phase_2d for one pixel per workgroup (PhaseSubpixelView.cc:231-326), in place.
// LDS (floats): twiddles 6 (C + R), the left spectrum 2 R C, the cross spectrum 2 R C, scratch max(4 R C, 2 up C).
__global__ void __launch_bounds__(PH_THREADS)
phase_refine_kernel(ph_args a) {
  extern __shared__ float sm[];
  __shared__ float red_v[PH_THREADS / 64];
  __shared__ int red_i[PH_THREADS / 64];
  __shared__ unsigned hist[256];
  __shared__ double terms[256];
  __shared__ double red_d[11];
  const int pix = blockIdx.x;
  const int y = a.y0 + pix / a.rw, x = a.x0 + pix % a.rw;
  const size_t p = (size_t)y * a.w + x;
  if (!a.v[p]) return;                       // the whole workgroup: skipped by the reference
  const int C = a.kx, R = a.ky, n = R * C, khw = C / 2, khh = R / 2;
  float* twc = sm;
  float* twr = twc + 2 * C;
  float* tw2c = twr + 2 * R;
  float* tw2r = tw2c + 4 * C;
  float* FL = tw2r + 4 * R;
  float* X = FL + 2 * n;
  float* S = X + 2 * n;
  for (int i = threadIdx.x; i < 6 * (C + R); i += PH_THREADS) sm[i] = a.tw[i];
  const float dx0 = a.dx[p], dy0 = a.dy[p];
  for (int i = threadIdx.x; i < n; i += PH_THREADS) {
    const int j = i / C, ii = i - j * C;
    S[i] = a.L[(size_t)(y - khh + j) * a.w + x - khw + ii];
  }
  __syncthreads();
  ph_to_u8(S, n, hist, terms, red_d);
  ph_forward(S, S + n, twc, twr, R, C, nullptr, FL);
  // the right window: the left window moved by Vector2i(d) (truncation); first crop through BilinearInterpolation at
  // integer positions = the zero-extended pixel
  const int rwx = x - khw + (int)dx0, rwy = y - khh + (int)dy0;
  for (int i = threadIdx.x; i < n; i += PH_THREADS) {
    const int j = i / C, ii = i - j * C;
    S[i] = ph_zero(a.R, a.w, a.h, rwx + ii, rwy + j);
  }
  __syncthreads();
  ph_to_u8(S, n, hist, terms, red_d);
  ph_forward(S, S + n, twc, twr, R, C, FL, X);
  const float2 d = ph_correlate(X, S, tw2c, tw2r, R, C, a.invs, a.c1, red_v, red_i);
  __syncthreads();
  // crop(translate(right, d, ZeroEdgeExtension, BicubicInterpolation), right_window)
  for (int i = threadIdx.x; i < n; i += PH_THREADS) {
    const int j = i / C, ii = i - j * C;
    S[i] = ph_bicubic(a.R, a.w, a.h, __dsub_rn((double)(rwx + ii), (double)d.x), __dsub_rn((double)(rwy + j), (double)d.y));
  }
  __syncthreads();
  ph_to_u8(S, n, hist, terms, red_d);
  ph_forward(S, S + n, twc, twr, R, C, FL, X);
  const float2 d2 = ph_correlate(X, S, tw2c, tw2r, R, C, a.invs, a.c2, red_v, red_i);
  if (threadIdx.x == 0) {
    const float ex = __fadd_rn(d.x, d2.x), ey = __fadd_rn(d.y, d2.y);
    double nn = 0.0;                         // norm_2: float squares summed in double, stored as float, sqrt in double
    nn = __dadd_rn(nn, (double)__fmul_rn(ex, ex));
    nn = __dadd_rn(nn, (double)__fmul_rn(ey, ey));
    if (__dsqrt_rn((double)(float)nn) > 3.0 || isnan(ex) || isnan(ey)) {
      a.v[p] = 0;
      atomicAdd(a.counters + 1, 1ull);
    } else {
      a.dx[p] = __fsub_rn(dx0, ex);
      a.dy[p] = __fsub_rn(dy0, ey);
    }
    atomicAdd(a.counters, 1ull);
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------

struct ph_host_call {
  int pad = 0, up = 0, mxc = 0, mxr = 0;
  float dft_shift = 0.0f;
  std::vector<float2> ec, er;
};

// the exp kernel table of partial_upsample_dft for an N-long axis at pad factor `pad`: the reference's own expression
void ph_exp_table(int N, int pad, int mx, std::vector<float2>& tab) {
  const std::complex<float> neg_i(0, -1);
  const float two_pi = 2.0 * M_PI;
  const std::complex<float> constant = neg_i * two_pi / static_cast<float>(N * pad);
  tab.resize((size_t)2 * mx + 1);
  for (int m = -mx; m <= mx; ++m) {
    const std::complex<float> e = std::exp(std::complex<float>((float)m, 0.0f) * constant);
    tab[(size_t)(m + mx)] = make_float2(e.real(), e.imag());
  }
}

// Largest |m| = |freq * (j - offset)| a call can form: |freq| <= N / 2, j < up, |offset| <= dft_shift + N pad / 2 + 2.
int ph_exp_bound(int N, int pad, int up, float dft_shift) {
  return (N / 2) * (up + (int)dft_shift + (N * pad + 1) / 2 + 3);
}

void ph_setup_call(int kx, int ky, int pad, ph_host_call& c) {
  c.pad = pad;
  if (pad <= 2) return;
  const float pr = (float)pad * 1.5f;
  c.up = (int)std::ceil((double)pr);
  c.dft_shift = (float)std::floor(std::ceil((double)pr) / 2);
  c.mxc = ph_exp_bound(kx, pad, c.up, c.dft_shift);
  c.mxr = ph_exp_bound(ky, pad, c.up, c.dft_shift);
  ph_exp_table(kx, pad, c.mxc, c.ec);
  ph_exp_table(ky, pad, c.mxr, c.er);
}

void ph_twiddles(int n, std::vector<float>& out) {
  const size_t b = out.size();
  out.resize(b + 2 * (size_t)n);
  for (int k = 0; k < n; ++k) {
    const double ang = 2.0 * M_PI * (double)k / (double)n;
    out[b + k] = (float)std::cos(ang);
    out[b + n + k] = (float)std::sin(ang);
  }
}

size_t ph_lds_bytes(int kx, int ky, int up_max) {
  const size_t n = (size_t)kx * ky;
  return 4 * (6 * (size_t)(kx + ky) + 4 * n + std::max(4 * n, 2 * (size_t)up_max * kx));
}

struct ph_state {
  ph_args base;
};

int ph_refine_level(vwgpu_ctx* ctx, const vwgpu_pyr_level_view& lv, int kx, int ky, int x0, int y0, int x1, int y1, void* user) {
  ph_state* st = static_cast<ph_state*>(user);
  ph_args a = st->base;
  a.L = lv.L; a.R = lv.R; a.dx = lv.dx; a.dy = lv.dy; a.v = lv.v;
  a.w = lv.w; a.h = lv.h;
  a.x0 = x0; a.y0 = y0; a.rw = x1 - x0;
  const long long npix = (long long)(x1 - x0) * (y1 - y0);
  const size_t lds = ph_lds_bytes(kx, ky, std::max(a.c1.up, a.c2.up));
  vwgpu_prof_scope ps(ctx, "phase_refine");
  // whole rows per launch: a launch holds at most 2^32 - 1 work-items in x, so at most (2^32 - 1) / PH_THREADS workgroups
  const long long max_rows = std::max<long long>(1, (0xffffffffLL / PH_THREADS) / a.rw);
  for (long long p0 = 0; p0 < npix; p0 += (long long)a.rw * max_rows) {
    const long long rows = std::min<long long>((npix - p0) / a.rw, max_rows);
    ph_args b = a;
    b.y0 = y0 + (int)(p0 / a.rw);
    hipLaunchKernelGGL(phase_refine_kernel, dim3((unsigned)(rows * a.rw)), dim3(PH_THREADS), lds, ctx->stream, b);
  }
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int ph_check(vwgpu_ctx* ctx, const void* disp, int w, int h, ptrdiff_t& dstride, const void* left, ptrdiff_t& lstride,
             const void* right, int rw, int rh, ptrdiff_t& rstride, int mode, int kx, int ky, int accuracy, const int* tiles,
             int ntiles, const void* out, ptrdiff_t& ostride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!disp || !left || !right || !out || w <= 0 || h <= 0 || rw <= 0 || rh <= 0 || ntiles < 0 || (ntiles > 0 && !tiles))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "phase_subpixel: empty image or null pointer");
  if (kx < 1 || ky < 1 || kx % 2 != 1 || ky % 2 != 1)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "phase_subpixel: Kernel input not sized with odd values.");
  if (mode != VWGPU_PREFILTER_NONE && mode != VWGPU_PREFILTER_MEANSUB && mode != VWGPU_PREFILTER_LOG)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "phase_subpixel: unknown prefilter mode %d", mode);
  if (kx > PH_MAX_KERNEL || ky > PH_MAX_KERNEL)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "phase_subpixel: kernel %d x %d is larger than %d x %d", kx, ky, PH_MAX_KERNEL,
                      PH_MAX_KERNEL);
  if (accuracy > PH_MAX_ACCURACY)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "phase_subpixel: accuracy %d is above %d", accuracy, PH_MAX_ACCURACY);
  if (dstride == 0) dstride = w;
  if (ostride == 0) ostride = w;
  if (lstride == 0) lstride = w;
  if (rstride == 0) rstride = rw;
  if (dstride < w || ostride < w || lstride < w || rstride < rw)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "phase_subpixel: row stride smaller than row width");
  for (int t = 0; t < ntiles; ++t) {
    const int* b = tiles + 4 * t;
    if (b[2] <= 0 || b[3] <= 0 || b[0] < 0 || b[1] < 0 || b[0] > w - b[2] || b[1] > h - b[3])
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "phase_subpixel: tile %d {%d, %d, %d, %d} is not inside the %d x %d image",
                        t, b[0], b[1], b[2], b[3], w, h);
  }
  return VWGPU_OK;
}

// tables, counters, the tile loop, the stats
int ph_run(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride, const float* d_left, ptrdiff_t lstride,
           const float* d_right, int rw, int rh, ptrdiff_t rstride, int mode, float width, int kx, int ky, int levels,
           int accuracy, const int* tiles, int ntiles, float* d_out, ptrdiff_t ostride, long long* stats) {
  ph_host_call c1, c2;
  ph_setup_call(kx, ky, accuracy / 2, c1);     // the first call gets accuracy / 2 (integer division)
  ph_setup_call(kx, ky, accuracy, c2);
  std::vector<float> tw;
  ph_twiddles(kx, tw);
  ph_twiddles(ky, tw);
  ph_twiddles(2 * kx, tw);
  ph_twiddles(2 * ky, tw);
  const size_t twb = vwgpu_align_up(tw.size() * 4, 256);
  const size_t b1c = vwgpu_align_up(c1.ec.size() * 8, 256), b1r = vwgpu_align_up(c1.er.size() * 8, 256);
  const size_t b2c = vwgpu_align_up(c2.ec.size() * 8, 256), b2r = vwgpu_align_up(c2.er.size() * 8, 256);
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, 256 + twb + b1c + b1r + b2c + b2r);
  if (rc) return rc;
  char* base = static_cast<char*>(ctx->scratch.base);
  unsigned long long* d_counters = reinterpret_cast<unsigned long long*>(base);
  float* d_tw = reinterpret_cast<float*>(base + 256);
  float2* e1c = reinterpret_cast<float2*>(base + 256 + twb);
  float2* e1r = reinterpret_cast<float2*>(base + 256 + twb + b1c);
  float2* e2c = reinterpret_cast<float2*>(base + 256 + twb + b1c + b1r);
  float2* e2r = reinterpret_cast<float2*>(base + 256 + twb + b1c + b1r + b2c);
  VWGPU_HIP(ctx, hipMemsetAsync(d_counters, 0, 16, ctx->stream));
  VWGPU_HIP(ctx, hipMemcpyAsync(d_tw, tw.data(), tw.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  if (!c1.ec.empty()) {
    VWGPU_HIP(ctx, hipMemcpyAsync(e1c, c1.ec.data(), c1.ec.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    VWGPU_HIP(ctx, hipMemcpyAsync(e1r, c1.er.data(), c1.er.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  if (!c2.ec.empty()) {
    VWGPU_HIP(ctx, hipMemcpyAsync(e2c, c2.ec.data(), c2.ec.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    VWGPU_HIP(ctx, hipMemcpyAsync(e2r, c2.er.data(), c2.er.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  ph_state st{};
  ph_args& a = st.base;
  a.kx = kx; a.ky = ky;
  a.tw = d_tw;
  a.invs = (float)(1.0 / (4.0 * ky * kx));
  a.c1 = ph_call{c1.pad, c1.up, c1.dft_shift, c1.mxc, c1.mxr, e1c, e1r};
  a.c2 = ph_call{c2.pad, c2.up, c2.dft_shift, c2.mxc, c2.mxr, e2c, e2r};
  a.counters = d_counters;
  const vwgpu_pyr_refiner refiner{ph_refine_level, &st};
  rc = vwgpu_pyramid_subpixel_tiles(ctx, d_disp, w, h, dstride, d_left, lstride, d_right, rw, rh, rstride, mode, width, kx, ky,
                                    levels, VWGPU_SUBPIXEL_PHASE, &refiner, tiles, ntiles, d_out, ostride, nullptr);
  if (rc) return rc;
  unsigned long long cnt[2] = {0, 0};
  VWGPU_HIP(ctx, hipMemcpyAsync(cnt, d_counters, 16, hipMemcpyDeviceToHost, ctx->stream));
  VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));   // also keeps the host tables alive until the copies are done
  if (stats) {
    stats[0] = (long long)cnt[0];
    stats[1] = (long long)cnt[1];
    stats[2] = ntiles;
  }
  return VWGPU_OK;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------

extern "C" {

int vwgpu_phase_subpixel_dev(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride,
                             const float* d_left, ptrdiff_t lstride, const float* d_right, int rw, int rh, ptrdiff_t rstride,
                             int mode, float width, int kx, int ky, int levels, int accuracy, const int* tiles, int ntiles,
                             float* d_out, ptrdiff_t ostride, long long* stats) {
  int rc = ph_check(ctx, d_disp, w, h, dstride, d_left, lstride, d_right, rw, rh, rstride, mode, kx, ky, accuracy, tiles, ntiles,
                    d_out, ostride);
  if (rc) return rc;
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  if (ntiles == 0) return VWGPU_OK;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return ph_run(ctx, d_disp, w, h, dstride, d_left, lstride, d_right, rw, rh, rstride, mode, width, kx, ky, levels < 0 ? 0 : levels,
                accuracy, tiles, ntiles, d_out, ostride, stats);
}

int vwgpu_phase_subpixel(vwgpu_ctx* ctx, const float* disp, int w, int h, ptrdiff_t dstride,
                         const float* left, ptrdiff_t lstride, const float* right, int rw, int rh, ptrdiff_t rstride,
                         int mode, float width, int kx, int ky, int levels, int accuracy, const int* tiles, int ntiles,
                         float* out, ptrdiff_t ostride, long long* stats) {
  int rc = ph_check(ctx, disp, w, h, dstride, left, lstride, right, rw, rh, rstride, mode, kx, ky, accuracy, tiles, ntiles, out,
                    ostride);
  if (rc) return rc;
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  if (ntiles == 0) return VWGPU_OK;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pd = st.add(disp, w, h, 12, dstride, VWGPU_STAGE_IN), po = st.add(out, w, h, 12, ostride, VWGPU_STAGE_INOUT);
  const int pl = st.add(left, w, h, 4, lstride, VWGPU_STAGE_IN), pr = st.add(right, rw, rh, 4, rstride, VWGPU_STAGE_IN);
  if ((rc = st.commit())) return rc;
  rc = ph_run(ctx, st.dev<float>(pd), w, h, w, st.dev<float>(pl), w, st.dev<float>(pr), rw, rh, rw, mode, width, kx, ky, levels < 0 ? 0 : levels,
              accuracy, tiles, ntiles, st.dev<float>(po), w, stats);
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
