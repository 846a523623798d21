// disparity_filters.hip — the disparity post-filters of src/vw/Stereo/Algorithms.{h,cc}: disparity_median_filter
// (Algorithms.cc:26-67), disparity_neighbor_filter (Algorithms.cc:69-110), texture_measure (Algorithms.h:144-209) and
// texture_preserving_disparity_filter<float> (Algorithms.h:215-281); tests/refimpl/disparity_filters_ref.cc restates them
// and DESIGN §4.15 lists what is reproduced.  Every box of a call is filtered as an image of its own.
//
// The reference's three disparity filters run IN PLACE (`disparity_out = disparity_in` is a shallow copy), so a window
// sees filtered values above and to the left.  Two schedulers share three per-pixel functors (df_median_px,
// df_neighbor_px, df_smooth_px), which read pixels through an accessor:
//   * df_snapshot_kernel (VWGPU_FILTER_SNAPSHOT): every window reads the unmodified input.  One workgroup per 16 x 16
//     pixels of one box, the tile and its halo staged in LDS once (df_lds), one lane per output pixel, every pixel of the
//     box written once.
//   * df_inplace_kernel (VWGPU_FILTER_REFERENCE): the raster-order recursion.  Pixel (c, r) needs the new values of row
//     r - 1 up to column c + h and the old values below, so row r may run h + 1 columns behind row r - 1: with
//     t = c + (h + 1) r all pixels of equal t are independent.  One workgroup per box, lane j on row band + j at column
//     t - (h + 1) j, one __syncthreads() per step, bands of blockDim.x rows one after the other.  The lanes read and
//     write the image itself (df_glob): a workgroup's global stores are visible to its own lanes after the barrier.
//     Nothing waits on another workgroup and every loop bound is known at launch.
// texture_measure writes a separate image and has one kernel (df_texture_kernel).
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "vwgpu_internal.h"

namespace {

constexpr int DF_TX = 16, DF_TY = 16, DF_THREADS = DF_TX * DF_TY;
constexpr int DF_INPLACE_LANES = 256;
constexpr int DF_MAX_MEDIAN = 31, DF_MAX_TEXTURE = 31, DF_MAX_SMOOTH = 31;   // include/vwgpu.h states these limits
enum { DF_MEDIAN = 0, DF_NEIGHBOR = 1, DF_SMOOTH = 2 };

struct df_box {
  int x, y, w, h;
  int nbx, pad;            // 16 x 16 blocks across
  long long b0;            // the box's first block in the flattened block list
};

struct df_args {
  const uint32_t* in;      // {dx, dy, valid} per pixel, float or int32 words
  long long istride;       // pixels
  uint32_t* out;
  long long ostride;
  const float* tex;        // DF_SMOOTH: the texture image
  long long tstride;
  int half;                // halo of a tile / skew of the in-place schedule: the largest half window of the call
  float tmax, tscale;      // DF_SMOOTH: texture_max and max_kernel_size / texture_max (float)
  int maxk;
  const df_box* boxes;
  int nboxes;
  unsigned long long* counters;   // [0] pixels changed; texture_measure: the largest score's bits
};

__device__ inline int df_find(const df_box* t, int n, long long k) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid].b0 <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct df_px {
  uint32_t a, b, v;
};

// the staged tile of the snapshot kernel: pitch x pitch pixels from box position (ox, oy), clamped to the box when staged
struct df_lds {
  const uint32_t* t;
  int ox, oy, pitch;
  __device__ df_px get(int c, int r) const {
    const uint32_t* p = t + ((r - oy) * pitch + (c - ox)) * 3;
    return {p[0], p[1], p[2]};
  }
};

// the box itself in global memory (the in-place kernel), positions clamped to the box
struct df_glob {
  const uint32_t* img;     // the box's (0, 0)
  long long stride;
  int w, h;
  __device__ df_px get(int c, int r) const {
    c = min(max(c, 0), w - 1);
    r = min(max(r, 0), h - 1);
    const uint32_t* p = img + ((long long)r * stride + c) * 3;
    return {p[0], p[1], p[2]};
  }
};

__device__ inline bool df_fvalid(uint32_t v) { return __uint_as_float(v) != 0.f; }
// order-preserving integer key of a float (-0 sorts below +0; NaNs sort to the ends and are excluded before selection)
__device__ inline uint32_t df_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ inline float df_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// disparity_median_filter at one pixel (Algorithms.cc:38-65).  destructive_median (Math/Functors.h:393-398) sorts the valid
// values as doubles and picks the middle one or (a + b) / 2.0 of the two middle ones; a selection returns the same
// elements: bisection over the keys finds the largest v with #(keys < v) <= rank, both channels in one sweep per bit.
template <class A>
__device__ bool df_median_px(const A& acc, int c, int r, int w, int h, int half, float& ox, float& oy) {
  if (c < half || r < half || c >= w - half || r >= h - half) return false;
  if (!df_fvalid(acc.get(c, r).v)) return false;
  int n = 0;
  bool nan = false;
  for (int rr = r - half; rr <= r + half; ++rr)
    for (int cc = c - half; cc <= c + half; ++cc) {
      const df_px p = acc.get(cc, rr);
      if (!df_fvalid(p.v)) continue;
      n += 1;
      nan = nan || isnan(__uint_as_float(p.a)) || isnan(__uint_as_float(p.b));
    }
  if (nan || n == 0) return false;   // std::sort over NaN is undefined in the reference: the pixel is left as it is
  const int lo = (n - 1) >> 1, hi = n >> 1;
  uint32_t ax = 0, ay = 0;
  for (uint32_t bit = 0x80000000u; bit; bit >>= 1) {
    const uint32_t cx = ax | bit, cy = ay | bit;
    int nx = 0, ny = 0;
    for (int rr = r - half; rr <= r + half; ++rr)
      for (int cc = c - half; cc <= c + half; ++cc) {
        const df_px p = acc.get(cc, rr);
        if (!df_fvalid(p.v)) continue;
        nx += df_key(p.a) < cx;
        ny += df_key(p.b) < cy;
      }
    if (nx <= lo) ax = cx;
    if (ny <= lo) ay = cy;
  }
  if (hi == lo) {
    ox = df_unkey(ax);
    oy = df_unkey(ay);
    return true;
  }
  // even count: the element of rank hi is ax again when more than hi keys are <= ax, else the smallest key above it
  int lex = 0, ley = 0;
  uint32_t gx = 0xffffffffu, gy = 0xffffffffu;
  for (int rr = r - half; rr <= r + half; ++rr)
    for (int cc = c - half; cc <= c + half; ++cc) {
      const df_px p = acc.get(cc, rr);
      if (!df_fvalid(p.v)) continue;
      const uint32_t kx = df_key(p.a), ky = df_key(p.b);
      lex += kx <= ax;
      ley += ky <= ay;
      if (kx > ax) gx = min(gx, kx);
      if (ky > ay) gy = min(gy, ky);
    }
  const uint32_t bx = lex > hi ? ax : gx, by = ley > hi ? ay : gy;
  ox = (float)(((double)df_unkey(ax) + (double)df_unkey(bx)) / 2.0);
  oy = (float)(((double)df_unkey(ay) + (double)df_unkey(by)) / 2.0);
  return true;
}

// disparity_neighbor_filter at one pixel (Algorithms.cc:81-107): a valid neighbour counts the neighbours equal to it in
// dx, dy and validity; the first strictly larger count wins; five or more replace the centre whatever its validity
template <class A>
__device__ bool df_neighbor_px(const A& acc, int c, int r, int w, int h, uint32_t& ox, uint32_t& oy) {
  if (c < 1 || r < 1 || c >= w - 1 || r >= h - 1) return false;
  const int off[8][2] = {{-1, -1}, {0, -1}, {1, -1}, {-1, 0}, {1, 0}, {-1, 1}, {0, 1}, {1, 1}};
  df_px v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = acc.get(c + off[i][0], r + off[i][1]);
  int max_count = 0;
  uint32_t bx = 0, by = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (v[i].v == 0) continue;
    int count = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) count += (v[j].v != 0 && v[j].a == v[i].a && v[j].b == v[i].b) ? 1 : 0;
    if (count > max_count) {
      max_count = count;
      bx = v[i].a;
      by = v[i].b;
    }
  }
  if (max_count < 5) return false;
  ox = bx;
  oy = by;
  return true;
}

// texture_preserving_disparity_filter<float> at one pixel (Algorithms.h:240-277): the window size from the texture in
// float, the clamped window's valid pixels summed in double (r outer, c inner), the quotient narrowed to float
template <class A>
__device__ bool df_smooth_px(const A& acc, int c, int r, float t, float tmax, float tscale, int maxk, float& ox, float& oy) {
  if (!df_fvalid(acc.get(c, r).v) || t < 0) return false;
  float adjusted = tmax - t;
  if (adjusted < 0) adjusted = 0;
  const float prod = adjusted * tscale;
  if (!isfinite(t) || !isfinite(prod)) return false;   // floor -> int is undefined in the reference: left as it is
  int ks = (int)floorf(prod);
  if (ks % 2 == 0) ks += 1;
  if (ks < 3 || ks > maxk) return false;
  const int half = (ks - 1) / 2;
  double sx = 0.0, sy = 0.0, count = 0.0;
  for (int rr = r - half; rr <= r + half; ++rr)
    for (int cc = c - half; cc <= c + half; ++cc) {
      const df_px p = acc.get(cc, rr);
      if (!df_fvalid(p.v)) continue;
      sx += (double)__uint_as_float(p.a);
      sy += (double)__uint_as_float(p.b);
      count += 1.0;
    }
  if (count < 1.0) return false;
  ox = (float)(sx / count);
  oy = (float)(sy / count);
  return true;
}

// one pixel of box B through accessor acc: whether it is replaced, and by what (the new pixel is valid)
template <int FILTER, class A>
__device__ inline bool df_pixel(const df_args& a, const df_box& B, const A& acc, int c, int r, uint32_t& nx, uint32_t& ny) {
  if (FILTER == DF_MEDIAN) {
    float fx, fy;
    if (!df_median_px(acc, c, r, B.w, B.h, a.half, fx, fy)) return false;
    nx = __float_as_uint(fx);
    ny = __float_as_uint(fy);
    return true;
  }
  if (FILTER == DF_NEIGHBOR) return df_neighbor_px(acc, c, r, B.w, B.h, nx, ny);
  float fx, fy;
  const float t = a.tex[(long long)(B.y + r) * a.tstride + B.x + c];
  if (!df_smooth_px(acc, c, r, t, a.tmax, a.tscale, a.maxk, fx, fy)) return false;
  nx = __float_as_uint(fx);
  ny = __float_as_uint(fy);
  return true;
}

// whether {nx, ny, valid} differs from the pixel it replaces in dx, dy (compared as numbers) or validity
template <int FILTER>
__device__ inline bool df_differs(const df_px& old, uint32_t nx, uint32_t ny) {
  if (FILTER == DF_NEIGHBOR) return !(old.v != 0 && old.a == nx && old.b == ny);
  return !(df_fvalid(old.v) && __uint_as_float(old.a) == __uint_as_float(nx) && __uint_as_float(old.b) == __uint_as_float(ny));
}

template <int FILTER>
__device__ inline uint32_t df_valid_word() { return FILTER == DF_NEIGHBOR ? 1u : __float_as_uint(1.0f); }

template <int FILTER>
__global__ __launch_bounds__(DF_THREADS) void df_snapshot_kernel(df_args a, long long blk_base) {
  extern __shared__ uint32_t df_tile[];
  const long long g = blk_base + blockIdx.x;
  const df_box B = a.boxes[df_find(a.boxes, a.nboxes, g)];
  const long long q = g - B.b0;
  const int x0 = (int)(q % B.nbx) * DF_TX, y0 = (int)(q / B.nbx) * DF_TY;
  const int pitch = DF_TX + 2 * a.half;
  const uint32_t* src = a.in + ((long long)B.y * a.istride + B.x) * 3;
  for (int o = threadIdx.x; o < pitch * pitch; o += DF_THREADS) {
    const int c = min(max(x0 - a.half + o % pitch, 0), B.w - 1), r = min(max(y0 - a.half + o / pitch, 0), B.h - 1);
    const uint32_t* p = src + ((long long)r * a.istride + c) * 3;
    df_tile[o * 3] = p[0];
    df_tile[o * 3 + 1] = p[1];
    df_tile[o * 3 + 2] = p[2];
  }
  __syncthreads();
  const df_lds acc{df_tile, x0 - a.half, y0 - a.half, pitch};
  const int c = x0 + threadIdx.x % DF_TX, r = y0 + threadIdx.x / DF_TX;
  int changed = 0;
  if (c < B.w && r < B.h) {
    const df_px old = acc.get(c, r);
    uint32_t nx = old.a, ny = old.b, nv = old.v;
    if (df_pixel<FILTER>(a, B, acc, c, r, nx, ny)) {
      nv = df_valid_word<FILTER>();
      changed = df_differs<FILTER>(old, nx, ny);
    }
    uint32_t* o = a.out + ((long long)(B.y + r) * a.ostride + B.x + c) * 3;
    o[0] = nx;
    o[1] = ny;
    o[2] = nv;
  }
  const int nc = __syncthreads_count(changed);
  if (threadIdx.x == 0 && nc) atomicAdd(a.counters, (unsigned long long)nc);
}

template <int FILTER>
__global__ __launch_bounds__(DF_INPLACE_LANES) void df_inplace_kernel(df_args a, int box0) {
  const df_box B = a.boxes[box0 + blockIdx.x];
  uint32_t* img = a.out + ((long long)B.y * a.ostride + B.x) * 3;
  const df_glob acc{img, a.ostride, B.w, B.h};
  const int lanes = blockDim.x, j = threadIdx.x, skew = a.half + 1;
  int changed = 0;
  for (int band = 0; band < B.h; band += lanes) {
    const int rows = min(lanes, B.h - band);
    const int steps = B.w + skew * (rows - 1);
    const int r = band + j;
    for (int t = 0; t < steps; ++t) {
      const int c = t - skew * j;
      if (j < rows && c >= 0 && c < B.w) {
        uint32_t nx, ny;
        if (df_pixel<FILTER>(a, B, acc, c, r, nx, ny)) {
          uint32_t* o = img + ((long long)r * a.ostride + c) * 3;
          changed += df_differs<FILTER>(df_px{o[0], o[1], o[2]}, nx, ny);
          o[0] = nx;
          o[1] = ny;
          o[2] = df_valid_word<FILTER>();
        }
      }
      __syncthreads();   // the step's stores are visible to the workgroup's next step
    }
  }
  if (changed) atomicAdd(a.counters, (unsigned long long)changed);
}

struct df_tex_args {
  const float* img;
  long long stride;
  float* out;
  long long ostride;
  int half;
  double gw, sw;
  const df_box* boxes;
  int nboxes;
  unsigned long long* counters;
};

// texture_measure (Algorithms.h:144-209) on a plain float image (every pixel valid).  The tile's clamped values and
// |dx| + |dy| of derivative_filter (kernel {0.5, 0, -0.5}, constant edge extension, the derivative images edge-extended
// again) are staged in LDS; each lane then runs the reference's two window loops in its order, sums in double.
__global__ __launch_bounds__(DF_THREADS) void df_texture_kernel(df_tex_args a, long long blk_base) {
  extern __shared__ float df_tex[];
  __shared__ unsigned int best;
  const long long g = blk_base + blockIdx.x;
  const df_box B = a.boxes[df_find(a.boxes, a.nboxes, g)];
  const long long q = g - B.b0;
  const int x0 = (int)(q % B.nbx) * DF_TX, y0 = (int)(q / B.nbx) * DF_TY;
  const int pitch = DF_TX + 2 * a.half;
  float* val = df_tex;
  float* grd = df_tex + pitch * pitch;
  const float* src = a.img + (long long)B.y * a.stride + B.x;
  if (threadIdx.x == 0) best = 0;
  for (int o = threadIdx.x; o < pitch * pitch; o += DF_THREADS) {
    const int c = min(max(x0 - a.half + o % pitch, 0), B.w - 1), r = min(max(y0 - a.half + o / pitch, 0), B.h - 1);
    const float v = src[(long long)r * a.stride + c];
    const float xl = src[(long long)r * a.stride + max(c - 1, 0)], xr = src[(long long)r * a.stride + min(c + 1, B.w - 1)];
    const float yu = src[(long long)max(r - 1, 0) * a.stride + c], yd = src[(long long)min(r + 1, B.h - 1) * a.stride + c];
    float dx = 0.0f, dy = 0.0f;
    dx = __fadd_rn(dx, __fmul_rn(-0.5f, xl));
    dx = __fadd_rn(dx, __fmul_rn(0.0f, v));
    dx = __fadd_rn(dx, __fmul_rn(0.5f, xr));
    dy = __fadd_rn(dy, __fmul_rn(-0.5f, yu));
    dy = __fadd_rn(dy, __fmul_rn(0.0f, v));
    dy = __fadd_rn(dy, __fmul_rn(0.5f, yd));
    val[o] = v;
    grd[o] = __fadd_rn(fabsf(dx), fabsf(dy));
  }
  __syncthreads();
  const int tx = threadIdx.x % DF_TX, ty = threadIdx.x / DF_TX;
  const int c = x0 + tx, r = y0 + ty, k = 2 * a.half + 1;
  if (c < B.w && r < B.h) {
    const float* v0 = val + ty * pitch + tx;
    const float* g0 = grd + ty * pitch + tx;
    double mean = 0.0, count = 0.0;
    for (int rr = 0; rr < k; ++rr)
      for (int cc = 0; cc < k; ++cc) {
        mean += (double)v0[rr * pitch + cc];
        count += 1.0;
      }
    mean /= count;
    double grad = 0.0, sd = 0.0;
    for (int rr = 0; rr < k; ++rr)
      for (int cc = 0; cc < k; ++cc) {
        grad += (double)g0[rr * pitch + cc];
        const double d = (double)v0[rr * pitch + cc] - mean;
        sd += d * d;
      }
    grad = grad / (2.0 * count);
    sd = sqrt(sd / count);
    const float score = (float)(grad * a.gw + sd * a.sw);
    a.out[(long long)(B.y + r) * a.ostride + B.x + c] = score;
    if (score > 0.0f) atomicMax(&best, __float_as_uint(score));   // positive floats order as their bits
  }
  __syncthreads();
  if (threadIdx.x == 0 && best) atomicMax(a.counters, (unsigned long long)best);
}

// ---- host side ---------------------------------------------------------------------------------------------------

int df_check_boxes(vwgpu_ctx* ctx, const char* name, int w, int h, const int* boxes, int nboxes) {
  if (nboxes < 0 || (nboxes > 0 && !boxes)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: null or negative box list", name);
  for (int t = 0; t < nboxes; ++t) {
    const int* b = boxes + 4 * t;
    if (b[2] <= 0 || b[3] <= 0 || b[0] < 0 || b[1] < 0 || b[0] > w - b[2] || b[1] > h - b[3])
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: box %d {%d, %d, %d, %d} is not inside the %d x %d image", name, t, b[0],
                        b[1], b[2], b[3], w, h);
  }
  // overlap: boxes sorted by their first row; a box is compared with those that start above its last row
  std::vector<int> idx((size_t)nboxes);
  std::iota(idx.begin(), idx.end(), 0);
  std::sort(idx.begin(), idx.end(), [&](int p, int q) { return boxes[4 * p + 1] < boxes[4 * q + 1]; });
  for (int i = 0; i < nboxes; ++i) {
    const int* p = boxes + 4 * idx[i];
    for (int j = i + 1; j < nboxes; ++j) {
      const int* q = boxes + 4 * idx[j];
      if (q[1] >= p[1] + p[3]) break;
      if (p[0] < q[0] + q[2] && q[0] < p[0] + p[2])
        return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: boxes %d and %d overlap", name, idx[i], idx[j]);
    }
  }
  return VWGPU_OK;
}

// device copies of the box table and the call's counter word; *nb: 16 x 16 blocks of all boxes; *area: their pixels
int df_tables(vwgpu_ctx* ctx, const int* boxes, int nboxes, df_box** d_boxes, unsigned long long** d_counters, long long* nb,
              long long* area) {
  std::vector<df_box> tab((size_t)nboxes);
  *nb = 0;
  *area = 0;
  for (int t = 0; t < nboxes; ++t) {
    df_box& B = tab[t];
    B.x = boxes[4 * t]; B.y = boxes[4 * t + 1]; B.w = boxes[4 * t + 2]; B.h = boxes[4 * t + 3];
    B.nbx = (B.w + DF_TX - 1) / DF_TX;
    B.pad = 0;
    B.b0 = *nb;
    *nb += (long long)B.nbx * ((B.h + DF_TY - 1) / DF_TY);
    *area += (long long)B.w * B.h;
  }
  const size_t tb = vwgpu_align_up(tab.size() * sizeof(df_box), 256);
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, 256 + tb);
  if (rc) return rc;
  char* base = static_cast<char*>(ctx->scratch.base);
  *d_counters = reinterpret_cast<unsigned long long*>(base);
  *d_boxes = reinterpret_cast<df_box*>(base + 256);
  VWGPU_HIP(ctx, hipMemsetAsync(base, 0, 256, ctx->stream));
  VWGPU_HIP(ctx, hipMemcpyAsync(*d_boxes, tab.data(), tab.size() * sizeof(df_box), hipMemcpyHostToDevice, ctx->stream));
  VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));   // keeps `tab` alive until the copy has read it
  return VWGPU_OK;
}

template <int FILTER>
int df_launch(vwgpu_ctx* ctx, const df_args& a, int semantics, long long nb, const char* name) {
  vwgpu_prof_scope ps(ctx, name);
  if (semantics == VWGPU_FILTER_SNAPSHOT) {
    const int pitch = DF_TX + 2 * a.half;
    const size_t lds = (size_t)pitch * pitch * 12;
    const long long max_blk = 0x7fffffffLL / DF_THREADS;
    for (long long b0 = 0; b0 < nb; b0 += max_blk)
      hipLaunchKernelGGL((df_snapshot_kernel<FILTER>), dim3((unsigned)std::min<long long>(nb - b0, max_blk)), dim3(DF_THREADS),
                         lds, ctx->stream, a, b0);
  } else {
    for (int b0 = 0; b0 < a.nboxes; b0 += 65535)
      hipLaunchKernelGGL((df_inplace_kernel<FILTER>), dim3((unsigned)std::min(a.nboxes - b0, 65535)), dim3(DF_INPLACE_LANES), 0,
                         ctx->stream, a, b0);
  }
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

struct df_call {
  int filter;
  int kernel_size;         // median
  const float* tex;        // smoothing
  ptrdiff_t tstride;
  float texture_max;
  int max_kernel_size;
};

const char* df_name(int filter) {
  return filter == DF_MEDIAN ? "disparity_median_filter" : filter == DF_NEIGHBOR ? "disparity_neighbor_filter"
                                                                                  : "texture_preserving_disparity_filter";
}

int df_check(vwgpu_ctx* ctx, const df_call& c, const void* in, int w, int h, ptrdiff_t& istride, int semantics, const int* boxes,
             int nboxes, const void* out, ptrdiff_t& ostride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  const char* name = df_name(c.filter);
  if (!in || !out || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: empty image or null pointer", name);
  if (semantics != VWGPU_FILTER_REFERENCE && semantics != VWGPU_FILTER_SNAPSHOT)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: semantics %d is neither reference nor snapshot", name, semantics);
  if (istride == 0) istride = w;
  if (ostride == 0) ostride = w;
  if (istride < w || ostride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
  if (in == out && (semantics == VWGPU_FILTER_SNAPSHOT || istride != ostride))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: input and output may be one image only in reference semantics", name);
  if (c.filter == DF_MEDIAN && c.kernel_size < 0)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: negative kernel_size %d", name, c.kernel_size);
  if (c.filter == DF_MEDIAN && c.kernel_size > DF_MAX_MEDIAN)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: kernel_size %d is larger than %d", name, c.kernel_size, DF_MAX_MEDIAN);
  if (c.filter == DF_SMOOTH) {
    if (!c.tex) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: null texture image", name);
    if (c.tstride != 0 && c.tstride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
    if (c.max_kernel_size < 0 || std::isnan(c.texture_max))
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: negative max_kernel_size or NaN texture_max", name);
    if (c.max_kernel_size > DF_MAX_SMOOTH)
      return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: max_kernel_size %d is larger than %d", name, c.max_kernel_size, DF_MAX_SMOOTH);
  }
  return df_check_boxes(ctx, name, w, h, boxes, nboxes);
}

// device images; d_in == d_out: in place (reference semantics only, checked)
int df_run(vwgpu_ctx* ctx, const df_call& c, const uint32_t* d_in, int w, int h, ptrdiff_t istride, int semantics,
           const int* boxes, int nboxes, uint32_t* d_out, ptrdiff_t ostride, long long* stats) {
  if (stats) stats[0] = 0;
  const bool idle = nboxes == 0 || (c.filter == DF_MEDIAN && c.kernel_size < 3) ||
                    (c.filter == DF_SMOOTH && (c.max_kernel_size < 3 || c.texture_max <= 0));
  df_box* d_boxes = nullptr;
  unsigned long long* d_counters = nullptr;
  long long nb = 0, area = 0;
  if (!idle) {
    int rc = df_tables(ctx, boxes, nboxes, &d_boxes, &d_counters, &nb, &area);
    if (rc) return rc;
  }
  // the snapshot kernel writes every pixel of every box; everything else starts as a copy of the input
  const bool covered = !idle && semantics == VWGPU_FILTER_SNAPSHOT && area == (long long)w * h;
  if (d_in != d_out && !covered)
    VWGPU_HIP(ctx, hipMemcpy2DAsync(d_out, (size_t)ostride * 12, d_in, (size_t)istride * 12, (size_t)w * 12, h,
                                    hipMemcpyDeviceToDevice, ctx->stream));
  if (idle) return VWGPU_OK;
  df_args a{};
  a.in = d_in; a.istride = istride; a.out = d_out; a.ostride = ostride;
  a.boxes = d_boxes; a.nboxes = nboxes; a.counters = d_counters;
  int rc;
  if (c.filter == DF_MEDIAN) {
    a.half = (c.kernel_size - 1) / 2;
    rc = df_launch<DF_MEDIAN>(ctx, a, semantics, nb, "disparity_median_filter");
  } else if (c.filter == DF_NEIGHBOR) {
    a.half = 1;
    rc = df_launch<DF_NEIGHBOR>(ctx, a, semantics, nb, "disparity_neighbor_filter");
  } else {
    a.half = (c.max_kernel_size - 1) / 2;
    a.tex = c.tex; a.tstride = c.tstride ? c.tstride : w;
    a.tmax = c.texture_max; a.maxk = c.max_kernel_size;
    a.tscale = c.max_kernel_size / c.texture_max;   // float, as Algorithms.h:222
    rc = df_launch<DF_SMOOTH>(ctx, a, semantics, nb, "texture_preserving_disparity_filter");
  }
  if (rc) return rc;
  if (stats) {
    unsigned long long cnt = 0;
    VWGPU_HIP(ctx, hipMemcpyAsync(&cnt, d_counters, 8, hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    stats[0] = (long long)cnt;
  }
  return VWGPU_OK;
}

int df_dev(vwgpu_ctx* ctx, const df_call& c, const void* d_in, int w, int h, ptrdiff_t istride, int semantics, const int* boxes,
           int nboxes, void* d_out, ptrdiff_t ostride, long long* stats) {
  int rc = df_check(ctx, c, d_in, w, h, istride, semantics, boxes, nboxes, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return df_run(ctx, c, static_cast<const uint32_t*>(d_in), w, h, istride, semantics, boxes, nboxes,
                static_cast<uint32_t*>(d_out), ostride, stats);
}

int df_host(vwgpu_ctx* ctx, df_call c, const void* in, int w, int h, ptrdiff_t istride, int semantics, const int* boxes,
            int nboxes, void* out, ptrdiff_t ostride, long long* stats) {
  int rc = df_check(ctx, c, in, w, h, istride, semantics, boxes, nboxes, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  // reference semantics run in place on the staged copy (the second piece is reserved all the same)
  const bool in_place = semantics == VWGPU_FILTER_REFERENCE;
  const int pi = st.add(in, w, h, 12, istride, VWGPU_STAGE_IN);
  const int po = st.add(out, w, h, 12, ostride, in_place ? VWGPU_STAGE_NONE : VWGPU_STAGE_OUT);
  const int pt = st.add(c.tex, w, h, 4, c.tstride ? c.tstride : w, VWGPU_STAGE_IN);
  if ((rc = st.commit())) return rc;
  if (c.tex) {
    c.tex = st.dev<float>(pt);
    c.tstride = w;
  }
  rc = df_run(ctx, c, st.dev<uint32_t>(pi), w, h, w, semantics, boxes, nboxes, st.dev<uint32_t>(in_place ? pi : po), w, stats);
  if (rc) return rc;
  if (in_place && (rc = st.download(pi, out, w, h, ostride))) return rc;
  return st.finish();
}

int tm_check(vwgpu_ctx* ctx, const void* img, int w, int h, ptrdiff_t& stride, int kernel_size, double gw, double sw,
             const int* boxes, int nboxes, const void* out, ptrdiff_t& ostride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!img || !out || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "texture_measure: empty image or null pointer");
  if (img == out) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "texture_measure: input and output must be different images");
  if (kernel_size < 1 || std::isnan(gw) || std::isnan(sw))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "texture_measure: kernel_size %d is not positive, or a weight is NaN", kernel_size);
  if (kernel_size > DF_MAX_TEXTURE)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "texture_measure: kernel_size %d is larger than %d", kernel_size, DF_MAX_TEXTURE);
  if (stride == 0) stride = w;
  if (ostride == 0) ostride = w;
  if (stride < w || ostride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "texture_measure: row stride smaller than row width");
  return df_check_boxes(ctx, "texture_measure", w, h, boxes, nboxes);
}

int tm_run(vwgpu_ctx* ctx, const float* d_img, int w, int h, ptrdiff_t stride, int kernel_size, double gw, double sw,
           const int* boxes, int nboxes, float* d_out, ptrdiff_t ostride, float* max_score) {
  if (max_score) *max_score = 0.0f;
  if (nboxes == 0) return VWGPU_OK;
  df_box* d_boxes = nullptr;
  unsigned long long* d_counters = nullptr;
  long long nb = 0, area = 0;
  int rc = df_tables(ctx, boxes, nboxes, &d_boxes, &d_counters, &nb, &area);
  if (rc) return rc;
  df_tex_args a{};
  a.img = d_img; a.stride = stride; a.out = d_out; a.ostride = ostride;
  a.half = (kernel_size - 1) / 2;
  a.gw = gw; a.sw = sw;
  a.boxes = d_boxes; a.nboxes = nboxes; a.counters = d_counters;
  {
    vwgpu_prof_scope ps(ctx, "texture_measure");
    const int pitch = DF_TX + 2 * a.half;
    const size_t lds = (size_t)pitch * pitch * 8;
    const long long max_blk = 0x7fffffffLL / DF_THREADS;
    for (long long b0 = 0; b0 < nb; b0 += max_blk)
      hipLaunchKernelGGL(df_texture_kernel, dim3((unsigned)std::min<long long>(nb - b0, max_blk)), dim3(DF_THREADS), lds,
                         ctx->stream, a, b0);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (max_score) {
    unsigned long long cnt = 0;
    VWGPU_HIP(ctx, hipMemcpyAsync(&cnt, d_counters, 8, hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned int bits = (unsigned int)cnt;
    std::memcpy(max_score, &bits, 4);
  }
  return VWGPU_OK;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------

extern "C" {

int vwgpu_disparity_median_filter_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, int kernel_size,
                                      int semantics, const int* boxes, int nboxes, float* d_out, ptrdiff_t ostride,
                                      long long* stats) {
  return df_dev(ctx, df_call{DF_MEDIAN, kernel_size, nullptr, 0, 0.f, 0}, d_in, w, h, istride, semantics, boxes, nboxes, d_out,
                ostride, stats);
}

int vwgpu_disparity_median_filter(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, int kernel_size,
                                  int semantics, const int* boxes, int nboxes, float* out, ptrdiff_t ostride, long long* stats) {
  return df_host(ctx, df_call{DF_MEDIAN, kernel_size, nullptr, 0, 0.f, 0}, in, w, h, istride, semantics, boxes, nboxes, out,
                 ostride, stats);
}

int vwgpu_disparity_neighbor_filter_dev(vwgpu_ctx* ctx, const int32_t* d_in, int w, int h, ptrdiff_t istride, int semantics,
                                        const int* boxes, int nboxes, int32_t* d_out, ptrdiff_t ostride, long long* stats) {
  return df_dev(ctx, df_call{DF_NEIGHBOR, 0, nullptr, 0, 0.f, 0}, d_in, w, h, istride, semantics, boxes, nboxes, d_out, ostride,
                stats);
}

int vwgpu_disparity_neighbor_filter(vwgpu_ctx* ctx, const int32_t* in, int w, int h, ptrdiff_t istride, int semantics,
                                    const int* boxes, int nboxes, int32_t* out, ptrdiff_t ostride, long long* stats) {
  return df_host(ctx, df_call{DF_NEIGHBOR, 0, nullptr, 0, 0.f, 0}, in, w, h, istride, semantics, boxes, nboxes, out, ostride,
                 stats);
}

int vwgpu_texture_preserving_disparity_filter_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride,
                                                  const float* d_texture, ptrdiff_t tstride, float texture_max,
                                                  int max_kernel_size, int semantics, const int* boxes, int nboxes,
                                                  float* d_out, ptrdiff_t ostride, long long* stats) {
  return df_dev(ctx, df_call{DF_SMOOTH, 0, d_texture, tstride, texture_max, max_kernel_size}, d_in, w, h, istride, semantics,
                boxes, nboxes, d_out, ostride, stats);
}

int vwgpu_texture_preserving_disparity_filter(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride,
                                              const float* texture, ptrdiff_t tstride, float texture_max, int max_kernel_size,
                                              int semantics, const int* boxes, int nboxes, float* out, ptrdiff_t ostride,
                                              long long* stats) {
  return df_host(ctx, df_call{DF_SMOOTH, 0, texture, tstride, texture_max, max_kernel_size}, in, w, h, istride, semantics, boxes,
                 nboxes, out, ostride, stats);
}

int vwgpu_texture_measure_dev(vwgpu_ctx* ctx, const float* d_image, int w, int h, ptrdiff_t stride, int kernel_size,
                              double gradient_weight, double stddev_weight, const int* boxes, int nboxes, float* d_out,
                              ptrdiff_t ostride, float* max_score) {
  int rc = tm_check(ctx, d_image, w, h, stride, kernel_size, gradient_weight, stddev_weight, boxes, nboxes, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return tm_run(ctx, d_image, w, h, stride, kernel_size, gradient_weight, stddev_weight, boxes, nboxes, d_out, ostride, max_score);
}

int vwgpu_texture_measure(vwgpu_ctx* ctx, const float* image, int w, int h, ptrdiff_t stride, int kernel_size,
                          double gradient_weight, double stddev_weight, const int* boxes, int nboxes, float* out,
                          ptrdiff_t ostride, float* max_score) {
  int rc = tm_check(ctx, image, w, h, stride, kernel_size, gradient_weight, stddev_weight, boxes, nboxes, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(image, w, h, 4, stride, VWGPU_STAGE_IN), po = st.add(out, w, h, 4, ostride, VWGPU_STAGE_INOUT);
  if ((rc = st.commit())) return rc;
  rc = tm_run(ctx, st.dev<float>(pi), w, h, w, kernel_size, gradient_weight, stddev_weight, boxes, nboxes, st.dev<float>(po), w, max_score);
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
