// disparity_map.hip — what a caller does with a finished disparity map, the remaining parallel operators of
// src/vw/Stereo/DisparityMap.h: get_disparity_range (:48-66, Image/Statistics.h:193-224, :283-290), missing_pixel_image
// (:68-87), disparity_range_mask (:255-300), transform_disparities in both overloads (:1016-1057, :1190-1224),
// DisparityTransform as transform(right, DisparityTransform(d)) (:1164-1187, Image/Interpolation.h:76-110),
// intersect_mask_and_data (:1226-1249), disparity_subsample and disparity_upsample (:1251-1358).
// tests/refimpl/disparity_map_ref.cc restates them and DESIGN §4.17 lists what is reproduced.
//
// Pixels are PixelMask<Vector2i> / PixelMask<Vector2f> as three 32-bit words {dx, dy, valid != 0}; a lane reads and
// writes its pixel as one 12-byte access, a row of lanes covers a contiguous run of the row.  Every operator is one pass:
// one lane per output pixel, blocks of 64 x 4, rows beyond the grid's reach taken in a stride loop.  The range is one
// grid-stride reduction (lanes, LDS, one partial per workgroup) and a one-workgroup fold.
//
// Arithmetic is the reference's types in the reference's order; the Makefile's -ffp-contract=off keeps products and
// sums apart.
#include <climits>
#include <cmath>
#include <cstring>

#include "vwgpu_internal.h"

namespace {

constexpr int DM_BX = 64, DM_BY = 4;
constexpr int DM_RED_THREADS = 256, DM_RED_MAX_BLOCKS = 2048;   // 8 wavefronts per SIMD on 256 CUs
constexpr unsigned long long DM_NO_INDEX = ~0ull;

struct dm_px { uint32_t a, b, v; };   // one 12-byte pixel

template <int TYPE>
struct dm_t;
template <>
struct dm_t<VWGPU_DISPARITY_I32> {
  typedef int32_t chan;
  static __device__ bool valid(uint32_t v) { return v != 0; }
  static __device__ chan get(uint32_t a) { return (int32_t)a; }
  static __device__ double val(uint32_t a) { return (double)(int32_t)a; }
  static __device__ uint32_t from_double(double d) { return (uint32_t)(int32_t)d; }   // C++ conversion: toward zero
  static __device__ uint32_t twice(uint32_t a) { return a * 2u; }
  static __device__ uint32_t one() { return 0x7fffffffu; }   // validate(): ChannelRange<int32>::max()
  static __device__ chan lowest() { return INT_MIN; }
  static __device__ chan highest() { return INT_MAX; }
  static __device__ bool is_nan(chan) { return false; }
  static __device__ float nan_or(chan c) { return (float)c; }
};
template <>
struct dm_t<VWGPU_DISPARITY_F32> {
  typedef float chan;
  static __device__ bool valid(uint32_t v) { return __uint_as_float(v) != 0.f; }
  static __device__ chan get(uint32_t a) { return __uint_as_float(a); }
  static __device__ double val(uint32_t a) { return (double)__uint_as_float(a); }
  static __device__ uint32_t from_double(double d) { return __float_as_uint((float)d); }
  static __device__ uint32_t twice(uint32_t a) { return __float_as_uint(__uint_as_float(a) * 2.0f); }
  static __device__ uint32_t one() { return __float_as_uint(1.0f); }   // ChannelRange<float>::max()
  static __device__ chan lowest() { return -INFINITY; }
  static __device__ chan highest() { return INFINITY; }
  static __device__ bool is_nan(chan c) { return c != c; }
  static __device__ float nan_or(chan c) { return c; }
};

__device__ inline const dm_px* dm_at(const uint32_t* base, long long stride, int x, int y) {
  return reinterpret_cast<const dm_px*>(base) + ((long long)y * stride + x);
}
__device__ inline dm_px* dm_at(uint32_t* base, long long stride, int x, int y) {
  return reinterpret_cast<dm_px*>(base) + ((long long)y * stride + x);
}

// ---- get_disparity_range ------------------------------------------------------------------------------------------
// EWMinMaxAccumulator under PixelAccumulator: the first VALID pixel sets min = max, later ones enter through
// `if (arg < min) .. else if (arg > max)`, which for ordered values is plain min / max and never admits a NaN.  So the
// result is the min / max over the valid non-NaN components, except that a NaN component of the FIRST valid pixel in
// raster order stays (both extrema): the reduction also carries the smallest raster index of a valid pixel.
template <class C>
struct dm_range_acc {
  C mnx, mny, mxx, mxy;
  unsigned long long first;
};

template <int TYPE>
__device__ inline void dm_range_take(dm_range_acc<typename dm_t<TYPE>::chan>& r, typename dm_t<TYPE>::chan x,
                                     typename dm_t<TYPE>::chan y, unsigned long long idx) {
  r.mnx = x < r.mnx ? x : r.mnx;
  r.mxx = x > r.mxx ? x : r.mxx;
  r.mny = y < r.mny ? y : r.mny;
  r.mxy = y > r.mxy ? y : r.mxy;
  r.first = idx < r.first ? idx : r.first;
}
template <class C>
__device__ inline void dm_range_merge(dm_range_acc<C>& r, const dm_range_acc<C>& o) {
  r.mnx = o.mnx < r.mnx ? o.mnx : r.mnx;
  r.mxx = o.mxx > r.mxx ? o.mxx : r.mxx;
  r.mny = o.mny < r.mny ? o.mny : r.mny;
  r.mxy = o.mxy > r.mxy ? o.mxy : r.mxy;
  r.first = o.first < r.first ? o.first : r.first;
}
template <class C>
__device__ inline dm_range_acc<C> dm_range_shfl_down(const dm_range_acc<C>& r, int delta) {
  dm_range_acc<C> o;
  o.mnx = __shfl_down(r.mnx, delta);
  o.mny = __shfl_down(r.mny, delta);
  o.mxx = __shfl_down(r.mxx, delta);
  o.mxy = __shfl_down(r.mxy, delta);
  o.first = __shfl_down(r.first, delta);
  return o;
}

// lanes of a wavefront by shuffles, wavefronts through LDS; the result is valid in thread 0
template <class C>
__device__ inline void dm_range_block_reduce(dm_range_acc<C>& r, dm_range_acc<C>* lds) {
  const int ws = warpSize;
  for (int d = ws >> 1; d > 0; d >>= 1) {
    const dm_range_acc<C> o = dm_range_shfl_down(r, d);
    dm_range_merge(r, o);
  }
  const int lane = threadIdx.x % ws, wave = threadIdx.x / ws, nw = (blockDim.x + ws - 1) / ws;
  if (lane == 0) lds[wave] = r;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < nw; ++k) dm_range_merge(r, lds[k]);
}

template <int TYPE>
__global__ __launch_bounds__(DM_RED_THREADS) void dm_range_partial_kernel(const uint32_t* __restrict__ in, long long istride,
                                                                           int w, int h,
                                                                           dm_range_acc<typename dm_t<TYPE>::chan>* partial) {
  using T = dm_t<TYPE>;
  using C = typename T::chan;
  __shared__ dm_range_acc<C> lds[DM_RED_THREADS / 32];
  dm_range_acc<C> r{T::highest(), T::highest(), T::lowest(), T::lowest(), DM_NO_INDEX};
  const unsigned long long n = (unsigned long long)w * (unsigned long long)h;
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    // the raster index in 32 bits when it fits: a 64-bit division per pixel costs more than the pixel's traffic
    int x, y;
    if (n <= 0xffffffffull) {
      const unsigned q = (unsigned)i / (unsigned)w;
      y = (int)q;
      x = (int)((unsigned)i - q * (unsigned)w);
    } else {
      const unsigned long long q = i / (unsigned long long)w;
      y = (int)q;
      x = (int)(i - q * (unsigned long long)w);
    }
    const dm_px p = *dm_at(in, istride, x, y);
    if (T::valid(p.v)) dm_range_take<TYPE>(r, T::get(p.a), T::get(p.b), i);
  }
  dm_range_block_reduce(r, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

template <int TYPE>
__global__ __launch_bounds__(DM_RED_THREADS) void dm_range_fold_kernel(const dm_range_acc<typename dm_t<TYPE>::chan>* partial,
                                                                        int npartial, const uint32_t* __restrict__ in,
                                                                        long long istride, int w, float* out) {
  using T = dm_t<TYPE>;
  using C = typename T::chan;
  __shared__ dm_range_acc<C> lds[DM_RED_THREADS / 32];
  dm_range_acc<C> r{T::highest(), T::highest(), T::lowest(), T::lowest(), DM_NO_INDEX};
  for (int k = threadIdx.x; k < npartial; k += blockDim.x) dm_range_merge(r, partial[k]);
  dm_range_block_reduce(r, lds);
  if (threadIdx.x != 0) return;
  float res[4] = {0.f, 0.f, 0.f, 0.f};
  if (r.first != DM_NO_INDEX) {
    const unsigned long long q = r.first / (unsigned long long)w;
    const dm_px p = *dm_at(in, istride, (int)(r.first - q * (unsigned long long)w), (int)q);
    const C fx = T::get(p.a), fy = T::get(p.b);
    // a NaN component of the first valid pixel: min = max = NaN, and nothing compares below or above it afterwards
    res[0] = T::is_nan(fx) ? T::nan_or(fx) : (float)r.mnx;
    res[2] = T::is_nan(fx) ? T::nan_or(fx) : (float)r.mxx;
    res[1] = T::is_nan(fy) ? T::nan_or(fy) : (float)r.mny;
    res[3] = T::is_nan(fy) ? T::nan_or(fy) : (float)r.mxy;
  }
  out[0] = res[0]; out[1] = res[1]; out[2] = res[2]; out[3] = res[3];
}

// ---- per-pixel operators ------------------------------------------------------------------------------------------

#define DM_FOR_PIXELS(W, H)                                             \
  const int x = blockIdx.x * DM_BX + threadIdx.x;                       \
  if (x >= (W)) return;                                                 \
  for (int y = blockIdx.y * DM_BY + threadIdx.y; y < (H); y += gridDim.y * DM_BY)

// MissingPixelImageFunc (DisparityMap.h:73-81)
template <int TYPE>
__global__ __launch_bounds__(DM_BX * DM_BY) void dm_missing_kernel(const uint32_t* __restrict__ in, long long istride, int w, int h,
                                                                    uint8_t* __restrict__ out, long long ostride) {
  using T = dm_t<TYPE>;
  DM_FOR_PIXELS(w, h) {
    const bool ok = T::valid(dm_at(in, istride, x, y)->v);
    uint8_t* o = out + ((long long)y * ostride + x) * 3;
    o[0] = ok ? 200 : 255;
    o[1] = ok ? 200 : 0;
    o[2] = ok ? 200 : 0;
  }
}

// DisparityRangeMaskFunc (DisparityMap.h:276-283).  The bounds arrive as doubles that hold channel-type values: min[0],
// the lower bound of y (min[0] in reference semantics, :279), max[0] - 1 and max[1] - 1 computed in the channel type.
struct dm_mask_args {
  const uint32_t* in;
  long long istride;
  int w, h;
  long long x0, y0;
  double lox, loy, hix, hiy;
  uint32_t* out;
  long long ostride;
  unsigned long long* counter;
};
template <int TYPE>
__global__ __launch_bounds__(DM_BX * DM_BY) void dm_range_mask_kernel(dm_mask_args a) {
  using T = dm_t<TYPE>;
  DM_FOR_PIXELS(a.w, a.h) {
    dm_px p = *dm_at(a.in, a.istride, x, y);
    bool masked = false;
    if (T::valid(p.v)) {
      const double px = (double)(a.x0 + x) + T::val(p.a), py = (double)(a.y0 + y) + T::val(p.b);
      masked = px < a.lox || px >= a.hix || py < a.loy || py >= a.hiy;
    }
    if (masked) p.a = p.b = p.v = 0;
    *dm_at(a.out, a.ostride, x, y) = p;
    const unsigned long long m = __ballot(masked);
    if (m != 0 && ((threadIdx.y * DM_BX + threadIdx.x) & (warpSize - 1)) == (unsigned)(__ffsll((long long)m) - 1))
      atomicAdd(a.counter, (unsigned long long)__popcll(m));
  }
}

// TransformDisparitiesFunc (DisparityMap.h:1030-1043) with m = the applied matrix, and transform_disparities(do_round,
// subregion, T, disparity) (:1206-1221) with m = T; (bx, by) is the image position of pixel (0, 0).  The homography is
// HomographyTransform::forward (Math/Transform.h:383-387): w first, then the two quotients.
struct dm_transform_args {
  const uint32_t* in;
  long long istride;
  int w, h;
  long long bx, by;
  double m[9];
  int round, zero_invalid;
  uint32_t* out;
  long long ostride;
};
template <int TYPE>
__global__ __launch_bounds__(DM_BX * DM_BY) void dm_transform_kernel(dm_transform_args a) {
  using T = dm_t<TYPE>;
  DM_FOR_PIXELS(a.w, a.h) {
    dm_px p = *dm_at(a.in, a.istride, x, y);
    if (a.zero_invalid && !T::valid(p.v)) {
      p.a = p.b = p.v = 0;
    } else {
      const double lx = (double)(a.bx + x), ly = (double)(a.by + y);
      const double ex = lx + T::val(p.a), ey = ly + T::val(p.b);
      const double ww = a.m[6] * ex + a.m[7] * ey + a.m[8];
      const double qx = (a.m[0] * ex + a.m[1] * ey + a.m[2]) / ww, qy = (a.m[3] * ex + a.m[4] * ey + a.m[5]) / ww;
      double dx = qx - lx, dy = qy - ly;
      if (a.round) {
        dx = round(dx);
        dy = round(dy);
      }
      p.a = T::from_double(dx);
      p.b = T::from_double(dy);
    }
    *dm_at(a.out, a.ostride, x, y) = p;
  }
}

// IntersectPixelMaskData (DisparityMap.h:1234-1240)
template <int TYPE>
__global__ __launch_bounds__(DM_BX * DM_BY) void dm_intersect_kernel(const uint32_t* __restrict__ data, long long dstride,
                                                                      const uint32_t* __restrict__ mask, long long mstride, int w,
                                                                      int h, uint32_t* out, long long ostride) {
  using T = dm_t<TYPE>;
  DM_FOR_PIXELS(w, h) {
    const dm_px d = *dm_at(data, dstride, x, y), m = *dm_at(mask, mstride, x, y);
    const bool from_mask = !T::valid(d.v) && T::valid(m.v);
    dm_px o;   // word by word: a select between two structs goes through private memory
    o.a = from_mask ? m.a : d.a;
    o.b = from_mask ? m.b : d.b;
    o.v = from_mask ? m.v : d.v;
    *dm_at(out, ostride, x, y) = o;
  }
}

// DisparitySubsampleView::operator() over a ConstantEdgeExtension child (DisparityMap.h:1267-1305).  The accumulator is
// AccumulatorType<channel> (Core/FundamentalTypes.h:118, :121): int64 for int32 pixels, double for float pixels.  The
// first three taps are cast to it before the product, the other six are multiplied in the pixel's own type (:1273-1299).
template <int TYPE>
struct dm_sub;
template <>
struct dm_sub<VWGPU_DISPARITY_I32> {
  typedef long long acc;
  static __device__ acc wide(int wt, uint32_t a) { return (acc)wt * (acc)(int32_t)a; }
  static __device__ acc narrow(int wt, uint32_t a) { return (acc)(int32_t)((uint32_t)wt * a); }   // an int32 product
  static __device__ uint32_t quot(acc b, acc c2) { return (uint32_t)(int32_t)(b / c2); }
};
template <>
struct dm_sub<VWGPU_DISPARITY_F32> {
  typedef double acc;
  static __device__ acc wide(int wt, uint32_t a) { return (double)wt * (double)__uint_as_float(a); }
  static __device__ acc narrow(int wt, uint32_t a) { return (double)((float)wt * __uint_as_float(a)); }
  static __device__ uint32_t quot(acc b, acc c2) { return __float_as_uint((float)(b / c2)); }
};
template <int TYPE>
__global__ __launch_bounds__(DM_BX * DM_BY) void dm_subsample_kernel(const uint32_t* __restrict__ in, long long istride, int w, int h,
                                                                      uint32_t* __restrict__ out, long long ostride, int ow, int oh) {
  using T = dm_t<TYPE>;
  using S = dm_sub<TYPE>;
  DM_FOR_PIXELS(ow, oh) {
    const int ci = x << 1, cj = y << 1;
    const int ox[9] = {0, 1, 0, -1, 0, 1, -1, -1, 1}, oy[9] = {0, 0, 1, 0, -1, 1, -1, 1, -1}, wt[9] = {10, 5, 5, 5, 5, 2, 2, 2, 2};
    typename S::acc bx = 0, by = 0, count = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int sx = min(max(ci + ox[k], 0), w - 1), sy = min(max(cj + oy[k], 0), h - 1);
      const dm_px p = *dm_at(in, istride, sx, sy);
      if (!T::valid(p.v)) continue;
      count += wt[k];
      if (k < 3) {
        bx += S::wide(wt[k], p.a);
        by += S::wide(wt[k], p.b);
      } else {
        bx += S::narrow(wt[k], p.a);
        by += S::narrow(wt[k], p.b);
      }
    }
    dm_px o{0, 0, 0};
    if (count > 0) {
      o.a = S::quot(bx, count * 2);
      o.b = S::quot(by, count * 2);
      o.v = T::one();
    }
    *dm_at(out, ostride, x, y) = o;
  }
}

// DisparityUpsampleView::operator() (DisparityMap.h:1340-1343): the child pixel times 2 in the pixel's type; the mask
// word travels with it
template <int TYPE>
__global__ __launch_bounds__(DM_BX * DM_BY) void dm_upsample_kernel(const uint32_t* __restrict__ in, long long istride, int ow, int oh,
                                                                     uint32_t* __restrict__ out, long long ostride) {
  using T = dm_t<TYPE>;
  DM_FOR_PIXELS(ow, oh) {
    dm_px p = *dm_at(in, istride, x >> 1, y >> 1);
    p.a = T::twice(p.a);
    p.b = T::twice(p.b);
    *dm_at(out, ostride, x, y) = p;
  }
}

// transform(right, DisparityTransform(disparity)): TransformView over ZeroEdgeExtension and BilinearInterpolation.
// DisparityTransform::reverse (DisparityMap.h:1181-1186) reads the offset image by NearestPixelInterpolation over
// ZeroEdgeExtension at an integer position; BilinearInterpolationImpl (Image/Interpolation.h:83-105) in float.
struct dm_warp_args {
  const float* right;
  long long rstride;
  int rw, rh;
  const uint32_t* disp;
  long long dstride;
  int dw, dh;
  float* out;
  long long ostride;
};
__device__ inline float dm_zero_ext(const dm_warp_args& a, int x, int y) {
  return (x >= 0 && y >= 0 && x < a.rw && y < a.rh) ? a.right[(long long)y * a.rstride + x] : 0.0f;
}
__global__ __launch_bounds__(DM_BX * DM_BY) void dm_warp_kernel(dm_warp_args a) {
  using T = dm_t<VWGPU_DISPARITY_F32>;
  DM_FOR_PIXELS(a.rw, a.rh) {
    double pi = -1.0, pj = (double)y;
    if (x < a.dw && y < a.dh) {
      const dm_px d = *dm_at(a.disp, a.dstride, x, y);
      if (T::valid(d.v)) {
        pi = (double)x + T::val(d.a);
        pj = (double)y + T::val(d.b);
      }
    }
    float res = 0.0f;
    const double lim = 1073741824.0;   // 2^30: beyond it (or NaN) _floor's conversion to int32 is undefined; 0 by definition
    if (pi >= -lim && pi <= lim && pj >= -lim && pj <= lim) {
      const int xi = (int)floor(pi), yi = (int)floor(pj);
      if ((double)xi == pi && (double)yi == pj) {
        res = dm_zero_ext(a, xi, yi);
      } else {
        const float normx = (float)pi - (float)xi, normy = (float)pj - (float)yi;
        const float norm1mx = 1.0f - normx, norm1my = 1.0f - normy;
        res = dm_zero_ext(a, xi, yi) * norm1mx;
        res += dm_zero_ext(a, xi + 1, yi) * normx;
        res *= norm1my;
        float row = dm_zero_ext(a, xi, yi + 1) * norm1mx;
        row += dm_zero_ext(a, xi + 1, yi + 1) * normx;
        res += row * normy;
      }
    }
    a.out[(long long)y * a.ostride + x] = res;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------

dim3 dm_grid(int w, int h) {
  const long long gy = ((long long)h + DM_BY - 1) / DM_BY;
  return dim3((unsigned)((w + DM_BX - 1) / DM_BX), (unsigned)(gy < 65535 ? gy : 65535));
}
const dim3 dm_block(DM_BX, DM_BY);

#define DM_LAUNCH(KERNEL, TYPE, GRID, ...)                                                                             \
  do {                                                                                                                 \
    if ((TYPE) == VWGPU_DISPARITY_I32)                                                                                 \
      hipLaunchKernelGGL((KERNEL<VWGPU_DISPARITY_I32>), (GRID), dm_block, 0, ctx->stream, __VA_ARGS__);                \
    else                                                                                                               \
      hipLaunchKernelGGL((KERNEL<VWGPU_DISPARITY_F32>), (GRID), dm_block, 0, ctx->stream, __VA_ARGS__);                \
    VWGPU_HIP(ctx, hipGetLastError());                                                                                 \
  } while (0)

// the checks every entry shares; strides of 0 become the packed ones
int dm_check(vwgpu_ctx* ctx, const char* name, int type, const void* in, int w, int h, ptrdiff_t& istride, const void* out,
             ptrdiff_t& ostride, int ow, bool in_place_ok) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (type != VWGPU_DISPARITY_I32 && type != VWGPU_DISPARITY_F32)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: disparity type %d is neither int32 nor float", name, type);
  if (!in || !out || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: empty image or null pointer", name);
  if (!in_place_ok && in == out) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: input and output must be different images", name);
  if (istride == 0) istride = w;
  if (ostride == 0) ostride = ow;
  if (istride < w || ostride < ow) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
  return VWGPU_OK;
}

// -- range
int range_check(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t& istride, const void* r0, const void* r1) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (type != VWGPU_DISPARITY_I32 && type != VWGPU_DISPARITY_F32)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "get_disparity_range: disparity type %d is neither int32 nor float", type);
  if (!in || (!r0 && !r1) || w <= 0 || h <= 0)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "get_disparity_range: empty image or null pointer");
  if (istride == 0) istride = w;
  if (istride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "get_disparity_range: row stride smaller than row width");
  return VWGPU_OK;
}

template <int TYPE>
void range_launch(vwgpu_ctx* ctx, const uint32_t* d_in, int w, int h, ptrdiff_t istride, void* d_partial, int blocks, float* d_out) {
  typedef dm_range_acc<typename dm_t<TYPE>::chan> acc;
  hipLaunchKernelGGL((dm_range_partial_kernel<TYPE>), dim3(blocks), dim3(DM_RED_THREADS), 0, ctx->stream, d_in, (long long)istride, w, h,
                     static_cast<acc*>(d_partial));
  hipLaunchKernelGGL((dm_range_fold_kernel<TYPE>), dim3(1), dim3(DM_RED_THREADS), 0, ctx->stream, static_cast<const acc*>(d_partial),
                     blocks, d_in, (long long)istride, w, d_out);
}

int range_run(vwgpu_ctx* ctx, int type, const uint32_t* d_in, int w, int h, ptrdiff_t istride, float* d_range, float* host_range) {
  const unsigned long long n = (unsigned long long)w * (unsigned long long)h;
  const unsigned long long want = (n + DM_RED_THREADS - 1) / DM_RED_THREADS;
  const int blocks = (int)(want < (unsigned long long)DM_RED_MAX_BLOCKS ? want : (unsigned long long)DM_RED_MAX_BLOCKS);
  const size_t partial_bytes = vwgpu_align_up((size_t)DM_RED_MAX_BLOCKS * sizeof(dm_range_acc<float>), 256);
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, partial_bytes + 256);
  if (rc) return rc;
  char* base = static_cast<char*>(ctx->scratch.base);
  float* d_out = d_range ? d_range : reinterpret_cast<float*>(base + partial_bytes);
  {
    vwgpu_prof_scope ps(ctx, "get_disparity_range");
    if (type == VWGPU_DISPARITY_I32) range_launch<VWGPU_DISPARITY_I32>(ctx, d_in, w, h, istride, base, blocks, d_out);
    else range_launch<VWGPU_DISPARITY_F32>(ctx, d_in, w, h, istride, base, blocks, d_out);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (host_range) {
    VWGPU_HIP(ctx, hipMemcpyAsync(host_range, d_out, 4 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return VWGPU_OK;
}

// -- range mask
int mask_check(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t& istride, const double* mn, const double* mx,
               int semantics, const void* out, ptrdiff_t& ostride) {
  int rc = dm_check(ctx, "disparity_range_mask", type, in, w, h, istride, out, ostride, w, true);
  if (rc) return rc;
  if (!mn || !mx) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_range_mask: null min or max");
  if (semantics != VWGPU_RANGE_MASK_REFERENCE && semantics != VWGPU_RANGE_MASK_FIXED)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_range_mask: semantics %d is neither reference nor fixed", semantics);
  for (int k = 0; k < 2; ++k) {
    if (std::isnan(mn[k]) || std::isnan(mx[k])) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_range_mask: a bound is NaN");
    if (type == VWGPU_DISPARITY_I32 && (mn[k] < -2147483648.0 || mn[k] > 2147483647.0 || mx[k] < -2147483647.0 || mx[k] > 2147483647.0))
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_range_mask: a bound does not fit the int32 pixel");
  }
  return VWGPU_OK;
}

int mask_run(vwgpu_ctx* ctx, int type, const uint32_t* d_in, int w, int h, ptrdiff_t istride, int x0, int y0, const double* mn,
             const double* mx, int semantics, uint32_t* d_out, ptrdiff_t ostride, long long* stats) {
  if (stats) stats[0] = 0;
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, 256);
  if (rc) return rc;
  unsigned long long* d_counter = static_cast<unsigned long long*>(ctx->scratch.base);
  VWGPU_HIP(ctx, hipMemsetAsync(d_counter, 0, 256, ctx->stream));
  dm_mask_args a{};
  a.in = d_in; a.istride = istride; a.w = w; a.h = h; a.x0 = x0; a.y0 = y0;
  a.out = d_out; a.ostride = ostride; a.counter = d_counter;
  // m_min, m_max are the pixel's channel type (DisparityMap.h:267-274); `m_max - 1` is computed in it
  double lo[2], hi[2];
  for (int k = 0; k < 2; ++k) {
    if (type == VWGPU_DISPARITY_I32) {
      lo[k] = (double)(int32_t)mn[k];
      hi[k] = (double)((int32_t)mx[k] - 1);
    } else {
      const float one_less = (float)mx[k] - 1.0f;
      lo[k] = (double)(float)mn[k];
      hi[k] = (double)one_less;
    }
  }
  a.lox = lo[0];
  a.loy = semantics == VWGPU_RANGE_MASK_REFERENCE ? lo[0] : lo[1];   // :279 compares y with m_min[0]
  a.hix = hi[0];
  a.hiy = hi[1];
  {
    vwgpu_prof_scope ps(ctx, "disparity_range_mask");
    DM_LAUNCH(dm_range_mask_kernel, type, dm_grid(w, h), a);
  }
  if (stats) {
    unsigned long long cnt = 0;
    VWGPU_HIP(ctx, hipMemcpyAsync(&cnt, d_counter, 8, hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    stats[0] = (long long)cnt;
  }
  return VWGPU_OK;
}

// -- transform
int transform_check(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t& istride, const double* m, int mode,
                    const void* out, ptrdiff_t& ostride) {
  int rc = dm_check(ctx, "transform_disparities", type, in, w, h, istride, out, ostride, w, true);
  if (rc) return rc;
  if (!m) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "transform_disparities: null matrix");
  for (int k = 0; k < 9; ++k)
    if (std::isnan(m[k])) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "transform_disparities: the matrix holds a NaN");
  if (mode != VWGPU_TRANSFORM_FUNCTOR && mode != VWGPU_TRANSFORM_SUBREGION && mode != VWGPU_TRANSFORM_SUBREGION_ROUND)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "transform_disparities: unknown mode %d", mode);
  return VWGPU_OK;
}

int transform_run(vwgpu_ctx* ctx, int type, const uint32_t* d_in, int w, int h, ptrdiff_t istride, int x0, int y0, const double* m,
                  int mode, uint32_t* d_out, ptrdiff_t ostride) {
  dm_transform_args a{};
  a.in = d_in; a.istride = istride; a.w = w; a.h = h; a.bx = x0; a.by = y0;
  std::memcpy(a.m, m, sizeof(a.m));
  a.round = mode == VWGPU_TRANSFORM_SUBREGION_ROUND;
  a.zero_invalid = mode != VWGPU_TRANSFORM_FUNCTOR;
  a.out = d_out; a.ostride = ostride;
  vwgpu_prof_scope ps(ctx, "transform_disparities");
  DM_LAUNCH(dm_transform_kernel, type, dm_grid(w, h), a);
  return VWGPU_OK;
}

int warp_check(vwgpu_ctx* ctx, const void* right, int rw, int rh, ptrdiff_t& rstride, const void* disp, int dw, int dh,
               ptrdiff_t& dstride, const void* out, ptrdiff_t& ostride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!right || !disp || !out || rw <= 0 || rh <= 0 || dw <= 0 || dh <= 0)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_warp: empty image or null pointer");
  if (right == out || disp == out) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_warp: input and output must be different images");
  if (rstride == 0) rstride = rw;
  if (dstride == 0) dstride = dw;
  if (ostride == 0) ostride = rw;
  if (rstride < rw || dstride < dw || ostride < rw)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_warp: row stride smaller than row width");
  return VWGPU_OK;
}

int warp_run(vwgpu_ctx* ctx, const float* d_right, int rw, int rh, ptrdiff_t rstride, const uint32_t* d_disp, int dw, int dh,
             ptrdiff_t dstride, float* d_out, ptrdiff_t ostride) {
  dm_warp_args a{d_right, (long long)rstride, rw, rh, d_disp, (long long)dstride, dw, dh, d_out, (long long)ostride};
  vwgpu_prof_scope ps(ctx, "disparity_warp");
  hipLaunchKernelGGL(dm_warp_kernel, dm_grid(rw, rh), dm_block, 0, ctx->stream, a);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int intersect_check(vwgpu_ctx* ctx, int type, const void* data, const void* mask, int w, int h, ptrdiff_t& dstride, ptrdiff_t& mstride,
                    const void* out, ptrdiff_t& ostride) {
  int rc = dm_check(ctx, "intersect_mask_and_data", type, data, w, h, dstride, out, ostride, w, true);
  if (rc) return rc;
  if (!mask) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "intersect_mask_and_data: empty image or null pointer");
  if (mstride == 0) mstride = w;
  if (mstride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "intersect_mask_and_data: row stride smaller than row width");
  return VWGPU_OK;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) --------------------------------------------------------------------

extern "C" {

int vwgpu_get_disparity_range_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, float* d_range,
                                  float* host_range) {
  int rc = range_check(ctx, type, d_in, w, h, istride, d_range, host_range);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return range_run(ctx, type, static_cast<const uint32_t*>(d_in), w, h, istride, d_range, host_range);
}

int vwgpu_get_disparity_range(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, float* range) {
  int rc = range_check(ctx, type, in, w, h, istride, range, nullptr);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 12, istride, VWGPU_STAGE_IN), po = st.add(range, 4, 1, 4, 4, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = range_run(ctx, type, st.dev<uint32_t>(pi), w, h, w, st.dev<float>(po), nullptr);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_disparity_range_mask_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, int x0, int y0,
                                   const double* min, const double* max, int semantics, void* d_out, ptrdiff_t ostride,
                                   long long* stats) {
  int rc = mask_check(ctx, type, d_in, w, h, istride, min, max, semantics, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return mask_run(ctx, type, static_cast<const uint32_t*>(d_in), w, h, istride, x0, y0, min, max, semantics,
                  static_cast<uint32_t*>(d_out), ostride, stats);
}

int vwgpu_disparity_range_mask(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, int x0, int y0,
                               const double* min, const double* max, int semantics, void* out, ptrdiff_t ostride, long long* stats) {
  int rc = mask_check(ctx, type, in, w, h, istride, min, max, semantics, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 12, istride, VWGPU_STAGE_IN), po = st.add(out, w, h, 12, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = mask_run(ctx, type, st.dev<uint32_t>(pi), w, h, w, x0, y0, min, max, semantics, st.dev<uint32_t>(po), w, stats);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_transform_disparities_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, int x0, int y0,
                                    const double* matrix, int mode, void* d_out, ptrdiff_t ostride) {
  int rc = transform_check(ctx, type, d_in, w, h, istride, matrix, mode, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return transform_run(ctx, type, static_cast<const uint32_t*>(d_in), w, h, istride, x0, y0, matrix, mode,
                       static_cast<uint32_t*>(d_out), ostride);
}

int vwgpu_transform_disparities(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, int x0, int y0,
                                const double* matrix, int mode, void* out, ptrdiff_t ostride) {
  int rc = transform_check(ctx, type, in, w, h, istride, matrix, mode, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 12, istride, VWGPU_STAGE_IN), po = st.add(out, w, h, 12, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = transform_run(ctx, type, st.dev<uint32_t>(pi), w, h, w, x0, y0, matrix, mode, st.dev<uint32_t>(po), w);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_disparity_subsample_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, void* d_out,
                                  ptrdiff_t ostride) {
  const int ow = 1 + (w - 1) / 2, oh = 1 + (h - 1) / 2;
  int rc = dm_check(ctx, "disparity_subsample", type, d_in, w, h, istride, d_out, ostride, ow, false);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope ps(ctx, "disparity_subsample");
  DM_LAUNCH(dm_subsample_kernel, type, dm_grid(ow, oh), static_cast<const uint32_t*>(d_in), (long long)istride, w, h,
            static_cast<uint32_t*>(d_out), (long long)ostride, ow, oh);
  return VWGPU_OK;
}

int vwgpu_disparity_subsample(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, void* out, ptrdiff_t ostride) {
  const int ow = 1 + (w - 1) / 2, oh = 1 + (h - 1) / 2;
  int rc = dm_check(ctx, "disparity_subsample", type, in, w, h, istride, out, ostride, ow, false);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 12, istride, VWGPU_STAGE_IN), po = st.add(out, ow, oh, 12, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_disparity_subsample_dev(ctx, type, st.dev<uint32_t>(pi), w, h, w, st.dev<uint32_t>(po), ow);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_disparity_upsample_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, void* d_out,
                                 ptrdiff_t ostride) {
  if (ctx && (w > INT_MAX / 2 || h > INT_MAX / 2)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_upsample: the output size overflows");
  int rc = dm_check(ctx, "disparity_upsample", type, d_in, w, h, istride, d_out, ostride, 2 * w, false);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope ps(ctx, "disparity_upsample");
  DM_LAUNCH(dm_upsample_kernel, type, dm_grid(2 * w, 2 * h), static_cast<const uint32_t*>(d_in), (long long)istride, 2 * w, 2 * h,
            static_cast<uint32_t*>(d_out), (long long)ostride);
  return VWGPU_OK;
}

int vwgpu_disparity_upsample(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, void* out, ptrdiff_t ostride) {
  if (ctx && (w > INT_MAX / 2 || h > INT_MAX / 2)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_upsample: the output size overflows");
  int rc = dm_check(ctx, "disparity_upsample", type, in, w, h, istride, out, ostride, 2 * w, false);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 12, istride, VWGPU_STAGE_IN), po = st.add(out, 2 * w, 2 * h, 12, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_disparity_upsample_dev(ctx, type, st.dev<uint32_t>(pi), w, h, w, st.dev<uint32_t>(po), 2 * w);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_disparity_warp_dev(vwgpu_ctx* ctx, const float* d_right, int rw, int rh, ptrdiff_t rstride, const float* d_disparity, int dw,
                             int dh, ptrdiff_t dstride, float* d_out, ptrdiff_t ostride) {
  int rc = warp_check(ctx, d_right, rw, rh, rstride, d_disparity, dw, dh, dstride, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return warp_run(ctx, d_right, rw, rh, rstride, reinterpret_cast<const uint32_t*>(d_disparity), dw, dh, dstride, d_out, ostride);
}

int vwgpu_disparity_warp(vwgpu_ctx* ctx, const float* right, int rw, int rh, ptrdiff_t rstride, const float* disparity, int dw, int dh,
                         ptrdiff_t dstride, float* out, ptrdiff_t ostride) {
  int rc = warp_check(ctx, right, rw, rh, rstride, disparity, dw, dh, dstride, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pr = st.add(right, rw, rh, 4, rstride, VWGPU_STAGE_IN), pd = st.add(disparity, dw, dh, 12, dstride, VWGPU_STAGE_IN),
            po = st.add(out, rw, rh, 4, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = warp_run(ctx, st.dev<float>(pr), rw, rh, rw, st.dev<uint32_t>(pd), dw, dh, dw, st.dev<float>(po), rw);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_missing_pixel_image_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, unsigned char* d_out,
                                  ptrdiff_t ostride) {
  int rc = dm_check(ctx, "missing_pixel_image", type, d_in, w, h, istride, d_out, ostride, w, false);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope ps(ctx, "missing_pixel_image");
  DM_LAUNCH(dm_missing_kernel, type, dm_grid(w, h), static_cast<const uint32_t*>(d_in), (long long)istride, w, h, d_out,
            (long long)ostride);
  return VWGPU_OK;
}

int vwgpu_missing_pixel_image(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, unsigned char* out,
                              ptrdiff_t ostride) {
  int rc = dm_check(ctx, "missing_pixel_image", type, in, w, h, istride, out, ostride, w, false);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 12, istride, VWGPU_STAGE_IN), po = st.add(out, w, h, 3, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_missing_pixel_image_dev(ctx, type, st.dev<uint32_t>(pi), w, h, w, st.dev<unsigned char>(po), w);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_intersect_mask_and_data_dev(vwgpu_ctx* ctx, int type, const void* d_data, ptrdiff_t dstride, const void* d_mask,
                                      ptrdiff_t mstride, int w, int h, void* d_out, ptrdiff_t ostride) {
  int rc = intersect_check(ctx, type, d_data, d_mask, w, h, dstride, mstride, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope ps(ctx, "intersect_mask_and_data");
  DM_LAUNCH(dm_intersect_kernel, type, dm_grid(w, h), static_cast<const uint32_t*>(d_data), (long long)dstride,
            static_cast<const uint32_t*>(d_mask), (long long)mstride, w, h, static_cast<uint32_t*>(d_out), (long long)ostride);
  return VWGPU_OK;
}

int vwgpu_intersect_mask_and_data(vwgpu_ctx* ctx, int type, const void* data, ptrdiff_t dstride, const void* mask, ptrdiff_t mstride,
                                  int w, int h, void* out, ptrdiff_t ostride) {
  int rc = intersect_check(ctx, type, data, mask, w, h, dstride, mstride, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pd = st.add(data, w, h, 12, dstride, VWGPU_STAGE_IN), pm = st.add(mask, w, h, 12, mstride, VWGPU_STAGE_IN),
            po = st.add(out, w, h, 12, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_intersect_mask_and_data_dev(ctx, type, st.dev<uint32_t>(pd), w, st.dev<uint32_t>(pm), w, w, h, st.dev<uint32_t>(po), w);
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
