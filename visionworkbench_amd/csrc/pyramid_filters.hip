// pyramid_filters.hip — the disparity clean-up chain of the pyramid correlator, on its own and as entry points:
//   rm_outliers_using_thresh / disparity_cleanup_using_thresh   src/vw/Stereo/DisparityMap.h:318-441
//   disparity_mask                                               src/vw/Stereo/DisparityMap.h:97-253
//   disparity_blob_filter                                        src/vw/Stereo/CorrelationView.cc:242-271
// The level loops of pyramid.hip call the three vwgpu_launch_* functions.
#include <algorithm>
#include <cmath>

#include "vwgpu_internal.h"

namespace {

// RmOutliersUsingThreshFunc (src/vw/Stereo/DisparityMap.h:357-385) evaluated over the output domain
// [ox0, ox0+ow) x [oy0, oy0+oh) of the constant-edge-extended input.  A 32 x 8 output tile and its (2 hh + 1) x (2 hv + 1)
// neighbourhood rim are staged in LDS once (the direct version read 121 x 12 B per pixel through the L1: 0.3 ms per 1024^2 level).
// `fabs((double)(a - b)) <= pthr` on int32 differences is the unsigned compare |a - b| <= floor(pthr) (thr; `never` for a
// negative or NaN threshold); the match ratio is compared in float64 as the reference does.
// Packed form: when every valid disparity of the tile is below 2^13 in magnitude and thr < 2^13 (always, in a pyramid) the tile is
// ALSO staged as one dword per pixel — (dx + 2^14) | (dy + 2^14) << 16, 0xffffffff for an invalid pixel — and a neighbour is one LDS
// read and four instructions: t = n + (thr - c) per half (v_pk_add_u16: |n - c| <= thr  <=>  t <= 2 thr as unsigned 16-bit values —
// a negative n - c + thr wraps to more than 2^15, and the invalid code gives 65535 - (c + 2^14) + thr, between 2^15 and 2^16: it
// never passes), max with 2 thr per half, compare with the splat, add the carry.  The three-array form took
// ten instructions and three LDS reads per neighbour: 160 us of an 870 us SAD tile went into this filter.
// HH > 0: hh == hv == HH known at compile time (the loops unroll: the small levels of a pyramid are latency bound here).
template <int HH>
__global__ void __launch_bounds__(256)
rm_outliers_kernel(const int32_t* __restrict__ src, int w, int h, int hh, int hv, unsigned thr, int never, double rthr,
                   int32_t* __restrict__ dst, int ow, int oh, int ox0, int oy0, size_t src_tile = 0, size_t dst_tile = 0) {
  extern __shared__ int32_t rm_sm[];
  src += blockIdx.z * src_tile; dst += blockIdx.z * dst_tile;     // tile groups: blockIdx.z = the tile, its images at a fixed stride (ints)
  if (HH > 0) { hh = HH; hv = HH; }
  const int tw = 32 + 2 * hh, th = 8 + 2 * hv, tn = tw * th;
  int32_t* sx = rm_sm;
  int32_t* sy = rm_sm + tn;
  unsigned* pk = reinterpret_cast<unsigned*>(rm_sm + 2 * tn);
  uint8_t* sv = reinterpret_cast<uint8_t*>(rm_sm + 3 * tn);
  const int tid = threadIdx.y * 32 + threadIdx.x;
  const int bx = blockIdx.x * 32 + ox0 - hh, by = blockIdx.y * 8 + oy0 - hv;      // source coordinates of the tile's corner
  bool big = thr >= 8192u;
  // (three pixels per thread and batch: their nine loads are requested together — the plain loop waited for every pixel's three words)
  for (int i0 = tid; i0 < tn; i0 += 3 * 256) {
    int32_t d0[3], d1[3], d2[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int i = i0 + b * 256;
      const int ty = i / tw, tx = i - ty * tw;
      int x = bx + tx, y = by + ty;
      x = x < 0 ? 0 : (x >= w ? w - 1 : x);
      y = y < 0 ? 0 : (y >= h ? h - 1 : y);
      const int32_t* c = src + ((size_t)y * w + x) * 3;
      const bool in = i < tn;
      d0[b] = in ? c[0] : 0; d1[b] = in ? c[1] : 0; d2[b] = in ? c[2] : 0;
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int i = i0 + b * 256;
      if (i >= tn) break;
      const bool v = d2[b] != 0;
      sx[i] = d0[b]; sy[i] = d1[b]; sv[i] = v;
      if (v) big = big || d0[b] <= -8192 || d0[b] >= 8192 || d1[b] <= -8192 || d1[b] >= 8192;
      pk[i] = v ? ((unsigned)(d0[b] + 16384) & 0xffffu) | ((unsigned)(d1[b] + 16384) << 16) : 0xffffffffu;
    }
  }
  const bool wide = __syncthreads_or(big ? 1 : 0) != 0;         // (also the barrier behind the staging)
  const int ox = blockIdx.x * 32 + threadIdx.x, oy = blockIdx.y * 8 + threadIdx.y;
  if (ox >= ow || oy >= oh) return;
  const int ci = (threadIdx.y + hv) * tw + threadIdx.x + hh;
  int32_t r0 = sx[ci], r1 = sy[ci], r2 = 0;
  if (sv[ci]) {
    // the valid flag is written back as the source has it
    const int x = min(max(ox + ox0, 0), w - 1), y = min(max(oy + oy0, 0), h - 1);
    r2 = src[((size_t)y * w + x) * 3 + 2];
    int matched = 0;
    if (!never && !wide) {
      typedef unsigned short us2_t __attribute__((ext_vector_type(2)));
      const unsigned cb = ((thr - (unsigned)(r0 + 16384)) & 0xffffu) | ((thr - (unsigned)(r1 + 16384)) << 16);      // thr - c per half (mod 2^16)
      const unsigned lim = (2u * thr) | ((2u * thr) << 16);
      auto one = [&](unsigned n) __attribute__((always_inline)) {
        const us2_t t = __builtin_bit_cast(us2_t, n) + __builtin_bit_cast(us2_t, cb);
        const us2_t m = __builtin_elementwise_max(t, __builtin_bit_cast(us2_t, lim));
        matched += __builtin_bit_cast(unsigned, m) == lim ? 1 : 0;
      };
      if (HH > 0) {
#pragma unroll
        for (int yk = 0; yk <= 2 * HH; ++yk) {
          const unsigned* row = pk + (threadIdx.y + yk) * tw + threadIdx.x;
#pragma unroll
          for (int xk = 0; xk <= 2 * HH; ++xk) one(row[xk]);
        }
      } else {
        for (int yk = 0; yk <= 2 * hv; ++yk) {
          const unsigned* row = pk + (threadIdx.y + yk) * tw + threadIdx.x;
          for (int xk = 0; xk <= 2 * hh; ++xk) one(row[xk]);
        }
      }
    } else if (!never) {
      for (int yk = 0; yk <= 2 * hv; ++yk) {
        const int row = (threadIdx.y + yk) * tw + threadIdx.x;
        for (int xk = 0; xk <= 2 * hh; ++xk) {
          const int i = row + xk;
          const int d0 = r0 - sx[i], d1 = r1 - sy[i];                         // int32 wrap-around, as the reference's subtraction
          const unsigned a0 = d0 < 0 ? 0u - (unsigned)d0 : (unsigned)d0, a1 = d1 < 0 ? 0u - (unsigned)d1 : (unsigned)d1;
          matched += (sv[i] && a0 <= thr && a1 <= thr) ? 1 : 0;
        }
      }
    }
    const int total = (2 * hh + 1) * (2 * hv + 1);
    if (((double)matched / (double)total) < rthr) { r0 = r1 = r2 = 0; }
  }
  int32_t* o = dst + ((size_t)oy * ow + ox) * 3;
  o[0] = r0; o[1] = r1; o[2] = r2;
}

// The same filter without the LDS tile, for neighbourhoods too large for it (64 KB).
__global__ void rm_outliers_direct_kernel(const int32_t* __restrict__ src, int w, int h, int hh, int hv, double pthr, double rthr,
                                   int32_t* __restrict__ dst, int ow, int oh, int ox0, int oy0) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y * blockDim.y + threadIdx.y;
  if (ox >= ow || oy >= oh) return;
  auto at = [&](int x, int y) -> const int32_t* {
    x = x < 0 ? 0 : (x >= w ? w - 1 : x);
    y = y < 0 ? 0 : (y >= h ? h - 1 : y);
    return src + ((size_t)y * w + x) * 3;
  };
  const int x = ox + ox0, y = oy + oy0;
  const int32_t* c = at(x, y);
  int32_t r0 = c[0], r1 = c[1], r2 = c[2];
  if (r2) {
    int matched = 0, total = 0;
    for (int yk = -hv; yk <= hv; ++yk)
      for (int xk = -hh; xk <= hh; ++xk) {
        const int32_t* n = at(x + xk, y + yk);
        if (n[2] && fabs((double)(r0 - n[0])) <= pthr && fabs((double)(r1 - n[1])) <= pthr) matched++;
        total++;
      }
    if (((double)matched / (double)total) < rthr) { r0 = r1 = r2 = 0; }
  }
  int32_t* o = dst + ((size_t)oy * ow + ox) * 3;
  o[0] = r0; o[1] = r1; o[2] = r2;
}

// second pass of disparity_cleanup_using_thresh: functor (1,1,3.0,0.20) over the inner VIEW, which is given here on
// the domain padded by one pixel (DisparityMap.h:427-441).
__global__ void cleanup_outer_kernel(const int32_t* __restrict__ inner, int w, int h, int32_t* __restrict__ dst) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  const int pw = w + 2;
  const int32_t* c = inner + ((size_t)(y + 1) * pw + (x + 1)) * 3;
  int32_t r0 = c[0], r1 = c[1], r2 = c[2];
  if (r2) {
    int matched = 0;
    for (int yk = -1; yk <= 1; ++yk)
      for (int xk = -1; xk <= 1; ++xk) {
        const int32_t* n = inner + ((size_t)(y + 1 + yk) * pw + (x + 1 + xk)) * 3;
        if (n[2] && fabs((double)(r0 - n[0])) <= 3.0 && fabs((double)(r1 - n[1])) <= 3.0) matched++;
      }
    if (((double)matched / 9.0) < 0.20) { r0 = r1 = r2 = 0; }
  }
  int32_t* o = dst + ((size_t)y * w + x) * 3;
  o[0] = r0; o[1] = r1; o[2] = r2;
}

// DisparityMaskView::operator() (DisparityMap.h:132-155), in place.
__global__ void disparity_mask_kernel(int32_t* __restrict__ d, int w, int h, const uint8_t* __restrict__ m1,
                                      const uint8_t* __restrict__ m2, int m2w, int m2h) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= w || j >= h) return;
  int32_t* p = d + ((size_t)j * w + i) * 3;
  bool keep = m1[(size_t)j * w + i] != 0 && p[2] != 0;
  if (keep) {
    const int x = i + p[0], y = j + p[1];
    keep = !(x < 0 || x >= m2w || y < 0 || y >= m2h || m2[(size_t)y * m2w + x] == 0);
  }
  if (!keep) { p[0] = 0; p[1] = 0; p[2] = 0; }
}

// ---- blob filter (disparity_blob_filter, CorrelationView.cc:242-271): 8-connected components of the valid pixels by a
// lock-free union-find (roots = smallest pixel index), component sizes by atomics, components of <= area pixels erased.
__device__ __forceinline__ int cc_find(int* L, int x) {
  int p = L[x];
  while (p != x) { const int g = L[p]; L[x] = g; x = p; p = g; }     // path halving; racy writes only ever shorten paths
  return x;
}
__device__ __forceinline__ void cc_unite(int* L, int a, int b) {
  while (true) {
    a = cc_find(L, a); b = cc_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }                     // hang the larger root under the smaller one
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}
__global__ void cc_init_kernel(const int32_t* __restrict__ d, int n, int* __restrict__ label, int* __restrict__ size) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  label[i] = d[(size_t)i * 3 + 2] ? i : -1;
  size[i] = 0;
}
__global__ void cc_union_kernel(int* label, int w, int h) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  const int i = y * w + x;
  if (label[i] < 0) return;
  if (x > 0 && label[i - 1] >= 0) cc_unite(label, i, i - 1);
  if (y > 0) {
    if (label[i - w] >= 0) cc_unite(label, i, i - w);
    if (x > 0 && label[i - w - 1] >= 0) cc_unite(label, i, i - w - 1);
    if (x + 1 < w && label[i - w + 1] >= 0) cc_unite(label, i, i - w + 1);
  }
}
// the forest is final after the union kernel: read-only root walks (a compressing find here would race with the readers)
__device__ __forceinline__ int cc_root(const int* L, int x) {
  int p = L[x];
  while (p != x) { x = p; p = L[x]; }
  return x;
}
__global__ void cc_count_kernel(const int* __restrict__ label, int n, int* __restrict__ size) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || label[i] < 0) return;
  atomicAdd(&size[cc_root(label, i)], 1);
}
__global__ void cc_erase_kernel(int32_t* __restrict__ d, const int* __restrict__ label, const int* __restrict__ size, int n, int area) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || label[i] < 0) return;
  if (size[cc_root(label, i)] <= area) { d[(size_t)i * 3] = 0; d[(size_t)i * 3 + 1] = 0; d[(size_t)i * 3 + 2] = 0; }
}

inline dim3 grid2(int w, int h) { return dim3((w + 63) / 64, (h + 3) / 4); }
const dim3 kBlk(64, 4);

}  // namespace

int vwgpu_launch_disparity_filter(vwgpu_ctx* ctx, const int32_t* src, int w, int h, int hh, int hv, double pthr, double rthr,
                                  bool cleanup, int32_t* tmp_padded, int32_t* dst, bool inner_only, int tiles, size_t tile_ints) {
  // tiles > 1 (the tile groups of vwgpu_pyramid_group_impl): the same filter over `tiles` images at a fixed stride of tile_ints ints, for the
  // source, the padded intermediate and the destination alike — one launch (blockIdx.z); the second pass is the caller's (inner_only)
  if (hh < 0 || hv < 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity filter: negative half kernel");
  const size_t rm_lds = (size_t)(32 + 2 * hh) * (8 + 2 * hv) * 13;
  const bool direct = rm_lds > 64 * 1024;
  if (tiles > 1 && (direct || (cleanup && !inner_only))) return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "disparity filter: this form is not built for tile groups");
  const size_t ts = tiles > 1 ? tile_ints : 0;
  // fabs((double)int32 difference) <= pthr  <=>  |difference| <= floor(pthr)
  const int never = !(pthr >= 0.0);                                   // negative or NaN: nothing matches
  const unsigned thr = never ? 0u : (pthr >= 4294967295.0 ? 0xffffffffu : (unsigned)std::floor(pthr));
  auto rm_grid = [tiles](int ww, int hh2) { return dim3((unsigned)((ww + 31) / 32), (unsigned)((hh2 + 7) / 8), (unsigned)std::max(tiles, 1)); };
  if (!cleanup) {
    vwgpu_prof_scope ps(ctx, "rm_outliers");
    if (direct) hipLaunchKernelGGL(rm_outliers_direct_kernel, grid2(w, h), kBlk, 0, ctx->stream, src, w, h, hh, hv, pthr, rthr, dst, w, h, 0, 0);
    else if (hh == 5 && hv == 5) hipLaunchKernelGGL(rm_outliers_kernel<5>, rm_grid(w, h), dim3(32, 8), rm_lds, ctx->stream, src, w, h, hh, hv, thr, never, rthr, dst, w, h, 0, 0, ts, ts);
    else hipLaunchKernelGGL(rm_outliers_kernel<0>, rm_grid(w, h), dim3(32, 8), rm_lds, ctx->stream, src, w, h, hh, hv, thr, never, rthr, dst, w, h, 0, 0, ts, ts);
  } else {
    {
      vwgpu_prof_scope ps(ctx, "rm_outliers");
      if (direct) hipLaunchKernelGGL(rm_outliers_direct_kernel, grid2(w + 2, h + 2), kBlk, 0, ctx->stream, src, w, h, hh, hv, pthr, rthr,
                                     tmp_padded, w + 2, h + 2, -1, -1);
      else if (hh == 5 && hv == 5) hipLaunchKernelGGL(rm_outliers_kernel<5>, rm_grid(w + 2, h + 2), dim3(32, 8), rm_lds, ctx->stream, src, w, h, hh, hv, thr, never, rthr,
                                                      tmp_padded, w + 2, h + 2, -1, -1, ts, ts);
      else hipLaunchKernelGGL(rm_outliers_kernel<0>, rm_grid(w + 2, h + 2), dim3(32, 8), rm_lds, ctx->stream, src, w, h, hh, hv, thr, never, rthr,
                              tmp_padded, w + 2, h + 2, -1, -1, ts, ts);
    }
    if (!inner_only) {                                              // (inner_only: the caller applies the second pass itself, see zone_extent_fused_kernel)
      vwgpu_prof_scope ps(ctx, "disparity_cleanup_outer");
      hipLaunchKernelGGL(cleanup_outer_kernel, grid2(w, h), kBlk, 0, ctx->stream, tmp_padded, w, h, dst);
    }
  }
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

// scratch: 2 x w*h ints
int vwgpu_launch_blob_filter(vwgpu_ctx* ctx, int32_t* d, int w, int h, int area, int* scratch) {
  if (area < 1) return VWGPU_OK;
  const int n = w * h;
  int* label = scratch; int* size = scratch + n;
  vwgpu_prof_scope ps(ctx, "blob_filter");
  const dim3 g1((n + 255) / 256), b1(256);
  hipLaunchKernelGGL(cc_init_kernel, g1, b1, 0, ctx->stream, d, n, label, size);
  hipLaunchKernelGGL(cc_union_kernel, grid2(w, h), kBlk, 0, ctx->stream, label, w, h);
  hipLaunchKernelGGL(cc_count_kernel, g1, b1, 0, ctx->stream, label, n, size);
  hipLaunchKernelGGL(cc_erase_kernel, g1, b1, 0, ctx->stream, d, label, size, n, area);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int vwgpu_launch_disparity_mask(vwgpu_ctx* ctx, int32_t* d, int w, int h, const uint8_t* m1, const uint8_t* m2, int m2w, int m2h) {
  vwgpu_prof_scope ps(ctx, "disparity_mask");
  hipLaunchKernelGGL(disparity_mask_kernel, grid2(w, h), kBlk, 0, ctx->stream, d, w, h, m1, m2, m2w, m2h);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

extern "C" {

int vwgpu_disparity_filter_dev(vwgpu_ctx* ctx, const int32_t* d_src, int w, int h, int hh, int hv,
                               double pthr, double rthr, int cleanup, int32_t* d_dst) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!d_src || !d_dst || w <= 0 || h <= 0 || d_src == d_dst) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "rm_outliers_using_thresh: bad image arguments");
  if (hh <= 0 || hv <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "RmOutliersFunc: half kernel sizes must be non-zero.");
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  int32_t* padded = nullptr;
  if (cleanup) {
    int rc = vwgpu_arena_reserve(ctx, &ctx->pyr, (size_t)(w + 2) * (h + 2) * 12);
    if (rc) return rc;
    padded = static_cast<int32_t*>(ctx->pyr.base);
  }
  return vwgpu_launch_disparity_filter(ctx, d_src, w, h, hh, hv, pthr, rthr, cleanup != 0, padded, d_dst);
}

int vwgpu_disparity_filter(vwgpu_ctx* ctx, const int32_t* src, int w, int h, int hh, int hv,
                           double pthr, double rthr, int cleanup, int32_t* dst) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!src || !dst || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "rm_outliers_using_thresh: bad image arguments");
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int ps = st.add(src, w, h, 12, w, VWGPU_STAGE_IN), pd = st.add(dst, w, h, 12, w, VWGPU_STAGE_OUT);
  int rc = st.commit();
  if (rc) return rc;
  rc = vwgpu_disparity_filter_dev(ctx, st.dev<int32_t>(ps), w, h, hh, hv, pthr, rthr, cleanup, st.dev<int32_t>(pd));
  if (rc) return rc;
  return st.finish();
}

int vwgpu_disparity_mask_dev(vwgpu_ctx* ctx, int32_t* d_disp, int w, int h, const uint8_t* m1, const uint8_t* m2, int rmw, int rmh) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!d_disp || !m1 || !m2 || w <= 0 || h <= 0 || rmw <= 0 || rmh <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_mask: bad image arguments");
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return vwgpu_launch_disparity_mask(ctx, d_disp, w, h, m1, m2, rmw, rmh);
}

int vwgpu_disparity_mask(vwgpu_ctx* ctx, int32_t* disp, int w, int h, const uint8_t* m1, const uint8_t* m2, int rmw, int rmh) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!disp || !m1 || !m2 || w <= 0 || h <= 0 || rmw <= 0 || rmh <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_mask: bad image arguments");
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pd = st.add(disp, w, h, 12, w, VWGPU_STAGE_INOUT), pa = st.add(m1, w, h, 1, w, VWGPU_STAGE_IN), pb = st.add(m2, rmw, rmh, 1, rmw, VWGPU_STAGE_IN);
  int rc = st.commit();
  if (rc) return rc;
  rc = vwgpu_launch_disparity_mask(ctx, st.dev<int32_t>(pd), w, h, st.dev<uint8_t>(pa), st.dev<uint8_t>(pb), rmw, rmh);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_disparity_blob_filter_dev(vwgpu_ctx* ctx, int32_t* d_disp, int w, int h, int max_blob_area) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!d_disp || w <= 0 || h <= 0 || (long long)w * h > 0x7fffffffLL) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_blob_filter: bad image arguments");
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  int rc = vwgpu_arena_reserve(ctx, &ctx->pyr, (size_t)w * h * 8);
  if (rc) return rc;
  return vwgpu_launch_blob_filter(ctx, d_disp, w, h, max_blob_area, static_cast<int*>(ctx->pyr.base));
}

int vwgpu_disparity_blob_filter(vwgpu_ctx* ctx, int32_t* disp, int w, int h, int max_blob_area) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!disp || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "disparity_blob_filter: bad image arguments");
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pd = st.add(disp, w, h, 12, w, VWGPU_STAGE_INOUT);
  int rc = st.commit();
  if (rc) return rc;
  rc = vwgpu_disparity_blob_filter_dev(ctx, st.dev<int32_t>(pd), w, h, max_blob_area);
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
