// pyramid.hip — one tile of pyramid_correlate (block matching): the coarse-to-fine level loop of
// vw::stereo::PyramidCorrelationView::prerasterize (src/vw/Stereo/CorrelationView.cc:273-886) with every image
// (pyramids, masks, per-level disparity) resident in HBM; only the per-level disparity crosses to the host, for the
// data-dependent zone scheduler (zones.h).
//
//   build_image_pyramids      CorrelationView.cc:67-239   edge-extended crops, nodata mean fill, [1 4 6 4 1]/16
//                                                          smoothing + decimation (filters.hip), mask decimation,
//                                                          per-level prefilter
//   zone loop                 CorrelationView.cc:596-700  calc_disparity per zone (bm_*.hip), R->L run + L/R check at
//                                                          level 0, += zone.disparity_range().min()
//   clean-up                  CorrelationView.cc:702-744  rm_outliers_using_thresh / disparity_cleanup_using_thresh
//                                                          (src/vw/Stereo/DisparityMap.h:318-441) + disparity_mask (:97-253)
//   zone refinement           CorrelationView.cc:754-799  subdivide_regions (zones.hip), x2, expand(2), crop
//   result                    CorrelationView.cc:876-885  + search_region.min(), cast to PixelMask<Vector2f>
//   SGM branch                CorrelationView.cc:391-595  per-level calc_disparity_sgm seeded by the previous level (sgm.hip),
//                                                          R->L run, sub-pixel view; blob filter (:242-271), lr_disp_diff
// Inputs whose box sums would round (prefiltered imagery, mean-filled nodata, deep levels with SSD / NCC) are matched in
// the reference's own summation order (bm_exact.hip); the class of every level is measured on the device.
// VW_CORRELATION_MGM runs every level with use_mgm, _FINAL_MGM only level 0 (:365-366).  collar_size is applied by the caller
// (PyramidCorrelationView::rasterize, CorrelationView.h:123-133: a larger tile is rasterised and cropped).
// The rules that are arithmetic on sizes, boxes and zone lists are in pyramid_plan.h (no HIP, tested on its own); the clean-up, blob and
// mask kernels in pyramid_filters.hip; the helper threads of a tile group in host_pool.hip.
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "vwgpu_internal.h"
#include "pyramid_plan.h"
#include "zones.h"

namespace {

using vwgpu::IBox;
using vwgpu::SearchZone;

// ---- small kernels ----------------------------------------------------------------------------------------------

// The six base crops of a tile (two float images, four mask crops) in ONE launch: job = blockIdx.z.
struct CropJob { const void* src; ptrdiff_t stride; int w, h, x0, y0; void* dst; int dw, dh; int is_float, edge; };
struct CropJobs { CropJob j[6]; };
__global__ void crop_jobs_kernel(CropJobs jobs) {
  const CropJob J = jobs.j[blockIdx.z];
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= J.dw || y >= J.dh) return;
  int sx = J.x0 + x, sy = J.y0 + y;
  const bool outside = sx < 0 || sy < 0 || sx >= J.w || sy >= J.h;
  sx = sx < 0 ? 0 : (sx >= J.w ? J.w - 1 : sx);
  sy = sy < 0 ? 0 : (sy >= J.h ? J.h - 1 : sy);
  if (J.is_float) {
    static_cast<float*>(J.dst)[(size_t)y * J.dw + x] = (J.edge == 1 && outside) ? 0.0f : static_cast<const float*>(J.src)[(ptrdiff_t)sy * J.stride + sx];
  } else {
    const uint8_t v = (J.edge == 1 && outside) ? (uint8_t)0 : (J.src ? static_cast<const uint8_t*>(J.src)[(ptrdiff_t)sy * J.stride + sx] : (uint8_t)255);
    static_cast<uint8_t*>(J.dst)[(size_t)y * J.dw + x] = v;
  }
}

// dst(x,y) = src(ext(x0+x, y0+y)); EDGE 0 = clamp, 1 = zero.  src == nullptr means "an all-255 mask".
template <class T, int EDGE>
__global__ void crop_ext_kernel(const T* __restrict__ src, ptrdiff_t stride, int w, int h, int x0, int y0,
                                T* __restrict__ dst, int dw, int dh) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= dw || y >= dh) return;
  int sx = x0 + x, sy = y0 + y;
  T v;
  if (EDGE == 1 && (sx < 0 || sy < 0 || sx >= w || sy >= h)) {
    v = T(0);
  } else {
    sx = sx < 0 ? 0 : (sx >= w ? w - 1 : sx);
    sy = sy < 0 ? 0 : (sy >= h ? h - 1 : sy);
    v = src ? src[(ptrdiff_t)sy * stride + sx] : T(255);
  }
  dst[(size_t)y * dw + x] = v;
}

// sum / count (double) of img over the valid pixels of every second row and column (mean_pixel_value(subsample(.,2)),
// CorrelationView.cc:137-149; MeanAccumulator sums in double, src/vw/Math/Functors.h:469-487).  Every workgroup writes ONE
// partial {sum, count} formed in a fixed order, and cell[] receives the lowest set bit / largest exponent of the summed
// pixels: when count * 2^(hi+1) / 2^lo < 2^53 every partial sum is exactly representable and the host adds the partials
// (any order returns the reference's serial sum); otherwise masked_mean_serial_kernel walks the pixels in raster order.
__global__ void __launch_bounds__(256)
masked_mean_kernel(const float* __restrict__ img, const uint8_t* __restrict__ mask, int w, int h,
                   double* __restrict__ part, int* __restrict__ cell) {
  __shared__ double ws[4][2];
  double s = 0.0, n = 0.0;
  int lo = INT_MAX, hi = INT_MIN, bad = 0;
  for (int y = 2 * (blockIdx.y * blockDim.y + threadIdx.y); y < h; y += 2 * gridDim.y * blockDim.y)
    for (int x = 2 * (blockIdx.x * blockDim.x + threadIdx.x); x < w; x += 2 * gridDim.x * blockDim.x)
      if (mask[(size_t)y * w + x]) {
        const float v = img[(size_t)y * w + x];
        s += (double)v; n += 1.0;
        const unsigned u = __float_as_uint(v);
        const int e = (int)((u >> 23) & 0xffu);
        unsigned m = u & 0x7fffffu;
        if (e == 0xff) bad = 1;
        else if (e != 0 || m != 0) {
          int base;
          if (e == 0) base = -149; else { m |= 0x800000u; base = e - 127 - 23; }
          lo = min(lo, base + (__ffs((int)m) - 1));
          hi = max(hi, base + (31 - __clz((int)m)));
        }
      }
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o); n += __shfl_xor(n, o);
    lo = min(lo, __shfl_xor(lo, o)); hi = max(hi, __shfl_xor(hi, o)); bad |= __shfl_xor(bad, o);
  }
  const int tid = threadIdx.y * blockDim.x + threadIdx.x;
  if ((tid & 63) == 0) {
    ws[tid >> 6][0] = s; ws[tid >> 6][1] = n;
    if (lo != INT_MAX) { atomicMin(&cell[0], lo); atomicMax(&cell[1], hi); }
    if (bad) atomicOr(&cell[2], 1);
  }
  __syncthreads();
  if (tid == 0) {
    double* p = part + 2 * (size_t)(blockIdx.y * gridDim.x + blockIdx.x);
    p[0] = ((ws[0][0] + ws[1][0]) + ws[2][0]) + ws[3][0];
    p[1] = ((ws[0][1] + ws[1][1]) + ws[2][1]) + ws[3][1];
  }
}

// The reference's serial accumulation (m_accum += value in raster order), one wave: 64 pixels are fetched at a time and
// added one by one.  Only for images whose sum is not exactly representable along the way (see above).
__global__ void __launch_bounds__(64)
masked_mean_serial_kernel(const float* __restrict__ img, const uint8_t* __restrict__ mask, int w, int h, double* __restrict__ acc2) {
  const int ws = (w + 1) / 2, hs = (h + 1) / 2;
  const long long total = (long long)ws * hs;
  double s = 0.0, n = 0.0;
  for (long long i0 = 0; i0 < total; i0 += 64) {
    const long long i = i0 + threadIdx.x;
    float v = 0.0f;
    int ok = 0;
    if (i < total) {
      const int y = 2 * (int)(i / ws), x = 2 * (int)(i % ws);
      ok = mask[(size_t)y * w + x] != 0;
      v = img[(size_t)y * w + x];
    }
    const unsigned long long okm = __ballot(ok);
#pragma unroll 8
    for (int l = 0; l < 64; ++l) {
      if ((okm >> l) & 1ull) { s += (double)__shfl(v, l); n += 1.0; }
    }
  }
  if (threadIdx.x == 0) { acc2[0] = s; acc2[1] = n; }
}

__global__ void fill_masked_kernel(float* __restrict__ img, const uint8_t* __restrict__ mask, size_t n, float value) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !mask[i]) img[i] = value;
}

// child += (ax, ay) on a crop of a PixelMask<Vector2i> image; validity untouched (PixelMask arithmetic computes the
// children regardless, src/vw/Image/PixelMask.h:322-360).
__global__ void add_offset_kernel(int32_t* __restrict__ d, ptrdiff_t stride_px, int w, int h, int ax, int ay) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  int32_t* p = d + ((ptrdiff_t)y * stride_px + x) * 3;
  p[0] += ax; p[1] += ay;
}

// disparity_mask_kernel + finish_kernel in one pass, for the last level of a block-matching tile when nothing else reads the masked image
__global__ void finish_masked_kernel(const int32_t* __restrict__ d, int w, int h, const uint8_t* __restrict__ m1, const uint8_t* __restrict__ m2,
                                     int m2w, int m2h, int ax, int ay, float* __restrict__ out, ptrdiff_t ostride_px) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= w || j >= h) return;
  const int32_t* p = d + ((size_t)j * w + i) * 3;
  int p0 = p[0], p1 = p[1], p2 = p[2];
  bool keep = m1[(size_t)j * w + i] != 0 && p2 != 0;
  if (keep) {
    const int x = i + p0, y = j + p1;
    keep = !(x < 0 || x >= m2w || y < 0 || y >= m2h || m2[(size_t)y * m2w + x] == 0);
  }
  if (!keep) { p0 = 0; p1 = 0; p2 = 0; }
  float* o = out + ((ptrdiff_t)j * ostride_px + i) * 3;
  o[0] = (float)(p0 + ax); o[1] = (float)(p1 + ay); o[2] = p2 ? 1.0f : 0.0f;
}

// out = PixelMask<Vector2f>(disparity + search.min)  (CorrelationView.cc:879-881)
__global__ void finish_kernel(const int32_t* __restrict__ d, int w, int h, int ax, int ay, float* __restrict__ out, ptrdiff_t ostride_px) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  const int32_t* p = d + ((size_t)y * w + x) * 3;
  float* o = out + ((ptrdiff_t)y * ostride_px + x) * 3;
  o[0] = (float)(p[0] + ax); o[1] = (float)(p[1] + ay); o[2] = p[2] ? 1.0f : 0.0f;
}

// SGM result: sub-pixel view + search.min, invalid where the filtered integer disparity is (CorrelationView.cc:862-875)
__global__ void finish_sgm_kernel(const int32_t* __restrict__ d, const float* __restrict__ sub, int w, int h, float ax, float ay,
                                  float* __restrict__ out, ptrdiff_t ostride_px) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  const size_t i = ((size_t)y * w + x) * 3;
  float* o = out + ((ptrdiff_t)y * ostride_px + x) * 3;
  o[0] = sub[i] + ax; o[1] = sub[i + 1] + ay; o[2] = (d[i + 2] && sub[i + 2] != 0.0f) ? 1.0f : 0.0f;
}

// pixels the filters removed lose their L-R / R-L discrepancy as well (CorrelationView.cc:846-855)
__global__ void lr_diff_invalidate_kernel(const int32_t* __restrict__ d, int w, int h, float* __restrict__ diff2, ptrdiff_t dstride, int ulx, int uly) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  if (!d[((size_t)y * w + x) * 3 + 2]) diff2[((ptrdiff_t)(y + uly) * dstride + (x + ulx)) * 2 + 1] = 0.0f;
}

// Zeroes `count` 16-byte words at the start of every tile's buffer (blockIdx.y = the tile; buffers at a fixed stride).  hipMemset2DAsync over
// slices ~100 MB apart took 170 us per call (its fill kernel walks the pitch) — as long as the level's matcher launches.
__global__ void __launch_bounds__(256)
zero_tiles_kernel(uint4* __restrict__ base, size_t tile_words, size_t count) {
  uint4* p = base + blockIdx.y * tile_words;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// finish_masked_kernel / finish_kernel / zero_out_kernel for the tiles of a group (blockIdx.z): per-tile images at a fixed stride, per-tile
// destinations from a table.  mode[t]: 0 = nothing to write, 1 = finish, 2 = mask + finish, 3 = zeros.
constexpr int VWGPU_MAX_GROUP = 16;
struct GroupOuts { float* out[VWGPU_MAX_GROUP]; ptrdiff_t os[VWGPU_MAX_GROUP]; int mode[VWGPU_MAX_GROUP]; };
__global__ void finish_group_kernel(GroupOuts g, const int32_t* __restrict__ d, size_t d_tile, int w, int h, const uint8_t* __restrict__ m1,
                                    const uint8_t* __restrict__ m2, size_t mask_tile, int m2w, int m2h, int ax, int ay) {
  const int t = blockIdx.z, mode = g.mode[t];
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (mode == 0 || i >= w || j >= h) return;
  float* o = g.out[t] + ((ptrdiff_t)j * g.os[t] + i) * 3;
  if (mode == 3) { o[0] = o[1] = o[2] = 0.0f; return; }
  const int32_t* p = d + t * d_tile + ((size_t)j * w + i) * 3;
  int p0 = p[0], p1 = p[1], p2 = p[2];
  if (mode == 2) {
    bool keep = m1[t * mask_tile + (size_t)j * w + i] != 0 && p2 != 0;
    if (keep) {
      const int x = i + p0, y = j + p1;
      keep = !(x < 0 || x >= m2w || y < 0 || y >= m2h || m2[t * mask_tile + (size_t)y * m2w + x] == 0);
    }
    if (!keep) { p0 = 0; p1 = 0; p2 = 0; }
  }
  o[0] = (float)(p0 + ax); o[1] = (float)(p1 + ay); o[2] = p2 ? 1.0f : 0.0f;
}

__global__ void zero_out_kernel(float* __restrict__ out, ptrdiff_t ostride_px, int w, int h) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y * blockDim.y + threadIdx.y;
  if (x >= w || y >= h) return;
  float* o = out + ((ptrdiff_t)y * ostride_px + x) * 3;
  o[0] = o[1] = o[2] = 0.0f;
}

inline dim3 grid2(int w, int h) { return dim3((w + 63) / 64, (h + 3) / 4); }
const dim3 kBlk(64, 4);

// Bump allocator over one arena; everything of a tile lives until the call returns.
struct Bump {
  char* base; size_t cap, off = 0;
  template <class T> T* take(size_t n) {
    off = vwgpu_align_up(off, 256);
    T* p = reinterpret_cast<T*>(base + off);
    off += n * sizeof(T);
    return off <= cap ? p : nullptr;
  }
};

struct DevImg { float* p = nullptr; int w = 0, h = 0; };
struct DevMask { uint8_t* p = nullptr; int w = 0, h = 0; };

}  // namespace

// Zone scheduler, device part: one wave per leaf box of the quad tree measures the element-wise min / max of the VALID
// disparities inside the box and inside the box grown by 1 px (clipped to the image) — what subdivide_regions reads
// (Correlation.cc:149-171).  out: 10 ints per leaf (vwgpu::LeafExtent).
__global__ void __launch_bounds__(64)
zone_extent_kernel(const int32_t* __restrict__ disp, int w, int h, const int4* __restrict__ rects, int n, int32_t* __restrict__ out, size_t disp_tile = 0) {
  const int leaf = blockIdx.x;
  if (leaf >= n) return;
  disp += blockIdx.y * disp_tile; out += (size_t)blockIdx.y * n * 10;      // tile groups: blockIdx.y = the tile
  const int4 r = rects[leaf];                       // x0, y0, x1, y1
  const int ax0 = max(r.x - 1, 0), ay0 = max(r.y - 1, 0), ax1 = min(r.z + 1, w), ay1 = min(r.w + 1, h);
  const int aw = ax1 - ax0, count = aw * (ay1 - ay0);
  int any = 0, lox = INT_MAX, loy = INT_MAX, hix = INT_MIN, hiy = INT_MIN;
  int anya = 0, loxa = INT_MAX, loya = INT_MAX, hixa = INT_MIN, hiya = INT_MIN;
  for (int i = threadIdx.x; i < count; i += 64) {
    const int yy = i / aw, x = ax0 + (i - yy * aw), y = ay0 + yy;
    const int32_t* p = disp + ((size_t)y * w + x) * 3;
    if (!p[2]) continue;
    const int dx = p[0], dy = p[1];
    anya = 1; loxa = min(loxa, dx); hixa = max(hixa, dx); loya = min(loya, dy); hiya = max(hiya, dy);
    if (x >= r.x && x < r.z && y >= r.y && y < r.w) {
      any = 1; lox = min(lox, dx); hix = max(hix, dx); loy = min(loy, dy); hiy = max(hiy, dy);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    any |= __shfl_xor(any, o); anya |= __shfl_xor(anya, o);
    lox = min(lox, __shfl_xor(lox, o)); loy = min(loy, __shfl_xor(loy, o));
    hix = max(hix, __shfl_xor(hix, o)); hiy = max(hiy, __shfl_xor(hiy, o));
    loxa = min(loxa, __shfl_xor(loxa, o)); loya = min(loya, __shfl_xor(loya, o));
    hixa = max(hixa, __shfl_xor(hixa, o)); hiya = max(hiya, __shfl_xor(hiya, o));
  }
  if (threadIdx.x == 0) {
    int32_t* o = out + (size_t)leaf * 10;
    o[0] = any; o[1] = lox; o[2] = loy; o[3] = hix; o[4] = hiy;
    o[5] = anya; o[6] = loxa; o[7] = loya; o[8] = hixa; o[9] = hiya;
  }
}

// The same measurement for an intermediate level of the block-matching branch, straight from the first pass of the clean-up filter: the
// level's finished disparity image — second pass of disparity_cleanup_using_thresh (cleanup_outer_kernel), then disparity_mask
// (disparity_mask_kernel) — is read by nothing but this scheduler, so the two point-wise passes are applied to the pixels a leaf looks
// at as they are read, and the image itself is never written (two launches per level less; the small levels are launch bound).
__global__ void __launch_bounds__(64)
zone_extent_fused_kernel(const int32_t* __restrict__ inner, int w, int h, const uint8_t* __restrict__ m1, const uint8_t* __restrict__ m2,
                         int m2w, int m2h, const int4* __restrict__ rects, int n, int32_t* __restrict__ out,
                         size_t inner_tile = 0, size_t mask_tile = 0) {
  const int leaf = blockIdx.x;
  if (leaf >= n) return;
  inner += blockIdx.y * inner_tile; m1 += blockIdx.y * mask_tile; m2 += blockIdx.y * mask_tile; out += (size_t)blockIdx.y * n * 10;      // tile groups
  const int4 r = rects[leaf];                       // x0, y0, x1, y1
  const int ax0 = max(r.x - 1, 0), ay0 = max(r.y - 1, 0), ax1 = min(r.z + 1, w), ay1 = min(r.w + 1, h);
  const int aw = ax1 - ax0, count = aw * (ay1 - ay0);
  const int pw = w + 2;
  int any = 0, lox = INT_MAX, loy = INT_MAX, hix = INT_MIN, hiy = INT_MIN;
  int anya = 0, loxa = INT_MAX, loya = INT_MAX, hixa = INT_MIN, hiya = INT_MIN;
  for (int i = threadIdx.x; i < count; i += 64) {
    const int yy = i / aw, x = ax0 + (i - yy * aw), y = ay0 + yy;
    const int32_t* c = inner + ((size_t)(y + 1) * pw + (x + 1)) * 3;
    const int dx = c[0], dy = c[1];
    if (!c[2]) continue;
    int matched = 0;                                 // cleanup_outer_kernel
    for (int yk = -1; yk <= 1; ++yk)
      for (int xk = -1; xk <= 1; ++xk) {
        const int32_t* q = inner + ((size_t)(y + 1 + yk) * pw + (x + 1 + xk)) * 3;
        if (q[2] && fabs((double)(dx - q[0])) <= 3.0 && fabs((double)(dy - q[1])) <= 3.0) matched++;
      }
    if (((double)matched / 9.0) < 0.20) continue;
    if (m1[(size_t)y * w + x] == 0) continue;        // disparity_mask_kernel
    const int tx = x + dx, ty = y + dy;
    if (tx < 0 || tx >= m2w || ty < 0 || ty >= m2h || m2[(size_t)ty * m2w + tx] == 0) continue;
    anya = 1; loxa = min(loxa, dx); hixa = max(hixa, dx); loya = min(loya, dy); hiya = max(hiya, dy);
    if (x >= r.x && x < r.z && y >= r.y && y < r.w) {
      any = 1; lox = min(lox, dx); hix = max(hix, dx); loy = min(loy, dy); hiy = max(hiy, dy);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    any |= __shfl_xor(any, o); anya |= __shfl_xor(anya, o);
    lox = min(lox, __shfl_xor(lox, o)); loy = min(loy, __shfl_xor(loy, o));
    hix = max(hix, __shfl_xor(hix, o)); hiy = max(hiy, __shfl_xor(hiy, o));
    loxa = min(loxa, __shfl_xor(loxa, o)); loya = min(loya, __shfl_xor(loya, o));
    hixa = max(hixa, __shfl_xor(hixa, o)); hiya = max(hiya, __shfl_xor(hiya, o));
  }
  if (threadIdx.x == 0) {
    int32_t* o = out + (size_t)leaf * 10;
    o[0] = any; o[1] = lox; o[2] = loy; o[3] = hix; o[4] = hiy;
    o[5] = anya; o[6] = loxa; o[7] = loya; o[8] = hixa; o[9] = hiya;
  }
}

// ---- what the single-tile and the tile-group level loops share (the rules themselves: pyramid_plan.h) ------------------
namespace {

using vwgpu::EdgeMargins;
using vwgpu::LevelClass;
using vwgpu::PyrLayout;
using vwgpu::TileGeom;
using vwgpu::ZoneLevel;
using vwgpu::ZoneTasks;
constexpr int CS = vwgpu::PYR_CS, NB = vwgpu::PYR_NB;

// development aid (VWGPU_OPT_TRACE bit 0): host-side timeline of a tile (n == 0) or of a group of n tiles on stderr
struct Stamp {
  bool on; int n;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  void operator()(const char* what, int level) const {
    if (!on) return;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (n) fprintf(stderr, "  [%8.1f us] group of %d, level %d: %s\n", us, n, level, what);
    else fprintf(stderr, "  [%8.1f us] level %d %s\n", us, level, what);
  }
};

// the tiles' slices of the arena: tile t's buffer at offset `off` of the layout
struct Slices {
  char* base; size_t slice;
  char* at(int t, size_t off) const { return base + (size_t)t * slice + off; }
  float* f(int t, size_t off) const { return reinterpret_cast<float*>(at(t, off)); }
  uint8_t* b(int t, size_t off) const { return reinterpret_cast<uint8_t*>(at(t, off)); }
  int32_t* i(int t, size_t off) const { return reinterpret_cast<int32_t*>(at(t, off)); }
};

struct PyrSource {       // the image pair and its masks (device pointers; masks may be null)
  const float* left; int lw, lh; ptrdiff_t ls;
  const float* right; int rw, rh; ptrdiff_t rs;
  const uint8_t* lmask; ptrdiff_t lms;
  const uint8_t* rmask; ptrdiff_t rms;
};

// build_image_pyramids (CorrelationView.cc:67-239) for n tiles of equal size in slices laid out by Y: base crops, nodata mean fill,
// smoothing + decimation chain with the masks, the prefiltered copies (where Y has them) and, with `classes`, the class of every level
// of every tile (cls[t * (Y.L + 1) + level]) in ONE read-back.  alive[t] = false: a fully masked image, the tile has no data (:318-327);
// stop_if_dead: return as soon as no tile is alive (the single-tile path: nothing else is queued for such a tile).
int build_pyramids(vwgpu_ctx* ctx, const PyrSource& I, const vwgpu_pyramid_params* P, int n, const TileGeom* G, const PyrLayout& Y, const Slices& S,
                   bool classes, bool stop_if_dead, const Stamp* stamp, bool* alive, LevelClass* cls) {
  hipStream_t st = ctx->stream;
  const int L = Y.L, bw = Y.lmw[0], bh = Y.lmh[0];
  int rc;
  // ---- base crops, nodata mean fill (:67-149) ----
  for (int t = 0; t < n; ++t) {
    const TileGeom& g = G[t];
    vwgpu_prof_scope ps(ctx, "pyramid_base_crops");
    CropJobs cj;
    cj.j[0] = CropJob{I.left, I.ls, I.lw, I.lh, g.lg.x0, g.lg.y0, S.f(t, Y.lp[0]), Y.lpw[0], Y.lph[0], 1, 0};
    cj.j[1] = CropJob{I.right, I.rs, I.rw, I.rh, g.rg.x0, g.rg.y0, S.f(t, Y.rp[0]), Y.rpw[0], Y.rph[0], 1, 0};
    cj.j[2] = CropJob{I.lmask, I.lms, I.lw, I.lh, g.lg.x0, g.lg.y0, S.b(t, Y.lmx), Y.lpw[0], Y.lph[0], 0, 0};
    cj.j[3] = CropJob{I.rmask, I.rms, I.rw, I.rh, g.rg.x0, g.rg.y0, S.b(t, Y.rmx), Y.rpw[0], Y.rph[0], 0, 0};
    cj.j[4] = CropJob{I.lmask, I.lms, I.lw, I.lh, g.bbox.x0, g.bbox.y0, S.b(t, Y.lmp[0]), bw, bh, 0, 1};
    cj.j[5] = CropJob{I.rmask, I.rms, I.rw, I.rh, g.rmb.x0, g.rmb.y0, S.b(t, Y.rmp[0]), Y.rmw[0], Y.rmh[0], 0, 1};
    const int cmw = std::max(std::max(Y.lpw[0], Y.rpw[0]), std::max(bw, Y.rmw[0])), cmh = std::max(std::max(Y.lph[0], Y.rph[0]), std::max(bh, Y.rmh[0]));
    hipLaunchKernelGGL(crop_jobs_kernel, dim3((cmw + 63) / 64, (cmh + 3) / 4, 6), kBlk, 0, st, cj);
    alive[t] = true;
  }
  // nodata mean fill (:130-149).  Without a user mask the mask of an image crop is all-valid (it is edge-extended like the image — only the
  // bbox crops lmp / rmp are zero outside the image): its mean is not needed and nothing is filled; when that is true of both images the two
  // reductions, the read-back and its host round trip are skipped altogether.
  const bool l_all = !I.lmask, r_all = !I.rmask;
  const size_t nl = (size_t)Y.lpw[0] * Y.lph[0], nr = (size_t)Y.rpw[0] * Y.rph[0];
  if (!(l_all && r_all)) {
    // the reductions of every tile are queued, ONE synchronisation brings all partial sums back
    double part1[4 * NB];                          // (a single tile: no heap)
    std::vector<double> partn;
    double* part = part1;
    if (n > 1) { partn.resize((size_t)n * 4 * NB); part = partn.data(); }
    int cell[VWGPU_MAX_GROUP * 8];
    double acc[VWGPU_MAX_GROUP * 4], got[VWGPU_MAX_GROUP * 4];
    bool serial[VWGPU_MAX_GROUP * 2];
    const int init[8] = {INT_MAX, INT_MIN, 0, 0, INT_MAX, INT_MIN, 0, 0};
    for (int t = 0; t < n; ++t) {
      double* d_part = reinterpret_cast<double*>(S.at(t, Y.d_part));
      int* d_cell = reinterpret_cast<int*>(S.at(t, Y.d_cell));
      VWGPU_HIP(ctx, hipMemcpyAsync(d_cell, init, sizeof init, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(masked_mean_kernel, dim3(16, 16), kBlk, 0, st, S.f(t, Y.lp[0]), S.b(t, Y.lmx), Y.lpw[0], Y.lph[0], d_part, d_cell);
      hipLaunchKernelGGL(masked_mean_kernel, dim3(16, 16), kBlk, 0, st, S.f(t, Y.rp[0]), S.b(t, Y.rmx), Y.rpw[0], Y.rph[0], d_part + 2 * NB, d_cell + 4);
      VWGPU_HIP(ctx, hipMemcpyAsync(part + (size_t)t * 4 * NB, d_part, 4 * NB * sizeof(double), hipMemcpyDeviceToHost, st));
      VWGPU_HIP(ctx, hipMemcpyAsync(cell + t * 8, d_cell, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    VWGPU_HIP(ctx, hipStreamSynchronize(st));
    bool any_serial = false;
    for (int t = 0; t < n; ++t)
      for (int im = 0; im < 2; ++im) {
        double s_ = 0.0, n_ = 0.0;
        for (int b = 0; b < NB; ++b) { s_ += part[(size_t)t * 4 * NB + (im * NB + b) * 2]; n_ += part[(size_t)t * 4 * NB + (im * NB + b) * 2 + 1]; }
        acc[t * 4 + 2 * im] = s_; acc[t * 4 + 2 * im + 1] = n_;
        const int lo = cell[t * 8 + 4 * im], hi = cell[t * 8 + 4 * im + 1];
        int lgn = 0;
        while ((1LL << lgn) < (long long)n_ + 1) ++lgn;
        // every partial sum of <= n pixels < 2^(hi+1), all multiples of 2^lo, is exact iff it needs <= 53 bits
        serial[t * 2 + im] = cell[t * 8 + 4 * im + 2] != 0 || (lo != INT_MAX && (long long)hi + 1 + lgn - lo > 53);
        any_serial = any_serial || serial[t * 2 + im];
      }
    if (any_serial) {
      for (int t = 0; t < n; ++t) {
        double* d_acc = reinterpret_cast<double*>(S.at(t, Y.d_acc));
        if (serial[t * 2]) hipLaunchKernelGGL(masked_mean_serial_kernel, dim3(1), dim3(64), 0, st, S.f(t, Y.lp[0]), S.b(t, Y.lmx), Y.lpw[0], Y.lph[0], d_acc);
        if (serial[t * 2 + 1]) hipLaunchKernelGGL(masked_mean_serial_kernel, dim3(1), dim3(64), 0, st, S.f(t, Y.rp[0]), S.b(t, Y.rmx), Y.rpw[0], Y.rph[0], d_acc + 2);
        if (serial[t * 2] || serial[t * 2 + 1]) VWGPU_HIP(ctx, hipMemcpyAsync(got + t * 4, d_acc, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
      }
      VWGPU_HIP(ctx, hipStreamSynchronize(st));
      for (int t = 0; t < n; ++t) {
        if (serial[t * 2]) { acc[t * 4] = got[t * 4]; acc[t * 4 + 1] = got[t * 4 + 1]; }
        if (serial[t * 2 + 1]) { acc[t * 4 + 2] = got[t * 4 + 2]; acc[t * 4 + 3] = got[t * 4 + 3]; }
      }
    }
    // A fully masked image.  Only an image with a user mask is asked: without one its crop mask is all 255 and its count is the number
    // of sampled pixels, never zero — which is why "either count is zero" and this test agree.
    bool any_alive = false;
    for (int t = 0; t < n; ++t) {
      alive[t] = !((!l_all && acc[t * 4 + 1] == 0.0) || (!r_all && acc[t * 4 + 3] == 0.0));
      any_alive = any_alive || alive[t];
    }
    if (stop_if_dead && !any_alive) return VWGPU_OK;
    for (int t = 0; t < n; ++t) {
      if (!alive[t]) continue;
      if (!l_all) hipLaunchKernelGGL(fill_masked_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st, S.f(t, Y.lp[0]), S.b(t, Y.lmx), nl, (float)(acc[t * 4] / acc[t * 4 + 1]));
      if (!r_all) hipLaunchKernelGGL(fill_masked_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, st, S.f(t, Y.rp[0]), S.b(t, Y.rmx), nr, (float)(acc[t * 4 + 2] / acc[t * 4 + 3]));
    }
  }
  // ---- smoothing + decimation chain, mask decimation (:205-216): the four jobs of every tile of a level, VWGPU_MAX_IMG_JOBS per launch ----
  const float k5[5] = {(float)(1.0 / 16.0), (float)(4.0 / 16.0), (float)(6.0 / 16.0), (float)(4.0 / 16.0), (float)(1.0 / 16.0)};
  for (int i = 1; i <= L; ++i) {
    vwgpu_img_job jobs[4 * VWGPU_MAX_GROUP];
    for (int t = 0; t < n; ++t) {
      jobs[4 * t + 0] = {S.f(t, Y.lp[i - 1]), Y.lpw[i - 1], Y.lpw[i - 1], Y.lph[i - 1], S.f(t, Y.lp[i]), Y.lpw[i], Y.lpw[i], Y.lph[i], 0, 0, nullptr, 0};
      jobs[4 * t + 1] = {S.f(t, Y.rp[i - 1]), Y.rpw[i - 1], Y.rpw[i - 1], Y.rph[i - 1], S.f(t, Y.rp[i]), Y.rpw[i], Y.rpw[i], Y.rph[i], 0, 0, nullptr, 0};
      jobs[4 * t + 2] = {S.b(t, Y.lmp[i - 1]), Y.lmw[i - 1], Y.lmw[i - 1], Y.lmh[i - 1], S.b(t, Y.lmp[i]), Y.lmw[i], Y.lmw[i], Y.lmh[i], 0, 0, nullptr, VWGPU_JOB_MASK_BY_TWO};
      jobs[4 * t + 3] = {S.b(t, Y.rmp[i - 1]), Y.rmw[i - 1], Y.rmw[i - 1], Y.rmh[i - 1], S.b(t, Y.rmp[i]), Y.rmw[i], Y.rmw[i], Y.rmh[i], 0, 0, nullptr, VWGPU_JOB_MASK_BY_TWO};
    }
    for (int j0 = 0; j0 < 4 * n; j0 += VWGPU_MAX_IMG_JOBS)
      if ((rc = vwgpu_launch_sepconv_jobs(ctx, jobs + j0, std::min(VWGPU_MAX_IMG_JOBS, 4 * n - j0), k5, 5, 2, k5, 5, 2, 0, 2))) return rc;
  }
  // ---- prefilter every level into copies (:232-236; the levels stay the unfiltered sources of the next level): every level of both
  // images of every tile through the same two launches (gaussian, then laplacian / subtraction), level by level ----
  if (Y.filtered) {
    std::vector<const float*> fs; std::vector<float*> fd; std::vector<int> fw, fh;
    for (int i = 0; i <= L; ++i)
      for (int t = 0; t < n; ++t) {
        fs.push_back(S.f(t, Y.lp[i])); fd.push_back(S.f(t, Y.lpf[i])); fw.push_back(Y.lpw[i]); fh.push_back(Y.lph[i]);
        fs.push_back(S.f(t, Y.rp[i])); fd.push_back(S.f(t, Y.rpf[i])); fw.push_back(Y.rpw[i]); fh.push_back(Y.rph[i]);
      }
    if ((rc = vwgpu_prefilter_images_dev(ctx, (int)fs.size(), fs.data(), fw.data(), fh.data(), P->prefilter_mode, P->prefilter_width, fd.data()))) return rc;
  }
  // ---- class of every level of every tile (pyramid_plan.h, level_class), measured on the device: ONE read-back ----
  if (classes) {
    std::vector<int> cells((size_t)n * CS * (L + 1), 0);
    for (int t = 0; t < n; ++t)
      for (int i = 0; i <= L; ++i) { int* c = cells.data() + ((size_t)t * (L + 1) + i) * CS; c[0] = INT_MAX; c[1] = INT_MIN; }
    std::vector<const float*> gi; std::vector<int> gw, gh; std::vector<ptrdiff_t> gs; std::vector<int*> gc;
    for (int t = 0; t < n; ++t)
      VWGPU_HIP(ctx, hipMemcpyAsync(S.at(t, Y.d_cells), cells.data() + (size_t)t * (L + 1) * CS, (size_t)(L + 1) * CS * sizeof(int), hipMemcpyHostToDevice, st));
    for (int i = 0; i <= L; ++i)
      for (int t = 0; t < n; ++t) {
        int* d_cells = reinterpret_cast<int*>(S.at(t, Y.d_cells));
        gi.push_back(S.f(t, Y.lpf[i])); gw.push_back(Y.lpw[i]); gh.push_back(Y.lph[i]); gs.push_back(Y.lpw[i]); gc.push_back(d_cells + CS * i);
        gi.push_back(S.f(t, Y.rpf[i])); gw.push_back(Y.rpw[i]); gh.push_back(Y.rph[i]); gs.push_back(Y.rpw[i]); gc.push_back(d_cells + CS * i);
      }
    vwgpu_launch_float_grain(ctx, (int)gi.size(), gi.data(), gw.data(), gh.data(), gs.data(), gc.data());
    for (int t = 0; t < n; ++t)
      VWGPU_HIP(ctx, hipMemcpyAsync(cells.data() + (size_t)t * (L + 1) * CS, S.at(t, Y.d_cells), (size_t)(L + 1) * CS * sizeof(int), hipMemcpyDeviceToHost, st));
    if (stamp) (*stamp)("pyramids queued, waiting for the level classes", L);
    VWGPU_HIP(ctx, hipStreamSynchronize(st));
    if (stamp) (*stamp)("level classes on the host", L);
    for (int t = 0; t < n; ++t)
      for (int i = 0; i <= L; ++i)
        cls[(size_t)t * (L + 1) + i] = vwgpu::level_class(P->cost_type, P->kernel_x, P->kernel_y, cells.data() + ((size_t)t * (L + 1) + i) * CS, ctx->certify != 0);
  }
  return VWGPU_OK;
}

// The leaf boxes of a level size on the device: the quad tree of boxes is fixed by (dw, dh), so its leaves go up once per context.
int leaf_rects_on_device(vwgpu_ctx* ctx, int dw, int dh, const int4** d_rects, size_t* nleaf) {
  const std::vector<vwgpu::IBox>& leaves = vwgpu::cached_leaves(dw, dh);
  const size_t nl = leaves.size();
  static_assert(sizeof(vwgpu::IBox) == sizeof(int4), "leaf boxes upload as int4");
  *nleaf = nl; *d_rects = nullptr;
  for (auto& lr : ctx->leaf_rects)
    if (lr.w == dw && lr.h == dh && lr.n == nl) *d_rects = static_cast<const int4*>(lr.d_rects);
  if (*d_rects) return VWGPU_OK;
  void* p = nullptr;
  VWGPU_HIP(ctx, hipMalloc(&p, std::max<size_t>(nl, 1) * sizeof(int4)));
  VWGPU_HIP(ctx, hipMemcpyAsync(p, leaves.data(), nl * sizeof(int4), hipMemcpyHostToDevice, ctx->stream));
  VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));                 // the host list may be evicted from its cache later
  if (ctx->leaf_rects.size() >= 64) { (void)hipFree(ctx->leaf_rects.front().d_rects); ctx->leaf_rects.erase(ctx->leaf_rects.begin()); }
  ctx->leaf_rects.push_back({dw, dh, nl, p});
  *d_rects = static_cast<const int4*>(p);
  return VWGPU_OK;
}

// Zone refinement, device part (:754-799): the leaves of the quad tree are measured on the device (box + 1-px neighbourhood) for n tiles
// in one launch, only that table comes back — to the pinned ring, or to `own` when it does not fit — and the host waits for it: the one
// synchronisation of a level.  fused: `img` is the first pass of the clean-up filter (padded) and the second pass and the mask (m1, m2)
// are applied as the kernel reads; otherwise `img` is the finished disparity image.  img_tile (ints) / mask_tile (bytes): the stride
// from a tile to the next (0 for a single tile).
int read_leaf_extents(vwgpu_ctx* ctx, int n, bool fused, const int32_t* img, size_t img_tile, int dw, int dh, const uint8_t* m1, const uint8_t* m2,
                      size_t mask_tile, int m2w, int m2h, const Stamp& stamp, int level, std::vector<vwgpu::LeafExtent>* own,
                      const vwgpu::LeafExtent** h_ext, size_t* nleaf) {
  hipStream_t st = ctx->stream;
  const int4* d_rects = nullptr;
  int rc = leaf_rects_on_device(ctx, dw, dh, &d_rects, nleaf);
  if (rc) return rc;
  const size_t ext_bytes = (size_t)n * *nleaf * sizeof(vwgpu::LeafExtent);
  if ((rc = vwgpu_arena_reserve(ctx, &ctx->zext, ext_bytes + 256))) return rc;
  int32_t* d_ext = static_cast<int32_t*>(ctx->zext.base);
  {
    vwgpu_prof_scope ps(ctx, "zone_extents");
    const dim3 grid((unsigned)*nleaf, (unsigned)n);
    if (fused)
      hipLaunchKernelGGL(zone_extent_fused_kernel, grid, dim3(64), 0, st, img, dw, dh, m1, m2, m2w, m2h, d_rects, (int)*nleaf, d_ext, img_tile, mask_tile);
    else
      hipLaunchKernelGGL(zone_extent_kernel, grid, dim3(64), 0, st, img, dw, dh, d_rects, (int)*nleaf, d_ext, img_tile);
  }
  *h_ext = static_cast<const vwgpu::LeafExtent*>(vwgpu_host_ring(ctx, ext_bytes));
  if (!*h_ext) { own->resize((size_t)n * *nleaf); *h_ext = own->data(); }
  VWGPU_HIP(ctx, hipMemcpyAsync(const_cast<vwgpu::LeafExtent*>(*h_ext), d_ext, ext_bytes, hipMemcpyDeviceToHost, st));
  stamp("level queued, waiting", level);
  VWGPU_HIP(ctx, hipStreamSynchronize(st));
  stamp("leaf extents on the host", level);
  return VWGPU_OK;
}

// One direction of a matching pass: image A matched against image B.
struct MatchPair { const float* a; int aw, ah; const float* b; int bw, bh; };

// Behind a certified pass: the zones of `tz` that the tile kernels flagged (hflag, on the host) — those of tile `img` only, or all with
// img < 0 — are redone in the reference's order.  The launch is sized by the flagged zones: gated launches over all 2000 zones of a
// border tile spent 0.1 ms each on workgroups that read a zero and left.  trace_level >= 0: say what was redone (VWGPU_OPT_TRACE bit 2).
int redo_flagged_zones(vwgpu_ctx* ctx, const vwgpu_pyramid_params* P, const MatchPair& m, const std::vector<vwgpu_zone_task>& tz, const int* hflag, int img,
                       int32_t* dst, int trace_level, size_t pass) {
  std::vector<vwgpu_zone_task> redo;
  for (size_t i = 0; i < tz.size(); ++i) if (hflag[i] && (img < 0 || tz[i].img == img)) redo.push_back(tz[i]);
  if (redo.empty()) return VWGPU_OK;
  if (trace_level >= 0 && (ctx->trace & 4)) {
    size_t px = 0, ev = 0;
    for (auto const& zt : redo) { px += (size_t)zt.zw * zt.zh; ev += (size_t)zt.zw * zt.zh * zt.sx * zt.sy; }
    fprintf(stderr, "  level %d pass %zu: %zu of %zu zones to the exact-order kernels, %zu px, %zu evaluations; largest:", trace_level, pass, redo.size(), tz.size(), px, ev);
    std::vector<vwgpu_zone_task> big(redo);
    std::sort(big.begin(), big.end(), [](vwgpu_zone_task const& a2, vwgpu_zone_task const& b2) { return (size_t)a2.zw * a2.zh * a2.sx * a2.sy > (size_t)b2.zw * b2.zh * b2.sx * b2.sy; });
    for (size_t i = 0; i < std::min<size_t>(4, big.size()); ++i) fprintf(stderr, " %dx%d x %dx%d", big[i].zw, big[i].zh, big[i].sx, big[i].sy);
    fprintf(stderr, "\n");
  }
  return vwgpu_launch_bm_exact(ctx, P->cost_type, m.a, m.aw, m.ah, m.aw, m.b, m.bw, m.bh, m.bw, P->kernel_x, P->kernel_y, redo.data(), (int)redo.size(), dst);
}

// certification statistics (VWGPU_OPT_TRACE bit 2), the end of a call: into the context's counters, and on stderr with `print`
int read_cert_stats(vwgpu_ctx* ctx, const unsigned long long* d_cert_stats, bool print) {
  if (!d_cert_stats) return VWGPU_OK;
  unsigned long long got[4] = {0, 0, 0, 0};
  VWGPU_HIP(ctx, hipMemcpyAsync(got, d_cert_stats, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
  VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->cert_px[0] += got[0]; ctx->cert_px[1] += got[1]; ctx->cert_px[2] += got[2];
  if (print)
    fprintf(stderr, "certification: %llu pixels in certified tiles, %llu in tiles that sent their zone to the exact-order kernels (%.2f %%); %llu in tiles "
            "the fp32 tier passed on to float64 (%.2f %%)\n",
            got[0], got[1], got[0] + got[1] ? 100.0 * (double)got[1] / (double)(got[0] + got[1]) : 0.0, got[2],
            got[0] + got[1] ? 100.0 * (double)got[2] / (double)(got[0] + got[1]) : 0.0);
  return VWGPU_OK;
}

const char* zone_err_text(vwgpu::ZoneErr e, bool group) {
  if (e == vwgpu::ZONE_TOO_LARGE) return "pyramid_correlate: zone too large";
  if (e == vwgpu::ZONE_TABLES_TOO_LARGE) return "pyramid_correlate: tile group too large for the zone tables";
  return group ? "pyramid_correlate: tile group too large for the L/R check buffers" : "pyramid_correlate: tile too large for the L/R check buffers";
}

}  // namespace

// All pointers are device pointers (masks may be null).  out: bw x bh x 3 floats.
int vwgpu_pyramid_correlate_impl(vwgpu_ctx* ctx, const float* left, int lw, int lh, ptrdiff_t ls,
                                 const float* right, int rw, int rh, ptrdiff_t rs,
                                 const uint8_t* lmask, ptrdiff_t lms, const uint8_t* rmask, ptrdiff_t rms,
                                 const vwgpu_pyramid_params* P, int bx, int by, int bw, int bh,
                                 float* out, ptrdiff_t os, float* lr_diff) {
  const int kx = P->kernel_x, ky = P->kernel_y;
  // lr_diff: DEVICE copy of P->lr_disp_diff (or null); its geometry comes from P
  const ptrdiff_t lr_stride = P->lr_disp_diff_stride ? P->lr_disp_diff_stride : P->lr_disp_diff_cols;
  const int lr_ulx = bx - P->region_ul_x, lr_uly = by - P->region_ul_y;       // tile origin inside the diff image
  const IBox search(P->search_min_x, P->search_min_y, P->search_max_x, P->search_max_y);
  hipStream_t st = ctx->stream;

  const int L = vwgpu::pyramid_levels(P, bw, bh);
  const int hkx = kx / 2, hky = ky / 2, up = 1 << L;
  const TileGeom G = vwgpu::tile_geom(bx, by, bw, bh, search, hkx, hky, up);
  const IBox &lg = G.lg, &rg = G.rg, &rmb = G.rmb;
  const bool use_sgm = P->algorithm != 0;
  // SGM/MGM run without a prefilter (CorrelationView.h:96-97) and without level classes
  const bool filtered = !use_sgm && (P->prefilter_mode == VWGPU_PREFILTER_LOG || P->prefilter_mode == VWGPU_PREFILTER_MEANSUB);
  const PyrLayout Y = vwgpu::pyr_layout(G, L, filtered);

  // arena: pyramids (4/3 of the bases, twice for the prefiltered copies), masks, disparities, scratch
  const size_t nl = (size_t)lg.dx() * lg.dy(), nr = (size_t)rg.dx() * rg.dy();
  const size_t need = 4 * (nl + nr) * 3 + (nl + nr) * 2 + (size_t)rmb.dx() * rmb.dy() * 2 + (size_t)bw * bh * (12 * 3 + 2) +
                      (size_t)(bw + 2) * (bh + 2) * 12 + (nl + nr) * 4 * 2 + (size_t)(rg.dx() + 2 * search.dx()) * (rg.dy() + 2 * search.dy()) * 20 +
                      (size_t)(lg.dx() + 2 * search.dx() + 2) * (lg.dy() + 2 * search.dy() + 2) * 4 + (1 << 20) +
                      // per-level tables taken inside the level loop: zone flags of both passes and the R->L need records (8 ints per
                      // zone; zones <= 4 per 16 x 16 px of the tile + 64) with one cell flag per 16 x 16 px of every zone's R->L image (a zone widened
                      // by its search range: at most (sdx / 16 + 3)(sdy / 16 + 3) cells for a leaf-sized zone)
                      (size_t)(L + 1) * ((size_t)bw * bh / 64 + 64) * (48 + (size_t)(search.dx() / 16 + 3) * (search.dy() / 16 + 3)) + 4096;
  // SGM: R->L crops (left image grown by twice the search), R->L masks, disparities of both directions and their history
  const size_t rl_px = (size_t)(bw + search.dx() + 8) * (bh + search.dy() + 8);
  const size_t lrev_px = (size_t)(lg.dx() + 2 * search.dx() + 8) * (lg.dy() + 2 * search.dy() + 8);
  const size_t need_blob = P->blob_filter_area > 0 ? (size_t)(bw + search.dx() + 8) * (bh + search.dy() + 8) * 8 + 1024 : 0;
  const size_t need_sgm = P->algorithm != 0 ? lrev_px * 4 + rl_px * (12 * 5 + 1) + lrev_px + (size_t)bw * bh * (12 + 12) + (1 << 16) : 0;
  int rc = vwgpu_arena_reserve(ctx, &ctx->pyr, need + need_sgm + need_blob);
  if (rc) return rc;
  Bump A{static_cast<char*>(ctx->pyr.base), ctx->pyr.cap};
  auto fail_mem = [&]() { return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "pyramid_correlate: internal arena too small"); };
  // the tile's slice (pyramids, masks, disparity images) comes first; the scratch of the level loop follows it
  const Slices S{A.take<char>(Y.slice), Y.slice};
  if (!S.base) return fail_mem();
  bool alive = true;
  LevelClass cls[vwgpu::PYR_MAX_LEVELS];
  const PyrSource src{left, lw, lh, ls, right, rw, rh, rs, lmask, lms, rmask, rms};
  if ((rc = build_pyramids(ctx, src, P, 1, &G, Y, S, !use_sgm, true, nullptr, &alive, cls))) return rc;
  if (!alive) {                                    // a fully masked image: the tile has no data (:318-327)
    hipLaunchKernelGGL(zero_out_kernel, grid2(bw, bh), kBlk, 0, st, out, os, bw, bh);
    VWGPU_HIP(ctx, hipGetLastError());
    return VWGPU_OK;
  }
  std::vector<DevImg> lp(L + 1), rp(L + 1);        // the levels the matchers read: the prefiltered copies where there are any
  std::vector<DevMask> lmp(L + 1), rmp(L + 1);
  for (int i = 0; i <= L; ++i) {
    lp[i].p = S.f(0, Y.lpf[i]); lp[i].w = Y.lpw[i]; lp[i].h = Y.lph[i];
    rp[i].p = S.f(0, Y.rpf[i]); rp[i].w = Y.rpw[i]; rp[i].h = Y.rph[i];
    lmp[i].p = S.b(0, Y.lmp[i]); lmp[i].w = Y.lmw[i]; lmp[i].h = Y.lmh[i];
    rmp[i].p = S.b(0, Y.rmp[i]); rmp[i].w = Y.rmw[i]; rmp[i].h = Y.rmh[i];
  }

  // certification statistics (VWGPU_OPT_TRACE bit 2): pixels in certified tiles / in tiles that flagged their zone
  unsigned long long* d_cert_stats = nullptr;
  if (ctx->trace & 4) {
    d_cert_stats = A.take<unsigned long long>(4);
    if (!d_cert_stats) return fail_mem();
    VWGPU_HIP(ctx, hipMemsetAsync(d_cert_stats, 0, 32, st));
  }
  // level loop
  int32_t* disp = S.i(0, Y.disp);
  int32_t* disp2 = S.i(0, Y.disp2);
  int32_t* padded = S.i(0, Y.padded);
  int32_t* rl = A.take<int32_t>((size_t)(rg.dx() + 2 * search.dx()) * (rg.dy() + 2 * search.dy()) * 3 + 64);
  // tmp_a also receives the edge-extended LEFT crop of an R->L run: (zone + 2 * search - 1) per axis, at most the level size + 2 * search
  const size_t tmp_a_px = std::max(nl + nr, (size_t)(lg.dx() + 2 * search.dx() + 2) * (lg.dy() + 2 * search.dy() + 2));
  const size_t tmp_b_px = (size_t)(rg.dx() + 2 * search.dx()) * (rg.dy() + 2 * search.dy());
  float* tmp_a = A.take<float>(tmp_a_px);
  float* tmp_b = A.take<float>(tmp_b_px);
  if (!rl || !tmp_a || !tmp_b) return fail_mem();
  int* blob_scratch = nullptr;
  if (P->blob_filter_area > 0) {
    blob_scratch = A.take<int>((size_t)(bw + search.dx() + 8) * (bh + search.dy() + 8) * 2);
    if (!blob_scratch) return fail_mem();
  }
  float* sgm_b = nullptr; float* sub = nullptr; uint8_t* rl_rmask = nullptr; uint8_t* rl_lmask = nullptr;
  int32_t *prev_disp = nullptr, *rl_a = nullptr, *rl_b = nullptr, *rl_pad = nullptr, *prev_rl = nullptr;
  if (use_sgm) {
    sgm_b = A.take<float>(lrev_px); sub = A.take<float>((size_t)bw * bh * 3);
    rl_rmask = A.take<uint8_t>(rl_px); rl_lmask = A.take<uint8_t>(lrev_px);
    prev_disp = A.take<int32_t>((size_t)bw * bh * 3);
    rl_a = A.take<int32_t>(rl_px * 3); rl_b = A.take<int32_t>(rl_px * 3); rl_pad = A.take<int32_t>(rl_px * 3 + 64); prev_rl = A.take<int32_t>(rl_px * 3);
    if (!sgm_b || !sub || !rl_rmask || !rl_lmask || !prev_disp || !rl_a || !rl_b || !rl_pad || !prev_rl) return fail_mem();
  }
  int pdw = 0, pdh = 0, prlw = 0, prlh = 0;
  bool have_prev_rl = false;
  vwgpu_sgm_params SP;
  SP.cost_type = P->cost_type; SP.use_mgm = 0; SP.kernel_size = kx; SP.subpixel_mode = P->sgm_subpixel_mode;
  SP.search_buffer_x = P->sgm_search_buffer_x; SP.search_buffer_y = P->sgm_search_buffer_y; SP.memory_limit_mb = P->memory_limit_mb;
  SP.p1 = 0; SP.p2 = 0; SP.ternary_census_threshold = 5; SP.num_threads = P->sgm_num_threads > 0 ? P->sgm_num_threads : 1;
  SP.allow_block_cost = 0;        // (the pyramid view only ever hands census costs to SGM, CorrelationView.cc:391-403)
  std::vector<vwgpu::LeafExtent> leaf_ext;
  std::vector<SearchZone> zones;
  zones.push_back(SearchZone{IBox(0, 0, lmp[L].w, lmp[L].h), IBox(0, 0, search.width() / up + 1, search.height() / up + 1)});
  // corr_timeout accounting (CorrelationView.cc:285-287,354-357,620-637): the estimate seconds_per_op * search volume is
  // replaced by the wall clock whenever it has advanced by more than measure_spacing (2 s) since the last measurement
  // (std::time: whole seconds), so a seconds_per_op calibrated for the CPU cannot make the GPU quit after milliseconds.
  double estim = 0.0, prev_estim = 0.0;
  const Stamp stamp{(ctx->trace & 1) != 0, 0};
  const auto t_start = stamp.t0;
  auto remeasure = [&]() {
    if (P->corr_timeout > 0 && estim - prev_estim > 2.0) {
      estim = std::floor(std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
      prev_estim = estim;
    }
  };
  const int saved_force = ctx->forced_path;
  int dw = 0, dh = 0;
  bool fused_finish = false;
  for (int level = L; level >= 0; --level) {
    const bool last = (level == 0);
    const int scaling = 1 << level;
    stamp("begin", level);
    dw = lmp[level].w; dh = lmp[level].h;
    VWGPU_HIP(ctx, hipMemsetAsync(disp, 0, (size_t)dw * dh * 12, st));
    const int rox = up * hkx / scaling, roy = up * hky / scaling;
    // cheapest zones first (CorrelationView.cc:601-606) — which only matters when a time budget may cut the list: the zones are disjoint
    // boxes, so without one every order gives the same image (and sorting 2000 leaf zones is 80 us with the device waiting)
    if (P->corr_timeout > 0)
      std::stable_sort(zones.begin(), zones.end(), [](SearchZone const& a, SearchZone const& b) { return a.volume() < b.volume(); });
    // dyadic / prefiltered data is not integer-valued: go straight to the float64 matcher there, or to the exact-order
    // kernels when the level's sums could round
    const int level_path = cls[level].exact ? VWGPU_PATH_EXACT_ORDER : ((level > 0 || filtered) ? VWGPU_PATH_GENERIC_F64 : VWGPU_PATH_NONE);
    ctx->forced_path = (saved_force != VWGPU_PATH_NONE) ? saved_force : level_path;
    const DevImg Lv = lp[level], Rv = rp[level];
    const bool lr_active = P->consistency_threshold >= 0 && last;
    // One launch for all zones of the level (bm_zones.hip) unless the kernel is too large for its LDS tiles, or the
    // level is a single big zone (max_pyramid_levels = 0: that is plain calc_disparity and has faster kernels).
    bool check_rl = false;
    int rlw = 0, rlh = 0, lrm_w = 0, lrm_h = 0;
    if (use_sgm) {                                                      // SGM branch (CorrelationView.cc:391-595)
      ctx->forced_path = saved_force;
      const int sx = search.width() / scaling, sy = search.height() / scaling;   // zone.disparity_range().size(), inclusive for SGM
      const IBox lr(rox - hkx, roy - hky, dw + rox + hkx, dh + roy + hky);
      const IBox rr(lr.x0, lr.y0, lr.x1 + sx, lr.y1 + sy);
      if ((size_t)rr.dx() * rr.dy() > tmp_b_px || (size_t)lr.dx() * lr.dy() > tmp_a_px) return fail_mem();
      hipLaunchKernelGGL((crop_ext_kernel<float, 0>), grid2(lr.dx(), lr.dy()), kBlk, 0, st, Lv.p, Lv.w, Lv.w, Lv.h, lr.x0, lr.y0, tmp_a, lr.dx(), lr.dy());
      hipLaunchKernelGGL((crop_ext_kernel<float, 0>), grid2(rr.dx(), rr.dy()), kBlk, 0, st, Rv.p, Rv.w, Rv.w, Rv.h, rr.x0, rr.y0, tmp_b, rr.dx(), rr.dy());
      const bool have_prev = level < L;
      SP.use_mgm = (P->algorithm == 2 || (P->algorithm == 3 && level == 0)) ? 1 : 0;      // CorrelationView.cc:365-366
      int ow = 0, oh = 0;
      rc = vwgpu_sgm_impl(ctx, &SP, tmp_a, lr.dx(), lr.dy(), lr.dx(), tmp_b, rr.dx(), rr.dy(), rr.dx(), sx, sy,
                          lmp[level].p, lmp[level].w, lmp[level].h, rmp[level].p, rmp[level].w, rmp[level].h,
                          have_prev ? prev_disp : nullptr, pdw, pdh, disp, last ? sub : nullptr, (size_t)dw * dh, &ow, &oh);
      if (rc) return rc;
      if (ow != dw || oh != dh) return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "pyramid_correlate: SGM output %d x %d does not match the level size %d x %d", ow, oh, dw, dh);
      if (P->consistency_threshold >= 0.0f && level >= P->min_consistency_level) {
        check_rl = true;
        const IBox lrev(lr.x0 - sx, lr.y0 - sy, lr.x1 + sx, lr.y1 + sy);          // (left_region - size).max += 2 size
        rlw = rr.dx() - 2 * hkx; rlh = rr.dy() - 2 * hky;
        lrm_w = lrev.dx() - 2 * hkx; lrm_h = lrev.dy() - 2 * hky;
        if ((size_t)lrev.dx() * lrev.dy() > lrev_px || (size_t)rlw * rlh > rl_px) return fail_mem();
        hipLaunchKernelGGL((crop_ext_kernel<uint8_t, 1>), grid2(rlw, rlh), kBlk, 0, st, rmp[level].p, rmp[level].w, rmp[level].w, rmp[level].h, 0, 0, rl_rmask, rlw, rlh);
        hipLaunchKernelGGL((crop_ext_kernel<uint8_t, 1>), grid2(lrm_w, lrm_h), kBlk, 0, st, lmp[level].p, lmp[level].w, lmp[level].w, lmp[level].h, -sx, -sy, rl_lmask, lrm_w, lrm_h);
        hipLaunchKernelGGL((crop_ext_kernel<float, 0>), grid2(lrev.dx(), lrev.dy()), kBlk, 0, st, Lv.p, Lv.w, Lv.w, Lv.h, lrev.x0, lrev.y0, sgm_b, lrev.dx(), lrev.dy());
        int row = 0, roh = 0;
        rc = vwgpu_sgm_impl(ctx, &SP, tmp_b, rr.dx(), rr.dy(), rr.dx(), sgm_b, lrev.dx(), lrev.dy(), lrev.dx(), sx, sy,
                            rl_rmask, rlw, rlh, rl_lmask, lrm_w, lrm_h, (have_prev && have_prev_rl) ? prev_rl : nullptr, prlw, prlh,
                            rl_a, nullptr, rl_px, &row, &roh);
        if (rc) return rc;
        if (row != rlw || roh != rlh) return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "pyramid_correlate: SGM R->L output size mismatch");
        hipLaunchKernelGGL(add_offset_kernel, grid2(rlw, rlh), kBlk, 0, st, rl_a, rlw, rlw, rlh, -sx, -sy);
        rc = vwgpu_launch_lr_check_diff(ctx, disp, dw, dh, dw, rl_a, rlw, rlh, rlw, P->consistency_threshold, last ? lr_diff : nullptr, lr_stride,
                                        lr_ulx, lr_uly);
        if (rc) return rc;
        hipLaunchKernelGGL(add_offset_kernel, grid2(rlw, rlh), kBlk, 0, st, rl_a, rlw, rlw, rlh, sx, sy);
      }
    }
    bool batched = !use_sgm && vwgpu_bm_zones_supported(kx, ky) && saved_force == VWGPU_PATH_NONE;
    if (batched && zones.size() == 1 && (double)zones[0].region.dx() * zones[0].region.dy() * zones[0].range.dx() * zones[0].range.dy() > 3.2e7)
      batched = false;
    if (batched) {
      ZoneTasks zt;
      std::vector<vwgpu_zone_task>&t1 = zt.a, &t2 = zt.b, &t3 = zt.c;
      t1.reserve(zones.size());
      if (lr_active) { t2.reserve(zones.size()); t3.reserve(zones.size()); }
      const ZoneLevel zl{rox, roy, hkx, hky, kx, ky, dw};
      const int diff_ul[2] = {lr_ulx, lr_uly};
      for (SearchZone const& z : zones) {
        // the time budget (see above): a zone's L->R run and its R->L run are accounted one after the other, and either may end the list
        IBox lr, rr;
        vwgpu::zone_boxes(z, zl, &lr, &rr);
        const double next = P->seconds_per_op * ((double)lr.width() * lr.height() * z.range.width() * z.range.height());
        if (P->corr_timeout > 0 && estim + next > P->corr_timeout) break;
        estim += next;
        remeasure();
        bool cut = false;
        if (lr_active && !vwgpu::zone_is_empty(z)) {
          const double next2 = P->seconds_per_op * ((double)rr.width() * rr.height() * z.range.width() * z.range.height());
          cut = P->corr_timeout > 0 && estim + next2 > P->corr_timeout;
          if (!cut) estim += next2;
        }
        const vwgpu::ZoneErr ze = vwgpu::zone_tasks(z, zl, lr_active, !cut, 0, 0, diff_ul, &zt);
        if (ze) { ctx->forced_path = saved_force; return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s", zone_err_text(ze, false)); }
        if (cut) break;
      }
      const size_t rl_pixels = zt.rl;
      ctx->forced_path = saved_force;
      stamp("zone tables built", level);
      bool exact = cls[level].exact;
      for (vwgpu_zone_task const& z : t1) exact = exact && vwgpu_bm_exact_supported(z.sx, z.sy);
      if (ctx->trace & 2) {           // development aid: the shape of a level's work
        size_t px = 0, ev = 0; int maxd = 0, maxw = 0, maxh = 0;
        for (vwgpu_zone_task const& z : t1) { px += (size_t)z.zw * z.zh; ev += (size_t)z.zw * z.zh * z.sx * z.sy; maxd = std::max(maxd, z.sx * z.sy); maxw = std::max(maxw, z.zw); maxh = std::max(maxh, z.zh); }
        fprintf(stderr, "level %d: %zu zones, %zu px, %zu evaluations, max D %d, max zone %d x %d, exact %d\n", level, t1.size(), px, ev, maxd, maxw, maxh, (int)exact);
        // histogram of zone shapes: (width bucket, height bucket, disparities bucket) -> zones, evaluations
        std::map<std::string, std::pair<size_t, size_t>> hist;
        for (vwgpu_zone_task const& z : t1) {
          char key[96];
          snprintf(key, sizeof key, "w<=%d h<=%d sx<=%d sy<=%d", (z.zw + 15) / 16 * 16, (z.zh + 15) / 16 * 16, (z.sx + 3) / 4 * 4, (z.sy + 3) / 4 * 4);
          hist[key].first += 1; hist[key].second += (size_t)z.zw * z.zh * z.sx * z.sy;
        }
        for (auto const& kv : hist) fprintf(stderr, "    %-34s %6zu zones %12zu evaluations\n", kv.first.c_str(), kv.second.first, kv.second.second);
      }
      if (lr_active && rl_pixels) { if ((rc = vwgpu_arena_reserve(ctx, &ctx->zrl, rl_pixels * 12))) return rc; }
      // One matching pass over a zone list: the tile kernels when the level is order free; the tile kernels WITH certification plus the
      // exact-order kernels gated by the zone flags when it is finite but not order free; the exact-order kernels alone otherwise.
      // The exact-order launches behind a certified pass are queued only if some zone was flagged: the two directions' "any zone
      // flagged" words come back in one small copy (one more host round trip per certified level, hidden by the other tile threads;
      // twelve gated launches of ~6 us that find nothing to do are not — measured 0.25 ms of a 2 ms LoG + NCC tile).
      struct Pending { MatchPair m; const std::vector<vwgpu_zone_task>* tz; int32_t* dst; int* zflag; };
      std::vector<Pending> pending;
      int* d_any = nullptr;
      const unsigned char* need_cells = nullptr;
      // the "cannot matter" certificate of the certified passes (pyramid_plan.h, edge_margins)
      const int edge_k = rox - hkx;
      const EdgeMargins em = vwgpu::edge_margins(P, last, lr_diff != nullptr, level, rmb.x0, rmp[0].w, rw, dw);
      const int cert_hi = cls[level].cert_hi;
      auto match = [&](const MatchPair& m, std::vector<vwgpu_zone_task> const& tz, int32_t* dst, const int* need, int edge_m, int edge_lo, int edge_hi) -> int {
        if (tz.empty()) return VWGPU_OK;
        if (!exact) return vwgpu_launch_bm_zones(ctx, P->cost_type, m.a, m.aw, m.ah, m.b, m.bw, m.bh, kx, ky, tz.data(), (int)tz.size(), dst, cls[level].f32,
                                                 INT_MIN, nullptr, nullptr, nullptr, need, need ? need_cells : nullptr);
        if (cert_hi != INT_MIN) {
          if (!d_any) {                                            // the two "any zone flagged" words and the zone flags of both passes: one block, one fill
            const size_t nflag = 64 + t1.size() + t2.size();
            d_any = A.take<int>(nflag);
            if (!d_any) return fail_mem();
            VWGPU_HIP(ctx, hipMemsetAsync(d_any, 0, nflag * sizeof(int), st));
          }
          int* zflag = d_any + 64 + (pending.empty() ? 0 : t1.size());
          int rc2 = vwgpu_launch_bm_zones(ctx, P->cost_type, m.a, m.aw, m.ah, m.b, m.bw, m.bh, kx, ky, tz.data(), (int)tz.size(), dst, 0, cert_hi, zflag, d_cert_stats,
                                          d_any + pending.size(), need, need ? need_cells : nullptr, edge_m, edge_k, edge_lo, edge_hi);
          if (rc2) return rc2;
          pending.push_back(Pending{m, &tz, dst, zflag});
          return VWGPU_OK;
        }
        return vwgpu_launch_bm_exact(ctx, P->cost_type, m.a, m.aw, m.ah, m.aw, m.b, m.bw, m.bh, m.bw, kx, ky, tz.data(), (int)tz.size(), dst);
      };
      int32_t* rlbuf = static_cast<int32_t*>(ctx->zrl.base);
      const MatchPair l2r{Lv.p, Lv.w, Lv.h, Rv.p, Rv.w, Rv.h}, r2l{Rv.p, Rv.w, Rv.h, Lv.p, Lv.w, Lv.h};
      if ((rc = match(l2r, t1, disp, nullptr, em.m_lr, em.lr_lo, em.lr_hi))) return rc;
      if (lr_active && !t2.empty()) {
        // The R->L pass only has to cover what the L/R check will look at: the positions the L->R disparities point to — about the zone
        // itself instead of the zone widened by its search range (3x the pixels for a 16 x 16 leaf with 32 disparities).  Only where the
        // tile kernels match (their pixels are independent of each other); the exact-order kernels need the whole zone for their sums.
        int* need = nullptr;
        if (!exact || cert_hi != INT_MIN) {
          const size_t ncells = vwgpu_zone_need_cells(t3.data(), (int)t3.size());
          need = A.take<int>(8 * t3.size() + (ncells + 16 + 3) / 4);      // records, then the cell flags: one block, one fill
          if (!need) return fail_mem();
          unsigned char* cells = reinterpret_cast<unsigned char*>(need + 8 * t3.size());
          if ((rc = vwgpu_launch_zone_need(ctx, t3.data(), (int)t3.size(), disp, pending.empty() ? nullptr : pending[0].zflag, need, cells, ncells))) return rc;
          need_cells = cells;
        }
        if ((rc = match(r2l, t2, rlbuf, need, em.m_rl, em.rl_lo, em.rl_hi))) return rc;
      }
      if (!pending.empty()) {
        int any[2] = {0, 0};
        VWGPU_HIP(ctx, hipMemcpyAsync(any, d_any, sizeof any, hipMemcpyDeviceToHost, st));
        VWGPU_HIP(ctx, hipStreamSynchronize(st));
        // the flags of a pass come back in a second small copy, only when there are any
        std::vector<int> hflag;
        for (size_t k = 0; k < pending.size(); ++k) {
          if (!any[k]) continue;
          const Pending& q = pending[k];
          hflag.resize(q.tz->size());
          VWGPU_HIP(ctx, hipMemcpyAsync(hflag.data(), q.zflag, hflag.size() * sizeof(int), hipMemcpyDeviceToHost, st));
          VWGPU_HIP(ctx, hipStreamSynchronize(st));
          if ((rc = redo_flagged_zones(ctx, P, q.m, *q.tz, hflag.data(), -1, q.dst, level, k))) return rc;
        }
      }
      if (lr_active && (rc = vwgpu_launch_zone_lr(ctx, t3.data(), (int)t3.size(), disp, rlbuf, P->consistency_threshold, lr_diff, lr_stride))) return rc;
    } else if (!use_sgm)
    for (SearchZone const& z : zones) {
      const IBox lr(z.region.x0 + rox - hkx, z.region.y0 + roy - hky, z.region.x1 + rox + hkx, z.region.y1 + roy + hky);
      const IBox rr(lr.x0 + z.range.x0, lr.y0 + z.range.y0, lr.x1 + z.range.x0 + z.range.dx(), lr.y1 + z.range.y0 + z.range.dy());
      const double next = P->seconds_per_op * ((double)lr.width() * lr.height() * z.range.width() * z.range.height());
      if (P->corr_timeout > 0 && estim + next > P->corr_timeout) break;
      estim += next;
      remeasure();
      const int zw = z.region.dx(), zh = z.region.dy(), sx = z.range.dx(), sy = z.range.dy();
      if (zw <= 0 || zh <= 0 || sx <= 0 || sy <= 0) continue;
      // the crops normally lie inside the level images; edge-extend into scratch when rounding makes them stick out
      const float* lptr; ptrdiff_t lstr; const float* rptr; ptrdiff_t rstr;
      const int rneed_w = lr.dx() + sx - 1, rneed_h = lr.dy() + sy - 1;
      if ((size_t)lr.dx() * lr.dy() > tmp_a_px || (size_t)rneed_w * rneed_h > tmp_b_px) { ctx->forced_path = saved_force; return fail_mem(); }
      if (lr.x0 >= 0 && lr.y0 >= 0 && lr.x1 <= Lv.w && lr.y1 <= Lv.h) { lptr = Lv.p + (size_t)lr.y0 * Lv.w + lr.x0; lstr = Lv.w; }
      else {
        hipLaunchKernelGGL((crop_ext_kernel<float, 0>), grid2(lr.dx(), lr.dy()), kBlk, 0, st, Lv.p, Lv.w, Lv.w, Lv.h, lr.x0, lr.y0, tmp_a, lr.dx(), lr.dy());
        lptr = tmp_a; lstr = lr.dx();
      }
      if (rr.x0 >= 0 && rr.y0 >= 0 && rr.x0 + rneed_w <= Rv.w && rr.y0 + rneed_h <= Rv.h) { rptr = Rv.p + (size_t)rr.y0 * Rv.w + rr.x0; rstr = Rv.w; }
      else {
        hipLaunchKernelGGL((crop_ext_kernel<float, 0>), grid2(rneed_w, rneed_h), kBlk, 0, st, Rv.p, Rv.w, Rv.w, Rv.h, rr.x0, rr.y0, tmp_b, rneed_w, rneed_h);
        rptr = tmp_b; rstr = rneed_w;
      }
      int32_t* zout = disp + ((size_t)z.region.y0 * dw + z.region.x0) * 3;
      if (saved_force == VWGPU_PATH_NONE && level_path == VWGPU_PATH_EXACT_ORDER)
        ctx->forced_path = vwgpu_bm_exact_supported(sx, sy) ? VWGPU_PATH_EXACT_ORDER : VWGPU_PATH_GENERIC_F64;
      rc = vwgpu_calc_disparity_dev(ctx, P->cost_type, lptr, lr.dx(), lr.dy(), lstr, rptr, rneed_w, rneed_h, rstr, kx, ky, sx, sy, zout, dw);
      if (rc) { ctx->forced_path = saved_force; return rc; }
      if (P->consistency_threshold >= 0 && last) {                    // R->L run + L/R check (:654-694)
        const double next2 = P->seconds_per_op * ((double)rr.width() * rr.height() * z.range.width() * z.range.height());
        if (P->corr_timeout > 0 && estim + next2 > P->corr_timeout) break;
        estim += next2;
        const int aw = rr.dx(), ah = rr.dy();                          // "left" of this run: the right crop (edge-extended)
        const int bw2 = aw + sx - 1, bh2 = ah + sy - 1;                // "right": the left image from (lr.min - s)
        if ((size_t)aw * ah > tmp_b_px || (size_t)bw2 * bh2 > tmp_a_px) { ctx->forced_path = saved_force; return fail_mem(); }
        hipLaunchKernelGGL((crop_ext_kernel<float, 0>), grid2(aw, ah), kBlk, 0, st, Rv.p, Rv.w, Rv.w, Rv.h, rr.x0, rr.y0, tmp_b, aw, ah);
        hipLaunchKernelGGL((crop_ext_kernel<float, 0>), grid2(bw2, bh2), kBlk, 0, st, Lv.p, Lv.w, Lv.w, Lv.h, lr.x0 - sx, lr.y0 - sy, tmp_a, bw2, bh2);
        const int rlw = aw - kx + 1, rlh = ah - ky + 1;
        rc = vwgpu_calc_disparity_dev(ctx, P->cost_type, tmp_b, aw, ah, aw, tmp_a, bw2, bh2, bw2, kx, ky, sx, sy, rl, rlw);
        if (rc) { ctx->forced_path = saved_force; return rc; }
        hipLaunchKernelGGL(add_offset_kernel, grid2(rlw, rlh), kBlk, 0, st, rl, rlw, rlw, rlh, -sx, -sy);
        rc = vwgpu_launch_lr_check_diff(ctx, zout, zw, zh, dw, rl, rlw, rlh, rlw, P->consistency_threshold, lr_diff, lr_stride,
                                        z.region.x0 + lr_ulx, z.region.y0 + lr_uly);
        if (rc) { ctx->forced_path = saved_force; return rc; }
      }
      hipLaunchKernelGGL(add_offset_kernel, grid2(zw, zh), kBlk, 0, st, zout, dw, zw, zh, z.range.x0, z.range.y0);
    }
    ctx->forced_path = saved_force;
    stamp("matchers queued", level);
    // clean-up filters (:702-744)
    // (an intermediate block-matching level: the second filter pass and the mask are applied by the zone scheduler's kernel as it reads)
    const bool fused_extents = !last && !use_sgm && P->filter_half_kernel > 0 && P->blob_filter_area <= 0;
    // (the last level: the mask is applied by the kernel that writes the tile when nothing else reads the masked image)
    fused_finish = last && !use_sgm && P->filter_half_kernel > 0 && P->blob_filter_area <= 0 && !lr_diff;
    if (P->filter_half_kernel > 0) {
      rc = vwgpu_launch_disparity_filter(ctx, disp, dw, dh, P->filter_half_kernel, P->filter_half_kernel, 3.0, 0.5, !last, padded, disp2, fused_extents);
      if (rc) return rc;
      if (!fused_extents) {
        std::swap(disp, disp2);
        if (!fused_finish) {
          rc = vwgpu_launch_disparity_mask(ctx, disp, dw, dh, lmp[level].p, rmp[level].p, rmp[level].w, rmp[level].h);
          if (rc) return rc;
        }
      }
      if (!last && check_rl && use_sgm) {           // the R->L result seeds the next level's R->L run (:722-730)
        rc = vwgpu_launch_disparity_filter(ctx, rl_a, rlw, rlh, P->filter_half_kernel, P->filter_half_kernel, 3.0, 0.5, true, rl_pad, rl_b);
        if (rc) return rc;
        std::swap(rl_a, rl_b);
        rc = vwgpu_launch_disparity_mask(ctx, rl_a, rlw, rlh, rl_rmask, rl_lmask, lrm_w, lrm_h);
        if (rc) return rc;
      }
    }
    // the kernel based filtering tends to leave isolated blobs behind (:746-750)
    if (P->blob_filter_area > 0) {
      const int area = P->blob_filter_area / scaling;
      if ((rc = vwgpu_launch_blob_filter(ctx, disp, dw, dh, area, blob_scratch))) return rc;
      if (check_rl && !last && use_sgm && (rc = vwgpu_launch_blob_filter(ctx, rl_a, rlw, rlh, area, blob_scratch))) return rc;
    }
    if (use_sgm && !last) {                         // prev_disparity / prev_disparity_rl of the next level (:368-371)
      VWGPU_HIP(ctx, hipMemcpyAsync(prev_disp, disp, (size_t)dw * dh * 12, hipMemcpyDeviceToDevice, st));
      pdw = dw; pdh = dh;
      have_prev_rl = check_rl;
      if (check_rl) { std::swap(prev_rl, rl_a); prlw = rlw; prlh = rlh; }
    }
    // zone refinement (:754-799): the scheduler is data dependent host logic
    if (!last && !use_sgm) {
      // the accept / retry / merge recursion runs on the leaf table the device measured (zones.hip)
      const vwgpu::LeafExtent* h_ext = nullptr;
      size_t nleaf = 0;
      if ((rc = read_leaf_extents(ctx, 1, fused_extents, fused_extents ? padded : disp, 0, dw, dh, lmp[level].p, rmp[level].p, 0, rmp[level].w, rmp[level].h,
                                  stamp, level, &leaf_ext, &h_ext, &nleaf))) return rc;
      zones.clear();
      vwgpu::subdivide_regions_from_leaves(dw, dh, kx, ky, h_ext, nleaf, zones);
      vwgpu::rescale_zones(zones, IBox(0, 0, lmp[level - 1].w, lmp[level - 1].h),
                           IBox(0, 0, rp[level - 1].w - lp[level - 1].w, rp[level - 1].h - lp[level - 1].h), search);
      stamp("zones of the next level ready", level);
    }
  }
  if (dw != bw || dh != bh) return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "PyramidCorrelation: Solved disparity doesn't match requested bbox size.");
  if (lr_diff) hipLaunchKernelGGL(lr_diff_invalidate_kernel, grid2(bw, bh), kBlk, 0, st, disp, bw, bh, lr_diff, lr_stride, lr_ulx, lr_uly);
  if (use_sgm)
    hipLaunchKernelGGL(finish_sgm_kernel, grid2(bw, bh), kBlk, 0, st, disp, sub, bw, bh, (float)search.x0, (float)search.y0, out, os);
  else if (fused_finish)
    hipLaunchKernelGGL(finish_masked_kernel, grid2(bw, bh), kBlk, 0, st, disp, bw, bh, lmp[0].p, rmp[0].p, rmp[0].w, rmp[0].h, search.x0, search.y0, out, os);
  else
    hipLaunchKernelGGL(finish_kernel, grid2(bw, bh), kBlk, 0, st, disp, bw, bh, search.x0, search.y0, out, os);
  VWGPU_HIP(ctx, hipGetLastError());
  return read_cert_stats(ctx, d_cert_stats, true);
}

// ---- tile groups (round 5) ------------------------------------------------------------------------------------------
// vwgpu_pyramid_correlate_batch: several tiles of ONE image pair, of equal size, through the level loop TOGETHER.  The reference runs one
// tile per thread (src/vw/Image/ImageIO.h:228-251, BlockProcessor.h:52-176); here a tile is ~50 dependent launches of which the coarse levels
// are pure latency (images of 40 .. 300 pixels), and the device advances only 3 - 4 such chains at once however many tile threads feed it
// (profiles/r04_ubench_streams.txt).  A group of tiles shares every launch: the tiles' buffers have the same sizes (same bbox size, search
// range and kernel) and live in per-tile slices of one arena at a FIXED STRIDE, so a kernel finds tile t's image at base + t * slice
// (blockIdx.z / .y = the tile) and the zone matcher takes the zones of all tiles in one table (vwgpu_zone_group).  One host round trip per
// level serves the whole group: the leaf extents of all tiles come back together and the zone scheduler (zones.hip) runs per tile on them.
// Every tile's result is what vwgpu_pyramid_correlate_impl computes for it alone: same kernels, same arithmetic, same zone lists — the tiles
// never read each other's data.  Eligible: block matching without an lr_disp_diff image, blob filter or time budget; anything else runs
// tile by tile through vwgpu_pyramid_correlate_impl.
namespace {
template <class F> void pool_for(vwgpu_ctx* ctx, int n, F& f) {
  vwgpu_pool_run(ctx, n, [](void* a, int i) { (*static_cast<F*>(a))(i); }, &f);
}
}  // namespace

bool vwgpu_pyramid_group_eligible(const vwgpu_ctx* ctx, const vwgpu_pyramid_params* P, int n, const int* bw, const int* bh) {
  if (n < 2 || n > VWGPU_MAX_GROUP) return false;
  if (P->algorithm != 0 || P->lr_disp_diff || P->blob_filter_area > 0 || P->corr_timeout > 0) return false;
  if (ctx->forced_path != VWGPU_PATH_NONE || !vwgpu_bm_zones_supported(P->kernel_x, P->kernel_y)) return false;
  if ((size_t)(32 + 2 * P->filter_half_kernel) * (8 + 2 * P->filter_half_kernel) * 13 > 64 * 1024) return false;      // (the LDS form of the clean-up filter)
  for (int i = 1; i < n; ++i) if (bw[i] != bw[0] || bh[i] != bh[0]) return false;
  return bw[0] > 0 && bh[0] > 0;
}

// All pointers are device pointers (masks may be null).  outs[t]: bw x bh x 3 floats with row stride oss[t] pixels.
int vwgpu_pyramid_group_impl(vwgpu_ctx* ctx, const float* left, int lw, int lh, ptrdiff_t ls, const float* right, int rw, int rh, ptrdiff_t rs,
                             const uint8_t* lmask, ptrdiff_t lms, const uint8_t* rmask, ptrdiff_t rms, const vwgpu_pyramid_params* P,
                             int n, const int* bxs, const int* bys, int bw, int bh, float* const* outs, const ptrdiff_t* oss) {
  const int kx = P->kernel_x, ky = P->kernel_y;
  const IBox search(P->search_min_x, P->search_min_y, P->search_max_x, P->search_max_y);
  hipStream_t st = ctx->stream;
  // levels, geometry and slice layout: the same for every tile of the group but for the tile's place in the images
  const int L = vwgpu::pyramid_levels(P, bw, bh);
  const int hkx = kx / 2, hky = ky / 2, up = 1 << L;
  const bool filtered = P->prefilter_mode == VWGPU_PREFILTER_LOG || P->prefilter_mode == VWGPU_PREFILTER_MEANSUB;
  const Stamp stamp{(ctx->trace & 1) != 0, n};
  TileGeom G[VWGPU_MAX_GROUP];
  for (int t = 0; t < n; ++t) G[t] = vwgpu::tile_geom(bxs[t], bys[t], bw, bh, search, hkx, hky, up);
  const PyrLayout Y = vwgpu::pyr_layout(G[0], L, filtered);
  // group-level tables behind the slices: the certified passes' flag words, the R->L need records and cells (bounds as in the single-tile arena)
  const size_t tables = (size_t)n * ((size_t)(L + 1) * ((size_t)bw * bh / 64 + 64) * (48 + (size_t)(search.dx() / 16 + 3) * (search.dy() / 16 + 3)) + 8192) + (1 << 16);
  int rc = vwgpu_arena_reserve(ctx, &ctx->pyr, (size_t)n * Y.slice + tables);
  if (rc) return rc;
  const Slices S{static_cast<char*>(ctx->pyr.base), Y.slice};
  Bump GA{S.base + (size_t)n * Y.slice, tables};
  auto fail_mem = [&]() { return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "pyramid_correlate (group): internal arena too small"); };
  const size_t slice_f = Y.slice / 4, slice_i = Y.slice / 4, slice_px = Y.slice / 12;

  bool alive[VWGPU_MAX_GROUP];             // false: a fully masked image (the tile is zeros, CorrelationView.cc:318-327)
  std::vector<LevelClass> cls((size_t)n * (L + 1));
  const PyrSource src{left, lw, lh, ls, right, rw, rh, rs, lmask, lms, rmask, rms};
  if ((rc = build_pyramids(ctx, src, P, n, G, Y, S, true, false, &stamp, alive, cls.data()))) return rc;
  std::vector<SearchZone> zones[VWGPU_MAX_GROUP];
  unsigned long long* d_cert_stats = nullptr;
  if (ctx->trace & 4) {
    d_cert_stats = GA.take<unsigned long long>(4);
    if (!d_cert_stats) return fail_mem();
    VWGPU_HIP(ctx, hipMemsetAsync(d_cert_stats, 0, 32, st));
  }
  for (int t = 0; t < n; ++t)
    if (alive[t]) zones[t].push_back(SearchZone{IBox(0, 0, Y.lmw[L], Y.lmh[L]), IBox(0, 0, search.width() / up + 1, search.height() / up + 1)});

  // ---- level loop ----
  size_t disp_off = Y.disp, disp2_off = Y.disp2;                   // (the two disparity buffers of every tile swap together)
  int dw = 0, dh = 0;
  for (int level = L; level >= 0; --level) {
    const bool last = (level == 0);
    const int scaling = 1 << level;
    dw = Y.lmw[level]; dh = Y.lmh[level];
    {
      const size_t words = ((size_t)dw * dh * 12 + 15) / 16;      // (the buffers are 256-byte aligned and sized for the largest level; rounding up stays inside)
      hipLaunchKernelGGL(zero_tiles_kernel, dim3((unsigned)std::min<size_t>(512, (words + 255) / 256), (unsigned)n), dim3(256), 0, st,
                         reinterpret_cast<uint4*>(S.at(0, disp_off)), Y.slice / 16, words);
    }
    int32_t* disp0 = S.i(0, disp_off);
    const int rox = up * hkx / scaling, roy = up * hky / scaling;
    const bool lr_active = P->consistency_threshold >= 0 && last;
    const int aw_ = Y.lpw[level], ah_ = Y.lph[level], bw_ = Y.rpw[level], bh_ = Y.rph[level];
    const float* A0 = S.f(0, Y.lpf[level]);
    const float* B0 = S.f(0, Y.rpf[level]);
    // zone tasks of every tile, sorted into the kernel classes of this level: 0 = order free with float32 sums, 1 = order free, 2 = certified,
    // 3 = the reference's order only (a non-finite pixel, or VWGPU_OPT_CERTIFY = 0)
    std::vector<vwgpu_zone_task> t1[4], t2[4], t3[4];
    int kcls[VWGPU_MAX_GROUP];
    std::fill(kcls, kcls + n, -1);
    size_t rl_pixels = 0;
    // per tile on the helper threads (R->L offsets local to the tile), then strung together per class
    struct TileTasks : ZoneTasks { vwgpu::ZoneErr err = vwgpu::ZONE_OK; };
    std::vector<TileTasks> TT((size_t)n);
    const ZoneLevel zl{rox, roy, hkx, hky, kx, ky, dw};
    auto build_tile = [&](int t) {
      TileTasks& tt = TT[t];
      if (!alive[t]) return;
      const LevelClass& lc = cls[(size_t)t * (L + 1) + level];
      bool exact = lc.exact;
      for (SearchZone const& z : zones[t])
        if (z.range.dx() > 0 && z.range.dy() > 0) exact = exact && vwgpu_bm_exact_supported(z.range.dx(), z.range.dy());      // (as the single-tile path: the tile kernels otherwise)
      kcls[t] = exact ? (lc.cert_hi != INT_MIN ? 2 : 3) : (lc.f32 ? 0 : 1);
      tt.a.reserve(zones[t].size());
      if (lr_active) { tt.b.reserve(zones[t].size()); tt.c.reserve(zones[t].size()); }
      for (SearchZone const& z : zones[t])
        if ((tt.err = vwgpu::zone_tasks(z, zl, lr_active, true, (long long)t * (long long)slice_px, t, nullptr, &tt))) return;
    };
    {
      size_t nz = 0;
      for (int t = 0; t < n; ++t) nz += zones[t].size();
      if (nz >= 1024) pool_for(ctx, n, build_tile);                 // (waking the helpers costs tens of microseconds: not for the coarse levels)
      else for (int t = 0; t < n; ++t) build_tile(t);
    }
    for (int t = 0; t < n; ++t) {
      TileTasks& tt = TT[t];
      if (tt.err) return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s", zone_err_text(tt.err, true));
      if (rl_pixels + tt.rl > (size_t)INT32_MAX / 2) return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s", zone_err_text(vwgpu::ZONE_LR_TOO_LARGE, true));
      if (kcls[t] < 0) continue;
      const int c = kcls[t], base = (int)rl_pixels;
      t1[c].insert(t1[c].end(), tt.a.begin(), tt.a.end());
      for (vwgpu_zone_task& b : tt.b) b.out_off += base;
      for (vwgpu_zone_task& cc : tt.c) cc.ax += base;
      t2[c].insert(t2[c].end(), tt.b.begin(), tt.b.end());
      t3[c].insert(t3[c].end(), tt.c.begin(), tt.c.end());
      rl_pixels += tt.rl;
    }
    stamp("zone tasks built", level);
    if (lr_active && rl_pixels) { if ((rc = vwgpu_arena_reserve(ctx, &ctx->zrl, rl_pixels * 12))) return rc; }
    int32_t* rlbuf = static_cast<int32_t*>(ctx->zrl.base);
    // the "cannot matter" certificate (pyramid_plan.h, edge_margins): margins per level, bounds per tile
    const int edge_k = rox - hkx;
    int edge_m_lr = 0, edge_m_rl = 0;
    int lr_lo[VWGPU_MAX_GROUP], lr_hi[VWGPU_MAX_GROUP], rl_lo[VWGPU_MAX_GROUP], rl_hi[VWGPU_MAX_GROUP], hi_img[VWGPU_MAX_GROUP];
    for (int t = 0; t < n; ++t) {
      const EdgeMargins em = vwgpu::edge_margins(P, last, false, level, G[t].rmb.x0, Y.rmw[0], rw, dw);
      edge_m_lr = em.m_lr; edge_m_rl = em.m_rl;
      lr_lo[t] = em.lr_lo; lr_hi[t] = em.lr_hi; rl_lo[t] = em.rl_lo; rl_hi[t] = em.rl_hi;
      hi_img[t] = cls[(size_t)t * (L + 1) + level].cert_hi;
    }
    const MatchPair l2r{A0, aw_, ah_, B0, bw_, bh_}, r2l{B0, bw_, bh_, A0, aw_, ah_};      // tile 0's; tile t's images lie t slices on
    auto of_tile = [&](MatchPair m, int t) { m.a += (size_t)t * slice_f; m.b += (size_t)t * slice_f; return m; };
    vwgpu_zone_group grp;
    grp.n_img = n; grp.a_stride = slice_f; grp.b_stride = slice_f;
    // certified classes: flag words {any per pass and tile: 2 n} + zone flags of both passes, one block, one fill
    int* d_any = nullptr; int* zflag1 = nullptr; int* zflag2 = nullptr;
    if (!t1[2].empty()) {
      const size_t nflag = 64 + 2 * (size_t)n + t1[2].size() + t2[2].size();
      d_any = GA.take<int>(nflag);
      if (!d_any) return fail_mem();
      VWGPU_HIP(ctx, hipMemsetAsync(d_any, 0, nflag * sizeof(int), st));
      zflag1 = d_any + 64 + 2 * n; zflag2 = zflag1 + t1[2].size();
    }
    for (int c = 0; c < 4; ++c) {
      if (t1[c].empty()) continue;
      if (c == 3) {                                              // the reference's order: tile by tile (zones of one image pair per call)
        for (int t = 0; t < n; ++t) {
          if (kcls[t] != 3) continue;
          std::vector<vwgpu_zone_task> za, zb;
          for (auto const& z : t1[3]) if (z.img == t) za.push_back(z);
          for (auto const& z : t2[3]) if (z.img == t) zb.push_back(z);
          const MatchPair m = of_tile(l2r, t);
          if (!za.empty() && (rc = vwgpu_launch_bm_exact(ctx, P->cost_type, m.a, aw_, ah_, aw_, m.b, bw_, bh_, bw_, kx, ky, za.data(), (int)za.size(), disp0))) return rc;
          if (!zb.empty() && (rc = vwgpu_launch_bm_exact(ctx, P->cost_type, m.b, bw_, bh_, bw_, m.a, aw_, ah_, aw_, kx, ky, zb.data(), (int)zb.size(), rlbuf))) return rc;
        }
        continue;
      }
      const bool cert = c == 2;
      grp.cert_hi = cert ? hi_img : nullptr;
      grp.edge_lo = lr_lo; grp.edge_hi = lr_hi;
      rc = vwgpu_launch_bm_zones(ctx, P->cost_type, A0, aw_, ah_, B0, bw_, bh_, kx, ky, t1[c].data(), (int)t1[c].size(), disp0, c == 0 ? 1 : 0,
                                 cert ? 0 : INT_MIN, cert ? zflag1 : nullptr, cert ? d_cert_stats : nullptr, cert ? d_any : nullptr, nullptr, nullptr,
                                 cert ? edge_m_lr : 0, edge_k, 0, 0, 0, 0, &grp);
      if (rc) return rc;
      if (lr_active && !t2[c].empty()) {
        const size_t ncells = vwgpu_zone_need_cells(t3[c].data(), (int)t3[c].size());
        int* need = GA.take<int>(8 * t3[c].size() + (ncells + 16 + 3) / 4);
        if (!need) return fail_mem();
        unsigned char* cells = reinterpret_cast<unsigned char*>(need + 8 * t3[c].size());
        if ((rc = vwgpu_launch_zone_need(ctx, t3[c].data(), (int)t3[c].size(), disp0, cert ? zflag1 : nullptr, need, cells, ncells))) return rc;
        std::swap(grp.a_stride, grp.b_stride);                    // (equal anyway: the R->L pass matches the right image against the left)
        grp.edge_lo = rl_lo; grp.edge_hi = rl_hi;
        rc = vwgpu_launch_bm_zones(ctx, P->cost_type, B0, bw_, bh_, A0, aw_, ah_, kx, ky, t2[c].data(), (int)t2[c].size(), rlbuf, c == 0 ? 1 : 0,
                                   cert ? 0 : INT_MIN, cert ? zflag2 : nullptr, cert ? d_cert_stats : nullptr, cert ? d_any + n : nullptr, need, cells,
                                   cert ? edge_m_rl : 0, edge_k, 0, 0, 0, 0, &grp);
        if (rc) return rc;
      }
    }
    stamp("matchers queued", level);
    if (d_any) {
      // the flagged zones of the certified passes, per tile: one small read-back for the group, a second one only when some zone was flagged
      std::vector<int> any(2 * (size_t)n, 0);
      VWGPU_HIP(ctx, hipMemcpyAsync(any.data(), d_any, any.size() * sizeof(int), hipMemcpyDeviceToHost, st));
      VWGPU_HIP(ctx, hipStreamSynchronize(st));
      bool some[2] = {false, false};
      for (int t = 0; t < n; ++t) { some[0] = some[0] || any[t]; some[1] = some[1] || any[n + t]; }
      for (int pass = 0; pass < 2; ++pass) {
        if (!some[pass]) continue;
        const std::vector<vwgpu_zone_task>& tz = pass ? t2[2] : t1[2];
        std::vector<int> hflag(tz.size());
        VWGPU_HIP(ctx, hipMemcpyAsync(hflag.data(), pass ? zflag2 : zflag1, hflag.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        VWGPU_HIP(ctx, hipStreamSynchronize(st));
        for (int t = 0; t < n; ++t)
          if (any[pass * n + t] && (rc = redo_flagged_zones(ctx, P, of_tile(pass ? r2l : l2r, t), tz, hflag.data(), t, pass ? rlbuf : disp0, -1, pass))) return rc;
      }
    }
    if (lr_active)
      for (int c = 0; c < 4; ++c)
        if (!t3[c].empty() && (rc = vwgpu_launch_zone_lr(ctx, t3[c].data(), (int)t3[c].size(), disp0, rlbuf, P->consistency_threshold, nullptr, 0))) return rc;
    // ---- clean-up filters (:702-744) ----
    int32_t* disp2_0 = S.i(0, disp2_off);
    int32_t* padded0 = S.i(0, Y.padded);
    const bool fused_extents = !last && P->filter_half_kernel > 0;       // second filter pass + mask applied by the zone scheduler's kernel as it reads
    if (P->filter_half_kernel > 0) {
      rc = vwgpu_launch_disparity_filter(ctx, disp0, dw, dh, P->filter_half_kernel, P->filter_half_kernel, 3.0, 0.5, !last, padded0, disp2_0, true, n, slice_i);
      if (rc) return rc;
      if (last) std::swap(disp_off, disp2_off);
    }
    // ---- zone refinement (:754-799): leaf extents of every tile in one launch, one copy, one synchronisation ----
    if (!last) {
      std::vector<vwgpu::LeafExtent> own;
      const vwgpu::LeafExtent* h_ext = nullptr;
      size_t nleaf = 0;
      if ((rc = read_leaf_extents(ctx, n, fused_extents, fused_extents ? padded0 : S.i(0, disp_off), slice_i, dw, dh, S.b(0, Y.lmp[level]), S.b(0, Y.rmp[level]),
                                  Y.slice, Y.rmw[level], Y.rmh[level], stamp, level, &own, &h_ext, &nleaf))) return rc;
      const IBox scale_search(0, 0, Y.rpw[level - 1] - Y.lpw[level - 1], Y.rph[level - 1] - Y.lph[level - 1]);
      const IBox next_size(0, 0, Y.lmw[level - 1], Y.lmh[level - 1]);
      auto refine_tile = [&](int t) {                               // (helper threads: the scheduler keeps its tree of boxes per thread)
        if (!alive[t]) return;
        zones[t].clear();
        vwgpu::subdivide_regions_from_leaves(dw, dh, kx, ky, h_ext + (size_t)t * nleaf, nleaf, zones[t]);
        vwgpu::rescale_zones(zones[t], next_size, scale_search, search);
      };
      if (nleaf * (size_t)n >= 2048) pool_for(ctx, n, refine_tile);
      else for (int t = 0; t < n; ++t) refine_tile(t);
      stamp("zones of the next level ready", level);
    }
  }
  stamp("last level queued", 0);
  if (dw != bw || dh != bh) return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "PyramidCorrelation: Solved disparity doesn't match requested bbox size.");
  {
    GroupOuts go;
    for (int t = 0; t < VWGPU_MAX_GROUP; ++t) { go.out[t] = nullptr; go.os[t] = 0; go.mode[t] = 0; }
    for (int t = 0; t < n; ++t) { go.out[t] = outs[t]; go.os[t] = oss[t]; go.mode[t] = !alive[t] ? 3 : (P->filter_half_kernel > 0 ? 2 : 1); }
    hipLaunchKernelGGL(finish_group_kernel, dim3((bw + 63) / 64, (bh + 3) / 4, (unsigned)n), kBlk, 0, st, go, S.i(0, disp_off), slice_i, bw, bh,
                       S.b(0, Y.lmp[0]), S.b(0, Y.rmp[0]), Y.slice, Y.rmw[0], Y.rmh[0], search.x0, search.y0);
  }
  VWGPU_HIP(ctx, hipGetLastError());
  return read_cert_stats(ctx, d_cert_stats, false);
}

// ---- extern "C" entry points ------------------------------------------------------------------------------------

extern "C" {

int vwgpu_subdivide_regions(const int32_t* disp, int w, int h, int kx, int ky, int32_t* zones, int cap) {
  if (!disp || w <= 0 || h <= 0 || kx < 1 || ky < 1 || cap < 0 || (cap && !zones)) return VWGPU_ERR_ARGUMENT;
  std::vector<SearchZone> list;
  vwgpu::subdivide_regions(disp, w, h, kx, ky, list);
  int n = 0;
  for (SearchZone const& z : list) {
    if (n < cap) {
      int32_t* o = zones + (size_t)n * 8;
      o[0] = z.region.x0; o[1] = z.region.y0; o[2] = z.region.x1; o[3] = z.region.y1;
      o[4] = z.range.x0; o[5] = z.range.y0; o[6] = z.range.x1; o[7] = z.range.y1;
    }
    ++n;
  }
  return n;
}

// a row stride of 0 stands for dense rows
static void default_strides(int lw, int rw, ptrdiff_t* ls, ptrdiff_t* rs, ptrdiff_t* lms, ptrdiff_t* rms) {
  if (*ls == 0) *ls = lw;
  if (*rs == 0) *rs = rw;
  if (*lms == 0) *lms = lw;
  if (*rms == 0) *rms = rw;
}

// CorrelationView.cc:277-283
static const char kLrDiffDomain[] = "The L-R to R-L difference image domain does not contain the current tile.";
static bool tile_outside_lr_diff(const vwgpu_pyramid_params* P, int bx, int by, int bw, int bh) {
  return P->lr_disp_diff && (bx < P->region_ul_x || by < P->region_ul_y || bx + bw > P->region_ul_x + P->lr_disp_diff_cols ||
                             by + bh > P->region_ul_y + P->lr_disp_diff_rows);
}

// the end of the run of consecutive tiles of equal size that begins at t0, at most `cap` tiles: what one group can take
static int equal_tiles_run(const int* bw, const int* bh, int t0, int n_tiles, int cap) {
  int t1 = t0 + 1;
  while (t1 < n_tiles && t1 - t0 < cap && bw[t1] == bw[t0] && bh[t1] == bh[t0]) ++t1;
  return t1;
}

static int check_pyramid_args(vwgpu_ctx* ctx, const void* l, int lw, int lh, const void* r, int rw, int rh,
                              const vwgpu_pyramid_params* P, int bw, int bh, const void* out) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!l || !r || !out || !P || lw <= 0 || lh <= 0 || rw <= 0 || rh <= 0 || bw <= 0 || bh <= 0)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate: empty image / tile or null pointer");
  if (P->kernel_x < 1 || P->kernel_y < 1 || P->kernel_x % 2 != 1 || P->kernel_y % 2 != 1)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate: Kernel input not sized with odd values.");
  if (P->search_max_x <= P->search_min_x || P->search_max_y <= P->search_min_y)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "PyramidCorrelationView: Invalid search region: (%d,%d)-(%d,%d); a box of zero height is empty (use height >= 1)",
                      P->search_min_x, P->search_min_y, P->search_max_x, P->search_max_y);
  if (P->algorithm == 0 && (P->cost_type < VWGPU_ABSOLUTE_DIFFERENCE || P->cost_type > VWGPU_CROSS_CORRELATION))
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "pyramid_correlate: cost type %d is not a block-matching cost", P->cost_type);
  if (P->algorithm < 0 || P->algorithm > 3)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "pyramid_correlate: algorithm %d is none of VW_CORRELATION_BM / _SGM / _MGM / _FINAL_MGM", P->algorithm);
  if (P->algorithm != 0) {
    if (P->cost_type != VWGPU_CENSUS_TRANSFORM && P->cost_type != VWGPU_TERNARY_CENSUS_TRANSFORM)
      return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "With SGM/MGM, only the census transform cost mode gives good results.");
    if (P->kernel_x != P->kernel_y || (P->kernel_x != 3 && P->kernel_x != 5 && P->kernel_x != 7 && P->kernel_x != 9))
      return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "Census transforms are only available in size 3, 5, 7, and 9.");
  }
  if (P->blob_filter_area < 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate: negative blob filter area");
  if (P->lr_disp_diff) {          // CorrelationView.cc:277-283
    const ptrdiff_t st = P->lr_disp_diff_stride ? P->lr_disp_diff_stride : P->lr_disp_diff_cols;
    if (P->lr_disp_diff_cols <= 0 || P->lr_disp_diff_rows <= 0 || st < P->lr_disp_diff_cols)
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate: bad lr_disp_diff geometry");
  }
  if (P->max_pyramid_levels < 0 || P->filter_half_kernel < 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate: negative level / filter size");
  return VWGPU_OK;
}

int vwgpu_pyramid_correlate_dev(vwgpu_ctx* ctx, const float* d_left, int lw, int lh, ptrdiff_t ls,
                                const float* d_right, int rw, int rh, ptrdiff_t rs,
                                const uint8_t* d_lmask, ptrdiff_t lms, const uint8_t* d_rmask, ptrdiff_t rms,
                                const vwgpu_pyramid_params* P, int bx, int by, int bw, int bh, float* d_out, ptrdiff_t os) {
  int rc = check_pyramid_args(ctx, d_left, lw, lh, d_right, rw, rh, P, bw, bh, d_out);
  if (rc) return rc;
  default_strides(lw, rw, &ls, &rs, &lms, &rms);
  if (os == 0) os = bw;
  if (ls < lw || rs < rw || lms < lw || rms < rw || os < bw) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate: row stride smaller than row width");
  if (tile_outside_lr_diff(P, bx, by, bw, bh)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, kLrDiffDomain);
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return vwgpu_pyramid_correlate_impl(ctx, d_left, lw, lh, ls, d_right, rw, rh, rs, d_lmask, lms, d_rmask, rms, P, bx, by, bw, bh, d_out, os,
                                      P->lr_disp_diff);
}

int vwgpu_pyramid_correlate_batch_dev(vwgpu_ctx* ctx, const float* d_left, int lw, int lh, ptrdiff_t ls,
                                      const float* d_right, int rw, int rh, ptrdiff_t rs,
                                      const uint8_t* d_lmask, ptrdiff_t lms, const uint8_t* d_rmask, ptrdiff_t rms,
                                      const vwgpu_pyramid_params* P, int n_tiles, const int* bx, const int* by, const int* bw, const int* bh,
                                      float* const* d_outs, const ptrdiff_t* os) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (n_tiles < 0 || (n_tiles > 0 && (!bx || !by || !bw || !bh || !d_outs))) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate_batch: null tile table");
  default_strides(lw, rw, &ls, &rs, &lms, &rms);
  for (int t = 0; t < n_tiles; ++t) {
    int rc = check_pyramid_args(ctx, d_left, lw, lh, d_right, rw, rh, P, bw[t], bh[t], d_outs[t]);
    if (rc) return rc;
    if (os && os[t] != 0 && os[t] < bw[t]) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate: row stride smaller than row width");
  }
  if (n_tiles == 0) return VWGPU_OK;
  if (ls < lw || rs < rw || lms < lw || rms < rw) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate: row stride smaller than row width");
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  // groups: runs of consecutive tiles of equal size, at most VWGPU_MAX_GROUP each; what a group cannot take (SGM / MGM, lr_disp_diff, blob
  // filter, time budget, a forced kernel family) and lone tiles go through the single-tile entry — same results either way
  int t0 = 0, cap = VWGPU_MAX_GROUP;                   // cap: halved when a group's arena does not fit the device
  while (t0 < n_tiles) {
    const int t1 = equal_tiles_run(bw, bh, t0, n_tiles, cap);
    const int m = t1 - t0;
    if (m > 1 && vwgpu_pyramid_group_eligible(ctx, P, m, bw + t0, bh + t0)) {
      ptrdiff_t oss[VWGPU_MAX_GROUP];
      for (int t = 0; t < m; ++t) oss[t] = (os && os[t0 + t]) ? os[t0 + t] : bw[t0 + t];
      int rc = vwgpu_pyramid_group_impl(ctx, d_left, lw, lh, ls, d_right, rw, rh, rs, d_lmask, lms, d_rmask, rms, P, m, bx + t0, by + t0, bw[t0], bh[t0], d_outs + t0, oss);
      if (rc == VWGPU_ERR_NOMEM) {
        // n slices + the group's tables did not fit where the single-tile entry's arena would: the batch entry must never be less robust
        // than a loop over the single-tile entry.  Nothing of the group has been written (the reservation comes first): smaller groups.
        ctx->err.clear();
        cap = m / 2;
        continue;
      }
      if (rc) return rc;
    } else {
      for (int t = t0; t < t1; ++t) {
        if (tile_outside_lr_diff(P, bx[t], by[t], bw[t], bh[t])) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, kLrDiffDomain);
        int rc = vwgpu_pyramid_correlate_impl(ctx, d_left, lw, lh, ls, d_right, rw, rh, rs, d_lmask, lms, d_rmask, rms, P, bx[t], by[t], bw[t], bh[t], d_outs[t],
                                              (os && os[t]) ? os[t] : bw[t], P->lr_disp_diff);
        if (rc) return rc;
      }
    }
    t0 = t1;
  }
  return VWGPU_OK;
}

// Only the window of the sources a tile can touch goes to the device — the reference's prerasterize also pulls just
// its padded ROIs through the views (CorrelationView.cc:89-97) — not the whole images: a 1024^2 tile of a 32768^2 pair
// stages ~2000^2 pixels per image.  Window = the box [x0, x1) x [y0, y1) (a tile, or the union of a run of tiles) grown by
// half_kernel * 2^max_levels (pyramid padding), twice the search extent (R->L runs of the SGM branch) and the search
// range itself, cut at the image borders; both images and masks share the window origin, so disparities and the edge
// extension at true image borders are unchanged.
struct pyr_window {
  int ox, oy, lww, lwh, rww, rwh;   // origin; sizes of the left and the right window
  long long gx, gy;                 // the growth of a side, border cuts aside, with the whole search range on either side (the run heuristic's measure)
};
static pyr_window pyramid_window(const vwgpu_pyramid_params* P, long long x0, long long y0, long long x1, long long y1, int lw, int lh, int rw, int rh) {
  const int upb = 1 << std::max(0, std::min(P->max_pyramid_levels, 12));
  const int sdx = P->search_max_x - P->search_min_x, sdy = P->search_max_y - P->search_min_y;
  const long long padx = (long long)(P->kernel_x / 2) * upb + 2LL * std::max(sdx, 0) + 8;
  const long long pady = (long long)(P->kernel_y / 2) * upb + 2LL * std::max(sdy, 0) + 8;
  const long long sx0 = std::min(P->search_min_x, 0), sy0 = std::min(P->search_min_y, 0);
  const long long sx1 = std::max(P->search_max_x, 0), sy1 = std::max(P->search_max_y, 0);
  const long long wx0 = std::max<long long>(0, x0 - padx + sx0), wy0 = std::max<long long>(0, y0 - pady + sy0);
  const long long wx1 = x1 + padx + sx1, wy1 = y1 + pady + sy1;
  pyr_window W;
  W.ox = (int)std::min<long long>(wx0, std::min(lw, rw)); W.oy = (int)std::min<long long>(wy0, std::min(lh, rh));
  W.lww = (int)(std::min<long long>(wx1, lw) - W.ox); W.lwh = (int)(std::min<long long>(wy1, lh) - W.oy);
  W.rww = (int)(std::min<long long>(wx1, rw) - W.ox); W.rwh = (int)(std::min<long long>(wy1, rh) - W.oy);
  W.gx = padx + sx1 - sx0; W.gy = pady + sy1 - sy0;
  return W;
}

// The two images and the two masks of a window: pieces 0 .. 3 of a plan.  The mask pieces are reserved whether or not there are masks.
static void stage_window(vwgpu_stage& st, const pyr_window& W, const float* left, ptrdiff_t ls, const float* right, ptrdiff_t rs,
                         const uint8_t* lmask, ptrdiff_t lms, const uint8_t* rmask, ptrdiff_t rms) {
  st.add(left + (ptrdiff_t)W.oy * ls + W.ox, W.lww, W.lwh, 4, ls, VWGPU_STAGE_IN);
  st.add(right + (ptrdiff_t)W.oy * rs + W.ox, W.rww, W.rwh, 4, rs, VWGPU_STAGE_IN);
  st.add(lmask ? lmask + (ptrdiff_t)W.oy * lms + W.ox : nullptr, W.lww, W.lwh, 1, lms, lmask ? VWGPU_STAGE_IN : VWGPU_STAGE_NONE);
  st.add(rmask ? rmask + (ptrdiff_t)W.oy * rms + W.ox : nullptr, W.rww, W.rwh, 1, rms, rmask ? VWGPU_STAGE_IN : VWGPU_STAGE_NONE);
}

// One run of tiles of the host batch entry: ONE staged window W (the union of what the run's tiles can touch), one device batch call.
static_assert(4 + VWGPU_MAX_GROUP <= vwgpu_stage::MAX_PIECES, "a run's window and outputs must fit one staging plan");
static int pyramid_batch_host_run(vwgpu_ctx* ctx, const pyr_window& W, const float* left, ptrdiff_t ls, const float* right, ptrdiff_t rs,
                                  const uint8_t* lmask, ptrdiff_t lms, const uint8_t* rmask, ptrdiff_t rms, const vwgpu_pyramid_params* P, int n_tiles,
                                  const int* bx, const int* by, const int* bw, const int* bh, float* const* outs, const ptrdiff_t* os) {
  if (W.lww <= 0 || W.lwh <= 0 || W.rww <= 0 || W.rwh <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate: the tiles lie outside the images");
  vwgpu_stage st(ctx);
  stage_window(st, W, left, ls, right, rs, lmask, lms, rmask, rms);
  for (int t = 0; t < n_tiles; ++t) st.add(outs[t], bw[t], bh[t], 12, (os && os[t]) ? os[t] : bw[t], VWGPU_STAGE_OUT);
  int rc = st.commit();
  if (rc) return rc;
  int wbx[VWGPU_MAX_GROUP], wby[VWGPU_MAX_GROUP];
  float* d_outs[VWGPU_MAX_GROUP];
  for (int t = 0; t < n_tiles; ++t) {
    wbx[t] = bx[t] - W.ox; wby[t] = by[t] - W.oy;
    d_outs[t] = st.dev<float>(4 + t);
  }
  rc = vwgpu_pyramid_correlate_batch_dev(ctx, st.dev<float>(0), W.lww, W.lwh, W.lww, st.dev<float>(1), W.rww, W.rwh, W.rww, lmask ? st.dev<uint8_t>(2) : nullptr, W.lww,
                                         rmask ? st.dev<uint8_t>(3) : nullptr, W.rww, P, n_tiles, wbx, wby, bw, bh, d_outs, nullptr);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_pyramid_correlate_batch(vwgpu_ctx* ctx, const float* left, int lw, int lh, ptrdiff_t ls,
                                  const float* right, int rw, int rh, ptrdiff_t rs,
                                  const uint8_t* lmask, ptrdiff_t lms, const uint8_t* rmask, ptrdiff_t rms,
                                  const vwgpu_pyramid_params* P, int n_tiles, const int* bx, const int* by, const int* bw, const int* bh,
                                  float* const* outs, const ptrdiff_t* os) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (n_tiles < 0 || (n_tiles > 0 && (!bx || !by || !bw || !bh || !outs))) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate_batch: null tile table");
  if (n_tiles == 0) return VWGPU_OK;
  // an lr_disp_diff image is staged per tile by the single-tile entry (concurrent tiles must not write back each other's pixels)
  if (P && P->lr_disp_diff) {
    for (int t = 0; t < n_tiles; ++t) {
      int rc = vwgpu_pyramid_correlate(ctx, left, lw, lh, ls, right, rw, rh, rs, lmask, lms, rmask, rms, P, bx[t], by[t], bw[t], bh[t], outs[t], os ? os[t] : 0);
      if (rc) return rc;
    }
    return VWGPU_OK;
  }
  for (int t = 0; t < n_tiles; ++t) {
    int rc = check_pyramid_args(ctx, left, lw, lh, right, rw, rh, P, bw[t], bh[t], outs[t]);
    if (rc) return rc;
  }
  default_strides(lw, rw, &ls, &rs, &lms, &rms);
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  // Staged per RUN of tiles (consecutive tiles of equal size, at most VWGPU_MAX_GROUP: what one device group takes), not per call: tiles
  // scattered over a large pair would otherwise upload nearly the whole pair.  A run whose union window is more than three
  // times the windows of its tiles taken one by one (tiles far apart inside the run) goes through the single-tile entry.
  int t0 = 0;
  while (t0 < n_tiles) {
    const int t1 = equal_tiles_run(bw, bh, t0, n_tiles, VWGPU_MAX_GROUP);
    long long ux0 = LLONG_MAX, uy0 = LLONG_MAX, ux1 = LLONG_MIN, uy1 = LLONG_MIN;
    for (int t = t0; t < t1; ++t) {
      ux0 = std::min<long long>(ux0, bx[t]); uy0 = std::min<long long>(uy0, by[t]);
      ux1 = std::max<long long>(ux1, (long long)bx[t] + bw[t]); uy1 = std::max<long long>(uy1, (long long)by[t] + bh[t]);
    }
    const pyr_window W = pyramid_window(P, ux0, uy0, ux1, uy1, lw, lh, rw, rh);
    const double each = (double)(t1 - t0) * ((double)(bw[t0] + 2 * W.gx) * (double)(bh[t0] + 2 * W.gy));      // (the tiles of a run are equal in size)
    const double uni = (double)(ux1 - ux0 + 2 * W.gx) * (double)(uy1 - uy0 + 2 * W.gy);
    if (t1 - t0 > 1 && uni <= 3.0 * each) {
      int rc = pyramid_batch_host_run(ctx, W, left, ls, right, rs, lmask, lms, rmask, rms, P, t1 - t0, bx + t0, by + t0, bw + t0, bh + t0, outs + t0, os ? os + t0 : nullptr);
      if (rc) return rc;
    } else {
      for (int t = t0; t < t1; ++t) {
        int rc = vwgpu_pyramid_correlate(ctx, left, lw, lh, ls, right, rw, rh, rs, lmask, lms, rmask, rms, P, bx[t], by[t], bw[t], bh[t], outs[t], os ? os[t] : 0);
        if (rc) return rc;
      }
    }
    t0 = t1;
  }
  return VWGPU_OK;
}

int vwgpu_pyramid_correlate(vwgpu_ctx* ctx, const float* left, int lw, int lh, ptrdiff_t ls,
                            const float* right, int rw, int rh, ptrdiff_t rs,
                            const uint8_t* lmask, ptrdiff_t lms, const uint8_t* rmask, ptrdiff_t rms,
                            const vwgpu_pyramid_params* P, int bx, int by, int bw, int bh, float* out, ptrdiff_t os) {
  int rc = check_pyramid_args(ctx, left, lw, lh, right, rw, rh, P, bw, bh, out);
  if (rc) return rc;
  default_strides(lw, rw, &ls, &rs, &lms, &rms);
  if (os == 0) os = bw;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  const pyr_window W = pyramid_window(P, bx, by, (long long)bx + bw, (long long)by + bh, lw, lh, rw, rh);
  if (W.lww <= 0 || W.lwh <= 0 || W.rww <= 0 || W.rwh <= 0)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "pyramid_correlate: the tile lies outside the images");
  if (tile_outside_lr_diff(P, bx, by, bw, bh)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, kLrDiffDomain);
  // The discrepancy image is shared by the tile threads (each writes its own pixels, CorrelationView.cc:683-694): only the
  // tile's rectangle of it is staged, so that concurrent tiles never write back each other's stale pixels.
  const ptrdiff_t hdst = P->lr_disp_diff_stride ? P->lr_disp_diff_stride : P->lr_disp_diff_cols;
  float* h_diff = P->lr_disp_diff ? P->lr_disp_diff + ((ptrdiff_t)(by - P->region_ul_y) * hdst + (bx - P->region_ul_x)) * 2 : nullptr;
  vwgpu_stage st(ctx);
  stage_window(st, W, left, ls, right, rs, lmask, lms, rmask, rms);
  const int pd = st.add(h_diff, bw, bh, 8, hdst, VWGPU_STAGE_INOUT), po = st.add(out, bw, bh, 12, os, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  vwgpu_pyramid_params Pd = *P;                     // the device-side discrepancy image is the tile's rectangle, dense
  Pd.lr_disp_diff_cols = bw; Pd.lr_disp_diff_rows = bh; Pd.lr_disp_diff_stride = bw;
  Pd.region_ul_x = bx - W.ox;                       // everything below runs in window coordinates
  Pd.region_ul_y = by - W.oy;
  rc = vwgpu_pyramid_correlate_impl(ctx, st.dev<float>(0), W.lww, W.lwh, W.lww, st.dev<float>(1), W.rww, W.rwh, W.rww, lmask ? st.dev<uint8_t>(2) : nullptr, W.lww,
                                    rmask ? st.dev<uint8_t>(3) : nullptr, W.rww, &Pd, bx - W.ox, by - W.oy, bw, bh, st.dev<float>(po), bw, st.dev<float>(pd));
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
