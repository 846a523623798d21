// packed_tile.h — what the packed-integer matchers share besides the u8 staging of u8_tile.h: the three-operand VALU wrappers, the
// staging of float image rows as u16 pixel pairs (bm_sad_u16.hip, bm_corr_u16.hip) and the lookup in a table of instantiated kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace vwgpu_packed {

__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) { uint32_t r; asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ uint32_t umax3(uint32_t a, uint32_t b, uint32_t c) { uint32_t r; asm("v_max3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float fmax3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
__device__ __forceinline__ float fmin3(float a, float b, float c) { float r; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }

// float -> unsigned integer with the exactness test of a packed path: integer-valued and inside [0, MAXV]
template <uint32_t MAXV>
__device__ __forceinline__ uint32_t to_uint(float v, bool& bad) {
  const float r = rintf(v);
  bad |= !(r == v && v >= 0.0f && v <= (float)MAXV);
  return (uint32_t)(int)fminf(fmaxf(r, 0.0f), (float)MAXV);
}

// dst[r][g] = pixels (x0 + 2g, x0 + 2g + 1) of row y0 + r as a u16 pair, zero outside the image
template <int NROWS, uint32_t MAXV, int NTHREADS>
__device__ __forceinline__ void stage_pair_rows(const float* __restrict__ img, ptrdiff_t stride, int w, int h, int x0, int y0,
                                                int npairs, uint32_t* __restrict__ dst, int tid, bool& bad) {
  for (int i = tid; i < NROWS * npairs; i += NTHREADS) {
    const int r = i / npairs, gq = i - r * npairs;
    const int x = x0 + 2 * gq, y = y0 + r;
    uint32_t p = 0;
    if (y < h) {
      const float* row = img + (ptrdiff_t)y * stride;
      if (x < w) p = to_uint<MAXV>(row[x], bad);
      if (x + 1 < w) p |= to_uint<MAXV>(row[x + 1], bad) << 16;
    }
    dst[i] = p;
  }
}

// One instantiated kernel of a matcher: the cost and window it serves, the rows of its tile and the kernel.
template <class Fn>
struct Launch { int cost, kx, ky, ty; Fn fn; };
template <class Fn, size_t N>
const Launch<Fn>* find_launch(const Launch<Fn> (&table)[N], int cost, int kx, int ky) {
  for (const Launch<Fn>& l : table)
    if (l.cost == cost && l.kx == kx && l.ky == ky) return &l;
  return nullptr;
}

}  // namespace vwgpu_packed
