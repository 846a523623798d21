// u8_tile.h — staging of float image tiles as packed u8 dwords in LDS, shared by the packed-u8 matchers
// (bm_sad_u8.hip, bm_corr_u8.hip).  Every pixel is checked on the way: the packed kernels are exact only for
// integer-valued pixels in [0,255]; anything else ORs a non-zero value into `acc`.
//
// The loads: every group of four pixels is ONE 16-byte load (global_load_dwordx4) — one per row and lane in the main part of a tile, four
// in flight per lane in the remainder columns — through a packed, 4-byte aligned struct (load_f4), for aligned images and for views cut
// at any column or with any row stride alike.  Only the group that straddles the right edge of the image is read pixel by pixel
// (patch_right_edge).  An earlier form chose per row between a float4 load and four scalar loads on a run-time alignment flag; the
// compiler merged the arms into four single-dword loads with selected addresses in every row but the last, so each lane fetched its 16
// bytes as four requests at a 16-byte lane stride.  tests/test_u8_tile_isa_cpu.py reads the instruction counts off the assembly.
// What staging costs with them (profiles/u8_staging_loads.md): a 7x7 tile pair of 1024 x 16 pixels at 129 disparities (22 input rows,
// 194 KB) takes 8.1-8.7 us when every CU stages one pair at the same moment and 15.4-15.6 us when it stages two — 10-11 bytes per clock
// and CU either way, the rate of an all-CU burst of wide loads: the phase is bound by the bytes it moves (13.5 and 20.4 us with the
// four-dword form, which was bound by its requests).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace vwgpu_u8 {

typedef uint32_t u32;

// float4 -> 4 packed u8 (v_cvt_pk_u8_f32 saturates) and the exactness test of the fast path: a pixel is
// representable iff converting the byte back gives the same float; the differences are OR-ed into `acc`
// (non-zero bits => some pixel was not an integer in [0,255]; NaN/Inf/-0.0 also land there).
__device__ __forceinline__ u32 pack4_check(float4 v, u32& acc) {
  u32 p = 0;
  p = __builtin_amdgcn_cvt_pk_u8_f32(v.x, 0, p);
  p = __builtin_amdgcn_cvt_pk_u8_f32(v.y, 1, p);
  p = __builtin_amdgcn_cvt_pk_u8_f32(v.z, 2, p);
  p = __builtin_amdgcn_cvt_pk_u8_f32(v.w, 3, p);
  acc |= __builtin_bit_cast(u32, v.x - (float)(p & 0xffu));
  acc |= __builtin_bit_cast(u32, v.y - (float)((p >> 8) & 0xffu));
  acc |= __builtin_bit_cast(u32, v.z - (float)((p >> 16) & 0xffu));
  acc |= __builtin_bit_cast(u32, v.w - (float)(p >> 24));
  return p;
}

// Groups straddling the right image edge (x < w <= x+3, at most one per row): the vector paths left them out.
template <int NROWS>
__device__ __forceinline__ void patch_right_edge(const float* __restrict__ img, ptrdiff_t stride, int w, int h,
                                                 int x0, int y0, int ndw, int dst_pitch_dw,
                                                 u32* __restrict__ dst, int tid, int nthreads, u32& acc) {
  const int ge = (w - x0) >> 2;
  if (ge >= 0 && ge < ndw && ((w - x0) & 3) != 0) {
    for (int r = tid; r < NROWS; r += nthreads) {
      const int y = y0 + r;
      u32 p = 0;
      if (y < h) {
        const float* row = img + (ptrdiff_t)y * stride;
        const int x = x0 + 4 * ge;
        // pixels behind the edge count as 0; the same conversion and exactness test as everywhere else
        const float4 v = make_float4(row[x], x + 1 < w ? row[x + 1] : 0.0f, x + 2 < w ? row[x + 2] : 0.0f, 0.0f);
        p = pack4_check(v, acc);
      }
      dst[r * dst_pitch_dw + ge] = p;
    }
  }
}

// Loads NROWS rows of a float image as packed u8 dwords into LDS: dst[r][g] = bytes (x0+4g .. x0+4g+3), zero
// outside [0,w) x [0,h).  Row base pointers are workgroup-uniform (scalar), the per-lane part of the address is one
// offset shared by all rows, and all NROWS loads of a thread are unconditional (out-of-range groups read offset 0 of
// a valid row and are zeroed afterwards), so they are in flight together, one 16-byte request each.
// Columns beyond the first `nthreads` groups (the search margin) are spread evenly over the workgroup.
// Groups straddling the right image edge (at most one per row) are patched by a scalar tail loop.
// (The dummy load reads four floats from the start of a row: inside the image for w >= 4, and from row 0 — whose successor exists, the
// matchers' windows have three rows or more — for narrower images.)
template <int NROWS>
struct U8MainLoads { float4 v[NROWS]; };

// Four consecutive floats of a row whose base is only known to be 4-byte aligned (an image view cut at any column, any row stride): the
// packed, 4-byte aligned struct makes the access one global_load_dwordx4 for every image, so there is no second, scalar form of the loads
// (the idiom of the SAD epilogue's stores, whose rows are 4-byte aligned as well).
struct __attribute__((packed, aligned(4))) F4U { float x, y, z, w; };
__device__ __forceinline__ float4 load_f4(const float* p) {
  const F4U u = *reinterpret_cast<const F4U*>(p);
  return make_float4(u.x, u.y, u.z, u.w);
}

// main part of a tile: group g = tid of every row.  `issue` requests the NROWS loads, `finish` converts and stores them.
template <int NROWS>
__device__ __forceinline__ void stage_u8_main_issue(const float* __restrict__ img, ptrdiff_t stride, int w, int h, int x0, int y0, int ndw,
                                                    int tid, U8MainLoads<NROWS>& ld) {
  if (tid < ndw) {
    const int x = x0 + 4 * tid;
    const int off = (x + 3 < w) ? x : 0;
    const int hv = w >= 4 ? h : 0;             // (an image narrower than a group has no full group: every load is the dummy one of row 0)
#pragma unroll
    for (int r = 0; r < NROWS; ++r) {
      const float* rowp = (y0 + r < hv) ? img + (ptrdiff_t)(y0 + r) * stride : img;   // uniform
      ld.v[r] = load_f4(rowp + off);
    }
  }
}
template <int NROWS>
__device__ __forceinline__ void stage_u8_main_finish(int w, int h, int x0, int y0, int ndw, int dst_pitch_dw, u32* __restrict__ dst, int tid,
                                                     const U8MainLoads<NROWS>& ld, u32& acc) {
  if (tid < ndw) {
    const int g = tid, x = x0 + 4 * g;
    const bool colin = x + 3 < w;
#pragma unroll
    for (int r = 0; r < NROWS; ++r) {
      u32 a = 0;
      const u32 p = pack4_check(ld.v[r], a);
      const bool inb = colin && (y0 + r < h);
      if (inb) acc |= a;
      if (colin || x >= w) dst[r * dst_pitch_dw + g] = inb ? p : 0u;   // a straddling group belongs to patch_right_edge
    }
  }
}

// remainder columns [nthreads, ndw): NROWS * rem items spread over all threads, 4 in flight per thread; then the straddling groups
template <int NROWS>
__device__ __forceinline__ void stage_u8_rest(const float* __restrict__ img, ptrdiff_t stride, int w, int h,
                                              int x0, int y0, int ndw, int dst_pitch_dw,
                                              u32* __restrict__ dst, int tid, int nthreads, u32& acc) {
  const int rem = ndw - nthreads;
  if (rem > 0) {
    const int total = NROWS * rem;
    const float inv = 1.0f / (float)rem;
    for (int i0 = 0; i0 < total; i0 += 4 * nthreads) {
      float4 v[4]; int di[4]; bool inb[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int idx = i0 + k * nthreads + tid;
        int r = (int)(((float)(idx < total ? idx : 0) + 0.5f) * inv);
        int c = (idx < total ? idx : 0) - r * rem;
        if (c < 0) { --r; c += rem; }
        if (c >= rem) { ++r; c -= rem; }
        const int g = nthreads + c, x = x0 + 4 * g;
        inb[k] = (idx < total) && (x + 3 < w) && (y0 + r < h);
        di[k] = (idx < total && (x + 3 < w || x >= w)) ? r * dst_pitch_dw + g : -1;   // not the straddling group
        const float* src = inb[k] ? img + (ptrdiff_t)(y0 + r) * stride + x : img;
        v[k] = load_f4(src);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        u32 a = 0;
        const u32 p = pack4_check(v[k], a);
        if (inb[k]) acc |= a;
        if (di[k] >= 0) dst[di[k]] = inb[k] ? p : 0u;
      }
    }
  }
  patch_right_edge<NROWS>(img, stride, w, h, x0, y0, ndw, dst_pitch_dw, dst, tid, nthreads, acc);
}

template <int NROWS>
__device__ __forceinline__ void stage_u8_rows(const float* __restrict__ img, ptrdiff_t stride, int w, int h,
                                              int x0, int y0, int ndw, int dst_pitch_dw,
                                              u32* __restrict__ dst, int tid, int nthreads, u32& acc) {
  U8MainLoads<NROWS> ld;
  stage_u8_main_issue<NROWS>(img, stride, w, h, x0, y0, ndw, tid, ld);
  stage_u8_main_finish<NROWS>(w, h, x0, y0, ndw, dst_pitch_dw, dst, tid, ld, acc);
  stage_u8_rest<NROWS>(img, stride, w, h, x0, y0, ndw, dst_pitch_dw, dst, tid, nthreads, acc);
}

}  // namespace vwgpu_u8
