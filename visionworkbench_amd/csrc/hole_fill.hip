// hole_fill.hip — filling the holes of a masked image: grassfire (src/vw/Image/Grassfire.h:79-228), the blob index over the
// whole image as one tile (Image/BlobIndex.h:113-306, :385-477), get_blob_sizes (:507-615), ErodeView (Image/ErodeView.h:199-221),
// InpaintView (Image/InpaintView.h:44-237), fill_holes_grass (:239-311) and fill_nodata_with_avg (:317-387).
// tests/refimpl/hole_fill_ref.cc restates them and DESIGN §4.23 describes the path.
//
// Pixel kinds (vwgpu_pixel_kind): a uint8 mask, PixelMask<float> as {value, valid}, PixelMask<Vector2i> / PixelMask<Vector2f> as
// {dx, dy, valid}; the validity word of a float kind is a float compared with 0.
//
// LABEL IMAGE.  The reference's blob_index() returns the PROVISIONAL labels of its raster pass: dst is never rewritten after the
// equivalences are consolidated (BlobIndex.h:267-304).  That is not reproduced: the label image here holds the consolidated 1-based
// number of the blob in the reference's blob order (the k-th blob is the one whose first pixel in raster order comes k-th), counted
// over the blobs that max_area and wipe_size keep, and 0 for every other pixel.
//
// Labelling: a lock-free union-find whose roots are the smallest pixel index of a component (as the blob filter of pyramid.hip), so the
// blob order is an exclusive prefix sum over "pixel i is a root"; sizes and bounding boxes by atomics on the blob's row, one per
// wavefront where a wavefront's run of a row lies in one blob; a second prefix sum over "blob is kept" numbers the table.
//
// Grassfire: the reference's two raster passes compute the L1 distance to the nearest zero (to the outside too, unless
// ignore_borders); the L1 distance separates: a scan along every row (nearest zero left and right), then a min-plus scan down and up
// every column.
//
// Inpaint: one workgroup of one wavefront per blob, the blob's box grown by one in LDS; see hf_inpaint_kernel.
#include <climits>
#include <cstring>

#include "vwgpu_internal.h"

namespace {

constexpr int HF_BX = 64, HF_BY = 4;
constexpr int HF_SCAN_THREADS = 256, HF_SCAN_ITEMS = 8, HF_SCAN_BLOCK = HF_SCAN_THREADS * HF_SCAN_ITEMS;

inline dim3 hf_grid(int w, int h) { return dim3((unsigned)((w + HF_BX - 1) / HF_BX), (unsigned)std::min((h + HF_BY - 1) / HF_BY, 65535)); }
const dim3 hf_block(HF_BX, HF_BY);
inline unsigned hf_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

inline int hf_kind_bytes(int kind) { return kind == VWGPU_PIXEL_MASK_U8 ? 1 : kind == VWGPU_PIXEL_MASKED_F32 ? 8 : 12; }

__device__ __forceinline__ bool hf_is_valid(int kind, const void* base, long long idx) {
  switch (kind) {
    case VWGPU_PIXEL_MASK_U8: return static_cast<const uint8_t*>(base)[idx] != 0;
    case VWGPU_PIXEL_MASKED_F32: return static_cast<const float*>(base)[2 * idx + 1] != 0.0f;
    case VWGPU_PIXEL_DISPARITY_I32: return static_cast<const int32_t*>(base)[3 * idx + 2] != 0;
    default: return static_cast<const float*>(base)[3 * idx + 2] != 0.0f;
  }
}

// ---- union-find (the four helpers of the blob filter, pyramid.hip) ---------------------------------------------------------------
__device__ __forceinline__ int hf_find(int* L, int x) {
  int p = L[x];
  while (p != x) { const int g = L[p]; L[x] = g; x = p; p = g; }     // path halving; racy writes only ever shorten paths
  return x;
}
__device__ __forceinline__ void hf_unite(int* L, int a, int b) {
  while (true) {
    a = hf_find(L, a); b = hf_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }                     // hang the larger root under the smaller one
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;
  }
}
// the forest is final after the union kernel: read-only root walks
__device__ __forceinline__ int hf_root(const int* L, int x) {
  int p = L[x];
  while (p != x) { x = p; p = L[x]; }
  return x;
}

__global__ void hf_init_kernel(int kind, const void* img, long long stride, int w, int h, int invert, int* __restrict__ L) {
  const int x = blockIdx.x * HF_BX + threadIdx.x;
  if (x >= w) return;
  for (int y = blockIdx.y * HF_BY + threadIdx.y; y < h; y += gridDim.y * HF_BY)
    L[y * w + x] = hf_is_valid(kind, img, (long long)y * stride + x) != (invert != 0) ? y * w + x : -1;
}
__global__ void hf_union_kernel(int* L, int w, int h) {
  const int x = blockIdx.x * HF_BX + threadIdx.x;
  if (x >= w) return;
  for (int y = blockIdx.y * HF_BY + threadIdx.y; y < h; y += gridDim.y * HF_BY) {
    const int i = y * w + x;
    if (L[i] < 0) continue;
    if (x > 0 && L[i - 1] >= 0) hf_unite(L, i, i - 1);
    if (y > 0) {
      if (L[i - w] >= 0) hf_unite(L, i, i - w);
      if (x > 0 && L[i - w - 1] >= 0) hf_unite(L, i, i - w - 1);
      if (x + 1 < w && L[i - w + 1] >= 0) hf_unite(L, i, i - w + 1);
    }
  }
}
__global__ void hf_roots_kernel(const int* __restrict__ L, int n, int* __restrict__ R) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  R[i] = L[i] < 0 ? -1 : hf_root(L, i);
}

// ---- exclusive prefix sums over a 0 / 1 flag: block counts, one workgroup over the counts, the ranks -------------------------------
// inclusive scan over the 256 threads of a workgroup; lds: 4 ints; *total = the workgroup's sum
__device__ __forceinline__ int hf_block_scan(int v, int* lds, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < HF_SCAN_THREADS / 64; ++k) {
    const int s = lds[k];
    if (k < wave) before += s;
    all += s;
  }
  __syncthreads();
  *total = all;
  return v + before;
}
template <class F>
__global__ __launch_bounds__(HF_SCAN_THREADS) void hf_scan_count_kernel(F f, int n, int* __restrict__ partial) {
  __shared__ int lds[4];
  const long long base = (long long)blockIdx.x * HF_SCAN_BLOCK + threadIdx.x * HF_SCAN_ITEMS;
  int c = 0;
  for (int k = 0; k < HF_SCAN_ITEMS; ++k)
    if (base + k < n) c += f((int)(base + k));
  int total;
  hf_block_scan(c, lds, &total);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}
__global__ __launch_bounds__(HF_SCAN_THREADS) void hf_scan_partials_kernel(int* partial, int nb, int* total) {
  __shared__ int lds[4];
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += HF_SCAN_THREADS) {
    const int i = b0 + threadIdx.x, v = i < nb ? partial[i] : 0;
    int all;
    const int inc = hf_block_scan(v, lds, &all);
    if (i < nb) partial[i] = carry + inc - v;
    carry += all;
  }
  if (threadIdx.x == 0) *total = carry;
}
template <class F, class O>
__global__ __launch_bounds__(HF_SCAN_THREADS) void hf_scan_apply_kernel(F f, O o, int n, const int* __restrict__ partial) {
  __shared__ int lds[4];
  const long long base = (long long)blockIdx.x * HF_SCAN_BLOCK + threadIdx.x * HF_SCAN_ITEMS;
  int c = 0;
  for (int k = 0; k < HF_SCAN_ITEMS; ++k)
    if (base + k < n) c += f((int)(base + k));
  int total;
  int run = partial[blockIdx.x] + hf_block_scan(c, lds, &total) - c;
  for (int k = 0; k < HF_SCAN_ITEMS; ++k)
    if (base + k < n && f((int)(base + k))) o((int)(base + k), run++);
}

struct hf_root_flag {
  const int* R;
  __device__ int operator()(int i) const { return R[i] == i; }
};
struct hf_rank_out {
  int* rank;
  __device__ void operator()(int i, int r) const { rank[i] = r; }
};
// per-blob statistics: five rows of nb ints {size, min x, min y, max x, max y} (max inclusive)
struct hf_keep_flag {
  const int* st;
  int nb, max_area, wipe;
  __device__ int operator()(int b) const {
    if (max_area > 0 && st[b] > max_area) return 0;
    if (wipe > 0 && (st[3 * nb + b] - st[nb + b] + 1 > wipe || st[4 * nb + b] - st[2 * nb + b] + 1 > wipe)) return 0;
    return 1;
  }
};
struct hf_newid_out {
  int* newid;
  __device__ void operator()(int b, int r) const { newid[b] = r + 1; }
};

__global__ void hf_stats_init_kernel(int* __restrict__ st, int nb) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  st[b] = 0; st[nb + b] = INT_MAX; st[2 * nb + b] = INT_MAX; st[3 * nb + b] = -1; st[4 * nb + b] = -1;
}
// A wavefront covers 64 consecutive pixels of one row; where they all lie in one blob (the inside of any large blob) one lane
// carries the run's count and extent, so a blob of millions of pixels does not serialise millions of atomics on five words.
__global__ void hf_stats_kernel(const int* __restrict__ R, const int* __restrict__ rank, int w, int h, int* __restrict__ st, int nb) {
  const int x = blockIdx.x * HF_BX + threadIdx.x;
  for (int y = blockIdx.y * HF_BY + threadIdx.y; y < h; y += gridDim.y * HF_BY) {
    int b = -1;
    if (x < w) {
      const int r = R[y * w + x];
      if (r >= 0) b = rank[r];
    }
    const unsigned long long act = __ballot(b >= 0);
    if (!act) continue;
    const int first = __ffsll((long long)act) - 1, last = 63 - __clzll((long long)act);
    const int b0 = __shfl(b, first);
    if (__all(b < 0 || b == b0)) {
      if ((int)threadIdx.x == first) {
        const int xa = blockIdx.x * HF_BX + first, xb = blockIdx.x * HF_BX + last;
        atomicAdd(&st[b0], __popcll(act));
        atomicMin(&st[nb + b0], xa); atomicMin(&st[2 * nb + b0], y);
        atomicMax(&st[3 * nb + b0], xb); atomicMax(&st[4 * nb + b0], y);
      }
    } else if (b >= 0) {
      atomicAdd(&st[b], 1);
      atomicMin(&st[nb + b], x); atomicMin(&st[2 * nb + b], y);
      atomicMax(&st[3 * nb + b], x); atomicMax(&st[4 * nb + b], y);
    }
  }
}
__global__ void hf_labels_kernel(const int* __restrict__ R, const int* __restrict__ rank, const int* __restrict__ newid, int w, int h,
                                 int32_t* __restrict__ labels, long long lstride) {
  const int x = blockIdx.x * HF_BX + threadIdx.x;
  if (x >= w) return;
  for (int y = blockIdx.y * HF_BY + threadIdx.y; y < h; y += gridDim.y * HF_BY) {
    const int r = R[y * w + x];
    labels[(long long)y * lstride + x] = r < 0 ? 0 : newid[rank[r]];
  }
}
__global__ void hf_table_kernel(const int* __restrict__ st, const int* __restrict__ newid, int nb, int32_t* __restrict__ table) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nb || newid[b] == 0) return;
  int32_t* row = table + 5 * (long long)(newid[b] - 1);
  row[0] = st[nb + b]; row[1] = st[2 * nb + b]; row[2] = st[3 * nb + b] + 1; row[3] = st[4 * nb + b] + 1; row[4] = st[b];
}
__global__ void hf_sizes_kernel(const int* __restrict__ R, const int* __restrict__ rank, const int* __restrict__ st, int w, int h,
                                uint32_t limit, uint32_t* __restrict__ out, long long ostride) {
  const int x = blockIdx.x * HF_BX + threadIdx.x;
  if (x >= w) return;
  for (int y = blockIdx.y * HF_BY + threadIdx.y; y < h; y += gridDim.y * HF_BY) {
    const int r = R[y * w + x];
    const uint32_t s = r < 0 ? 0u : (uint32_t)st[rank[r]];
    out[(long long)y * ostride + x] = s < limit ? s : limit;
  }
}
// ErodeView: a pixel of a blob of at most max_area pixels becomes the default pixel (every word 0)
__global__ void hf_erase_kernel(const int* __restrict__ R, const int* __restrict__ rank, const int* __restrict__ st, int w, int h,
                                int max_area, int kind, void* out, long long ostride) {
  const int x = blockIdx.x * HF_BX + threadIdx.x;
  if (x >= w) return;
  for (int y = blockIdx.y * HF_BY + threadIdx.y; y < h; y += gridDim.y * HF_BY) {
    const int r = R[y * w + x];
    if (r < 0 || st[rank[r]] > max_area) continue;
    const long long o = (long long)y * ostride + x;
    if (kind == VWGPU_PIXEL_MASK_U8) static_cast<uint8_t*>(out)[o] = 0;
    else {
      const int words = kind == VWGPU_PIXEL_MASKED_F32 ? 2 : 3;
      for (int c = 0; c < words; ++c) static_cast<uint32_t*>(out)[o * words + c] = 0u;
    }
  }
}

// ---- grassfire ------------------------------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ bool hf_zero(T v) { return v == T(); }   // a NaN is not zero, -0.0f is

__global__ void hf_zero_kernel(int32_t* __restrict__ out, long long ostride, int w, int h) {
  const int x = blockIdx.x * HF_BX + threadIdx.x;
  if (x >= w) return;
  for (int y = blockIdx.y * HF_BY + threadIdx.y; y < h; y += gridDim.y * HF_BY) out[(long long)y * ostride + x] = 0;
}
// One wavefront per row: out(x) = min(x - the nearest zero at or left of x, the nearest zero at or right of x - x, cap), the outside
// counting as zero unless ignore_borders.  The nearest zero is a max- / min-scan of "x where the pixel is zero" over the 64 lanes,
// carried from chunk to chunk.
template <class T>
__global__ __launch_bounds__(256) void hf_grass_rows_kernel(const T* __restrict__ src, long long sstride, int w, int h, int ignore_borders,
                                                            int cap, int32_t* __restrict__ out, long long ostride) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (y >= h) return;                                   // a whole wavefront leaves
  const T* s = src + (long long)y * sstride;
  int32_t* o = out + (long long)y * ostride;
  const long long far = (long long)cap + w + 2;
  long long carry = ignore_borders ? -far : -1;
  for (int x0 = 0; x0 < w; x0 += 64) {
    const int x = x0 + lane;
    long long lz = (x < w && hf_zero(s[x])) ? x : -far;
    for (int d = 1; d < 64; d <<= 1) {
      const long long t = __shfl_up(lz, d);
      if (lane >= d) lz = t > lz ? t : lz;
    }
    lz = lz > carry ? lz : carry;
    carry = __shfl(lz, 63);
    if (x < w) { const long long g = x - lz; o[x] = (int32_t)(g < cap ? g : cap); }
  }
  carry = ignore_borders ? far + w : w;
  for (int x0 = ((w - 1) / 64) * 64; x0 >= 0; x0 -= 64) {
    const int x = x0 + lane;
    long long rz = (x < w && hf_zero(s[x])) ? x : far + w;
    for (int d = 1; d < 64; d <<= 1) {
      const long long t = __shfl_down(rz, d);
      if (lane + d < 64) rz = t < rz ? t : rz;
    }
    rz = rz < carry ? rz : carry;
    carry = __shfl(rz, 0);
    if (x < w) { const long long g = rz - x; if (g < o[x]) o[x] = (int32_t)g; }
  }
}
// One lane per column: d(y) = min over y' of (row distance at y' + |y - y'|), the outside rows counting as zero unless
// ignore_borders: t = min(g, t + 1) down, then up.  The loads of a group of rows do not depend on the chain and go out together.
__global__ __launch_bounds__(64) void hf_grass_cols_kernel(int32_t* __restrict__ out, long long ostride, int w, int h, int ignore_borders, int cap) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= w) return;
  constexpr int G = 8;
  int t = ignore_borders ? cap : 0;
  for (int y0 = 0; y0 < h; y0 += G) {
    int g[G];
#pragma unroll
    for (int k = 0; k < G; ++k) g[k] = y0 + k < h ? out[(long long)(y0 + k) * ostride + x] : 0;
#pragma unroll
    for (int k = 0; k < G; ++k)
      if (y0 + k < h) {
        t = t < cap ? t + 1 : cap;
        t = g[k] < t ? g[k] : t;
        out[(long long)(y0 + k) * ostride + x] = t;
      }
  }
  t = ignore_borders ? cap : 0;
  for (int y1 = h - 1; y1 >= 0; y1 -= G) {
    int g[G];
#pragma unroll
    for (int k = 0; k < G; ++k) g[k] = y1 - k >= 0 ? out[(long long)(y1 - k) * ostride + x] : 0;
#pragma unroll
    for (int k = 0; k < G; ++k)
      if (y1 - k >= 0) {
        t = t < cap ? t + 1 : cap;
        t = g[k] < t ? g[k] : t;
        out[(long long)(y1 - k) * ostride + x] = t;
      }
  }
}

// ---- inpaint --------------------------------------------------------------------------------------------------------------------
struct hf_inpaint_args {
  const float* in; long long istride;
  float* out; long long ostride;
  const int32_t* labels; long long lstride;
  const int32_t* table;
  int w, h, semantics, max_len, overlap;
};

// The blobs InpaintTask leaves alone (InpaintView.h:76-80): the box grown by one, half-open [x0, x1) x [y0, y1)
__device__ __forceinline__ bool hf_blob_skipped(int x0, int y0, int x1, int y1, int w, int h, int semantics) {
  if (x0 < 0 || y0 < 0) return true;
  return semantics == VWGPU_HOLE_EDGE_REFERENCE ? (x1 >= w || y1 >= h) : (x1 > w || y1 > h);
}

__device__ __forceinline__ int hf_wave_max(int v) {
  for (int d = 32; d > 0; d >>= 1) { const int t = __shfl_xor(v, d); v = t > v ? t : v; }
  return v;
}

// One workgroup of one wavefront per blob (blockIdx.x = its row of the table).  LDS, sized by max_len (P = (max_len + 2)^2,
// N = max_len^2 words): C float planes of the patch (the blob's box grown by one), one word of {distance, level} per patch pixel, the
// list of the blob's pixels sorted by bucket, the bucket ends.
//
// The reference updates the blob's pixels one at a time, sweep after sweep, in the order (distance, column, row), in place.  Update k of
// pixel p reads update k of the neighbours that come earlier and update k - 1 of those that come later, so the serial order is only a
// partial order: with level(p) = 1 + max level(q) over the blob pixels q among p's 8 neighbours that come earlier, the pixels of one
// level are mutually non-adjacent and may be updated together.  Update k of p is run at step k * T + level(p) with
// T = 1 + max(level(q) - level(p)) over adjacent pairs with q later than p: then q's update k - 1 (step (k - 1) T + level(q)) comes
// before p's update k and p's update k before q's update k (read after write), and p's update k + 1 comes after q's update k has read p
// (write after read); two pixels updated in one step differ in level by a multiple of T and so are not adjacent.  T = the largest level
// (overlap == 0) is the schedule without overlap between sweeps.  Every word equals the serial Gauss-Seidel: each update reads exactly
// the values the serial order would and sums them in the reference's order.  The step count is known before the loop; nothing waits.
template <int C>
__global__ __launch_bounds__(64) void hf_inpaint_kernel(hf_inpaint_args a) {
  extern __shared__ unsigned hf_lds[];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int32_t* row = a.table + 5 * (long long)k;
  const int bw = row[2] - row[0], bh = row[3] - row[1];
  const int x0 = row[0] - 1, y0 = row[1] - 1, x1 = row[2] + 1, y1 = row[3] + 1;
  if (bw <= 0 || bh <= 0 || bw > a.max_len || bh > a.max_len) return;       // uniform: the whole workgroup leaves
  if (hf_blob_skipped(x0, y0, x1, y1, a.w, a.h, a.semantics)) return;
  const int pw = bw + 2, ph = bh + 2, P = pw * ph;
  const int Pmax = (a.max_len + 2) * (a.max_len + 2), Nmax = a.max_len * a.max_len;
  float* val = reinterpret_cast<float*>(hf_lds);
  unsigned* meta = hf_lds + C * Pmax;      // distance in bits 0-7, level above
  unsigned* list = meta + Pmax;            // patch index | (level / T) << 16, sorted by level % T
  unsigned* ends = list + Nmax;            // T words: where bucket r ends

  for (int idx = tid; idx < P; idx += 64) {
    const int i = idx % pw, j = idx / pw;
    const long long g = (long long)(y0 + j) * a.istride + (x0 + i);
    for (int c = 0; c < C; ++c) val[c * Pmax + idx] = a.in[g * (C + 1) + c];
    const bool inside = i > 0 && j > 0 && i < pw - 1 && j < ph - 1;
    meta[idx] = (inside && a.labels[(long long)(y0 + j) * a.lstride + (x0 + i)] == k + 1) ? 255u : 0u;
  }
  __syncthreads();
  // grassfire of the mask: rows, then columns; the ring is zero, so every chain starts from 0
  for (int j = tid; j < ph; j += 64) {
    unsigned d = 0;
    for (int i = 0; i < pw; ++i) { d = meta[j * pw + i] ? d + 1 : 0; meta[j * pw + i] = d; }
    d = 0;
    for (int i = pw - 1; i >= 0; --i) { const unsigned v = meta[j * pw + i]; d = v < d + 1 ? v : d + 1; meta[j * pw + i] = d; }
  }
  __syncthreads();
  int maxd = 0;
  for (int i = tid; i < pw; i += 64) {
    unsigned d = 0;
    for (int j = 0; j < ph; ++j) { const unsigned v = meta[j * pw + i]; d = v < d + 1 ? v : d + 1; meta[j * pw + i] = d; }
    d = 0;
    for (int j = ph - 1; j >= 0; --j) {
      const unsigned v = meta[j * pw + i];
      d = v < d + 1 ? v : d + 1;
      meta[j * pw + i] = d ? (d | 256u) : 0u;        // level 1
      maxd = (int)d > maxd ? (int)d : maxd;
    }
  }
  maxd = hf_wave_max(maxd);
  __syncthreads();
  const int off8[8] = {-pw - 1, -pw, -pw + 1, -1, 1, pw - 1, pw, pw + 1};
  const int di8[8] = {-1, 0, 1, -1, 1, -1, 0, 1}, dj8[8] = {-1, -1, -1, 0, 0, 1, 1, 1};
  // levels: a fixed point from below; at most one pass per level, and never more passes than the patch has pixels
  for (int pass = 0; pass <= P; ++pass) {
    int changed = 0;
    for (int idx = tid; idx < P; idx += 64) {
      const unsigned me = meta[idx];
      const int dp = me & 255u;
      if (!dp) continue;
      const int i = idx % pw, j = idx / pw;
      int best = 0;
#pragma unroll
      for (int n = 0; n < 8; ++n) {
        const unsigned mq = meta[idx + off8[n]];
        const int dq = mq & 255u, iq = i + di8[n], jq = j + dj8[n];
        const bool earlier = dq && (dq < dp || (dq == dp && (iq < i || (iq == i && jq < j))));
        if (earlier && (int)(mq >> 8) > best) best = (int)(mq >> 8);
      }
      if (best + 1 > (int)(me >> 8)) { meta[idx] = (unsigned)dp | ((unsigned)(best + 1) << 8); changed = 1; }
    }
    if (!__syncthreads_or(changed)) break;
  }
  int maxlevel = 0, maxdiff = 0;
  for (int idx = tid; idx < P; idx += 64) {
    const unsigned me = meta[idx];
    const int dp = me & 255u, lp = (int)(me >> 8);
    if (!dp) continue;
    maxlevel = lp > maxlevel ? lp : maxlevel;
    const int i = idx % pw, j = idx / pw;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const unsigned mq = meta[idx + off8[n]];
      const int dq = mq & 255u, iq = i + di8[n], jq = j + dj8[n];
      const bool later = dq && (dq > dp || (dq == dp && (iq > i || (iq == i && jq > j))));
      if (later && (int)(mq >> 8) - lp > maxdiff) maxdiff = (int)(mq >> 8) - lp;
    }
  }
  maxlevel = hf_wave_max(maxlevel);
  maxdiff = hf_wave_max(maxdiff);
  if (maxlevel == 0) return;                                 // no pixel of the patch carries the blob's label (uniform)
  const int T = a.overlap ? 1 + maxdiff : maxlevel;          // 1 <= T <= maxlevel <= the blob's pixels <= Nmax
  const int qmax = maxlevel / T;
  const int sweeps = 10 * maxd * maxd;
  // counting sort of the blob's pixels by level % T
  for (int r = tid; r < T; r += 64) ends[r] = 0;
  __syncthreads();
  for (int idx = tid; idx < P; idx += 64) {
    const unsigned me = meta[idx];
    if (me & 255u) atomicAdd(&ends[(me >> 8) % T], 1u);
  }
  __syncthreads();
  {
    unsigned carry = 0;                                     // exclusive scan: ends[r] = where bucket r begins
    for (int r0 = 0; r0 < T; r0 += 64) {
      const int r = r0 + tid;
      const unsigned c = r < T ? ends[r] : 0u;
      unsigned v = c;
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(v, d);
        if (tid >= d) v += t;
      }
      if (r < T) ends[r] = carry + v - c;
      carry += __shfl(v, 63);
    }
  }
  __syncthreads();
  for (int idx = tid; idx < P; idx += 64) {
    const unsigned me = meta[idx];
    if (!(me & 255u)) continue;
    const unsigned lv = me >> 8;
    const unsigned pos = atomicAdd(&ends[lv % T], 1u);      // the cursor of a bucket ends where the next one begins
    list[pos] = (unsigned)idx | ((lv / T) << 16);
  }
  __syncthreads();

  const double w_diag = .176765, w_side = .073235;
  const int rounds = sweeps > 0 ? sweeps + qmax : 0;
  for (int round = 0; round < rounds; ++round) {
    unsigned begin = 0;
    for (int r = 0; r < T; ++r) {
      const unsigned end = ends[r];
      for (unsigned e = begin + tid; e < end; e += 64) {
        const unsigned entry = list[e];
        const int sweep = round - (int)(entry >> 16);
        if (sweep < 0 || sweep >= sweeps) continue;
        const int p = entry & 0xffffu;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          float* v = val + c * Pmax + p;
          float sum = 0.0f;
          sum = (float)((double)sum + w_diag * (double)v[-pw - 1]);
          sum = (float)((double)sum + w_side * (double)v[-pw]);
          sum = (float)((double)sum + w_diag * (double)v[-pw + 1]);
          sum = (float)((double)sum + w_side * (double)v[-1]);
          sum = (float)((double)sum + w_side * (double)v[1]);
          sum = (float)((double)sum + w_diag * (double)v[pw - 1]);
          sum = (float)((double)sum + w_side * (double)v[pw]);
          sum = (float)((double)sum + w_diag * (double)v[pw + 1]);
          v[0] = sum;
        }
      }
      begin = end;
      __syncthreads();
    }
  }
  for (int idx = tid; idx < P; idx += 64) {
    if (!(meta[idx] & 255u)) continue;
    const int i = idx % pw, j = idx / pw;
    float* o = a.out + ((long long)(y0 + j) * a.ostride + (x0 + i)) * (C + 1);
    for (int c = 0; c < C; ++c) o[c] = val[c * Pmax + idx];
    o[C] = 1.0f;                                            // validate(): ChannelRange<float>::max()
  }
}

// use_grassfire == false: the pixels of every blob that is not skipped become the default pixel as given
template <int C>
__global__ void hf_inpaint_default_kernel(hf_inpaint_args a, int count, float d0, float d1, float d2) {
  const int x = blockIdx.x * HF_BX + threadIdx.x;
  if (x >= a.w) return;
  for (int y = blockIdx.y * HF_BY + threadIdx.y; y < a.h; y += gridDim.y * HF_BY) {
    const int lab = a.labels[(long long)y * a.lstride + x];
    if (lab <= 0 || lab > count) continue;
    const int32_t* row = a.table + 5 * (long long)(lab - 1);
    if (row[2] - row[0] > a.max_len || row[3] - row[1] > a.max_len) continue;
    if (hf_blob_skipped(row[0] - 1, row[1] - 1, row[2] + 1, row[3] + 1, a.w, a.h, a.semantics)) continue;
    float* o = a.out + ((long long)y * a.ostride + x) * (C + 1);
    o[0] = d0; o[1] = d1;
    if (C == 2) o[2] = d2;
  }
}

// FillNoDataWithAvg::operator(): one lane per pixel; the window's valid values summed in float, column outer, row inner
__global__ void hf_avg_kernel(const float* __restrict__ in, long long istride, int w, int h, int k2, float* __restrict__ out, long long ostride) {
  const int x = blockIdx.x * HF_BX + threadIdx.x;
  if (x >= w) return;
  for (int y = blockIdx.y * HF_BY + threadIdx.y; y < h; y += gridDim.y * HF_BY) {
    const float* p = in + ((long long)y * istride + x) * 2;
    float val = p[0], v = p[1];
    if (v == 0.0f) {
      float sum = 0.0f;
      int n = 0;
      const int c0 = x - k2 > 0 ? x - k2 : 0, c1 = x + k2 < w - 1 ? x + k2 : w - 1;
      const int r0 = y - k2 > 0 ? y - k2 : 0, r1 = y + k2 < h - 1 ? y + k2 : h - 1;
      for (int c = c0; c <= c1; ++c)
        for (int r = r0; r <= r1; ++r) {
          const float* q = in + ((long long)r * istride + c) * 2;
          if (q[1] == 0.0f) continue;
          sum += q[0];
          ++n;
        }
      if (n) { val = sum / (float)n; v = 1.0f; }
    }
    float* o = out + ((long long)y * ostride + x) * 2;
    o[0] = val; o[1] = v;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int hf_check_image(vwgpu_ctx* ctx, const char* name, int kind, const void* in, int w, int h, ptrdiff_t& istride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (kind < VWGPU_PIXEL_MASK_U8 || kind > VWGPU_PIXEL_DISPARITY_F32) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: unknown pixel kind %d", name, kind);
  if (!in || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: empty image or null pointer", name);
  if ((long long)w * h > INT_MAX) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: more than 2^31 - 1 pixels", name);
  if (istride == 0) istride = w;
  if (istride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
  return VWGPU_OK;
}
int hf_check_out(vwgpu_ctx* ctx, const char* name, const void* out, int w, ptrdiff_t& ostride, bool optional = false) {
  if (!out && !optional) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: empty image or null pointer", name);
  if (ostride == 0) ostride = w;
  if (ostride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
  return VWGPU_OK;
}

// One labelling: R[i] = the root (smallest pixel index) of pixel i's blob or -1, rank[root] = the blob's place in the reference's
// order, st = the statistics of the nb blobs.  Waits for the device once, for nb.
struct hf_labelling {
  int *R = nullptr, *rank = nullptr, *st = nullptr, *partial = nullptr, *total = nullptr;
  int nb = 0;
  int* extra = nullptr;       // `extra_ints` more ints of ctx->hole_tab for the caller
};
int hf_label(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t stride, int invert, size_t extra_ints, hf_labelling* lab) {
  const int n = w * h;
  const size_t nblk = hf_blocks(n, HF_SCAN_BLOCK);
  const size_t ints = vwgpu_align_up((size_t)n, 64) * 2 + vwgpu_align_up(nblk + 1, 64) + 64;
  int rc = vwgpu_arena_reserve(ctx, &ctx->hole, ints * sizeof(int));
  if (rc) return rc;
  int* L = static_cast<int*>(ctx->hole.base);
  lab->R = L + vwgpu_align_up((size_t)n, 64);
  lab->rank = L;
  lab->partial = lab->R + vwgpu_align_up((size_t)n, 64);
  lab->total = lab->partial + vwgpu_align_up(nblk + 1, 64);
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(hf_init_kernel, hf_grid(w, h), hf_block, 0, s, kind, img, (long long)stride, w, h, invert, L);
  hipLaunchKernelGGL(hf_union_kernel, hf_grid(w, h), hf_block, 0, s, L, w, h);
  hipLaunchKernelGGL(hf_roots_kernel, dim3(hf_blocks(n, 256)), dim3(256), 0, s, L, n, lab->R);
  const hf_root_flag flag{lab->R};
  hipLaunchKernelGGL(hf_scan_count_kernel<hf_root_flag>, dim3((unsigned)nblk), dim3(HF_SCAN_THREADS), 0, s, flag, n, lab->partial);
  hipLaunchKernelGGL(hf_scan_partials_kernel, dim3(1), dim3(HF_SCAN_THREADS), 0, s, lab->partial, (int)nblk, lab->total);
  hipLaunchKernelGGL((hf_scan_apply_kernel<hf_root_flag, hf_rank_out>), dim3((unsigned)nblk), dim3(HF_SCAN_THREADS), 0, s, flag, hf_rank_out{L}, n,
                     lab->partial);      // L is dead once R is written: the ranks take its place, at the roots only
  VWGPU_HIP(ctx, hipMemcpyAsync(&lab->nb, lab->total, sizeof(int), hipMemcpyDeviceToHost, s));
  VWGPU_HIP(ctx, hipStreamSynchronize(s));
  const size_t nb = (size_t)lab->nb;
  rc = vwgpu_arena_reserve(ctx, &ctx->hole_tab, (vwgpu_align_up(5 * nb, 64) + extra_ints + 64) * sizeof(int));
  if (rc) return rc;
  lab->st = static_cast<int*>(ctx->hole_tab.base);
  lab->extra = lab->st + vwgpu_align_up(5 * nb, 64);
  if (nb) {
    hipLaunchKernelGGL(hf_stats_init_kernel, dim3(hf_blocks((long long)nb, 256)), dim3(256), 0, s, lab->st, (int)nb);
    hipLaunchKernelGGL(hf_stats_kernel, hf_grid(w, h), hf_block, 0, s, lab->R, lab->rank, w, h, lab->st, (int)nb);
  }
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

// The blobs that max_area and wipe_size keep, numbered in order: newid[b] = 1-based number or 0 (nb ints at `newid`, scan partials
// behind them).  Waits for the device once, for *kept.
size_t hf_select_ints(size_t nb) { return vwgpu_align_up(nb, 64) + vwgpu_align_up(hf_blocks((long long)nb, HF_SCAN_BLOCK) + 1, 64) + 64; }
int hf_select(vwgpu_ctx* ctx, const hf_labelling& lab, int max_area, int wipe, int* newid, int* kept) {
  *kept = 0;
  if (!lab.nb) return VWGPU_OK;
  hipStream_t s = ctx->stream;
  const int nb = lab.nb;
  const unsigned nblk = hf_blocks(nb, HF_SCAN_BLOCK);
  int* partial = newid + vwgpu_align_up((size_t)nb, 64);
  int* total = partial + vwgpu_align_up((size_t)nblk + 1, 64);
  VWGPU_HIP(ctx, hipMemsetAsync(newid, 0, (size_t)nb * sizeof(int), s));
  const hf_keep_flag flag{lab.st, nb, max_area, wipe};
  hipLaunchKernelGGL(hf_scan_count_kernel<hf_keep_flag>, dim3(nblk), dim3(HF_SCAN_THREADS), 0, s, flag, nb, partial);
  hipLaunchKernelGGL(hf_scan_partials_kernel, dim3(1), dim3(HF_SCAN_THREADS), 0, s, partial, (int)nblk, total);
  hipLaunchKernelGGL((hf_scan_apply_kernel<hf_keep_flag, hf_newid_out>), dim3(nblk), dim3(HF_SCAN_THREADS), 0, s, flag, hf_newid_out{newid}, nb, partial);
  VWGPU_HIP(ctx, hipMemcpyAsync(kept, total, sizeof(int), hipMemcpyDeviceToHost, s));
  VWGPU_HIP(ctx, hipStreamSynchronize(s));
  return VWGPU_OK;
}

int hf_copy_image(vwgpu_ctx* ctx, int kind, const void* in, ptrdiff_t istride, void* out, ptrdiff_t ostride, int w, int h) {
  if (in == out) return VWGPU_OK;
  const size_t e = (size_t)hf_kind_bytes(kind);
  VWGPU_HIP(ctx, hipMemcpy2DAsync(out, (size_t)ostride * e, in, (size_t)istride * e, (size_t)w * e, (size_t)h, hipMemcpyDeviceToDevice, ctx->stream));
  return VWGPU_OK;
}

size_t hf_inpaint_lds(int channels, int max_len) {
  const size_t P = (size_t)(max_len + 2) * (max_len + 2), N = (size_t)max_len * max_len;
  return (channels * P + P + 2 * N + 2) * 4;
}

// the blobs of `table` into out (which already holds the image)
int hf_inpaint_run(vwgpu_ctx* ctx, int kind, const void* in, int w, int h, ptrdiff_t istride, const int32_t* labels, ptrdiff_t lstride,
                   const int32_t* table, int count, int use_grassfire, const float* default_px, int semantics, int max_len, void* out,
                   ptrdiff_t ostride) {
  if (count <= 0 || max_len <= 0) return VWGPU_OK;
  const int C = kind == VWGPU_PIXEL_MASKED_F32 ? 1 : 2;
  hf_inpaint_args a{static_cast<const float*>(in), (long long)istride, static_cast<float*>(out), (long long)ostride, labels, (long long)lstride,
                    table, w, h, semantics, max_len, ctx->inpaint_overlap};
  hipStream_t s = ctx->stream;
  if (!use_grassfire) {
    const float d0 = default_px ? default_px[0] : 0.0f, d1 = default_px ? default_px[1] : 0.0f, d2 = default_px && C == 2 ? default_px[2] : 0.0f;
    if (C == 1) hipLaunchKernelGGL(hf_inpaint_default_kernel<1>, hf_grid(w, h), hf_block, 0, s, a, count, d0, d1, d2);
    else hipLaunchKernelGGL(hf_inpaint_default_kernel<2>, hf_grid(w, h), hf_block, 0, s, a, count, d0, d1, d2);
  } else {
    const size_t lds = hf_inpaint_lds(C, max_len);
    if (C == 1) {
      VWGPU_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(hf_inpaint_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(hf_inpaint_kernel<1>, dim3((unsigned)count), dim3(64), lds, s, a);
    } else {
      VWGPU_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(hf_inpaint_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(hf_inpaint_kernel<2>, dim3((unsigned)count), dim3(64), lds, s, a);
    }
  }
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int hf_float_kind_check(vwgpu_ctx* ctx, const char* name, int kind) {
  if (kind != VWGPU_PIXEL_MASKED_F32 && kind != VWGPU_PIXEL_DISPARITY_F32)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: pixel kind %d is neither PixelMask<float> nor a float disparity", name, kind);
  return VWGPU_OK;
}
int hf_edge_len_check(vwgpu_ctx* ctx, const char* name, int semantics, int len) {
  if (semantics != VWGPU_HOLE_EDGE_REFERENCE && semantics != VWGPU_HOLE_EDGE_FIXED)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: unknown edge semantics %d", name, semantics);
  if (len < 0 || len > VWGPU_HOLE_FILL_MAX_LEN)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: a hole length of %d is outside [0, %d]", name, len, VWGPU_HOLE_FILL_MAX_LEN);
  return VWGPU_OK;
}

int grassfire_check(vwgpu_ctx* ctx, int src_type, const void* src, int w, int h, ptrdiff_t& sstride, const void* out, ptrdiff_t& ostride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (src_type < VWGPU_GRASSFIRE_U8 || src_type > VWGPU_GRASSFIRE_F32) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "grassfire: unknown source type %d", src_type);
  if (!src || !out || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "grassfire: empty image or null pointer");
  if ((long long)w + h > INT_MAX / 2) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "grassfire: cols + rows overflows");
  if (sstride == 0) sstride = w;
  if (ostride == 0) ostride = w;
  if (sstride < w || ostride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "grassfire: row stride smaller than row width");
  return VWGPU_OK;
}

int blob_index_check(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t& istride, const void* labels, ptrdiff_t& lstride,
                     const void* table, int table_cap, const int* count) {
  int rc = hf_check_image(ctx, "blob_index", kind, img, w, h, istride);
  if (rc) return rc;
  if (!count) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "blob_index: empty image or null pointer");
  if (table && table_cap < 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "blob_index: negative table capacity");
  return hf_check_out(ctx, "blob_index", labels, w, lstride, true);
}
int blob_index_run(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, int invert, int max_area, int wipe,
                   int32_t* labels, ptrdiff_t lstride, int32_t* table, int table_cap, int* count) {
  vwgpu_prof_scope ps(ctx, "blob_index");
  hf_labelling lab;
  int rc = hf_label(ctx, kind, img, w, h, istride, invert, 0, &lab);
  if (rc) return rc;
  // the numbering of the kept blobs, sized now that nb is known
  rc = vwgpu_arena_reserve(ctx, &ctx->misc, hf_select_ints((size_t)lab.nb) * sizeof(int));
  if (rc) return rc;
  int* newid = static_cast<int*>(ctx->misc.base);
  if ((rc = hf_select(ctx, lab, max_area, wipe, newid, count))) return rc;
  hipStream_t s = ctx->stream;
  if (labels) {
    if (lab.nb) hipLaunchKernelGGL(hf_labels_kernel, hf_grid(w, h), hf_block, 0, s, lab.R, lab.rank, newid, w, h, labels, (long long)lstride);
    else hipLaunchKernelGGL(hf_zero_kernel, hf_grid(w, h), hf_block, 0, s, labels, (long long)lstride, w, h);
  }
  if (table) {
    if (*count > table_cap) return vwgpu_fail(ctx, VWGPU_ERR_CAPACITY, "blob_index: %d blobs, the table holds %d", *count, table_cap);
    if (lab.nb) hipLaunchKernelGGL(hf_table_kernel, dim3(hf_blocks(lab.nb, 256)), dim3(256), 0, s, lab.st, newid, lab.nb, table);
  }
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int sizes_erode_check(vwgpu_ctx* ctx, const char* name, int kind, const void* img, int w, int h, ptrdiff_t& istride, const void* out,
                      ptrdiff_t& ostride) {
  int rc = hf_check_image(ctx, name, kind, img, w, h, istride);
  if (rc) return rc;
  return hf_check_out(ctx, name, out, w, ostride);
}

int inpaint_check(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t& istride, const void* labels, ptrdiff_t& lstride,
                  const void* table, int count, int semantics, int max_len, const void* out, ptrdiff_t& ostride) {
  int rc = hf_check_image(ctx, "inpaint", kind, img, w, h, istride);
  if (rc) return rc;
  if ((rc = hf_float_kind_check(ctx, "inpaint", kind))) return rc;
  if ((rc = hf_edge_len_check(ctx, "inpaint", semantics, max_len))) return rc;
  if (count < 0 || !labels || (count > 0 && !table)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "inpaint: empty image or null pointer");
  if (lstride == 0) lstride = w;
  if (lstride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "inpaint: row stride smaller than row width");
  return hf_check_out(ctx, "inpaint", out, w, ostride);
}

int fill_holes_check(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t& istride, int len, int semantics, const void* out,
                     ptrdiff_t& ostride) {
  int rc = hf_check_image(ctx, "fill_holes_grass", kind, img, w, h, istride);
  if (rc) return rc;
  if ((rc = hf_float_kind_check(ctx, "fill_holes_grass", kind))) return rc;
  if ((rc = hf_edge_len_check(ctx, "fill_holes_grass", semantics, len))) return rc;
  return hf_check_out(ctx, "fill_holes_grass", out, w, ostride);
}

int avg_check(vwgpu_ctx* ctx, const void* img, int w, int h, ptrdiff_t& istride, int kernel_size, const void* out, ptrdiff_t& ostride) {
  int rc = hf_check_image(ctx, "fill_nodata_with_avg", VWGPU_PIXEL_MASKED_F32, img, w, h, istride);
  if (rc) return rc;
  if (kernel_size <= 0 || kernel_size % 2 == 0)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "fill_nodata_with_avg: Expecting odd and positive kernel size.");
  if (out == img) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "fill_nodata_with_avg: input and output must be different images");
  return hf_check_out(ctx, "fill_nodata_with_avg", out, w, ostride);
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) --------------------------------------------------------------------

extern "C" {

int vwgpu_grassfire_dev(vwgpu_ctx* ctx, int src_type, const void* d_src, int w, int h, ptrdiff_t sstride, int ignore_borders,
                        int32_t* d_out, ptrdiff_t ostride) {
  int rc = grassfire_check(ctx, src_type, d_src, w, h, sstride, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope ps(ctx, "grassfire");
  hipStream_t s = ctx->stream;
  if (w <= 1 || h <= 1) {
    hipLaunchKernelGGL(hf_zero_kernel, hf_grid(w, h), hf_block, 0, s, d_out, (long long)ostride, w, h);
  } else {
    const int ib = ignore_borders != 0, cap = w + h;
    const dim3 rg((unsigned)((h + 3) / 4)), rb(256);
    switch (src_type) {
      case VWGPU_GRASSFIRE_U8:
        hipLaunchKernelGGL(hf_grass_rows_kernel<uint8_t>, rg, rb, 0, s, static_cast<const uint8_t*>(d_src), (long long)sstride, w, h, ib, cap, d_out, (long long)ostride);
        break;
      case VWGPU_GRASSFIRE_I32:
        hipLaunchKernelGGL(hf_grass_rows_kernel<int32_t>, rg, rb, 0, s, static_cast<const int32_t*>(d_src), (long long)sstride, w, h, ib, cap, d_out, (long long)ostride);
        break;
      default:
        hipLaunchKernelGGL(hf_grass_rows_kernel<float>, rg, rb, 0, s, static_cast<const float*>(d_src), (long long)sstride, w, h, ib, cap, d_out, (long long)ostride);
    }
    hipLaunchKernelGGL(hf_grass_cols_kernel, dim3((unsigned)((w + 63) / 64)), dim3(64), 0, s, d_out, (long long)ostride, w, h, ib, cap);
  }
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int vwgpu_grassfire(vwgpu_ctx* ctx, int src_type, const void* src, int w, int h, ptrdiff_t sstride, int ignore_borders, int32_t* out,
                    ptrdiff_t ostride) {
  int rc = grassfire_check(ctx, src_type, src, w, h, sstride, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(src, w, h, src_type == VWGPU_GRASSFIRE_U8 ? 1 : 4, sstride, VWGPU_STAGE_IN), po = st.add(out, w, h, 4, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_grassfire_dev(ctx, src_type, st.dev<void>(pi), w, h, w, ignore_borders, st.dev<int32_t>(po), w);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_blob_index_dev(vwgpu_ctx* ctx, int kind, const void* d_img, int w, int h, ptrdiff_t istride, int invert, int max_area,
                         int wipe_size, int32_t* d_labels, ptrdiff_t lstride, int32_t* d_table, int table_cap, int* count) {
  int rc = blob_index_check(ctx, kind, d_img, w, h, istride, d_labels, lstride, d_table, table_cap, count);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return blob_index_run(ctx, kind, d_img, w, h, istride, invert, max_area, wipe_size, d_labels, lstride, d_table, table_cap, count);
}

int vwgpu_blob_index(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, int invert, int max_area, int wipe_size,
                     int32_t* labels, ptrdiff_t lstride, int32_t* table, int table_cap, int* count) {
  int rc = blob_index_check(ctx, kind, img, w, h, istride, labels, lstride, table, table_cap, count);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(img, w, h, hf_kind_bytes(kind), istride, VWGPU_STAGE_IN), pl = st.add(labels, w, h, 4, lstride, VWGPU_STAGE_OUT),
            pt = st.add(table ? table : nullptr, 5, table_cap, 4, 5, table ? VWGPU_STAGE_NONE : VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = blob_index_run(ctx, kind, st.dev<void>(pi), w, h, w, invert, max_area, wipe_size, st.dev<int32_t>(pl), w,
                      table ? st.dev<int32_t>(pt) : nullptr, table_cap, count);
  if (rc) return rc;
  if (table && (rc = st.download(pt, table, 5, *count, 5))) return rc;
  return st.finish();
}

int vwgpu_blob_sizes_dev(vwgpu_ctx* ctx, int kind, const void* d_img, int w, int h, ptrdiff_t istride, uint32_t limit, uint32_t* d_out,
                         ptrdiff_t ostride) {
  int rc = sizes_erode_check(ctx, "blob_sizes", kind, d_img, w, h, istride, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope ps(ctx, "blob_sizes");
  hf_labelling lab;
  if ((rc = hf_label(ctx, kind, d_img, w, h, istride, 0, 0, &lab))) return rc;
  if (lab.nb) hipLaunchKernelGGL(hf_sizes_kernel, hf_grid(w, h), hf_block, 0, ctx->stream, lab.R, lab.rank, lab.st, w, h, limit, d_out, (long long)ostride);
  else hipLaunchKernelGGL(hf_zero_kernel, hf_grid(w, h), hf_block, 0, ctx->stream, reinterpret_cast<int32_t*>(d_out), (long long)ostride, w, h);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int vwgpu_blob_sizes(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, uint32_t limit, uint32_t* out,
                     ptrdiff_t ostride) {
  int rc = sizes_erode_check(ctx, "blob_sizes", kind, img, w, h, istride, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(img, w, h, hf_kind_bytes(kind), istride, VWGPU_STAGE_IN), po = st.add(out, w, h, 4, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_blob_sizes_dev(ctx, kind, st.dev<void>(pi), w, h, w, limit, st.dev<uint32_t>(po), w);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_erode_blobs_dev(vwgpu_ctx* ctx, int kind, const void* d_img, int w, int h, ptrdiff_t istride, int max_area, void* d_out,
                          ptrdiff_t ostride) {
  int rc = sizes_erode_check(ctx, "erode_blobs", kind, d_img, w, h, istride, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope ps(ctx, "erode_blobs");
  if ((rc = hf_copy_image(ctx, kind, d_img, istride, d_out, ostride, w, h))) return rc;
  if (max_area < 1) return VWGPU_OK;
  hf_labelling lab;
  if ((rc = hf_label(ctx, kind, d_img, w, h, istride, 0, 0, &lab))) return rc;
  if (lab.nb) hipLaunchKernelGGL(hf_erase_kernel, hf_grid(w, h), hf_block, 0, ctx->stream, lab.R, lab.rank, lab.st, w, h, max_area, kind, d_out, (long long)ostride);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int vwgpu_erode_blobs(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, int max_area, void* out, ptrdiff_t ostride) {
  int rc = sizes_erode_check(ctx, "erode_blobs", kind, img, w, h, istride, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int e = hf_kind_bytes(kind);
  const int pi = st.add(img, w, h, e, istride, VWGPU_STAGE_IN), po = st.add(out, w, h, e, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_erode_blobs_dev(ctx, kind, st.dev<void>(pi), w, h, w, max_area, st.dev<void>(po), w);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_inpaint_dev(vwgpu_ctx* ctx, int kind, const void* d_img, int w, int h, ptrdiff_t istride, const int32_t* d_labels, ptrdiff_t lstride,
                      const int32_t* d_table, int count, int use_grassfire, const float* default_pixel, int semantics, int max_len,
                      void* d_out, ptrdiff_t ostride) {
  int rc = inpaint_check(ctx, kind, d_img, w, h, istride, d_labels, lstride, d_table, count, semantics, max_len, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope ps(ctx, "inpaint");
  if ((rc = hf_copy_image(ctx, kind, d_img, istride, d_out, ostride, w, h))) return rc;
  return hf_inpaint_run(ctx, kind, d_img, w, h, istride, d_labels, lstride, d_table, count, use_grassfire, default_pixel, semantics, max_len,
                        d_out, ostride);
}

int vwgpu_inpaint(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, const int32_t* labels, ptrdiff_t lstride,
                  const int32_t* table, int count, int use_grassfire, const float* default_pixel, int semantics, int max_len, void* out,
                  ptrdiff_t ostride) {
  int rc = inpaint_check(ctx, kind, img, w, h, istride, labels, lstride, table, count, semantics, max_len, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int e = hf_kind_bytes(kind);
  const bool in_place = out == img;
  const int pi = st.add(img, w, h, e, istride, in_place ? VWGPU_STAGE_INOUT : VWGPU_STAGE_IN),
            po = in_place ? pi : st.add(out, w, h, e, ostride, VWGPU_STAGE_OUT), pl = st.add(labels, w, h, 4, lstride, VWGPU_STAGE_IN),
            pt = st.add(table, 5, count, 4, 5, VWGPU_STAGE_IN);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_inpaint_dev(ctx, kind, st.dev<void>(pi), w, h, w, st.dev<int32_t>(pl), w, st.dev<int32_t>(pt), count, use_grassfire, default_pixel,
                         semantics, max_len, st.dev<void>(po), w);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_fill_holes_grass_dev(vwgpu_ctx* ctx, int kind, const void* d_img, int w, int h, ptrdiff_t istride, int hole_fill_len, int semantics,
                               void* d_out, ptrdiff_t ostride) {
  int rc = fill_holes_check(ctx, kind, d_img, w, h, istride, hole_fill_len, semantics, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope ps(ctx, "fill_holes_grass");
  if (hole_fill_len == 0) return hf_copy_image(ctx, kind, d_img, istride, d_out, ostride, w, h);      // wipe_big_blobs(0) leaves no blob
  // the label image (n ints) is reserved with the statistics; the numbering and the table (6 nb ints and partials) follow once nb is known
  const size_t n = (size_t)w * h;
  hf_labelling lab;
  if ((rc = hf_label(ctx, kind, d_img, w, h, istride, 1, vwgpu_align_up(n, 64), &lab))) return rc;
  if ((rc = hf_copy_image(ctx, kind, d_img, istride, d_out, ostride, w, h))) return rc;
  if (!lab.nb) return VWGPU_OK;
  const size_t nb = (size_t)lab.nb;
  rc = vwgpu_arena_reserve(ctx, &ctx->misc, (hf_select_ints(nb) + vwgpu_align_up(5 * nb, 64)) * sizeof(int));
  if (rc) return rc;
  int* newid = static_cast<int*>(ctx->misc.base);
  int32_t* table = newid + hf_select_ints(nb);
  int32_t* labels = lab.extra;
  int kept = 0;
  // wipe_big_blobs(len) implies the area limit len * len of the constructor
  if ((rc = hf_select(ctx, lab, hole_fill_len * hole_fill_len, hole_fill_len, newid, &kept))) return rc;
  if (!kept) return VWGPU_OK;
  hipStream_t s = ctx->stream;
  hipLaunchKernelGGL(hf_labels_kernel, hf_grid(w, h), hf_block, 0, s, lab.R, lab.rank, newid, w, h, labels, (long long)w);
  hipLaunchKernelGGL(hf_table_kernel, dim3(hf_blocks(lab.nb, 256)), dim3(256), 0, s, lab.st, newid, lab.nb, table);
  return hf_inpaint_run(ctx, kind, d_img, w, h, istride, labels, w, table, kept, 1, nullptr, semantics, hole_fill_len, d_out, ostride);
}

int vwgpu_fill_holes_grass(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, int hole_fill_len, int semantics,
                           void* out, ptrdiff_t ostride) {
  int rc = fill_holes_check(ctx, kind, img, w, h, istride, hole_fill_len, semantics, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int e = hf_kind_bytes(kind);
  const bool in_place = out == img;
  const int pi = st.add(img, w, h, e, istride, in_place ? VWGPU_STAGE_INOUT : VWGPU_STAGE_IN),
            po = in_place ? pi : st.add(out, w, h, e, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_fill_holes_grass_dev(ctx, kind, st.dev<void>(pi), w, h, w, hole_fill_len, semantics, st.dev<void>(po), w);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_fill_nodata_with_avg_dev(vwgpu_ctx* ctx, const float* d_img, int w, int h, ptrdiff_t istride, int kernel_size, float* d_out,
                                   ptrdiff_t ostride) {
  int rc = avg_check(ctx, d_img, w, h, istride, kernel_size, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope ps(ctx, "fill_nodata_with_avg");
  hipLaunchKernelGGL(hf_avg_kernel, hf_grid(w, h), hf_block, 0, ctx->stream, d_img, (long long)istride, w, h, kernel_size / 2, d_out, (long long)ostride);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int vwgpu_fill_nodata_with_avg(vwgpu_ctx* ctx, const float* img, int w, int h, ptrdiff_t istride, int kernel_size, float* out,
                               ptrdiff_t ostride) {
  int rc = avg_check(ctx, img, w, h, istride, kernel_size, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(img, w, h, 8, istride, VWGPU_STAGE_IN), po = st.add(out, w, h, 8, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_fill_nodata_with_avg_dev(ctx, st.dev<float>(pi), w, h, w, kernel_size, st.dev<float>(po), w);
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
