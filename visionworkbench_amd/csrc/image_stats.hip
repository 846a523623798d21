// image_stats.hip — input conditioning, the stage before everything else: the whole-image statistics of
// src/vw/Image/Statistics.h (find_image_min_max :113-127, min_max_channel_values :98-108, sum / mean / stddev / median
// _channel_value :129-186) with the accumulators of src/vw/Math/Functors.h (:355-518), vw::histogram, otsu_threshold,
// percentile_scale_convert and u8_convert of src/vw/Image/ImageThresh.h over math::Histogram (src/vw/Math/Statistics.cc:
// 34-104), clamp / normalize / threshold of src/vw/Image/Algorithms.h and normalize(image, low, high) of
// src/vw/Image/AutoNormalize.h.  tests/refimpl/image_stats_ref.cc restates them and DESIGN §4.25 lists what is reproduced.
//
// One visiting scheme serves every reduction (is_visit): a work item is four consecutive pixels of one row, read as one
// 16-byte load where the four lie inside the row on a 16-byte boundary and as scalar loads at the ragged ends; the mask's
// four bytes likewise as one dword or four bytes.  Reductions whose result does not depend on the order (extrema, counts)
// shift the items of a row so that its interior is aligned whatever the pointer and the stride are; the moments cut every
// row at x = 0, 4, 8, .. so that the order of the additions depends on the image's size alone.
//   range      lanes -> wavefront (shuffles) -> workgroup (LDS) -> one slab row per workgroup -> a one-workgroup fold
//   moments    the same, in double, every step in a fixed order (no float atomics: the sums must be reproducible)
//   histogram  one private sub-histogram per wavefront in LDS (integer LDS adds; lanes of a wavefront that meet in a bin
//              are counted by one add), folded across the workgroup, one 64-bit integer global add per non-empty bin per
//              workgroup.  Integer counts: every order gives the same words.
//   select     the k-th smallest value by three histogram passes over the digits of the order-preserving key, the digit
//              chosen by a one-workgroup kernel in device memory, so that no pass waits for the host
//   rescale    one lane per four pixels, 16-byte loads and stores where both rows allow
// Arithmetic is the reference's types in the reference's order; the Makefile's -ffp-contract=off keeps products and sums
// apart.
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "vwgpu_internal.h"

namespace {

constexpr int IS_THREADS = 256, IS_WAVES = IS_THREADS / 64, IS_MAX_BLOCKS = 1024;   // 4 workgroups per CU on 256 CUs
constexpr unsigned long long IS_NONE = ~0ull;

// layout of ctx->istats
constexpr size_t IS_OFF_RANGE = 0, IS_OFF_MOMENTS = 256, IS_OFF_PARAMS = 512, IS_OFF_ORDER = 1024, IS_OFF_COUNTS = 2048,
                 IS_OFF_SLAB = 36864, IS_OFF_TABLES = 90112;
static_assert(IS_OFF_COUNTS + (VWGPU_HISTOGRAM_MAX_BINS + 2) * 8 <= IS_OFF_SLAB, "the bins overlap the slab");

struct is_view {
  const float* in; long long is;
  const uint8_t* mask; long long ms;
  int w, h;
  const int *xs, *ys;   // sampling tables (device), or nullptr
  int sc, sr;
};

// f(value, valid, raster index of the visit) for every pixel the view names; all four slots of an item are offered, so that
// the lanes of a wavefront stay together inside f.  ALIGN: shift the items of a row onto its 16-byte boundaries.
template <bool ALIGN, class F>
__device__ inline void is_visit(const is_view& V, F&& f) {
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  const unsigned long long start = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (V.xs) {
    const unsigned long long n = (unsigned long long)V.sc * (unsigned long long)V.sr;
    for (unsigned long long i = start; i < n; i += step) {
      const unsigned long long r = i / (unsigned)V.sc;
      const int x = V.xs[(int)(i - r * (unsigned)V.sc)], y = V.ys[(int)r];
      const bool ok = !V.mask || V.mask[(long long)y * V.ms + x] != 0;
      f(V.in[(long long)y * V.is + x], ok, i);
    }
    return;
  }
  const unsigned nu = ALIGN ? ((unsigned)V.w + 6u) >> 2 : ((unsigned)V.w + 3u) >> 2;   // items per row: a shifted row has up to one more
  const unsigned long long n = (unsigned long long)nu * (unsigned long long)V.h;
  for (unsigned long long i = start; i < n; i += step) {
    // the row in 32 bits when it fits: a 64-bit division per item costs more than the item's traffic
    const unsigned y = n <= 0xffffffffull ? (unsigned)i / nu : (unsigned)(i / nu);
    const unsigned u = (unsigned)(i - (unsigned long long)y * nu);
    const float* row = V.in + (long long)y * V.is;
    const int lead = ALIGN ? (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3) : 0;
    const int x0 = (int)(4u * u) - lead;
    if (x0 >= V.w) continue;
    const uint8_t* mrow = V.mask ? V.mask + (long long)y * V.ms : nullptr;
    const unsigned long long base = (unsigned long long)y * (unsigned)V.w;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    bool ok[4];
    if (x0 >= 0 && x0 + 4 <= V.w && (reinterpret_cast<uintptr_t>(row + x0) & 15) == 0) {
      const float4 q = *reinterpret_cast<const float4*>(row + x0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
      if (!mrow) {
        ok[0] = ok[1] = ok[2] = ok[3] = true;
      } else if ((reinterpret_cast<uintptr_t>(mrow + x0) & 3) == 0) {
        const uint32_t m = *reinterpret_cast<const uint32_t*>(mrow + x0);
        ok[0] = (m & 0xffu) != 0; ok[1] = (m & 0xff00u) != 0; ok[2] = (m & 0xff0000u) != 0; ok[3] = (m & 0xff000000u) != 0;
      } else {
        for (int k = 0; k < 4; ++k) ok[k] = mrow[x0 + k] != 0;
      }
    } else {
      for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        ok[k] = x >= 0 && x < V.w;
        if (ok[k]) {
          v[k] = row[x];
          if (mrow) ok[k] = mrow[x] != 0;
        }
      }
    }
    for (int k = 0; k < 4; ++k) f(v[k], ok[k], base + (unsigned long long)(long long)(x0 + k));
  }
}

__device__ inline unsigned long long is_wave_sum(unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;
}

// ---- extrema and counts -------------------------------------------------------------------------------------------
// Both modes are the min / max over the valid non-NaN pixels (`val < min`, `val > max`, `max < arg` never admit a NaN);
// MinMaxAccumulator also keeps a NaN that is its first sample, so the reduction carries the smallest raster index of a
// valid pixel and of a valid NaN pixel: the two are equal exactly when the first sample is a NaN.
struct is_range_acc {
  float mn, mx;
  unsigned long long count, nan, first, first_nan;
};

__device__ inline void is_range_merge(is_range_acc& r, const is_range_acc& o) {
  r.mn = o.mn < r.mn ? o.mn : r.mn;
  r.mx = o.mx > r.mx ? o.mx : r.mx;
  r.count += o.count;
  r.nan += o.nan;
  r.first = o.first < r.first ? o.first : r.first;
  r.first_nan = o.first_nan < r.first_nan ? o.first_nan : r.first_nan;
}

// lanes of a wavefront by shuffles, wavefronts through LDS; the result is valid in thread 0
__device__ inline void is_range_block_reduce(is_range_acc& r, is_range_acc* lds) {
  for (int d = 32; d > 0; d >>= 1) {
    is_range_acc o;
    o.mn = __shfl_down(r.mn, d); o.mx = __shfl_down(r.mx, d);
    o.count = __shfl_down(r.count, d); o.nan = __shfl_down(r.nan, d);
    o.first = __shfl_down(r.first, d); o.first_nan = __shfl_down(r.first_nan, d);
    is_range_merge(r, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = r;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < IS_WAVES; ++k) is_range_merge(r, lds[k]);
}

__global__ __launch_bounds__(IS_THREADS) void is_range_partial_kernel(is_view V, is_range_acc* partial) {
  __shared__ is_range_acc lds[IS_WAVES];
  is_range_acc r{INFINITY, -INFINITY, 0, 0, IS_NONE, IS_NONE};
  is_visit<true>(V, [&](float v, bool ok, unsigned long long idx) {
    if (!ok) return;
    r.count++;
    r.first = idx < r.first ? idx : r.first;
    if (v != v) {
      r.nan++;
      r.first_nan = idx < r.first_nan ? idx : r.first_nan;
    } else {
      r.mn = v < r.mn ? v : r.mn;
      r.mx = v > r.mx ? v : r.mx;
    }
  });
  is_range_block_reduce(r, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ __launch_bounds__(IS_THREADS) void is_range_fold_kernel(const is_range_acc* partial, int n, int mode, vwgpu_image_range* out) {
  __shared__ is_range_acc lds[IS_WAVES];
  is_range_acc r{INFINITY, -INFINITY, 0, 0, IS_NONE, IS_NONE};
  for (int i = threadIdx.x; i < n; i += IS_THREADS) is_range_merge(r, partial[i]);
  is_range_block_reduce(r, lds);
  if (threadIdx.x != 0) return;
  vwgpu_image_range o;
  o.count = (long long)r.count;
  o.nan_count = (long long)r.nan;
  if (mode == VWGPU_MIN_MAX_FIND) {           // the comparisons against DBL_MAX / -DBL_MAX, which an infinity of the wrong sign fails
    o.min = (double)r.mn < DBL_MAX ? (double)r.mn : DBL_MAX;
    o.max = (double)r.mx > -DBL_MAX ? (double)r.mx : -DBL_MAX;
  } else if (r.count == 0) {
    o.min = o.max = 0.0;
  } else if (r.first_nan == r.first) {
    o.min = o.max = (double)NAN;
  } else {
    o.min = (double)r.mn;
    o.max = (double)r.mx;
  }
  *out = o;
}

// ---- moments -------------------------------------------------------------------------------------------------------
struct is_mom_acc { double n, s, q; };

__device__ inline void is_mom_block_reduce(is_mom_acc& r, is_mom_acc* lds) {
  for (int d = 32; d > 0; d >>= 1) {
    r.n += __shfl_down(r.n, d);
    r.s += __shfl_down(r.s, d);
    r.q += __shfl_down(r.q, d);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = r;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < IS_WAVES; ++k) { r.n += lds[k].n; r.s += lds[k].s; r.q += lds[k].q; }
}

__global__ __launch_bounds__(IS_THREADS) void is_moments_partial_kernel(is_view V, is_mom_acc* partial) {
  __shared__ is_mom_acc lds[IS_WAVES];
  is_mom_acc r{0.0, 0.0, 0.0};
  is_visit<false>(V, [&](float v, bool ok, unsigned long long) {
    if (!ok) return;
    const double x = (double)v;
    r.n += 1.0;
    r.s += x;
    r.q += x * x;     // (accum_type) arg * arg, Functors.h:504
  });
  is_mom_block_reduce(r, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ __launch_bounds__(IS_THREADS) void is_moments_fold_kernel(const is_mom_acc* partial, int n, double* out) {
  __shared__ is_mom_acc lds[IS_WAVES];
  is_mom_acc r{0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += IS_THREADS) { r.n += partial[i].n; r.s += partial[i].s; r.q += partial[i].q; }
  is_mom_block_reduce(r, lds);
  if (threadIdx.x == 0) { out[0] = r.n; out[1] = r.s; out[2] = r.q; }
}

// ---- histogram -----------------------------------------------------------------------------------------------------
// The state of one radix select: the digits fixed so far and the rank left inside them.
struct is_sel {
  uint32_t prefix, pmask;
  unsigned long long k, len, nan;
  float value; int pad;
};
struct is_order_block { is_sel sel[2]; double result; };

__device__ inline uint32_t is_key(float v) {       // ascending floats -> ascending keys (-0.0 directly below +0.0)
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float is_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// One count into a wavefront's sub-histogram.  The lanes that hold the bin of the first pending lane are counted by ONE
// add, twice over; what is left adds on its own.  A constant region (every lane in one bin, or in two neighbours) would
// otherwise be 64 adds on one LDS word, one after the other.
__device__ inline void is_lds_count(uint32_t* hist, int bin, bool pending) {
  const int lane = threadIdx.x & 63;
  for (int round = 0; round < 2; ++round) {
    const unsigned long long m = __ballot(pending);
    if (!m) return;
    const int leader = __ffsll((long long)m) - 1;
    const int b0 = __shfl(bin, leader);
    const bool same = pending && bin == b0;
    const unsigned long long ms = __ballot(same);
    if (lane == leader) atomicAdd(&hist[b0], (uint32_t)__popcll(ms));
    pending = pending && !same;
  }
  if (pending) atomicAdd(&hist[bin], 1u);
}

// KEYS = false: the bins of math::Histogram::add_value between mn and mx (d_range, when given, holds them).
// KEYS = true: digit (key >> shift) & (nb - 1) of the pixels whose key agrees with sel->prefix on sel->pmask.
// counts: nb bins, then the total, then the NaN count (64-bit integer adds: counts must have been zeroed or hold earlier tiles).
template <bool KEYS>
__global__ __launch_bounds__(IS_THREADS) void is_hist_kernel(is_view V, int nb, int copies, double mn, double mx, const vwgpu_image_range* d_range,
                                                             const is_sel* sel, int shift, unsigned long long* counts) {
  extern __shared__ uint32_t is_hist_lds[];     // copies * nb words
  for (int i = threadIdx.x; i < copies * nb; i += IS_THREADS) is_hist_lds[i] = 0;
  __syncthreads();
  uint32_t* mine = is_hist_lds + ((threadIdx.x >> 6) % copies) * nb;
  unsigned long long total = 0, nans = 0;
  double scale = 0.0, range = 1.0;
  uint32_t prefix = 0, pmask = 0;
  if (KEYS) {
    prefix = sel->prefix; pmask = sel->pmask;
  } else {
    if (d_range) { mn = d_range->min; mx = d_range->max; }
    if (mx == mn) mx = mn + 1.0;       // ImageThresh.h:61-62
    range = mx - mn;                   // Statistics.cc:48
    scale = (double)(nb - 1);          // m_max_bin
  }
  is_visit<true>(V, [&](float v, bool ok, unsigned long long) {
    int bin = 0;
    if (ok) {
      if (KEYS) {
        const uint32_t key = is_key(v);
        if (v != v) { nans++; ok = false; }
        else if ((key & pmask) != prefix) ok = false;
        else bin = (int)((key >> shift) & (uint32_t)(nb - 1));
      } else {
        const double a = scale * (((double)v - mn) / range);      // Statistics.cc:59
        if (a != a) { nans++; ok = false; }
        else {
          const double r = round(a);
          bin = r < 0.0 ? 0 : r >= (double)nb ? nb - 1 : (int)r;   // saturate = true, :61-72
        }
      }
      if (ok) total++;
    }
    is_lds_count(mine, bin, ok);
  });
  __syncthreads();
  for (int b = threadIdx.x; b < nb; b += IS_THREADS) {
    unsigned long long s = 0;
    for (int c = 0; c < copies; ++c) s += is_hist_lds[c * nb + b];
    if (s) atomicAdd(&counts[b], s);
  }
  total = is_wave_sum(total);
  nans = is_wave_sum(nans);
  if ((threadIdx.x & 63) == 0) {
    if (total) atomicAdd(&counts[nb], total);
    if (nans) atomicAdd(&counts[nb + 1], nans);
  }
}

// One digit of a radix select (one workgroup).  first: take len and the rank from the pass's total; last: the key is
// complete, write the value.  rank 0 / 1: the lower and the upper middle of a median.
__global__ __launch_bounds__(IS_THREADS) void is_select_kernel(const unsigned long long* counts, int nb, int shift, int first, int last,
                                                               int kind, double arg, int rank, is_order_block* blk, double* d_result) {
  __shared__ unsigned long long chunk[IS_THREADS];
  __shared__ unsigned long long k_sh;
  is_sel* s = &blk->sel[rank];
  const int per = (nb + IS_THREADS - 1) / IS_THREADS;
  unsigned long long sum = 0;
  for (int j = 0; j < per; ++j) {
    const int b = threadIdx.x * per + j;
    if (b < nb) sum += counts[b];
  }
  chunk[threadIdx.x] = sum;
  if (threadIdx.x == 0) {
    if (first) {
      const unsigned long long len = counts[nb];
      unsigned long long k = 0;
      if (len) {
        if (kind == VWGPU_ORDER_MEDIAN) {
          k = rank ? len / 2 : (len - 1) / 2;
        } else if (kind == VWGPU_ORDER_PERCENTILE) {
          long long index = (long long)ceil((arg / 100.0) * (double)len);      // Functors.h:435-441
          index--;
          if (index < 0) index = 0;
          if (index >= (long long)len) index = (long long)len - 1;
          k = (unsigned long long)index;
        } else {
          k = arg >= (double)len ? len - 1 : (unsigned long long)arg;
        }
      }
      s->prefix = 0; s->pmask = 0; s->k = k; s->len = len; s->nan = counts[nb + 1]; s->value = 0.f; s->pad = 0;
    }
    k_sh = s->k;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned long long k = k_sh;
  int digit = nb - 1;
  if (s->len) {
    int t = 0;
    while (t < IS_THREADS - 1 && k >= chunk[t]) { k -= chunk[t]; ++t; }
    int b = t * per;
    const int end = min(nb, b + per) - 1;
    while (b < end && k >= counts[b]) { k -= counts[b]; ++b; }
    digit = min(b, nb - 1);
  }
  s->prefix |= (uint32_t)digit << shift;
  s->pmask |= (uint32_t)(nb - 1) << shift;
  s->k = k;
  if (!last) return;
  const bool bad = s->len == 0 || s->nan != 0;
  s->value = is_unkey(s->prefix);
  double res = (double)s->value;
  if (kind == VWGPU_ORDER_MEDIAN) {
    if (rank == 0) return;
    const float lo = blk->sel[0].value;
    res = (s->len & 1) ? (double)s->value : (lo + s->value) / 2.0;      // Functors.h:397: a float sum, divided in double
  }
  if (bad) res = (double)NAN;
  blk->result = res;
  if (d_result) *d_result = res;
}

// ---- rescale -------------------------------------------------------------------------------------------------------
enum { IS_RS_CLAMP = 1, IS_RS_NORMALIZE = 2, IS_RS_THRESHOLD = 4 };
struct is_rs {
  float lo, hi;             // ChannelClampFunctor
  float old_min, new_min;   // ChannelNormalizeFunctor
  double ratio;
  float thresh, tlow, thigh;
  int ops;
  int status, pad;          // non-zero: the statistics gave no stretch (no valid pixel, no bin at the percentile)
  double report[4];
};

__host__ __device__ inline void is_rs_normalize(is_rs& P, float old_min, float old_max, float new_min, float new_max) {
  P.old_min = old_min;
  P.new_min = new_min;
  P.ratio = old_max == old_min ? 0.0 : (new_max - new_min) / (double)(old_max - old_min);      // Algorithms.h:114-118
  P.ops |= IS_RS_NORMALIZE;
}

__device__ inline float is_rs_apply(const is_rs& P, float v) {
  if (P.ops & IS_RS_CLAMP) v = v > P.hi ? P.hi : v < P.lo ? P.lo : v;                                   // Algorithms.h:43-47
  if (P.ops & IS_RS_NORMALIZE) v = (float)((double)(v - P.old_min) * P.ratio + (double)P.new_min);     // :122-125
  if (P.ops & IS_RS_THRESHOLD) v = v > P.thresh ? P.thigh : P.tlow;                                    // :205-207
  return v;
}
__device__ inline uint32_t is_to_u8(float v) { return v >= 256.f ? 255u : v >= 0.f ? (uint32_t)v : 0u; }      // a NaN fails both: 0

template <int OUT>
__global__ __launch_bounds__(IS_THREADS) void is_rescale_kernel(const float* in, long long is, int w, int h, is_rs pv, const is_rs* d_params,
                                                                void* outv, long long os) {
  const is_rs P = d_params ? *d_params : pv;
  const unsigned nu = ((unsigned)w + 6u) >> 2;
  const unsigned long long n = (unsigned long long)nu * (unsigned long long)h;
  const unsigned long long step = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const unsigned y = n <= 0xffffffffull ? (unsigned)i / nu : (unsigned)(i / nu);
    const unsigned u = (unsigned)(i - (unsigned long long)y * nu);
    const float* row = in + (long long)y * is;
    const int x0 = (int)(4u * u) - (int)((reinterpret_cast<uintptr_t>(row) >> 2) & 3);
    if (x0 >= w) continue;
    const bool whole = x0 >= 0 && x0 + 4 <= w;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (whole && (reinterpret_cast<uintptr_t>(row + x0) & 15) == 0) {
      const float4 q = *reinterpret_cast<const float4*>(row + x0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      for (int k = 0; k < 4; ++k)
        if (x0 + k >= 0 && x0 + k < w) v[k] = row[x0 + k];
    }
    for (int k = 0; k < 4; ++k) v[k] = is_rs_apply(P, v[k]);
    if (OUT == VWGPU_PIXEL_U8) {
      uint8_t* orow = static_cast<uint8_t*>(outv) + (long long)y * os;
      uint32_t b[4];
      for (int k = 0; k < 4; ++k) b[k] = is_to_u8(v[k]);
      if (whole && (reinterpret_cast<uintptr_t>(orow + x0) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(orow + x0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
      } else {
        for (int k = 0; k < 4; ++k)
          if (x0 + k >= 0 && x0 + k < w) orow[x0 + k] = (uint8_t)b[k];
      }
    } else {
      float* orow = static_cast<float*>(outv) + (long long)y * os;
      if (OUT == VWGPU_PIXEL_U8_AS_F32)
        for (int k = 0; k < 4; ++k) v[k] = (float)is_to_u8(v[k]);
      if (whole && (reinterpret_cast<uintptr_t>(orow + x0) & 15) == 0) {
        *reinterpret_cast<float4*>(orow + x0) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        for (int k = 0; k < 4; ++k)
          if (x0 + k >= 0 && x0 + k < w) orow[x0 + k] = v[k];
      }
    }
  }
}

// The stretch of percentile_scale_convert (what 0), u8_convert (1) and normalize(image, low, high) (2) from the statistics on
// the device (one workgroup).  The percentile is Histogram::get_percentile (Statistics.cc:93-101): the quotients are formed
// by all lanes, the running sum by one lane in bin order, in the doubles of vwgpu_histogram_percentile.
enum { IS_STRETCH_PERCENTILE = 0, IS_STRETCH_MIN_MAX = 1, IS_STRETCH_AUTO = 2 };
__global__ __launch_bounds__(IS_THREADS) void is_stretch_kernel(int what, const vwgpu_image_range* range, const unsigned long long* counts, int nb,
                                                                double lowp, double highp, float new_low, float new_high, is_rs* out) {
  extern __shared__ double is_quot[];      // nb quotients (what 0)
  __shared__ int bins[2];
  const double mn = range->min, mx = range->max;
  if (what == IS_STRETCH_PERCENTILE) {
    const double sum = (double)counts[nb];
    for (int i = threadIdx.x; i < nb; i += IS_THREADS) is_quot[i] = (double)counts[i] / sum;
    __syncthreads();
    if (threadIdx.x == 0 || threadIdx.x == 64) {
      const double p = threadIdx.x == 0 ? lowp : highp;
      double running = 0;
      int found = -1;
      for (int i = 0; i < nb; ++i) {
        running += is_quot[i];
        if (running >= p) { found = i; break; }
      }
      bins[threadIdx.x >> 6] = found;
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  is_rs P;
  memset(&P, 0, sizeof(P));
  double lo = mn, hi = mx;
  if (what == IS_STRETCH_PERCENTILE) {
    const double mxa = mx == mn ? mn + 1.0 : mx;            // ImageThresh.h:61-62
    const double bin_width = (mxa - mn) / (double)nb;      // Statistics.cc:48-49
    if (bins[0] < 0 || bins[1] < 0 || range->count == range->nan_count) { P.status = 1; bins[0] = bins[1] = 0; }
    lo = (double)(bins[0] + 1) * bin_width + mn;           // ImageThresh.h:264-265
    hi = (double)(bins[1] + 1) * bin_width + mn;
  } else if (what == IS_STRETCH_MIN_MAX) {
    if (range->count == range->nan_count) P.status = 1;
    if (hi == lo) hi = lo + 1.0;                           // ImageThresh.h:282-283
  } else if (range->count == 0) {
    P.status = 1;
  }
  if (what == IS_STRETCH_AUTO) {
    is_rs_normalize(P, (float)lo, (float)hi, new_low, new_high);
    P.report[2] = (double)new_low; P.report[3] = (double)new_high;
  } else {
    P.ops = IS_RS_CLAMP;
    P.lo = (float)lo; P.hi = (float)hi;
    is_rs_normalize(P, (float)lo, (float)hi, 0.0f, 255.0f);
    P.report[2] = lo; P.report[3] = hi;
  }
  P.report[0] = mn; P.report[1] = mx;
  if (P.status) {            // the reference throws: every output pixel is new_low
    P.ops = IS_RS_NORMALIZE;
    P.ratio = 0.0;
  }
  *out = P;
}

// ---- host side -----------------------------------------------------------------------------------------------------

int is_fail_arg(vwgpu_ctx* ctx, const char* name, const char* what) { return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: %s", name, what); }

int is_check_image(vwgpu_ctx* ctx, const char* name, const void* in, int w, int h, ptrdiff_t& istride, const void* mask, ptrdiff_t& mstride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!in || w <= 0 || h <= 0) return is_fail_arg(ctx, name, "empty image or null pointer");
  if (istride == 0) istride = w;
  if (mstride == 0) mstride = w;
  if (istride < w || (mask && mstride < w)) return is_fail_arg(ctx, name, "row stride smaller than row width");
  return VWGPU_OK;
}

int is_check_sampling(vwgpu_ctx* ctx, const char* name, int sc, int sr) {
  if (sc == 0 && sr == 0) return VWGPU_OK;
  if (sc < 2 || sr < 2) return is_fail_arg(ctx, name, "sampling counts must both be 0 or both be at least 2");
  return VWGPU_OK;
}

char* is_base(vwgpu_ctx* ctx) { return static_cast<char*>(ctx->istats.base); }

// Reserves the arena and fills the view; with sampling, builds the two index tables (ImageThresh.h:156-166) and queues their upload.
int is_make_view(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride, int sc, int sr,
                 is_view* V) {
  const size_t tab = sc ? ((size_t)sc + (size_t)sr) * sizeof(int) : 0;
  int rc = vwgpu_arena_reserve(ctx, &ctx->istats, IS_OFF_TABLES + vwgpu_align_up(tab, 256));
  if (rc) return rc;
  *V = is_view{d_in, (long long)istride, d_mask, (long long)mstride, w, h, nullptr, nullptr, 0, 0};
  if (!sc) return VWGPU_OK;
  int* d_tab = reinterpret_cast<int*>(is_base(ctx) + IS_OFF_TABLES);
  int* ring = static_cast<int*>(vwgpu_host_ring(ctx, tab));
  std::vector<int> own;
  int* t = ring;
  if (!t) { own.resize((size_t)sc + sr); t = own.data(); }
  const double col_ratio = double(w - 1.0) / double(sc - 1.0), row_ratio = double(h - 1.0) / double(sr - 1.0);
  for (int i = 0; i < sc; ++i) t[i] = std::min(w - 1, std::max(0, (int)round(i * col_ratio)));
  for (int i = 0; i < sr; ++i) t[sc + i] = std::min(h - 1, std::max(0, (int)round(i * row_ratio)));
  VWGPU_HIP(ctx, hipMemcpyAsync(d_tab, t, tab, hipMemcpyHostToDevice, ctx->stream));
  if (!ring) VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));     // the copy reads memory that ends with this function
  V->xs = d_tab; V->ys = d_tab + sc; V->sc = sc; V->sr = sr;
  return VWGPU_OK;
}

int is_blocks(const is_view& V) {
  const unsigned long long items = V.xs ? (unsigned long long)V.sc * V.sr : (unsigned long long)(((unsigned)V.w + 6u) >> 2) * (unsigned)V.h;
  const unsigned long long want = (items + IS_THREADS - 1) / IS_THREADS;
  return (int)std::max(1ull, std::min(want, (unsigned long long)IS_MAX_BLOCKS));
}

int is_range_run(vwgpu_ctx* ctx, const is_view& V, int mode, vwgpu_image_range* d_result, vwgpu_image_range* host_result) {
  is_range_acc* slab = reinterpret_cast<is_range_acc*>(is_base(ctx) + IS_OFF_SLAB);
  static_assert(IS_OFF_SLAB + IS_MAX_BLOCKS * sizeof(is_range_acc) <= IS_OFF_TABLES, "the slab overlaps the tables");
  vwgpu_image_range* d_out = d_result ? d_result : reinterpret_cast<vwgpu_image_range*>(is_base(ctx) + IS_OFF_RANGE);
  const int blocks = is_blocks(V);
  {
    vwgpu_prof_scope ps(ctx, "image_min_max");
    hipLaunchKernelGGL(is_range_partial_kernel, dim3(blocks), dim3(IS_THREADS), 0, ctx->stream, V, slab);
    hipLaunchKernelGGL(is_range_fold_kernel, dim3(1), dim3(IS_THREADS), 0, ctx->stream, slab, blocks, mode, d_out);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (host_result) {
    VWGPU_HIP(ctx, hipMemcpyAsync(host_result, d_out, sizeof(*host_result), hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (mode == VWGPU_MIN_MAX_ACCUM && host_result->count == 0) return is_fail_arg(ctx, "image_min_max", "MinMaxAccumulator: no valid samples");
  }
  return VWGPU_OK;
}

int is_moments_run(vwgpu_ctx* ctx, const is_view& V, double* d_result, double* host_result) {
  is_mom_acc* slab = reinterpret_cast<is_mom_acc*>(is_base(ctx) + IS_OFF_SLAB);
  double* d_out = d_result ? d_result : reinterpret_cast<double*>(is_base(ctx) + IS_OFF_MOMENTS);
  // the grid follows from the image's size alone (the unshifted items): the order of the additions must not depend on anything else
  const unsigned long long items = V.xs ? (unsigned long long)V.sc * V.sr : (unsigned long long)(((unsigned)V.w + 3u) >> 2) * (unsigned)V.h;
  const int blocks = (int)std::max(1ull, std::min((items + IS_THREADS - 1) / IS_THREADS, (unsigned long long)IS_MAX_BLOCKS));
  {
    vwgpu_prof_scope ps(ctx, "image_moments");
    hipLaunchKernelGGL(is_moments_partial_kernel, dim3(blocks), dim3(IS_THREADS), 0, ctx->stream, V, slab);
    hipLaunchKernelGGL(is_moments_fold_kernel, dim3(1), dim3(IS_THREADS), 0, ctx->stream, slab, blocks, d_out);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (host_result) {
    VWGPU_HIP(ctx, hipMemcpyAsync(host_result, d_out, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return VWGPU_OK;
}

int is_hist_copies(int nb) { return nb <= 2048 ? IS_WAVES : 2; }      // at most 32 KB of LDS: five workgroups per CU

// values between mn and mx (or d_range's) into d_counts
int is_hist_run(vwgpu_ctx* ctx, const is_view& V, int nb, double mn, double mx, const vwgpu_image_range* d_range, int accumulate,
                unsigned long long* d_counts) {
  if (!accumulate) VWGPU_HIP(ctx, hipMemsetAsync(d_counts, 0, ((size_t)nb + 2) * 8, ctx->stream));
  const int copies = is_hist_copies(nb);
  vwgpu_prof_scope ps(ctx, "image_histogram");
  hipLaunchKernelGGL(is_hist_kernel<false>, dim3(is_blocks(V)), dim3(IS_THREADS), (size_t)copies * nb * 4, ctx->stream, V, nb, copies, mn, mx,
                     d_range, (const is_sel*)nullptr, 0, d_counts);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int is_order_run(vwgpu_ctx* ctx, const is_view& V, int kind, double arg, double* d_result, double* host_result) {
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(is_base(ctx) + IS_OFF_COUNTS);
  is_order_block* blk = reinterpret_cast<is_order_block*>(is_base(ctx) + IS_OFF_ORDER);
  static_assert(IS_OFF_ORDER + sizeof(is_order_block) <= IS_OFF_COUNTS, "the select state overlaps the bins");
  static const int SHIFT[3] = {20, 8, 0}, BINS[3] = {4096, 4096, 256};
  const int ranks = kind == VWGPU_ORDER_MEDIAN ? 2 : 1, blocks = is_blocks(V);
  vwgpu_prof_scope ps(ctx, "image_order_statistic");
  for (int rank = 0; rank < ranks; ++rank)
    for (int pass = 0; pass < 3; ++pass) {
      const int nb = BINS[pass], copies = is_hist_copies(nb);
      if (pass > 0 || rank == 0) {      // the first digit's counts serve both ranks
        VWGPU_HIP(ctx, hipMemsetAsync(counts, 0, ((size_t)nb + 2) * 8, ctx->stream));
        if (pass == 0 && rank == 0) VWGPU_HIP(ctx, hipMemsetAsync(blk, 0, sizeof(*blk), ctx->stream));
        hipLaunchKernelGGL(is_hist_kernel<true>, dim3(blocks), dim3(IS_THREADS), (size_t)copies * nb * 4, ctx->stream, V, nb, copies, 0.0, 0.0,
                           (const vwgpu_image_range*)nullptr, (const is_sel*)&blk->sel[rank], SHIFT[pass], counts);
      }
      if (pass == 0 && rank == 0 && ranks == 2)      // both ranks take their first digit now, before the bins are reused
        hipLaunchKernelGGL(is_select_kernel, dim3(1), dim3(IS_THREADS), 0, ctx->stream, counts, nb, SHIFT[0], 1, 0, kind, arg, 1, blk,
                           (double*)nullptr);
      if (pass == 0 && rank == 1) continue;
      hipLaunchKernelGGL(is_select_kernel, dim3(1), dim3(IS_THREADS), 0, ctx->stream, counts, nb, SHIFT[pass], pass == 0 ? 1 : 0,
                         pass == 2 ? 1 : 0, kind, arg, rank, blk, rank == ranks - 1 ? d_result : (double*)nullptr);
    }
  VWGPU_HIP(ctx, hipGetLastError());
  if (host_result) {
    is_order_block hb;
    VWGPU_HIP(ctx, hipMemcpyAsync(&hb, blk, sizeof(hb), hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *host_result = hb.result;
    if (hb.sel[0].len == 0) return is_fail_arg(ctx, "image_order_statistic", "no valid samples");
    if (hb.sel[0].nan != 0) return is_fail_arg(ctx, "image_order_statistic", "a NaN among the valid pixels: their order is not defined");
  }
  return VWGPU_OK;
}

int is_rescale_launch(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const is_rs& P, const is_rs* d_params, int out_type,
                      void* d_out, ptrdiff_t ostride) {
  const unsigned long long items = (unsigned long long)(((unsigned)w + 6u) >> 2) * (unsigned)h;
  const int blocks = (int)std::max(1ull, std::min((items + IS_THREADS - 1) / IS_THREADS, (unsigned long long)IS_MAX_BLOCKS * 4));
  vwgpu_prof_scope ps(ctx, "image_rescale");
  const dim3 g(blocks), b(IS_THREADS);
  if (out_type == VWGPU_PIXEL_F32)
    hipLaunchKernelGGL(is_rescale_kernel<VWGPU_PIXEL_F32>, g, b, 0, ctx->stream, d_in, (long long)istride, w, h, P, d_params, d_out, (long long)ostride);
  else if (out_type == VWGPU_PIXEL_U8)
    hipLaunchKernelGGL(is_rescale_kernel<VWGPU_PIXEL_U8>, g, b, 0, ctx->stream, d_in, (long long)istride, w, h, P, d_params, d_out, (long long)ostride);
  else
    hipLaunchKernelGGL(is_rescale_kernel<VWGPU_PIXEL_U8_AS_F32>, g, b, 0, ctx->stream, d_in, (long long)istride, w, h, P, d_params, d_out,
                       (long long)ostride);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int is_check_out(vwgpu_ctx* ctx, const char* name, int out_type, const void* in, const void* out, int w, ptrdiff_t& ostride) {
  if (out_type != VWGPU_PIXEL_F32 && out_type != VWGPU_PIXEL_U8 && out_type != VWGPU_PIXEL_U8_AS_F32) return is_fail_arg(ctx, name, "unknown out_type");
  if (!out) return is_fail_arg(ctx, name, "null output");
  if (ostride == 0) ostride = w;
  if (ostride < w) return is_fail_arg(ctx, name, "row stride smaller than row width");
  if (out == in && out_type == VWGPU_PIXEL_U8) return is_fail_arg(ctx, name, "in == out needs a float output");
  return VWGPU_OK;
}

int is_rescale_params(vwgpu_ctx* ctx, int mode, const double* p, is_rs* P) {
  static const int COUNT[4] = {2, 4, 6, 3};
  if (mode < 0 || mode > 3) return is_fail_arg(ctx, "image_rescale", "unknown mode");
  if (!p) return is_fail_arg(ctx, "image_rescale", "null params");
  for (int i = 0; i < COUNT[mode]; ++i)
    if (std::isnan(p[i])) return is_fail_arg(ctx, "image_rescale", "a parameter is NaN");
  memset(P, 0, sizeof(*P));
  if (mode == VWGPU_RESCALE_CLAMP || mode == VWGPU_RESCALE_CLAMP_NORMALIZE) {
    P->ops = IS_RS_CLAMP;
    P->lo = (float)p[0]; P->hi = (float)p[1];
    p += 2;
  }
  if (mode == VWGPU_RESCALE_NORMALIZE || mode == VWGPU_RESCALE_CLAMP_NORMALIZE) is_rs_normalize(*P, (float)p[0], (float)p[1], (float)p[2], (float)p[3]);
  if (mode == VWGPU_RESCALE_THRESHOLD) {
    P->ops = IS_RS_THRESHOLD;
    P->thresh = (float)p[0]; P->tlow = (float)p[1]; P->thigh = (float)p[2];
  }
  return VWGPU_OK;
}

// statistics -> stretch -> convert, all on the stream
int is_stretch_run(vwgpu_ctx* ctx, const char* name, int what, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask,
                   ptrdiff_t mstride, double lowp, double highp, int nb, float new_low, float new_high, int out_type, void* d_out,
                   ptrdiff_t ostride, double* host_params, bool must_report) {
  is_view V;
  int rc = is_make_view(ctx, d_in, w, h, istride, d_mask, mstride, 0, 0, &V);
  if (rc) return rc;
  vwgpu_image_range* d_range = reinterpret_cast<vwgpu_image_range*>(is_base(ctx) + IS_OFF_RANGE);
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(is_base(ctx) + IS_OFF_COUNTS);
  is_rs* d_params = reinterpret_cast<is_rs*>(is_base(ctx) + IS_OFF_PARAMS);
  static_assert(IS_OFF_PARAMS + sizeof(is_rs) <= IS_OFF_ORDER, "the stretch overlaps the select state");
  if ((rc = is_range_run(ctx, V, what == IS_STRETCH_AUTO ? VWGPU_MIN_MAX_ACCUM : VWGPU_MIN_MAX_FIND, d_range, nullptr))) return rc;
  if (what == IS_STRETCH_PERCENTILE && (rc = is_hist_run(ctx, V, nb, 0.0, 0.0, d_range, 0, counts))) return rc;
  hipLaunchKernelGGL(is_stretch_kernel, dim3(1), dim3(IS_THREADS), what == IS_STRETCH_PERCENTILE ? (size_t)nb * 8 : 0, ctx->stream, what, d_range,
                     counts, nb, lowp, highp, new_low, new_high, d_params);
  VWGPU_HIP(ctx, hipGetLastError());
  is_rs none;
  memset(&none, 0, sizeof(none));
  if ((rc = is_rescale_launch(ctx, d_in, w, h, istride, none, d_params, out_type, d_out, ostride))) return rc;
  if (host_params || must_report) {
    is_rs hp;
    VWGPU_HIP(ctx, hipMemcpyAsync(&hp, d_params, sizeof(hp), hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (host_params) memcpy(host_params, hp.report, sizeof(hp.report));
    if (hp.status) return is_fail_arg(ctx, name, "no valid samples, or no bin reaches a percentile");
  }
  return VWGPU_OK;
}

int is_check_stretch(vwgpu_ctx* ctx, const char* name, int what, const void* in, int w, int h, ptrdiff_t& istride, const void* mask,
                     ptrdiff_t& mstride, double a, double b, int nb, int out_type, const void* out, ptrdiff_t& ostride) {
  int rc = is_check_image(ctx, name, in, w, h, istride, mask, mstride);
  if (rc) return rc;
  if ((rc = is_check_out(ctx, name, out_type, in, out, w, ostride))) return rc;
  if (what == IS_STRETCH_PERCENTILE) {
    if (!(a >= 0 && a <= 1.0) || !(b >= 0 && b <= 1.0)) return is_fail_arg(ctx, name, "illegal percentile request");
    if (nb < 1 || nb > VWGPU_HISTOGRAM_MAX_BINS) return is_fail_arg(ctx, name, "num_bins outside [1, VWGPU_HISTOGRAM_MAX_BINS]");
  }
  if (what == IS_STRETCH_AUTO && (std::isnan(a) || std::isnan(b))) return is_fail_arg(ctx, name, "low or high is NaN");
  return VWGPU_OK;
}

int is_check_min_max(vwgpu_ctx* ctx, const void* in, int w, int h, ptrdiff_t& istride, const void* mask, ptrdiff_t& mstride, int sc, int sr, int mode,
                     const void* r0, const void* r1) {
  int rc = is_check_image(ctx, "image_min_max", in, w, h, istride, mask, mstride);
  if (rc) return rc;
  if ((rc = is_check_sampling(ctx, "image_min_max", sc, sr))) return rc;
  if (mode != VWGPU_MIN_MAX_FIND && mode != VWGPU_MIN_MAX_ACCUM) return is_fail_arg(ctx, "image_min_max", "unknown mode");
  if (!r0 && !r1) return is_fail_arg(ctx, "image_min_max", "no result pointer");
  return VWGPU_OK;
}

int is_check_moments(vwgpu_ctx* ctx, const void* in, int w, int h, ptrdiff_t& istride, const void* mask, ptrdiff_t& mstride, int sc, int sr,
                     const void* r0, const void* r1) {
  int rc = is_check_image(ctx, "image_moments", in, w, h, istride, mask, mstride);
  if (rc) return rc;
  if ((rc = is_check_sampling(ctx, "image_moments", sc, sr))) return rc;
  if (!r0 && !r1) return is_fail_arg(ctx, "image_moments", "no result pointer");
  return VWGPU_OK;
}

int is_check_otsu(vwgpu_ctx* ctx, const void* in, int w, int h, ptrdiff_t& istride, const void* mask, ptrdiff_t& mstride, int sc, int sr,
                  int num_bins, int overload, const void* threshold) {
  int rc = is_check_image(ctx, "otsu_threshold", in, w, h, istride, mask, mstride);
  if (rc) return rc;
  if ((rc = is_check_sampling(ctx, "otsu_threshold", sc, sr))) return rc;
  if (!threshold) return is_fail_arg(ctx, "otsu_threshold", "null threshold");
  if (overload != 1 && overload != 2) return is_fail_arg(ctx, "otsu_threshold", "overload must be 1 or 2");
  if (overload == 1 && (num_bins != 256 || sc)) return is_fail_arg(ctx, "otsu_threshold", "overload 1 has 256 bins and no sampling");
  if (num_bins < 1 || num_bins > VWGPU_HISTOGRAM_MAX_BINS) return is_fail_arg(ctx, "otsu_threshold", "num_bins outside [1, VWGPU_HISTOGRAM_MAX_BINS]");
  return VWGPU_OK;
}

int is_check_order(vwgpu_ctx* ctx, const void* in, int w, int h, ptrdiff_t& istride, const void* mask, ptrdiff_t& mstride, int kind, double arg,
                   const void* r0, const void* r1) {
  const char* name = "image_order_statistic";
  int rc = is_check_image(ctx, name, in, w, h, istride, mask, mstride);
  if (rc) return rc;
  if (kind != VWGPU_ORDER_RANK && kind != VWGPU_ORDER_MEDIAN && kind != VWGPU_ORDER_PERCENTILE) return is_fail_arg(ctx, name, "unknown kind");
  if (kind != VWGPU_ORDER_MEDIAN && !(arg >= 0)) return is_fail_arg(ctx, name, "arg is negative or NaN");
  if (kind == VWGPU_ORDER_PERCENTILE && arg > 100.0) return is_fail_arg(ctx, name, "Percentile must be between 0 and 100.");
  if ((long long)w * h > INT_MAX) return is_fail_arg(ctx, name, "more than INT_MAX pixels");
  if (!r0 && !r1) return is_fail_arg(ctx, name, "no result pointer");
  return VWGPU_OK;
}

size_t is_out_elem(int out_type) { return out_type == VWGPU_PIXEL_U8 ? 1 : 4; }

int is_stretch_host(vwgpu_ctx* ctx, const char* name, int what, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask,
                    ptrdiff_t mstride, double a, double b, int nb, int out_type, void* out, ptrdiff_t ostride, double* host_params) {
  int rc = is_check_stretch(ctx, name, what, in, w, h, istride, mask, mstride, a, b, nb, out_type, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 4, istride, VWGPU_STAGE_IN), pm = st.add(mask, w, h, 1, mstride, VWGPU_STAGE_IN);
  const int po = st.add(out, w, h, is_out_elem(out_type), ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  const bool pct = what == IS_STRETCH_PERCENTILE;
  const int run = is_stretch_run(ctx, name, what, st.dev<float>(pi), w, h, w, st.dev<uint8_t>(pm), w, pct ? a : 0.0, pct ? b : 0.0, nb,
                                 pct ? 0.f : (float)a, pct ? 0.f : (float)b, out_type, st.dev<void>(po), w, host_params, true);
  if (run && run != VWGPU_ERR_ARGUMENT) return run;
  const std::string text = ctx->err;
  if ((rc = st.finish())) return rc;
  if (run) ctx->err = text;
  return run;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) --------------------------------------------------------------------

extern "C" {

int vwgpu_image_min_max_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                            int sample_cols, int sample_rows, int mode, vwgpu_image_range* d_result, vwgpu_image_range* host_result) {
  int rc = is_check_min_max(ctx, d_in, w, h, istride, d_mask, mstride, sample_cols, sample_rows, mode, d_result, host_result);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  is_view V;
  if ((rc = is_make_view(ctx, d_in, w, h, istride, d_mask, mstride, sample_cols, sample_rows, &V))) return rc;
  return is_range_run(ctx, V, mode, d_result, host_result);
}

int vwgpu_image_min_max(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                        int sample_cols, int sample_rows, int mode, vwgpu_image_range* result) {
  int rc = is_check_min_max(ctx, in, w, h, istride, mask, mstride, sample_cols, sample_rows, mode, nullptr, result);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 4, istride, VWGPU_STAGE_IN), pm = st.add(mask, w, h, 1, mstride, VWGPU_STAGE_IN);
  if ((rc = st.commit())) return rc;
  return vwgpu_image_min_max_dev(ctx, st.dev<float>(pi), w, h, w, st.dev<uint8_t>(pm), w, sample_cols, sample_rows, mode, nullptr, result);
}

int vwgpu_image_moments_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                            int sample_cols, int sample_rows, double* d_result, double* host_result) {
  int rc = is_check_moments(ctx, d_in, w, h, istride, d_mask, mstride, sample_cols, sample_rows, d_result, host_result);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  is_view V;
  if ((rc = is_make_view(ctx, d_in, w, h, istride, d_mask, mstride, sample_cols, sample_rows, &V))) return rc;
  return is_moments_run(ctx, V, d_result, host_result);
}

int vwgpu_image_moments(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                        int sample_cols, int sample_rows, double* result) {
  int rc = is_check_moments(ctx, in, w, h, istride, mask, mstride, sample_cols, sample_rows, nullptr, result);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 4, istride, VWGPU_STAGE_IN), pm = st.add(mask, w, h, 1, mstride, VWGPU_STAGE_IN);
  if ((rc = st.commit())) return rc;
  return vwgpu_image_moments_dev(ctx, st.dev<float>(pi), w, h, w, st.dev<uint8_t>(pm), w, sample_cols, sample_rows, nullptr, result);
}

int vwgpu_moments_mean(const double* m, double* mean) {
  if (!m || !mean || !m[0]) return VWGPU_ERR_ARGUMENT;      // MeanAccumulator: no valid samples
  *mean = m[1] / m[0];
  return VWGPU_OK;
}

int vwgpu_moments_stddev(const double* m, double* stddev) {
  if (!m || !stddev || !m[0]) return VWGPU_ERR_ARGUMENT;    // StdDevAccumulator(): no valid samples.
  *stddev = sqrt(m[2] / m[0] - (m[1] / m[0]) * (m[1] / m[0]));
  return VWGPU_OK;
}

static int is_check_hist(vwgpu_ctx* ctx, const char* name, int sc, int sr, int nb, double mn, double mx, const void* counts) {
  int rc = is_check_sampling(ctx, name, sc, sr);
  if (rc) return rc;
  if (nb < 1 || nb > VWGPU_HISTOGRAM_MAX_BINS) return is_fail_arg(ctx, name, "num_bins outside [1, VWGPU_HISTOGRAM_MAX_BINS]");
  if (std::isnan(mn) || std::isnan(mx)) return is_fail_arg(ctx, name, "min or max is NaN");
  if (!counts) return is_fail_arg(ctx, name, "null counts");
  return VWGPU_OK;
}

int vwgpu_image_histogram_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                              int sample_cols, int sample_rows, int num_bins, double min, double max, int accumulate,
                              uint64_t* d_counts, double* bin_width) {
  int rc = is_check_image(ctx, "image_histogram", d_in, w, h, istride, d_mask, mstride);
  if (rc) return rc;
  if ((rc = is_check_hist(ctx, "image_histogram", sample_cols, sample_rows, num_bins, min, max, d_counts))) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  is_view V;
  if ((rc = is_make_view(ctx, d_in, w, h, istride, d_mask, mstride, sample_cols, sample_rows, &V))) return rc;
  if (bin_width) *bin_width = ((max == min ? min + 1.0 : max) - min) / (double)num_bins;      // Statistics.cc:48-49
  return is_hist_run(ctx, V, num_bins, min, max, nullptr, accumulate, reinterpret_cast<unsigned long long*>(d_counts));
}

int vwgpu_image_histogram(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                          int sample_cols, int sample_rows, int num_bins, double min, double max, int accumulate,
                          uint64_t* counts, double* bin_width) {
  int rc = is_check_image(ctx, "image_histogram", in, w, h, istride, mask, mstride);
  if (rc) return rc;
  if ((rc = is_check_hist(ctx, "image_histogram", sample_cols, sample_rows, num_bins, min, max, counts))) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 4, istride, VWGPU_STAGE_IN), pm = st.add(mask, w, h, 1, mstride, VWGPU_STAGE_IN);
  const int pc = st.add(counts, num_bins + 2, 1, 8, num_bins + 2, accumulate ? VWGPU_STAGE_INOUT : VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_image_histogram_dev(ctx, st.dev<float>(pi), w, h, w, st.dev<uint8_t>(pm), w, sample_cols, sample_rows, num_bins, min, max,
                                 accumulate, st.dev<uint64_t>(pc), bin_width);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_histogram_percentile(const uint64_t* counts, int num_bins, uint64_t total, double percentile, int* bin) {
  if (!counts || !bin || num_bins < 1 || !(percentile >= 0 && percentile <= 1.0)) return VWGPU_ERR_ARGUMENT;
  const double sum = static_cast<double>(total);
  double running_percentile = 0;
  for (int i = 0; i < num_bins; ++i) {
    const double this_percent = (double)counts[i] / sum;
    running_percentile += this_percent;
    if (running_percentile >= percentile) { *bin = i; return VWGPU_OK; }
  }
  return VWGPU_ERR_LOGIC;      // get_histogram_percentile: Illegal histogram encountered!
}

int vwgpu_otsu_from_histogram(const uint64_t* counts, int num_bins, uint64_t total, double min_val, double max_val, int overload,
                              double* threshold) {
  if (!counts || !threshold || num_bins < 1 || (overload != 1 && overload != 2)) return VWGPU_ERR_ARGUMENT;
  *threshold = 0.0;
  if (total == 0) return VWGPU_OK;
  if (overload == 1) {      // ImageThresh.h:97-144
    const double sum = static_cast<double>(total);
    double totalAccum = 0.0;
    for (int i = 0; i < num_bins; i++) totalAccum += i * ((double)counts[i] / sum);
    std::vector<double> V(num_bins, 0.0);
    double leftProb = 0.0, leftAccum = 0.0, rightProb = 0.0, rightAccum = 0.0;
    for (int i = 0; i < num_bins; i++) {
      leftProb += (double)counts[i] / sum;
      leftAccum += i * ((double)counts[i] / sum);
      rightProb = 1.0 - leftProb;
      rightAccum = totalAccum - leftAccum;
      if (leftProb == 0 || rightProb == 0.0) continue;
      const double leftMean = leftAccum / leftProb, rightMean = rightAccum / rightProb;
      V[i] = leftProb * rightProb * (leftMean - rightMean) * (leftMean - rightMean);
    }
    const double maxV = *std::max_element(V.begin(), V.end());
    double indexSum = 0, numIndices = 0;
    for (size_t i = 0; i < V.size(); i++)
      if (V[i] == maxV) { indexSum += i; numIndices++; }
    const double meanIndex = indexSum / numIndices;
    const double normalized_index = meanIndex / (num_bins - 1.0);
    *threshold = min_val + normalized_index * (max_val - min_val);
    return VWGPU_OK;
  }
  // ImageThresh.h:207-238
  double mu = 0;
  const double scale = 1.0 / double(total);
  for (int i = 0; i < num_bins; i++) mu += i * (double)counts[i];
  mu *= scale;
  double mu1 = 0, q1 = 0, max_sigma = 0, max_pos = 0;
  for (int i = 0; i < num_bins; i++) {
    const double p_i = (double)counts[i] * scale;
    mu1 *= q1;
    q1 += p_i;
    const double q2 = 1.0 - q1;
    if (std::min(q1, q2) < FLT_EPSILON || std::max(q1, q2) > 1.0 - FLT_EPSILON) continue;
    mu1 = (mu1 + i * p_i) / q1;
    const double mu2 = (mu - q1 * mu1) / q2;
    const double sigma = q1 * q2 * (mu1 - mu2) * (mu1 - mu2);
    if (sigma > max_sigma) { max_sigma = sigma; max_pos = i; }
  }
  *threshold = (max_val - min_val) * (max_pos / (num_bins - 1.0)) + min_val;
  return VWGPU_OK;
}

int vwgpu_otsu_threshold_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                             int sample_cols, int sample_rows, int num_bins, int overload, double* threshold) {
  int rc = is_check_otsu(ctx, d_in, w, h, istride, d_mask, mstride, sample_cols, sample_rows, num_bins, overload, threshold);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  is_view V;
  if ((rc = is_make_view(ctx, d_in, w, h, istride, d_mask, mstride, sample_cols, sample_rows, &V))) return rc;
  vwgpu_image_range r;
  if ((rc = is_range_run(ctx, V, VWGPU_MIN_MAX_FIND, nullptr, &r))) return rc;
  if (r.max == r.min) r.max++;      // ImageThresh.h:91-92, :176-177
  unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(is_base(ctx) + IS_OFF_COUNTS);
  if ((rc = is_hist_run(ctx, V, num_bins, r.min, r.max, nullptr, 0, d_counts))) return rc;
  std::vector<uint64_t> counts((size_t)num_bins + 2);
  VWGPU_HIP(ctx, hipMemcpyAsync(counts.data(), d_counts, counts.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return vwgpu_otsu_from_histogram(counts.data(), num_bins, counts[num_bins], r.min, r.max, overload, threshold);
}

int vwgpu_otsu_threshold(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                         int sample_cols, int sample_rows, int num_bins, int overload, double* threshold) {
  int rc = is_check_otsu(ctx, in, w, h, istride, mask, mstride, sample_cols, sample_rows, num_bins, overload, threshold);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 4, istride, VWGPU_STAGE_IN), pm = st.add(mask, w, h, 1, mstride, VWGPU_STAGE_IN);
  if ((rc = st.commit())) return rc;
  return vwgpu_otsu_threshold_dev(ctx, st.dev<float>(pi), w, h, w, st.dev<uint8_t>(pm), w, sample_cols, sample_rows, num_bins, overload, threshold);
}

int vwgpu_image_order_statistic_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask,
                                    ptrdiff_t mstride, int kind, double arg, double* d_result, double* host_result) {
  int rc = is_check_order(ctx, d_in, w, h, istride, d_mask, mstride, kind, arg, d_result, host_result);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  is_view V;
  if ((rc = is_make_view(ctx, d_in, w, h, istride, d_mask, mstride, 0, 0, &V))) return rc;
  return is_order_run(ctx, V, kind, arg, d_result, host_result);
}

int vwgpu_image_order_statistic(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                                int kind, double arg, double* result) {
  int rc = is_check_order(ctx, in, w, h, istride, mask, mstride, kind, arg, nullptr, result);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 4, istride, VWGPU_STAGE_IN), pm = st.add(mask, w, h, 1, mstride, VWGPU_STAGE_IN);
  if ((rc = st.commit())) return rc;
  return vwgpu_image_order_statistic_dev(ctx, st.dev<float>(pi), w, h, w, st.dev<uint8_t>(pm), w, kind, arg, nullptr, result);
}

int vwgpu_image_rescale_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, int mode, const double* params,
                            int out_type, void* d_out, ptrdiff_t ostride) {
  ptrdiff_t none = 0;
  int rc = is_check_image(ctx, "image_rescale", d_in, w, h, istride, nullptr, none);
  if (rc) return rc;
  if ((rc = is_check_out(ctx, "image_rescale", out_type, d_in, d_out, w, ostride))) return rc;
  is_rs P;
  if ((rc = is_rescale_params(ctx, mode, params, &P))) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return is_rescale_launch(ctx, d_in, w, h, istride, P, nullptr, out_type, d_out, ostride);
}

int vwgpu_image_rescale(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, int mode, const double* params,
                        int out_type, void* out, ptrdiff_t ostride) {
  ptrdiff_t none = 0;
  int rc = is_check_image(ctx, "image_rescale", in, w, h, istride, nullptr, none);
  if (rc) return rc;
  if ((rc = is_check_out(ctx, "image_rescale", out_type, in, out, w, ostride))) return rc;
  is_rs P;
  if ((rc = is_rescale_params(ctx, mode, params, &P))) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(in, w, h, 4, istride, VWGPU_STAGE_IN), po = st.add(out, w, h, is_out_elem(out_type), ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  if ((rc = is_rescale_launch(ctx, st.dev<float>(pi), w, h, w, P, nullptr, out_type, st.dev<void>(po), w))) return rc;
  return st.finish();
}

int vwgpu_percentile_scale_convert_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask,
                                       ptrdiff_t mstride, double low_percentile, double high_percentile, int num_bins, int out_type,
                                       void* d_out, ptrdiff_t ostride, double* host_params) {
  int rc = is_check_stretch(ctx, "percentile_scale_convert", IS_STRETCH_PERCENTILE, d_in, w, h, istride, d_mask, mstride, low_percentile,
                            high_percentile, num_bins, out_type, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return is_stretch_run(ctx, "percentile_scale_convert", IS_STRETCH_PERCENTILE, d_in, w, h, istride, d_mask, mstride, low_percentile,
                        high_percentile, num_bins, 0.f, 0.f, out_type, d_out, ostride, host_params, false);
}

int vwgpu_percentile_scale_convert(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask,
                                   ptrdiff_t mstride, double low_percentile, double high_percentile, int num_bins, int out_type,
                                   void* out, ptrdiff_t ostride, double* host_params) {
  return is_stretch_host(ctx, "percentile_scale_convert", IS_STRETCH_PERCENTILE, in, w, h, istride, mask, mstride, low_percentile,
                         high_percentile, num_bins, out_type, out, ostride, host_params);
}

int vwgpu_u8_convert_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                         int out_type, void* d_out, ptrdiff_t ostride, double* host_params) {
  int rc = is_check_stretch(ctx, "u8_convert", IS_STRETCH_MIN_MAX, d_in, w, h, istride, d_mask, mstride, 0, 0, 1, out_type, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return is_stretch_run(ctx, "u8_convert", IS_STRETCH_MIN_MAX, d_in, w, h, istride, d_mask, mstride, 0, 0, 1, 0.f, 0.f, out_type, d_out, ostride,
                        host_params, false);
}

int vwgpu_u8_convert(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                     int out_type, void* out, ptrdiff_t ostride, double* host_params) {
  return is_stretch_host(ctx, "u8_convert", IS_STRETCH_MIN_MAX, in, w, h, istride, mask, mstride, 0, 0, 1, out_type, out, ostride, host_params);
}

int vwgpu_auto_normalize_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                             double low, double high, float* d_out, ptrdiff_t ostride, double* host_params) {
  int rc = is_check_stretch(ctx, "auto_normalize", IS_STRETCH_AUTO, d_in, w, h, istride, d_mask, mstride, low, high, 1, VWGPU_PIXEL_F32, d_out,
                            ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return is_stretch_run(ctx, "auto_normalize", IS_STRETCH_AUTO, d_in, w, h, istride, d_mask, mstride, 0, 0, 1, (float)low, (float)high,
                        VWGPU_PIXEL_F32, d_out, ostride, host_params, false);
}

int vwgpu_auto_normalize(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                         double low, double high, float* out, ptrdiff_t ostride, double* host_params) {
  return is_stretch_host(ctx, "auto_normalize", IS_STRETCH_AUTO, in, w, h, istride, mask, mstride, low, high, 1, VWGPU_PIXEL_F32, out, ostride,
                         host_params);
}

}  // extern "C"
