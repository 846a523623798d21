// ip_detect.hip — the detectors ipfind runs without OpenCV: IntegralAutoGainDetector ("iagd") and
// IntegralInterestPointDetector ("obalog") of src/vw/InterestPoint/IntegralDetector.cc over the OBALoG interest operator of
// IntegralInterestOperator.h, with the SURF-style orientation of the latter, and IntegralImage itself.
//
// One call takes one image and n tile rectangles; every tile is an independent crop with its own integral image, as
// detect_interest_points has it (DetectorBase.h:225-236).  The stages, each one launch over all tiles of a batch:
//   integral   ip_integral.h: the reference's summation order, one wave per tile
//   planes     |sum of six weighted box sums| per pixel and scale, stored; the plane's min and max by atomics on the float's
//              bits (the values are >= 0, so their order is that of the bits)
//   extrema    a pixel of a middle plane strictly above its 26 neighbours; the threshold (a fixed one for OBALoG, 0.1 % of
//              the plane's range for IAGD) and the Harris test on the interest plane; survivors are appended to the tile's
//              candidate list with one atomic per wave
//   cull       the counts go to the host, which applies the cull rule; every candidate then counts the candidates that
//              precede it in the total order (interest descending, scale, y, x) or (scale, y, x) and that count is its place in
//              the output, so the output is in the stable sort's order whatever order the atomics produced
//   orientation (OBALoG) one wave per kept point
// An extremum is above its eight neighbours, so a 2 x 2 block holds at most one and the candidate list of a tile has a
// hard bound; it cannot overflow.  Tiles are taken in batches whose scratch stays below VWGPU_OPT_IP_SCRATCH_MB (1 GiB by
// default) and whose tile x scale count fits a grid dimension.
#include <cmath>
#include <cstring>
#include <numeric>

#include "image_sample.h"
#include "ip_atan2.h"
#include "ip_haar.h"
#include "ip_integral.h"
#include "ip_obalog.h"
#include "vwgpu_internal.h"

namespace {

constexpr int IPD_GRID_LIMIT = 65535;      // grid y and z
constexpr int IPD_ORI_SAMPLES = 113;      // the (i, j) of -6 .. 6 with i^2 + j^2 <= 36
constexpr int IPD_ORI_SLICES = 13;        // a = 0, 0.5, .. 6 < 2 pi

struct ipd_tile { int x, y, w, h, written, by_interest, pad0, pad1; };
struct ipd_cand { unsigned long long key; float interest; int pad; };      // key = scale << 40 | y << 20 | x, tile coordinates

struct ipd_args {
  const ipd_tile* tiles;
  int ntiles, scales, detector, capacity;
  double threshold;
  const float* img; long long stride;
  float* integ; long long integ_slot;
  float* planes; long long plane_slot;
  unsigned* minmax;          // [tile][scale][2]
  unsigned* counters;        // [tile][2] = extrema, passed
  ipd_cand* cand; long long cand_slot;
  vwgpu_ip_points out;       // segments of `capacity` per tile, tile0 tiles in
  int tile0;
};
struct ipd_harris_weights { float w[81]; };
struct ipd_ori_table { float w[IPD_ORI_SAMPLES]; signed char i[IPD_ORI_SAMPLES], j[IPD_ORI_SAMPLES]; };

// ---- the total orders of the cull (InterestPoint::operator<, InterestPoint.h:108-110, under a stable sort) --------------------
__host__ __device__ inline bool ipd_before(bool by_interest, float ia, unsigned long long ka, float ib, unsigned long long kb) {
  if (by_interest) {
    if (ia > ib) return true;
    if (ib > ia) return false;
  }
  return ka < kb;
}
// IntegralDetector.cc:227-237 (OBALoG sorts whenever a limit is set) and :354-367 (IAGD only when it cuts)
inline void ipd_cull_rule(int detector, int limit, int count, int* by_interest, int* written) {
  const bool cuts = limit > 0 && limit < count;
  *by_interest = detector == VWGPU_IP_DETECTOR_OBALOG ? limit > 0 : cuts;
  *written = cuts ? limit : count;
}

// ---- integral ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) ipd_integral_kernel(ipd_args a) {
  const ipd_tile T = a.tiles[blockIdx.x];
  ipi_wave_integral<true>(a.img + (long long)T.y * a.stride + T.x, a.stride, T.w, T.h, a.integ + blockIdx.x * a.integ_slot, T.w + 1);
}

struct ipd_single { const float* src; long long sstride; int w, h; float* out; long long ostride; };
__global__ void __launch_bounds__(64) ipd_integral_single_kernel(ipd_single s) {
  ipi_wave_integral<true>(s.src, s.sstride, s.w, s.h, s.out, s.ostride);
}

// ---- planes: BoxFilterView under abs (BoxFilter.h:50-114, IntegralInterestOperator.h:96-114) ---------------------------------
__device__ inline float ipd_plane_value(const float* I, long long is, int w, int h, int scale, int x, int y) {
  const int pb = ipo_pixel_buffer(scale);
  if (x < pb || x >= w - pb || y < pb || y >= h - pb) return 0.0f;
  const float* p = I + (long long)y * is + x;
  float result = 0.0f;
#pragma unroll
  for (int b = 0; b < IPO_BOXES; ++b) {
    const ipo_box box = ipo_box_of(scale, b);
    const int sx = -(box.w >> 1), sy = -(box.h >> 1);
    float box_sum = 0.0f;
    box_sum += p[(long long)sy * is + sx];
    box_sum -= p[(long long)sy * is + sx + box.w];
    box_sum -= p[(long long)(sy + box.h) * is + sx];
    box_sum += p[(long long)(sy + box.h) * is + sx + box.w];
    result += (float)box.weight * box_sum;
  }
  return fabsf(result);
}

__global__ void __launch_bounds__(256) ipd_planes_kernel(ipd_args a) {
  const int tile = blockIdx.z / a.scales, scale = blockIdx.z % a.scales;
  const ipd_tile T = a.tiles[tile];
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (blockIdx.x * 64 >= T.w || blockIdx.y * 4 >= T.h) return;
  const bool live = x < T.w && y < T.h;
  float v = 0.0f;
  if (live) {
    v = ipd_plane_value(a.integ + tile * a.integ_slot, T.w + 1, T.w, T.h, scale, x, y);
    a.planes[((long long)tile * a.scales + scale) * a.plane_slot + (long long)y * T.w + x] = v;
  }
  // min_max_pixel_values of the plane (IAGD); a NaN takes part in neither, as a comparison with it is false
  unsigned lo = live && v == v ? __float_as_uint(v) : 0x7f800000u, hi = live && v == v ? __float_as_uint(v) : 0u;
  for (int d = 32; d > 0; d >>= 1) {
    lo = min(lo, (unsigned)__shfl_xor((int)lo, d));
    hi = max(hi, (unsigned)__shfl_xor((int)hi, d));
  }
  if (threadIdx.x == 0) {
    unsigned* mm = a.minmax + ((long long)tile * a.scales + scale) * 2;
    atomicMin(mm, lo);
    atomicMax(mm + 1, hi);
  }
}

// ---- extrema, threshold, Harris (IntegralDetector.cc:106-134, IntegralInterestOperator.h:124-153) -----------------------------
__device__ inline float ipd_at(const float* P, int w, int h, int x, int y) {
  return x >= 0 && y >= 0 && x < w && y < h ? P[(long long)y * w + x] : 0.0f;      // the reads stay inside; the guard costs nothing
}

__device__ inline bool ipd_harris(const float* P, int w, int h, int ix, int iy, float sigma, const ipd_harris_weights& g) {
  const int step = (int)sigma, offset = 4 * step;
  float sum_lx2 = 0.0f, sum_ly2 = 0.0f, sum_lxly = 0.0f;
  for (int y = iy - offset, ky = 0; y <= iy + offset; y += step, ++ky)
    for (int x = ix - offset, kx = 0; x <= ix + offset; x += step, ++kx) {
      const float lx = ipd_at(P, w, h, x - 1, y) - ipd_at(P, w, h, x + 1, y);
      const float ly = ipd_at(P, w, h, x, y - 1) - ipd_at(P, w, h, x, y + 1);
      const float weight = g.w[ky * 9 + kx];
      sum_lx2 += lx * lx * weight;
      sum_ly2 += ly * ly * weight;
      sum_lxly += lx * ly * weight;
    }
  const float trace = sum_lx2 + sum_ly2;
  const float det = sum_lx2 * sum_ly2 - sum_lxly * sum_lxly;
  return __fdiv_rn(trace * trace, det) < 12.0f;
}

__global__ void __launch_bounds__(256) ipd_extrema_kernel(ipd_args a, ipd_harris_weights g) {
  const int mids = a.scales - 2;
  const int tile = blockIdx.z / mids, m = blockIdx.z % mids + 1;
  const ipd_tile T = a.tiles[tile];
  if ((int)(blockIdx.x * 64) >= T.w - 2 || (int)(blockIdx.y * 4) >= T.h - 2) return;
  const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
  const bool live = c < T.w - 2 && r < T.h - 2;
  const int px = c + 1, py = r + 1;
  const float* mid = a.planes + ((long long)tile * a.scales + m) * a.plane_slot;
  const float *low = mid - a.plane_slot, *high = mid + a.plane_slot;
  bool ext = false;
  float v = 0.0f;
  if (live) {
    const long long at = (long long)py * T.w + px;
    v = mid[at];
    ext = !(v <= low[at]) && !(v <= high[at]);
    for (int dy = -1; dy <= 1 && ext; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (dx == 0 && dy == 0) continue;
        const long long n = at + (long long)dy * T.w + dx;
        if (v <= low[n] || v <= mid[n] || v <= high[n]) { ext = false; break; }
      }
  }
  bool pass = false;
  // IAGD puts the point on the extremum, OBALoG one pixel right and down of it (IntegralDetector.cc:203 against :324), and
  // the Harris test runs where the point was put
  const int shift = a.detector == VWGPU_IP_DETECTOR_OBALOG ? 1 : 0;
  const int ix = px + shift, iy = py + shift;
  if (ext) {
    if (a.detector == VWGPU_IP_DETECTOR_OBALOG) {
      pass = !((double)v < a.threshold);
    } else {
      const unsigned* mm = a.minmax + ((long long)tile * a.scales + m) * 2;
      const float imin = __uint_as_float(mm[0]), imax = __uint_as_float(mm[1]);
      const float lvl = (float)((double)imin + 0.001 * (double)(imax - imin));
      pass = !(v < lvl);
    }
    if (pass) pass = ipd_harris(mid, T.w, T.h, ix, iy, (float)ipo_sigma(m), g);
  }
  const unsigned long long em = __ballot(ext), pm = __ballot(pass);
  const int lane = threadIdx.x & 63;
  unsigned base = 0;
  if (lane == 0) {
    if (em) atomicAdd(&a.counters[tile * 2], (unsigned)__popcll(em));
    if (pm) base = atomicAdd(&a.counters[tile * 2 + 1], (unsigned)__popcll(pm));
  }
  base = (unsigned)__shfl((int)base, 0);
  if (pass) {
    const long long slot = (long long)base + __popcll(pm & ((1ull << lane) - 1ull));
    if (slot < a.cand_slot) {
      ipd_cand k;
      k.key = ((unsigned long long)m << 40) | ((unsigned long long)iy << 20) | (unsigned long long)ix;
      k.interest = v;
      k.pad = 0;
      a.cand[tile * a.cand_slot + slot] = k;
    }
  }
}

// ---- cull: a candidate's place is the number of candidates before it ------------------------------------------------------------
__global__ void __launch_bounds__(256) ipd_rank_kernel(ipd_args a) {
  const int tile = blockIdx.y;
  const ipd_tile T = a.tiles[tile];
  const long long count = min((long long)a.counters[tile * 2 + 1], a.cand_slot);
  if ((long long)blockIdx.x * 256 >= count) return;
  const ipd_cand* list = a.cand + tile * a.cand_slot;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool have = i < count;
  ipd_cand my{};
  if (have) my = list[i];
  __shared__ unsigned long long keys[256];
  __shared__ float ints[256];
  long long pos = 0;
  for (long long j0 = 0; j0 < count; j0 += 256) {
    const long long j = j0 + threadIdx.x;
    if (j < count) { keys[threadIdx.x] = list[j].key; ints[threadIdx.x] = list[j].interest; }
    __syncthreads();
    const int n = (int)min((long long)256, count - j0);
    if (have)
      for (int k = 0; k < n; ++k) pos += ipd_before(T.by_interest != 0, ints[k], keys[k], my.interest, my.key) ? 1 : 0;
    __syncthreads();
  }
  if (!have || pos >= T.written || pos >= a.capacity) return;
  const int m = (int)(my.key >> 40), iy = (int)((my.key >> 20) & 0xfffff), ix = (int)(my.key & 0xfffff);
  const long long o = (long long)(a.tile0 + tile) * a.capacity + pos;
  // InterestPoint(x, y, scale, interest) then the tile's origin is added to x, y, ix, iy (DetectorBase.h:231-236)
  a.out.x[o] = (float)ix + (float)T.x;
  a.out.y[o] = (float)iy + (float)T.y;
  a.out.ix[o] = ix + T.x;
  a.out.iy[o] = iy + T.y;
  a.out.orientation[o] = 0.0f;
  a.out.scale[o] = (float)ipo_sigma(m);
  a.out.interest[o] = my.interest;
}

// ---- orientation: AssignOrientation (IntegralDetector.cc:37-104) ----------------------------------------------------------------
struct ipd_ori_args {
  const ipd_tile* tiles;       // nullptr: one integral image, n points
  const float* integ; long long integ_slot, istride;
  int iw, ih, n, capacity, tile0;
  const int32_t *ix, *iy;
  const float* scale;
  float* orientation;
};

__global__ void __launch_bounds__(64) ipd_orientation_kernel(ipd_ori_args a, ipd_ori_table tab) {
  long long p = blockIdx.x;
  is_src s{};
  int ox = 0, oy = 0;
  if (a.tiles) {
    const ipd_tile T = a.tiles[blockIdx.y];
    if ((int)blockIdx.x >= T.written) return;
    p += (long long)(a.tile0 + blockIdx.y) * a.capacity;
    s.px = a.integ + blockIdx.y * a.integ_slot; s.stride = T.w + 1; s.w = T.w + 1; s.h = T.h + 1;
    ox = T.x; oy = T.y;
  } else {
    s.px = a.integ; s.stride = a.istride; s.w = a.iw; s.h = a.ih;
  }
  s.edge = VWGPU_TRANSFORM_EDGE_CONSTANT;
  const int ix = a.ix[p] - ox, iy = a.iy[p] - oy;
  const float scale = a.scale[p];
  __shared__ float hs[IPD_ORI_SAMPLES], vs[IPD_ORI_SAMPLES], an[IPD_ORI_SAMPLES];
  __shared__ float sx[IPD_ORI_SLICES], sy[IPD_ORI_SLICES];
  const int lane = threadIdx.x;
  for (int m = lane; m < IPD_ORI_SAMPLES; m += 64) {
    const double lx = (double)ix + (double)scale * (double)tab.i[m], ly = (double)iy + (double)scale * (double)tab.j[m];
    float h, v;
    iph_haar(s, lx, ly, scale * 4, &h, &v);
    h = tab.w[m] * h;
    v = tab.w[m] * v;
    hs[m] = h; vs[m] = v; an[m] = ipa_atan2f(v, h);
  }
  __syncthreads();
  const float pi_6 = (float)(3.14159265358979323846 / 6.0), two_pi = (float)(2 * 3.14159265358979323846);
  if (lane < IPD_ORI_SLICES) {
    const float a0 = 0.5f * lane;      // for (float a = 0; a < two_pi; a += 0.5): the halves are exact
    float sumx = 0.0f, sumy = 0.0f;
    for (int m = 0; m < IPD_ORI_SAMPLES; ++m) {
      const float g = an[m];
      if ((g > a0 - pi_6 && g < a0 + pi_6) || (g + two_pi > a0 - pi_6 && g + two_pi < a0 + pi_6) ||
          (g - two_pi > a0 - pi_6 && g - two_pi < a0 + pi_6)) {
        sumx += hs[m];
        sumy += vs[m];
      }
    }
    sx[lane] = sumx; sy[lane] = sumy;
  }
  __syncthreads();
  if (lane == 0) {
    float greatest_mod = 0.0f, greatest_ori = 0.0f;
    for (int k = 0; k < IPD_ORI_SLICES; ++k) {
      const float mod = sx[k] * sx[k] + sy[k] * sy[k];
      if (mod > greatest_mod) { greatest_mod = mod; greatest_ori = ipa_atan2f(sy[k], sx[k]); }
    }
    a.orientation[p] = greatest_ori;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

// generate_gaussian_kernel(kernel, 2, 9) in double (src/vw/Image/Filter.tcc:37-79, the odd branch) and the 81 products
// float(g[ix] * g[iy]) of the Harris test
ipd_harris_weights ipd_make_harris() {
  double g[9], sum = 0.0;
  const double z = 1 / (std::sqrt(2.0) * 2.0);
  for (int i = 1; i <= 4; ++i) {
    const double tap = std::erf((i + 0.5) * z) - std::erf((i - 0.5) * z);
    sum += tap;
    g[4 + i] = g[4 - i] = tap;
  }
  sum *= 2.0;
  const double tap = std::erf(0.5 * z) - std::erf(-0.5 * z);
  sum += tap;
  g[4] = tap;
  const double norm = 1.0 / sum;
  for (double& t : g) t *= norm;
  ipd_harris_weights w;
  for (int iy = 0; iy < 9; ++iy)
    for (int ix = 0; ix < 9; ++ix) w.w[iy * 9 + ix] = (float)(g[ix] * g[iy]);
  return w;
}

// float weight = exp(-distance_2 / 8) / 5.0133 with distance_2 a float (IntegralDetector.cc:54-59), in the loops' order
ipd_ori_table ipd_make_ori() {
  ipd_ori_table t;
  int m = 0;
  for (int i = -6; i <= 6; ++i)
    for (int j = -6; j <= 6; ++j) {
      const float distance_2 = (float)(i * i + j * j);
      if (distance_2 > 36) continue;
      t.w[m] = (float)(std::exp((double)(-distance_2 / 8)) / 5.0133);
      t.i[m] = (signed char)i; t.j[m] = (signed char)j;
      ++m;
    }
  return t;
}

struct ipd_call {
  const float* img; int w, h; ptrdiff_t stride;
  const int* tiles; int ntiles;
  const vwgpu_ip_detect_params* params;
  const int* desired; int capacity;
  const vwgpu_ip_points* out;
  int* stats;
};

int ipd_check(vwgpu_ctx* ctx, ipd_call& c) {
  const char* name = "ip_detect";
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!c.img || !c.tiles || !c.params || !c.out || !c.stats) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: null pointer", name);
  const vwgpu_ip_points& o = *c.out;
  if (!o.x || !o.y || !o.ix || !o.iy || !o.orientation || !o.scale || !o.interest)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: every output array must be given", name);
  if (c.w < 1 || c.h < 1 || c.ntiles < 1 || c.capacity < 1) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: sizes must be at least 1", name);
  if (c.stride == 0) c.stride = c.w;
  if (c.stride < c.w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than the width", name);
  const vwgpu_ip_detect_params& P = *c.params;
  if (P.detector != VWGPU_IP_DETECTOR_IAGD && P.detector != VWGPU_IP_DETECTOR_OBALOG)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: detector %d out of range", name, P.detector);
  if (P.scales < 1) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: scales must be at least 1", name);
  if (std::isnan(P.threshold)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: the threshold is NaN", name);
  for (int i = 0; i < c.ntiles; ++i) {
    const int* t = c.tiles + 4 * i;
    if (t[2] < 1 || t[3] < 1 || t[0] < 0 || t[1] < 0 || t[0] > c.w - t[2] || t[1] > c.h - t[3])
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: tile %d is empty or leaves the image", name, i);
    if (t[2] > 0xfffff || t[3] > 0xfffff) return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: a tile side above 1048575 is not implemented", name);
  }
  if (P.scales > IPO_SCALES)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: more than %d scales are not implemented (the reference's rows 8 and 9 are placeholders)", name,
                      IPO_SCALES);
  return VWGPU_OK;
}

// all array pointers are device pointers; tiles, desired and stats are host arrays
int ipd_run(vwgpu_ctx* ctx, const ipd_call& c) {
  const vwgpu_ip_detect_params& P = *c.params;
  for (int i = 0; i < 3 * c.ntiles; ++i) c.stats[i] = 0;
  if (P.scales < 3) return VWGPU_OK;      // no middle scale: no points
  static const ipd_harris_weights harris = ipd_make_harris();
  static const ipd_ori_table ori = ipd_make_ori();
  int maxw = 0, maxh = 0;
  for (int i = 0; i < c.ntiles; ++i) { maxw = std::max(maxw, c.tiles[4 * i + 2]); maxh = std::max(maxh, c.tiles[4 * i + 3]); }
  const long long integ_slot = (long long)vwgpu_align_up((size_t)(maxw + 1) * (maxh + 1), 64);
  const long long plane_slot = (long long)vwgpu_align_up((size_t)maxw * maxh, 64);
  const long long cand_slot = std::max<long long>(1, (long long)(P.scales - 2) * ((std::max(maxw - 2, 0) + 1) / 2) * ((std::max(maxh - 2, 0) + 1) / 2));
  const size_t per_tile = 4 * (size_t)integ_slot + 4 * (size_t)plane_slot * P.scales + sizeof(ipd_cand) * (size_t)cand_slot;
  const size_t budget = (size_t)ctx->ip_scratch_mb << 20;
  const int batch = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(c.ntiles, budget / per_tile), IPD_GRID_LIMIT / P.scales));
  const size_t words = vwgpu_align_up((size_t)batch * (sizeof(ipd_tile) + 8 + 8 * (size_t)P.scales), 256);
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, words + (size_t)batch * per_tile + 1024);
  if (rc) return rc;
  char* base = static_cast<char*>(ctx->scratch.base);
  ipd_args a{};
  a.tiles = reinterpret_cast<ipd_tile*>(base);
  a.counters = reinterpret_cast<unsigned*>(base + (size_t)batch * sizeof(ipd_tile));
  a.minmax = a.counters + 2 * (size_t)batch;
  a.integ = reinterpret_cast<float*>(base + words); a.integ_slot = integ_slot;
  a.planes = a.integ + (size_t)batch * integ_slot; a.plane_slot = plane_slot;
  a.cand = reinterpret_cast<ipd_cand*>(a.planes + (size_t)batch * plane_slot * P.scales); a.cand_slot = cand_slot;
  a.scales = P.scales; a.detector = P.detector; a.threshold = P.threshold; a.capacity = c.capacity;
  a.img = c.img; a.stride = c.stride; a.out = *c.out;
  std::vector<ipd_tile> table(batch);
  std::vector<unsigned> words_h(2 * (size_t)batch + 2 * (size_t)batch * P.scales);
  bool over = false;
  for (int t0 = 0; t0 < c.ntiles; t0 += batch) {
    const int n = std::min(batch, c.ntiles - t0);
    a.ntiles = n; a.tile0 = t0;
    for (int i = 0; i < n; ++i) {
      const int* t = c.tiles + 4 * (t0 + i);
      table[i] = ipd_tile{t[0], t[1], t[2], t[3], 0, 0, 0, 0};
    }
    for (int i = 0; i < n; ++i) {
      words_h[2 * i] = words_h[2 * i + 1] = 0;
      for (int s = 0; s < P.scales; ++s) {
        words_h[2 * (size_t)batch + ((size_t)i * P.scales + s) * 2] = 0x7f800000u;
        words_h[2 * (size_t)batch + ((size_t)i * P.scales + s) * 2 + 1] = 0u;
      }
    }
    VWGPU_HIP(ctx, hipMemcpyAsync(const_cast<ipd_tile*>(a.tiles), table.data(), n * sizeof(ipd_tile), hipMemcpyHostToDevice, ctx->stream));
    VWGPU_HIP(ctx, hipMemcpyAsync(a.counters, words_h.data(), words_h.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    {
      vwgpu_prof_scope sc(ctx, "ip_integral");
      hipLaunchKernelGGL(ipd_integral_kernel, dim3(n), dim3(64), 0, ctx->stream, a);
      VWGPU_HIP(ctx, hipGetLastError());
    }
    {
      vwgpu_prof_scope sc(ctx, "ip_planes");
      hipLaunchKernelGGL(ipd_planes_kernel, dim3((maxw + 63) / 64, (maxh + 3) / 4, n * P.scales), dim3(64, 4), 0, ctx->stream, a);
      VWGPU_HIP(ctx, hipGetLastError());
    }
    if (maxw > 2 && maxh > 2) {
      vwgpu_prof_scope sc(ctx, "ip_extrema");
      hipLaunchKernelGGL(ipd_extrema_kernel, dim3((maxw - 2 + 63) / 64, (maxh - 2 + 3) / 4, n * (P.scales - 2)), dim3(64, 4), 0, ctx->stream, a, harris);
      VWGPU_HIP(ctx, hipGetLastError());
    }
    VWGPU_HIP(ctx, hipMemcpyAsync(words_h.data(), a.counters, 2 * (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    long long most = 0;
    int most_written = 0;
    for (int i = 0; i < n; ++i) {
      const int count = (int)std::min<long long>(words_h[2 * i + 1], cand_slot);
      const int limit = c.desired && c.desired[t0 + i] > 0 ? c.desired[t0 + i] : P.max_points;
      ipd_cull_rule(P.detector, limit, count, &table[i].by_interest, &table[i].written);
      int* st = c.stats + 3 * (t0 + i);
      st[0] = (int)words_h[2 * i]; st[1] = count; st[2] = table[i].written;
      if (table[i].written > c.capacity) { over = true; table[i].written = 0; }
      most = std::max<long long>(most, count);
      most_written = std::max(most_written, table[i].written);
    }
    if (over || most_written == 0) continue;      // the remaining batches still fill their stats
    VWGPU_HIP(ctx, hipMemcpyAsync(const_cast<ipd_tile*>(a.tiles), table.data(), n * sizeof(ipd_tile), hipMemcpyHostToDevice, ctx->stream));
    {
      vwgpu_prof_scope sc(ctx, "ip_cull");
      hipLaunchKernelGGL(ipd_rank_kernel, dim3((unsigned)((most + 255) / 256), n), dim3(256), 0, ctx->stream, a);
      VWGPU_HIP(ctx, hipGetLastError());
    }
    if (P.detector == VWGPU_IP_DETECTOR_OBALOG) {
      ipd_ori_args o{};
      o.tiles = a.tiles; o.integ = a.integ; o.integ_slot = integ_slot; o.capacity = c.capacity; o.tile0 = t0;
      o.ix = c.out->ix; o.iy = c.out->iy; o.scale = c.out->scale; o.orientation = c.out->orientation;
      vwgpu_prof_scope sc(ctx, "ip_orientation");
      hipLaunchKernelGGL(ipd_orientation_kernel, dim3(most_written, n), dim3(64), 0, ctx->stream, o, ori);
      VWGPU_HIP(ctx, hipGetLastError());
    }
    if (t0 + batch < c.ntiles) VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the next batch reuses the scratch and the tables
  }
  if (over)
    return vwgpu_fail(ctx, VWGPU_ERR_CAPACITY, "ip_detect: a tile has more points than the capacity of %d; the stats say how many", c.capacity);
  return VWGPU_OK;
}

int ipd_integral_check(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t& ss, float* out, ptrdiff_t& os) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!src || !out) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "integral_image: null pointer");
  if (w < 1 || h < 1) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "integral_image: the image is empty");
  if (ss == 0) ss = w;
  if (os == 0) os = w + 1;
  if (ss < w || os < w + 1) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "integral_image: row stride smaller than the width");
  if ((const void*)src == (const void*)out) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "integral_image: the output must not be the input");
  return VWGPU_OK;
}

int ipd_orientation_check(vwgpu_ctx* ctx, const float* integ, int iw, int ih, ptrdiff_t& is, int n, const int32_t* ix, const int32_t* iy,
                          const float* scale, float* orientation) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!integ || !ix || !iy || !scale || !orientation) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "ip_orientation: null pointer");
  if (iw < 2 || ih < 2 || n < 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "ip_orientation: an integral image of at least 2 x 2 and n >= 0");
  if (is == 0) is = iw;
  if (is < iw) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "ip_orientation: row stride smaller than the width");
  return VWGPU_OK;
}

int ipd_orientation_run(vwgpu_ctx* ctx, const float* integ, int iw, int ih, ptrdiff_t is, int n, const int32_t* ix, const int32_t* iy,
                        const float* scale, float* orientation) {
  if (n == 0) return VWGPU_OK;
  static const ipd_ori_table ori = ipd_make_ori();
  ipd_ori_args o{};
  o.integ = integ; o.istride = is; o.iw = iw; o.ih = ih; o.n = n;
  o.ix = ix; o.iy = iy; o.scale = scale; o.orientation = orientation;
  vwgpu_prof_scope sc(ctx, "ip_orientation");
  hipLaunchKernelGGL(ipd_orientation_kernel, dim3(n), dim3(64), 0, ctx->stream, o, ori);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------------------------

extern "C" {

int vwgpu_integral_image_dev(vwgpu_ctx* ctx, const float* d_src, int w, int h, ptrdiff_t sstride, float* d_out, ptrdiff_t ostride) {
  int rc = ipd_integral_check(ctx, d_src, w, h, sstride, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_prof_scope sc(ctx, "ip_integral");
  hipLaunchKernelGGL(ipd_integral_single_kernel, dim3(1), dim3(64), 0, ctx->stream, ipd_single{d_src, sstride, w, h, d_out, ostride});
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int vwgpu_integral_image(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t sstride, float* out, ptrdiff_t ostride) {
  int rc = ipd_integral_check(ctx, src, w, h, sstride, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int a = st.add(src, w, h, 4, sstride, VWGPU_STAGE_IN), b = st.add(out, w + 1, h + 1, 4, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  if ((rc = vwgpu_integral_image_dev(ctx, st.dev<float>(a), w, h, w, st.dev<float>(b), w + 1))) return rc;
  return st.finish();
}

int vwgpu_ip_detect_dev(vwgpu_ctx* ctx, const float* d_img, int w, int h, ptrdiff_t stride, const int* tiles, int n_tiles,
                        const vwgpu_ip_detect_params* params, const int* desired_num_ip, int capacity, const vwgpu_ip_points* d_out,
                        int* stats) {
  ipd_call c{d_img, w, h, stride, tiles, n_tiles, params, desired_num_ip, capacity, d_out, stats};
  int rc = ipd_check(ctx, c);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return ipd_run(ctx, c);
}

int vwgpu_ip_detect(vwgpu_ctx* ctx, const float* img, int w, int h, ptrdiff_t stride, const int* tiles, int n_tiles,
                    const vwgpu_ip_detect_params* params, const int* desired_num_ip, int capacity, const vwgpu_ip_points* out, int* stats) {
  ipd_call c{img, w, h, stride, tiles, n_tiles, params, desired_num_ip, capacity, out, stats};
  int rc = ipd_check(ctx, c);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int qi = st.add(img, w, h, 4, c.stride, VWGPU_STAGE_IN);
  void* host[7] = {out->x, out->y, out->ix, out->iy, out->orientation, out->scale, out->interest};
  int q[7];
  for (int k = 0; k < 7; ++k) q[k] = st.add(host[k], capacity, n_tiles, 4, capacity, VWGPU_STAGE_NONE);
  if ((rc = st.commit())) return rc;
  vwgpu_ip_points d{st.dev<float>(q[0]), st.dev<float>(q[1]), st.dev<int32_t>(q[2]), st.dev<int32_t>(q[3]),
                    st.dev<float>(q[4]), st.dev<float>(q[5]), st.dev<float>(q[6])};
  ipd_call dc = c;
  dc.img = st.dev<float>(qi); dc.stride = w; dc.out = &d;
  if ((rc = ipd_run(ctx, dc))) return rc;
  for (int i = 0; i < n_tiles; ++i) {      // only what was written comes back
    const int n = stats[3 * i + 2];
    for (int k = 0; k < 7; ++k)
      VWGPU_HIP(ctx, hipMemcpyAsync(static_cast<char*>(host[k]) + (size_t)i * capacity * 4, st.dev<char>(q[k]) + (size_t)i * capacity * 4,
                                    (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  return st.finish();
}

int vwgpu_ip_orientation_dev(vwgpu_ctx* ctx, const float* d_integral, int iw, int ih, ptrdiff_t istride, int n, const int32_t* d_ix,
                             const int32_t* d_iy, const float* d_scale, float* d_orientation) {
  int rc = ipd_orientation_check(ctx, d_integral, iw, ih, istride, n, d_ix, d_iy, d_scale, d_orientation);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return ipd_orientation_run(ctx, d_integral, iw, ih, istride, n, d_ix, d_iy, d_scale, d_orientation);
}

int vwgpu_ip_orientation(vwgpu_ctx* ctx, const float* integral, int iw, int ih, ptrdiff_t istride, int n, const int32_t* ix, const int32_t* iy,
                         const float* scale, float* orientation) {
  int rc = ipd_orientation_check(ctx, integral, iw, ih, istride, n, ix, iy, scale, orientation);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return VWGPU_OK;
  vwgpu_stage st(ctx);
  const int qi = st.add(integral, iw, ih, 4, istride, VWGPU_STAGE_IN), qx = st.add(ix, n, 1, 4, n, VWGPU_STAGE_IN),
            qy = st.add(iy, n, 1, 4, n, VWGPU_STAGE_IN), qs = st.add(scale, n, 1, 4, n, VWGPU_STAGE_IN),
            qo = st.add(orientation, n, 1, 4, n, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  if ((rc = ipd_orientation_run(ctx, st.dev<float>(qi), iw, ih, iw, n, st.dev<int32_t>(qx), st.dev<int32_t>(qy), st.dev<float>(qs),
                                st.dev<float>(qo))))
    return rc;
  return st.finish();
}

int vwgpu_ip_cull_order(int detector, int limit, int n, const float* interest, int32_t* order, int* n_out) {
  if ((detector != VWGPU_IP_DETECTOR_IAGD && detector != VWGPU_IP_DETECTOR_OBALOG) || n < 0 || (n > 0 && (!interest || !order)) || !n_out)
    return VWGPU_ERR_ARGUMENT;
  int by_interest = 0, written = 0;
  ipd_cull_rule(detector, limit, n, &by_interest, &written);
  std::vector<int32_t> idx(n);
  std::iota(idx.begin(), idx.end(), 0);
  std::sort(idx.begin(), idx.end(), [&](int32_t p, int32_t q) {
    return ipd_before(by_interest != 0, interest[p], (unsigned long long)p, interest[q], (unsigned long long)q);
  });
  for (int i = 0; i < written; ++i) order[i] = idx[i];
  *n_out = written;
  return VWGPU_OK;
}

}  // extern "C"
