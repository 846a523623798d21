// corr_eval.hip — vw::stereo::corr_eval (src/vw/Stereo/CorrEval.{h,cc}): for each sampled pixel of a tile, the NCC of
// the left patch against the bilinearly resampled right patch at p + d(p), the mean patch standard deviation, or an
// uncertainty sigma from the curvature of the NCC peak.  One CorrEval::prerasterize(bbox) per tile; the semantics the
// port reproduces (and tests/refimpl/corr_eval_ref.cc restates) are listed at vwgpu_corr_eval in include/vwgpu.h and in
// DESIGN §4.14.  Two launches per call on the context's stream:
//   1. ce_box_kernel: the sampled pixels of every tile grow the tile's right_box (CorrEval.cc:189-203): min / max of
//      floor and ceil of the right coordinate, folded per workgroup and merged with atomicMin / atomicMax
//      (order-independent), with flags for non-finite or out-of-range values;
//   2. ce_eval_kernel: one workgroup per 16 x 16 sampled pixels of one tile (tiles flattened into a block list), one lane
//      per sampled pixel.  The workgroup expands its tile's box as BBox2i::expand does (a no-op on an empty box), stages
//      the left window block (values and validity) in LDS, then evaluates the pixel's patches in the reference's order
//      (c outer, r inner, double sums) with the right taps read through L1.
#include <cfloat>
#include <climits>
#include <cmath>
#include <vector>

#include "vwgpu_internal.h"

namespace {

constexpr int CE_TX = 16, CE_TY = 16, CE_THREADS = CE_TX * CE_TY;
constexpr int CE_MAX_KERNEL = 63;                 // include/vwgpu.h states this limit
constexpr size_t CE_LDS_BUDGET = 64 * 1024;       // the left block is staged when it fits (always at sample rates <= 3)
constexpr int CE_BIG = INT_MAX - 1;               // BBox2i's empty box: min = big, max = -big (Math/BBox.tcc:38-45)
enum { CE_NCC = 0, CE_STDDEV = 1, CE_PARABOLA = 2, CE_CRAMER = 3 };
enum { CE_BAD_DISP = 1, CE_BAD_COORD = 2, CE_BAD_BOX = 4 };

struct ce_tile {
  int x, y, w, h;          // the tile (prerasterize's bbox)
  int nsx, nsy;            // sampled columns and rows: ceil(w / rate), ceil(h / rate)
  int nbx, flags;          // workgroup blocks across (ceil(nsx / CE_TX)); CE_BAD_* of the tile (atomicOr)
  long long b0;            // the tile's first block in the flattened block list of the evaluation
  int bmin[2], bmax[2];    // right_box before expansion, grown from {big, big} / {-big, -big}
};

struct ce_args {
  const float* disp;       // {dx, dy, valid} per pixel
  long long dstride;
  const float* L;
  const uint8_t* Lv;       // nullptr: all valid
  long long lstride;
  int w, h;
  const float* R;
  const uint8_t* Rv;
  long long rstride;
  int rw, rh;
  int kx, ky, rate, round, pad;   // pad: m_extra_padding = (int)ceil(prefilter_kernel_width) + 5, >= 0
  int sx, sy;              // staged left block: min((CE_TX - 1) rate, widest tile - 1) + kx by the same for rows and ky
  float* out;              // {value, valid} per pixel
  long long ostride;
  ce_tile* tiles;
  int ntiles;
  unsigned long long* counters;   // {CE_BAD_* of the call, pixels evaluated, valid results, degenerate tiles}
  int stats;
};

// the tile whose block range holds k (the last tile whose first block is <= k); every tile holds at least one block
__device__ inline int ce_find(const ce_tile* t, int n, long long k) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid].b0 <= k) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// math::impl::_floor (Math/Functions.h:74-81) on the in-range values the box check admits; clamped so that the
// conversion stays defined on every input
__device__ inline long long ce_floor(double v) {
  return (long long)fmin(fmax(floor(v), (double)INT_MIN), (double)INT_MAX);
}

// One workgroup row per tile (tile0 + blockIdx.y), gridDim.x workgroups striding over the tile's sampled pixels.  Each lane
// keeps its own bounds, the workgroup folds them with LDS atomics and adds one global atomic per bound: a global atomic per
// pixel on the tile's four words would serialise the whole pass.
__global__ __launch_bounds__(256) void ce_box_kernel(ce_args a, int tile0) {
  __shared__ int red[4], red_flags;
  ce_tile* T = a.tiles + tile0 + blockIdx.y;
  if (threadIdx.x == 0) {
    red[0] = red[1] = CE_BIG;
    red[2] = red[3] = -CE_BIG;
    red_flags = 0;
  }
  __syncthreads();
  int mnx = CE_BIG, mny = CE_BIG, mxx = -CE_BIG, mxy = -CE_BIG, fl = 0;
  const long long n = (long long)T->nsx * T->nsy;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (long long)gridDim.x * blockDim.x) {
    const int col = (int)(q % T->nsx) * a.rate, row = (int)(q / T->nsx) * a.rate;
    const float* d = a.disp + ((long long)(T->y + row) * a.dstride + T->x + col) * 3;
    if (!(d[2] != 0.f)) continue;
    float dx = d[0], dy = d[1];
    if (a.round) { dx = roundf(dx); dy = roundf(dy); }   // CorrEval.cc:145-151, before the box is built
    if (!isfinite(dx) || !isfinite(dy)) {
      fl |= CE_BAD_DISP;
      continue;
    }
    // bbox.min() + Vector2(col, row) + disp (CorrEval.cc:198-201), in double
    const double px = (double)(T->x + col) + (double)dx, py = (double)(T->y + row) + (double)dy;
    const double fx = floor(px), fy = floor(py), cx = ceil(px), cy = ceil(py);
    if (fx < (double)INT_MIN || fy < (double)INT_MIN || cx > (double)INT_MAX || cy > (double)INT_MAX) {
      fl |= CE_BAD_COORD;
      continue;
    }
    mnx = min(mnx, (int)fx);
    mny = min(mny, (int)fy);
    mxx = max(mxx, (int)cx);
    mxy = max(mxy, (int)cy);
  }
  atomicMin(&red[0], mnx);
  atomicMin(&red[1], mny);
  atomicMax(&red[2], mxx);
  atomicMax(&red[3], mxy);
  if (fl) atomicOr(&red_flags, fl);
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicMin(&T->bmin[0], red[0]);
    atomicMin(&T->bmin[1], red[1]);
    atomicMax(&T->bmax[0], red[2]);
    atomicMax(&T->bmax[1], red[3]);
    if (red_flags) {
      atomicOr(&T->flags, red_flags);
      atomicOr(a.counters, (unsigned long long)red_flags);
    }
  }
}

struct ce_pix {
  float v;
  bool ok;
};

// the expanded right_box of a tile: crop origin and size (a 0 size reads nodata everywhere)
struct ce_crop {
  long long mnx, mny, cw, ch;
};

// one pixel of crop(edge_extend(right, nodata), right_box) at crop position (x, y); nodata is {0, invalid}
template <bool VALID>
__device__ inline ce_pix ce_tap(const ce_args& a, const ce_crop& cr, long long x, long long y) {
  const long long gx = x + cr.mnx, gy = y + cr.mny;
  if (x < 0 || y < 0 || x >= cr.cw || y >= cr.ch || gx < 0 || gy < 0 || gx >= a.rw || gy >= a.rh) return {0.f, false};
  const long long o = gy * a.rstride + gx;
  return {a.R[o], VALID ? (a.Rv ? a.Rv[o] != 0 : true) : true};
}

// a right sample at crop coordinates (i, j): BilinearInterpolationImpl<PixelMask<float>> (Interpolation.h:76-106) with
// real_type float and the integer shortcut on the double coordinates, or the integer read of round_to_int
template <bool VALID>
__device__ inline ce_pix ce_right(const ce_args& a, const ce_crop& cr, double i, double j) {
  if (a.round) return ce_tap<VALID>(a, cr, (long long)i, (long long)j);
  const long long x = ce_floor(i), y = ce_floor(j);
  if ((double)x == i && (double)y == j) return ce_tap<VALID>(a, cr, x, y);
  const float nx = (float)i - (float)x, ny = (float)j - (float)y, n1x = 1.f - nx, n1y = 1.f - ny;
  const ce_pix p00 = ce_tap<VALID>(a, cr, x, y), p10 = ce_tap<VALID>(a, cr, x + 1, y);
  const ce_pix p01 = ce_tap<VALID>(a, cr, x, y + 1), p11 = ce_tap<VALID>(a, cr, x + 1, y + 1);
  float r = p00.v * n1x;
  r = r + p10.v * nx;
  r = r * n1y;
  float row = p01.v * n1x;
  row = row + p11.v * nx;
  r = r + row * ny;
  return {r, p00.ok && p10.ok && p01.ok && p11.ok};
}

// where a lane's left patch lives: the block in LDS (STAGE) or the image
struct ce_lane {
  const float* lv;          // STAGE: LDS values, row pitch a.sx
  const uint8_t* lm;        // STAGE: LDS validity
  int lo;                   // STAGE: offset of the patch's (0, 0) in the block
  long long px0, py0;       // the patch's (0, 0) in the left image: bbox.min + (col, row) - half_kernel
};

template <bool STAGE, bool VALID>
__device__ inline ce_pix ce_left(const ce_args& a, const ce_lane& ln, int c, int r) {
  if (STAGE) {
    const int o = ln.lo + r * a.sx + c;
    return {ln.lv[o], VALID ? ln.lm[o] != 0 : true};
  }
  const long long gx = ln.px0 + c, gy = ln.py0 + r;
  if (gx < 0 || gy < 0 || gx >= a.w || gy >= a.h) return {0.f, false};
  const long long o = gy * a.lstride + gx;
  return {a.L[o], VALID ? (a.Lv ? a.Lv[o] != 0 : true) : true};
}

// calc_ncc over calc_patches (CorrEval.cc:15-96): every sample's stored value counts (the reference's validity test is
// always true), num / sqrt(den1 den2) in double, c outer, r inner; -1 unless both sums are positive.  a b, a a and b b
// of floats are exact in double, so the fma gives the bits of multiply-then-add.
template <bool STAGE>
__device__ double ce_ncc(const ce_args& a, const ce_lane& ln, const ce_crop& cr, float dx, float dy) {
  double num = 0.0, den1 = 0.0, den2 = 0.0;
  for (int c = 0; c < a.kx; ++c) {
    const double i = ((double)(ln.px0 + c) + (double)dx) - (double)cr.mnx;
    for (int r = 0; r < a.ky; ++r) {
      const double j = ((double)(ln.py0 + r) + (double)dy) - (double)cr.mny;
      const double va = ce_left<STAGE, false>(a, ln, c, r).v;
      const double vb = ce_right<false>(a, cr, i, j).v;
      num = fma(va, vb, num);
      den1 = fma(va, va, den1);
      den2 = fma(vb, vb, den2);
    }
  }
  if (den1 > 0.0 && den2 > 0.0) return num / sqrt(den1 * den2);
  return -1.0;
}

// (calc_stddev(left) + calc_stddev(right)) / 2 (CorrEval.cc:100-137, 265-270): two passes in double over the valid
// samples of each patch; (v - mean)^2 is not exact, so its multiply and add stay separate (-ffp-contract=off)
template <bool STAGE>
__device__ double ce_stddev(const ce_args& a, const ce_lane& ln, const ce_crop& cr, float dx, float dy) {
  int nl = 0, nr = 0;
  double ml = 0.0, mr = 0.0;
  for (int c = 0; c < a.kx; ++c) {
    const double i = ((double)(ln.px0 + c) + (double)dx) - (double)cr.mnx;
    for (int r = 0; r < a.ky; ++r) {
      const double j = ((double)(ln.py0 + r) + (double)dy) - (double)cr.mny;
      const ce_pix pa = ce_left<STAGE, true>(a, ln, c, r), pb = ce_right<true>(a, cr, i, j);
      if (pa.ok) { nl += 1; ml += pa.v; }
      if (pb.ok) { nr += 1; mr += pb.v; }
    }
  }
  if (nl == 0 || nr == 0) return -1.0;
  ml /= nl;
  mr /= nr;
  double sl = 0.0, sr = 0.0;
  for (int c = 0; c < a.kx; ++c) {
    const double i = ((double)(ln.px0 + c) + (double)dx) - (double)cr.mnx;
    for (int r = 0; r < a.ky; ++r) {
      const double j = ((double)(ln.py0 + r) + (double)dy) - (double)cr.mny;
      const ce_pix pa = ce_left<STAGE, true>(a, ln, c, r), pb = ce_right<true>(a, cr, i, j);
      if (pa.ok) sl += (pa.v - ml) * (pa.v - ml);
      if (pb.ok) sr += (pb.v - mr) * (pb.v - mr);
    }
  }
  return (sqrt(sl / nl) + sqrt(sr / nr)) / 2.0;
}

template <int METRIC, bool STAGE>
__global__ __launch_bounds__(CE_THREADS) void ce_eval_kernel(ce_args a, long long blk_base) {
  extern __shared__ float ce_lds[];
  const long long g = blk_base + blockIdx.x;
  const ce_tile T = a.tiles[ce_find(a.tiles, a.ntiles, g)];   // the box pass has finished (previous launch)
  if (T.flags) return;
  const long long q = g - T.b0;
  const int bx = (int)(q % T.nbx), by = (int)(q / T.nbx);
  const int tx = threadIdx.x % CE_TX, ty = threadIdx.x / CE_TX;
  const int hkx = a.kx / 2, hky = a.ky / 2;

  // right_box.expand(half_kernel), (pixel_buffer = 1), (2), (m_extra_padding) and, for the curvature metrics, (1)
  // (CorrEval.cc:205-214).  BBox::expand returns at once on an empty box (min >= max on an axis, Math/BBox.tcc:228-246);
  // every expansion is >= 0, so a box is either empty throughout or expanded by the sum.
  long long mn[2] = {T.bmin[0], T.bmin[1]}, mx[2] = {T.bmax[0], T.bmax[1]};
  const bool empty = mn[0] >= mx[0] || mn[1] >= mx[1];
  const bool degenerate = empty && mn[0] <= mx[0];   // grown by a sampled valid pixel, yet empty
  if (!empty) {
    const long long e = 1 + 2 + a.pad + ((METRIC == CE_PARABOLA || METRIC == CE_CRAMER) ? 1 : 0);
    mn[0] -= hkx + e; mn[1] -= hky + e; mx[0] += hkx + e; mx[1] += hky + e;
  }
  const ce_crop cr{mn[0], mn[1], mx[0] > mn[0] ? mx[0] - mn[0] : 0, mx[1] > mn[1] ? mx[1] - mn[1] : 0};
  if (mn[0] < INT_MIN || mn[1] < INT_MIN || mx[0] > INT_MAX || mx[1] > INT_MAX || cr.cw > INT_MAX || cr.ch > INT_MAX) {
    if (threadIdx.x == 0) atomicOr(a.counters, (unsigned long long)CE_BAD_BOX);
    return;
  }

  ce_lane ln;
  ln.lv = ce_lds;
  ln.lm = reinterpret_cast<const uint8_t*>(ce_lds + a.sx * a.sy);
  if (STAGE) {
    // the block's left windows: a.sx columns from bbox.min + block origin - half_kernel; nodata outside
    const long long bx0 = (long long)T.x + (long long)bx * CE_TX * a.rate - hkx;
    const long long by0 = (long long)T.y + (long long)by * CE_TY * a.rate - hky;
    uint8_t* lm = reinterpret_cast<uint8_t*>(ce_lds + a.sx * a.sy);
    for (int o = threadIdx.x; o < a.sx * a.sy; o += CE_THREADS) {
      const long long gx = bx0 + o % a.sx, gy = by0 + o / a.sx;
      float v = 0.f;
      uint8_t m = 0;
      if (gx >= 0 && gy >= 0 && gx < a.w && gy < a.h) {
        const long long p = gy * a.lstride + gx;
        v = a.L[p];
        m = a.Lv ? (a.Lv[p] != 0) : 1;
      }
      ce_lds[o] = v;
      if (METRIC == CE_STDDEV) lm[o] = m;
    }
    __syncthreads();
  }

  const int sxi = bx * CE_TX + tx, syi = by * CE_TY + ty;
  int evaluated = 0, good = 0;
  if (sxi < T.nsx && syi < T.nsy) {
    // inside the tile, so col < T.w, row < T.h, and the patch lies in the staged block
    const int col = sxi * a.rate, row = syi * a.rate;
    ln.lo = ty * a.rate * a.sx + tx * a.rate;
    ln.px0 = (long long)T.x + col - hkx;
    ln.py0 = (long long)T.y + row - hky;
    const float* d = a.disp + ((long long)(T.y + row) * a.dstride + T.x + col) * 3;
    float val = 0.f;
    if (d[2] != 0.f) {
      evaluated = 1;
      float dx = d[0], dy = d[1];
      if (a.round) { dx = roundf(dx); dy = roundf(dy); }
      double res = -1.0;
      if (METRIC == CE_NCC) {
        res = ce_ncc<STAGE>(a, ln, cr, dx, dy);
        good = res >= 0;
      } else if (METRIC == CE_STDDEV) {
        res = ce_stddev<STAGE>(a, ln, cr, dx, dy);
        good = res >= 0;
      } else {
        // CorrEval.cc:279-309; the neighbour disparity is d + shift in float (Vector2f += Vector2f)
        const double C = ce_ncc<STAGE>(a, ln, cr, dx, dy);
        if (C >= 0) {
          const float sh[4][2] = {{1.f, 0.f}, {-1.f, 0.f}, {0.f, 1.f}, {0.f, -1.f}};
          double nbr[4];
          bool ok = true;
          for (int s = 0; s < 4 && ok; ++s) {
            const float sdx = dx + sh[s][0], sdy = dy + sh[s][1];
            nbr[s] = ce_ncc<STAGE>(a, ln, cr, sdx, sdy);
            if (nbr[s] < 0) ok = false;
          }
          if (ok) {
            const double kxc = 2.0 * C - nbr[0] - nbr[1];
            const double kyc = 2.0 * C - nbr[2] - nbr[3];
            if (kxc > 0 && kyc > 0) {
              double sigma = sqrt(1.0 / kxc + 1.0 / kyc);
              if (METRIC == CE_CRAMER) {
                double resid = 1.0 - C;
                if (resid < 0) resid = 0;
                sigma *= sqrt(resid);
              }
              res = sigma;
              good = 1;
            }
          }
        }
      }
      if (good) val = (float)res;
    }
    // the lane's rate x rate cell of the tile: its sampled pixel, the others invalid (CorrEval.cc:236-248)
    for (int r = 0; r < a.rate && row + r < T.h; ++r)
      for (int c = 0; c < a.rate && col + c < T.w; ++c) {
        float* o = a.out + ((long long)(T.y + row + r) * a.ostride + T.x + col + c) * 2;
        const bool here = r == 0 && c == 0 && good;
        o[0] = here ? val : 0.f;
        o[1] = here ? 1.f : 0.f;
      }
  }
  if (a.stats) {
    const int ne = __syncthreads_count(evaluated), ng = __syncthreads_count(good);
    if (threadIdx.x == 0) {
      if (ne) atomicAdd(a.counters + 1, (unsigned long long)ne);
      if (ng) atomicAdd(a.counters + 2, (unsigned long long)ng);
      if (q == 0 && degenerate) atomicAdd(a.counters + 3, 1ull);
    }
  }
}

template <int METRIC>
void ce_launch(const ce_args& a, bool stage, unsigned nblk, size_t lds, hipStream_t s, long long base) {
  if (stage)
    hipLaunchKernelGGL((ce_eval_kernel<METRIC, true>), dim3(nblk), dim3(CE_THREADS), lds, s, a, base);
  else
    hipLaunchKernelGGL((ce_eval_kernel<METRIC, false>), dim3(nblk), dim3(CE_THREADS), 0, s, a, base);
}

int ce_check(vwgpu_ctx* ctx, const void* disp, int w, int h, ptrdiff_t& dstride, const void* left, ptrdiff_t& lstride,
             const void* right, int rw, int rh, ptrdiff_t& rstride, int kx, int ky, int metric, int rate, float width,
             const int* tiles, int ntiles, const void* out, ptrdiff_t& ostride) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!disp || !left || !right || !out || w <= 0 || h <= 0 || rw <= 0 || rh <= 0 || ntiles < 0 || (ntiles > 0 && !tiles))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "corr_eval: empty image or null pointer");
  if (kx <= 0 || ky <= 0 || kx % 2 != 1 || ky % 2 != 1)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "CorrEval: The kernel dimensions must be positive and odd.");
  if (metric < VWGPU_CORR_EVAL_NCC || metric > VWGPU_CORR_EVAL_CRAMER_RAO)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "CorrEval: Invalid metric: %d.", metric);
  if (rate < 1)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "corr_eval: sample_rate %d is not positive", rate);
  if (!std::isfinite(width) || std::ceil((double)width) < -5.0 || std::ceil((double)width) > (double)(INT_MAX - 5))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "corr_eval: prefilter_kernel_width %g gives no padding in [0, INT_MAX]",
                      (double)width);
  if (kx > CE_MAX_KERNEL || ky > CE_MAX_KERNEL)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "corr_eval: kernel %d x %d is larger than %d x %d", kx, ky, CE_MAX_KERNEL,
                      CE_MAX_KERNEL);
  if (dstride == 0) dstride = w;
  if (ostride == 0) ostride = w;
  if (lstride == 0) lstride = w;
  if (rstride == 0) rstride = rw;
  if (dstride < w || ostride < w || lstride < w || rstride < rw)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "corr_eval: row stride smaller than row width");
  for (int t = 0; t < ntiles; ++t) {
    const int* b = tiles + 4 * t;
    if (b[2] <= 0 || b[3] <= 0 || b[0] < 0 || b[1] < 0 || b[0] > w - b[2] || b[1] > h - b[3])
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "corr_eval: tile %d {%d, %d, %d, %d} is not inside the %d x %d image", t,
                        b[0], b[1], b[2], b[3], w, h);
  }
  return VWGPU_OK;
}

int ce_run(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride, const float* d_left, const uint8_t* d_lv,
           ptrdiff_t lstride, const float* d_right, const uint8_t* d_rv, int rw, int rh, ptrdiff_t rstride, int kx, int ky,
           int metric, int rate, int round, float width, const int* tiles, int ntiles, float* d_out, ptrdiff_t ostride,
           long long* stats) {
  std::vector<ce_tile> tab((size_t)ntiles);
  long long nb = 0;
  for (int t = 0; t < ntiles; ++t) {
    ce_tile& T = tab[t];
    T.x = tiles[4 * t]; T.y = tiles[4 * t + 1]; T.w = tiles[4 * t + 2]; T.h = tiles[4 * t + 3];
    T.nsx = (int)(((long long)T.w + rate - 1) / rate);
    T.nsy = (int)(((long long)T.h + rate - 1) / rate);
    T.nbx = (T.nsx + CE_TX - 1) / CE_TX;
    T.flags = 0;
    T.b0 = nb;
    T.bmin[0] = T.bmin[1] = CE_BIG;
    T.bmax[0] = T.bmax[1] = -CE_BIG;
    nb += (long long)T.nbx * ((T.nsy + CE_TY - 1) / CE_TY);
  }
  const size_t tb = vwgpu_align_up(tab.size() * sizeof(ce_tile), 256);
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, 256 + tb);
  if (rc) return rc;
  char* base = static_cast<char*>(ctx->scratch.base);
  ce_args a{};
  a.counters = reinterpret_cast<unsigned long long*>(base);
  a.tiles = reinterpret_cast<ce_tile*>(base + 256);
  a.ntiles = ntiles;
  a.disp = d_disp; a.dstride = dstride;
  a.L = d_left; a.Lv = d_lv; a.lstride = lstride; a.w = w; a.h = h;
  a.R = d_right; a.Rv = d_rv; a.rstride = rstride; a.rw = rw; a.rh = rh;
  a.kx = kx; a.ky = ky; a.rate = rate; a.round = round ? 1 : 0;
  a.pad = (int)std::ceil(width) + 5;   // CorrEval.h:77
  a.out = d_out; a.ostride = ostride;
  a.stats = stats != nullptr;
  // The left block is staged when it fits the budget; otherwise (large sample rates, whose windows hardly overlap) the
  // lanes read the left image through L1.  A block's sampled pixels inside a tile lie within min((CE_TX - 1) rate,
  // tile width - 1) columns of its first one (rows alike), so that bounds the block's extent for any rate.
  int most_w = 1, most_h = 1;
  for (const ce_tile& T : tab) {
    most_w = std::max(most_w, T.w);
    most_h = std::max(most_h, T.h);
  }
  const long long sx = std::min((long long)(CE_TX - 1) * rate, (long long)most_w - 1) + kx;
  const long long sy = std::min((long long)(CE_TY - 1) * rate, (long long)most_h - 1) + ky;
  const bool small = sx <= (long long)CE_LDS_BUDGET && sy <= (long long)CE_LDS_BUDGET;   // the product below stays in range
  const long long lds = small ? sx * sy * (metric == VWGPU_CORR_EVAL_STDDEV ? 5 : 4) : 0;
  const bool stage = small && lds <= (long long)CE_LDS_BUDGET;
  a.sx = stage ? (int)sx : 0;
  a.sy = stage ? (int)sy : 0;
  VWGPU_HIP(ctx, hipMemsetAsync(a.counters, 0, 32, ctx->stream));
  VWGPU_HIP(ctx, hipMemcpyAsync(a.tiles, tab.data(), tab.size() * sizeof(ce_tile), hipMemcpyHostToDevice, ctx->stream));
  const long long max_blk = 0xffffffffLL / CE_THREADS;   // a launch holds at most 2^32 - 1 work-items in x
  {
    vwgpu_prof_scope ps(ctx, "corr_eval_box");
    long long most = 1;
    for (const ce_tile& T : tab) most = std::max(most, (long long)T.nsx * T.nsy);
    const unsigned gx = (unsigned)std::min<long long>((most + 255) / 256, 64);
    for (int t0 = 0; t0 < ntiles; t0 += 65535)
      hipLaunchKernelGGL(ce_box_kernel, dim3(gx, (unsigned)std::min(ntiles - t0, 65535)), dim3(256), 0, ctx->stream, a, t0);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  {
    vwgpu_prof_scope ps(ctx, "corr_eval");
    for (long long b0 = 0; b0 < nb; b0 += max_blk) {
      const unsigned n = (unsigned)std::min<long long>(nb - b0, max_blk);
      switch (metric) {
        case VWGPU_CORR_EVAL_NCC: ce_launch<CE_NCC>(a, stage, n, (size_t)lds, ctx->stream, b0); break;
        case VWGPU_CORR_EVAL_STDDEV: ce_launch<CE_STDDEV>(a, stage, n, (size_t)lds, ctx->stream, b0); break;
        case VWGPU_CORR_EVAL_PARABOLA_CURVATURE: ce_launch<CE_PARABOLA>(a, stage, n, (size_t)lds, ctx->stream, b0); break;
        default: ce_launch<CE_CRAMER>(a, stage, n, (size_t)lds, ctx->stream, b0); break;
      }
    }
    VWGPU_HIP(ctx, hipGetLastError());
  }
  unsigned long long cnt[4] = {0, 0, 0, 0};
  VWGPU_HIP(ctx, hipMemcpyAsync(cnt, a.counters, 32, hipMemcpyDeviceToHost, ctx->stream));
  VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the box pass's argument checks; also keeps `tab` alive
  if (cnt[0] & CE_BAD_DISP)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "corr_eval: a sampled valid disparity is not finite");
  if (cnt[0] & (CE_BAD_COORD | CE_BAD_BOX))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "corr_eval: a right coordinate or a tile's right box is outside int32");
  if (stats) {
    stats[0] = (long long)cnt[1];
    stats[1] = (long long)cnt[2];
    stats[2] = ntiles;
    stats[3] = (long long)cnt[3];
  }
  return VWGPU_OK;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------

extern "C" {

int vwgpu_corr_eval_dev(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride, const float* d_left,
                        const uint8_t* d_left_valid, ptrdiff_t lstride, const float* d_right, const uint8_t* d_right_valid,
                        int rw, int rh, ptrdiff_t rstride, int kx, int ky, int metric, int sample_rate, int round_to_int,
                        int prefilter_mode, float prefilter_kernel_width, const int* tiles, int ntiles, float* d_out,
                        ptrdiff_t ostride, long long* stats) {
  (void)prefilter_mode;   // accepted and unused, as in the reference
  int rc = ce_check(ctx, d_disp, w, h, dstride, d_left, lstride, d_right, rw, rh, rstride, kx, ky, metric, sample_rate,
                    prefilter_kernel_width, tiles, ntiles, d_out, ostride);
  if (rc) return rc;
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (ntiles == 0) return VWGPU_OK;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return ce_run(ctx, d_disp, w, h, dstride, d_left, d_left_valid, lstride, d_right, d_right_valid, rw, rh, rstride, kx, ky,
                metric, sample_rate, round_to_int, prefilter_kernel_width, tiles, ntiles, d_out, ostride, stats);
}

int vwgpu_corr_eval(vwgpu_ctx* ctx, const float* disp, int w, int h, ptrdiff_t dstride, const float* left,
                    const uint8_t* left_valid, ptrdiff_t lstride, const float* right, const uint8_t* right_valid, int rw,
                    int rh, ptrdiff_t rstride, int kx, int ky, int metric, int sample_rate, int round_to_int,
                    int prefilter_mode, float prefilter_kernel_width, const int* tiles, int ntiles, float* out,
                    ptrdiff_t ostride, long long* stats) {
  (void)prefilter_mode;
  int rc = ce_check(ctx, disp, w, h, dstride, left, lstride, right, rw, rh, rstride, kx, ky, metric, sample_rate,
                    prefilter_kernel_width, tiles, ntiles, out, ostride);
  if (rc) return rc;
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (ntiles == 0) return VWGPU_OK;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pd = st.add(disp, w, h, 12, dstride, VWGPU_STAGE_IN), po = st.add(out, w, h, 8, ostride, VWGPU_STAGE_INOUT);
  const int pl = st.add(left, w, h, 4, lstride, VWGPU_STAGE_IN), pr = st.add(right, rw, rh, 4, rstride, VWGPU_STAGE_IN);
  const int plv = st.add(left_valid, w, h, 1, lstride, VWGPU_STAGE_IN), prv = st.add(right_valid, rw, rh, 1, rstride, VWGPU_STAGE_IN);
  if ((rc = st.commit())) return rc;
  rc = ce_run(ctx, st.dev<float>(pd), w, h, w, st.dev<float>(pl), st.dev<uint8_t>(plv), w, st.dev<float>(pr), st.dev<uint8_t>(prv), rw, rh, rw,
              kx, ky, metric, sample_rate, round_to_int, prefilter_kernel_width, tiles, ntiles, st.dev<float>(po), w, stats);
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
