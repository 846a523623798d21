// pyramid_plan.h — the host plan of the pyramid correlator: every rule of PyramidCorrelationView::prerasterize
// (src/vw/Stereo/CorrelationView.cc:273-886) that is arithmetic on sizes, boxes and zone lists, written once for the
// single-tile and the tile-group level loops of pyramid.hip.  No HIP in here: a plain C++ compiler builds it
// (tests/cpp/test_pyramid_plan.cc).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "vwgpu.h"
#include "zone_task.h"
#include "zones.h"

// bm_exact.hip (plain host functions)
bool vwgpu_sums_order_free(int cost_type, int kx, int ky, int lo, int hi, int nonfinite);
int vwgpu_sums_bits(int cost_type, int kx, int ky, int lo, int hi, int nonfinite);

namespace vwgpu {

// constructor + 1.0): number of levels (CorrelationView.h:99-105, CorrelationView.cc:301-310)
inline int pyramid_levels(const vwgpu_pyramid_params* P, int bw, int bh) {
  const IBox search(P->search_min_x, P->search_min_y, P->search_max_x, P->search_max_y);
  const int kx = P->kernel_x, ky = P->kernel_y;
  const int largest_search = std::max(search.dx(), search.dy());
  int by_search = (int)(std::floor(std::log(float(largest_search)) / std::log(2.0f)) - 1);
  by_search = std::max(0, std::min(by_search, P->max_pyramid_levels));
  int L = (int)std::floor(std::log((double)std::min(bw, bh)) / std::log(2.0f) - std::log((double)std::max(kx, ky)) / std::log(2.0f));
  L = std::min(L, by_search);
  if (L < 1) L = 0;
  return L;
}

// geometry of level 0: the tile, the left and right image crops (grown by the half kernel at the coarsest level, the right one by
// the search range as well) and the crop of the right mask
struct TileGeom { IBox bbox, lg, rg, rmb; };
inline TileGeom tile_geom(int bx, int by, int bw, int bh, IBox const& search, int hkx, int hky, int up) {
  TileGeom g;
  g.bbox = IBox(bx, by, bx + bw, by + bh);
  g.lg = g.bbox; g.lg.x0 -= hkx * up; g.lg.x1 += hkx * up; g.lg.y0 -= hky * up; g.lg.y1 += hky * up;
  g.rg = IBox(g.lg.x0 + search.x0, g.lg.y0 + search.y0, g.lg.x1 + search.x0 + search.dx(), g.lg.y1 + search.y0 + search.dy());
  g.rmb = IBox(g.bbox.x0 + search.x0, g.bbox.y0 + search.y0, g.bbox.x1 + search.x0 + search.dx(), g.bbox.y1 + search.y0 + search.dy());
  return g;
}

// The buffers of ONE tile: sizes per level, and byte offsets inside the tile's slice of the arena.  The tiles of a group have the same
// sizes and live in slices at a fixed stride, so a kernel finds tile t's image at base + t * slice.
constexpr int PYR_MAX_LEVELS = 32;         // levels <= log2 of the search range, an int
constexpr int PYR_CS = 16;                 // ints per level-class cell: a cache line per level (same-line atomics queue up at the L2)
constexpr int PYR_NB = 256;                // workgroups per image of the nodata mean
struct PyrLayout {
  int L = 0;
  bool filtered = false;
  size_t lp[PYR_MAX_LEVELS], rp[PYR_MAX_LEVELS], lpf[PYR_MAX_LEVELS], rpf[PYR_MAX_LEVELS], lmp[PYR_MAX_LEVELS], rmp[PYR_MAX_LEVELS];
  int lpw[PYR_MAX_LEVELS], lph[PYR_MAX_LEVELS], rpw[PYR_MAX_LEVELS], rph[PYR_MAX_LEVELS];
  int lmw[PYR_MAX_LEVELS], lmh[PYR_MAX_LEVELS], rmw[PYR_MAX_LEVELS], rmh[PYR_MAX_LEVELS];
  size_t lmx = 0, rmx = 0, d_acc = 0, d_part = 0, d_cell = 0, d_cells = 0, disp = 0, disp2 = 0, padded = 0;
  size_t slice = 0;
};
// filtered: the levels are prefiltered into copies (lpf / rpf); otherwise lpf / rpf name the levels themselves
inline PyrLayout pyr_layout(TileGeom const& g, int L, bool filtered) {
  PyrLayout Y;
  Y.L = L; Y.filtered = filtered;
  size_t off = 0;
  auto take = [&off](size_t bytes) { off = (off + 255) / 256 * 256; const size_t p = off; off += bytes; return p; };
  const int bw = g.bbox.dx(), bh = g.bbox.dy();
  Y.lpw[0] = g.lg.dx(); Y.lph[0] = g.lg.dy(); Y.rpw[0] = g.rg.dx(); Y.rph[0] = g.rg.dy();
  Y.lmw[0] = bw; Y.lmh[0] = bh; Y.rmw[0] = g.rmb.dx(); Y.rmh[0] = g.rmb.dy();
  const size_t nl = (size_t)Y.lpw[0] * Y.lph[0], nr = (size_t)Y.rpw[0] * Y.rph[0];
  take(256);                                                      // (offset 0 stays unused: a null offset means "not there")
  Y.lp[0] = take(nl * 4); Y.rp[0] = take(nr * 4);
  Y.lmx = take(nl); Y.rmx = take(nr);
  Y.lmp[0] = take((size_t)bw * bh); Y.rmp[0] = take((size_t)Y.rmw[0] * Y.rmh[0]);
  Y.d_acc = take(4 * 8); Y.d_part = take(2 * 2 * PYR_NB * 8); Y.d_cell = take(8 * 4);
  for (int i = 1; i <= L; ++i) {
    Y.lpw[i] = 1 + (Y.lpw[i - 1] - 1) / 2; Y.lph[i] = 1 + (Y.lph[i - 1] - 1) / 2; Y.rpw[i] = 1 + (Y.rpw[i - 1] - 1) / 2; Y.rph[i] = 1 + (Y.rph[i - 1] - 1) / 2;
    Y.lmw[i] = 1 + (Y.lmw[i - 1] - 1) / 2; Y.lmh[i] = 1 + (Y.lmh[i - 1] - 1) / 2; Y.rmw[i] = 1 + (Y.rmw[i - 1] - 1) / 2; Y.rmh[i] = 1 + (Y.rmh[i - 1] - 1) / 2;
    Y.lp[i] = take((size_t)Y.lpw[i] * Y.lph[i] * 4); Y.rp[i] = take((size_t)Y.rpw[i] * Y.rph[i] * 4);
    Y.lmp[i] = take((size_t)Y.lmw[i] * Y.lmh[i]); Y.rmp[i] = take((size_t)Y.rmw[i] * Y.rmh[i]);
  }
  for (int i = 0; i <= L; ++i) {
    Y.lpf[i] = filtered ? take((size_t)Y.lpw[i] * Y.lph[i] * 4) : Y.lp[i];
    Y.rpf[i] = filtered ? take((size_t)Y.rpw[i] * Y.rph[i] * 4) : Y.rp[i];
  }
  Y.d_cells = take(PYR_CS * (size_t)(L + 1) * 4);
  Y.disp = take((size_t)bw * bh * 12); Y.disp2 = take((size_t)bw * bh * 12);
  Y.padded = take((size_t)(bw + 2) * (bh + 2) * 12);
  Y.slice = (off + 256 + 767) / 768 * 768;                        // a multiple of 12 (a disparity pixel), of 8 and of 256
  return Y;
}

// Class of a level, from the cell the float-grain kernel filled ({lowest set bit, largest exponent, flags} of both images): when the box
// sums of a level could round (exact), its zones are matched in the reference's own summation order (bm_exact.hip); integer imagery and
// most float imagery are order free and take the tile kernels.  f32: the window sums are exact in float32 as well (byte imagery under
// SAD, bm_zones.hip).  cert_hi != INT_MIN: the level is not order free but finite — its zones go through the tile kernels first, which
// certify every pixel against a bound on the difference to the reference's running sums and flag the zones that hold a pixel they
// cannot certify; only those are redone in the reference's order (certify == false: every zone of such a level).
struct LevelClass { bool exact = false, f32 = false; int cert_hi = INT_MIN; };
inline LevelClass level_class(int cost_type, int kx, int ky, const int* cell, bool certify) {
  LevelClass c;
  c.exact = !vwgpu_sums_order_free(cost_type, kx, ky, cell[0], cell[1], cell[2]);
  c.f32 = vwgpu_sums_bits(cost_type, kx, ky, cell[0], cell[1], cell[2]) <= 24;
  if (c.exact && certify && (cell[2] & 1) == 0 && cell[0] != INT_MAX      // (bit 0: a non-finite pixel; bit 1 only says "negative pixels")
      && cell[1] < 60 && cell[1] > -60)
    c.cert_hi = cell[1];
  return c;
}

// ---- zone tasks of a level -------------------------------------------------------------------------------------------
struct ZoneLevel { int rox, roy, hkx, hky, kx, ky, dw; };      // offset of the tile inside the level images, kernel, width of the level's disparity image
// the input boxes of a zone: lr in the left level image, rr in the right one (CorrelationView.cc:607-618)
inline void zone_boxes(SearchZone const& z, ZoneLevel const& g, IBox* lr, IBox* rr) {
  *lr = IBox(z.region.x0 + g.rox - g.hkx, z.region.y0 + g.roy - g.hky, z.region.x1 + g.rox + g.hkx, z.region.y1 + g.roy + g.hky);
  *rr = IBox(lr->x0 + z.range.x0, lr->y0 + z.range.y0, lr->x1 + z.range.x0 + z.range.dx(), lr->y1 + z.range.y0 + z.range.dy());
}
inline bool zone_is_empty(SearchZone const& z) { return z.region.dx() <= 0 || z.region.dy() <= 0 || z.range.dx() <= 0 || z.range.dy() <= 0; }

enum ZoneErr { ZONE_OK = 0, ZONE_TOO_LARGE = 1, ZONE_TABLES_TOO_LARGE = 2, ZONE_LR_TOO_LARGE = 3 };
// a: the L->R match of every zone; b: its R->L match (output: a dense rlw x rlh image at pixel offset `rl` of the R->L buffer);
// c: its L/R check.  rl: pixels of the R->L images so far.
struct ZoneTasks { std::vector<vwgpu_zone_task> a, b, c; size_t rl = 0; };
// Appends the tasks of one zone (an empty zone has none).  lr_active: the level ends with an L/R check (the a task then leaves the
// zone's range offset to the c task); with_rl: also append b and c (false only when a time budget cuts the list between the two).
// out_base: pixel offset of the tile's disparity image in the output buffer; img: the tile.  diff_ul: origin of the tile in an
// lr_disp_diff image — the (sx, sy) slots of a c task are the zone's origin there (ul_corner_offset, CorrelationView.cc:683-687) —
// or nullptr where there is no such image (zeros).
inline ZoneErr zone_tasks(SearchZone const& z, ZoneLevel const& g, bool lr_active, bool with_rl, long long out_base, int img, const int* diff_ul,
                          ZoneTasks* out) {
  if (zone_is_empty(z)) return ZONE_OK;
  IBox lr, rr;
  zone_boxes(z, g, &lr, &rr);
  const int zw = z.region.dx(), zh = z.region.dy(), sx = z.range.dx(), sy = z.range.dy();
  if (zw > 65535 * 32 || zh > 65535 * 32) return ZONE_TOO_LARGE;
  const long long out_off = out_base + (long long)z.region.y0 * g.dw + z.region.x0;
  if (out_off > INT32_MAX) return ZONE_TABLES_TOO_LARGE;
  const vwgpu_zone_task a{lr.x0, lr.y0, rr.x0, rr.y0, zw, zh, sx, sy, (int)out_off, g.dw, lr_active ? 0 : z.range.x0, lr_active ? 0 : z.range.y0, img};
  out->a.push_back(a);
  if (lr_active && with_rl) {
    const int rlw = rr.dx() - g.kx + 1, rlh = rr.dy() - g.ky + 1;
    out->b.push_back(vwgpu_zone_task{rr.x0, rr.y0, lr.x0 - sx, lr.y0 - sy, rlw, rlh, sx, sy, (int)out->rl, rlw, -sx, -sy, img});
    out->c.push_back(vwgpu_zone_task{(int)out->rl, 0, rlw, rlh, zw, zh, diff_ul ? z.region.x0 + diff_ul[0] : 0, diff_ul ? z.region.y0 + diff_ul[1] : 0,
                                     a.out_off, g.dw, z.range.x0, z.range.y0, img});
    out->rl += (size_t)rlw * rlh;
    if (out->rl > (size_t)INT32_MAX / 2) return ZONE_LR_TOO_LARGE;
  }
  return ZONE_OK;
}

// ---- the "cannot matter" certificate of the certified passes (bm_zones.hip, ZEdge) and its premises -------------------
// L->R: a mask pass follows the clean-up filter (both sit behind filter_half_kernel > 0, CorrelationView.cc:702-744) and erases a pixel
// that points outside the right image; the filters before it compare disparities within 3 px over +- half kernel, hence the margin; no
// lr_disp_diff image (its entries keep the discrepancy of pixels the filters removed).  R->L: read by the L/R check alone.
// Margin.  Last level: ONE filter pass (rm_outliers, hk x hk, 3 px) — a far pixel M must not be counted by a pixel that can survive the
// mask, i.e. |dx(M) - dx(N)| > 3 for every N within hk columns whose target lies inside: hk + 3 + 1.  Intermediate levels:
// disparity_cleanup_using_thresh is TWO passes (inner (hk, hk, 3, 0.5), then outer (1, 1, 3, 0.2) on the inner pass's output,
// DisparityMap.h:427-441): a kept pixel K (target inside) has an outer-pass neighbour N within 1 column and 3 px — N's target up to 4
// columns outside — whose inner-pass count sees M within hk columns and 3 px: M's target up to hk + 7 columns outside must still be
// treated as "can matter", so far starts at hk + 8.
struct EdgeMargins { int m_lr, m_rl, lr_lo, lr_hi, rl_lo, rl_hi; };
// rmb_x0: left edge of the tile's right-mask crop in the right image (width rw); rmask_w0: width of that crop; dw: width of the level
inline EdgeMargins edge_margins(const vwgpu_pyramid_params* P, bool last, bool has_lr_diff, int level, int rmb_x0, int rmask_w0, int rw, int dw) {
  EdgeMargins e;
  e.m_lr = (P->filter_half_kernel > 0 && !(last && has_lr_diff)) ? P->filter_half_kernel + (last ? 4 : 8) : 0;
  e.m_rl = (P->consistency_threshold >= 0 && P->consistency_threshold < 1e6) ? (int)std::floor(P->consistency_threshold) + 2 : 0;
  // columns of the right mask of this level that can be non-zero: the part of the crop inside the right image, halved per level the way
  // subsample_mask_by_two does (a column is kept when one of its two source columns is)
  const int rv0 = std::max(0, -rmb_x0) >> level, rv1 = (std::min(rmask_w0, rw - rmb_x0) + (1 << level) - 1) >> level;
  e.lr_lo = rv0 - e.m_lr + 1; e.lr_hi = rv1 + e.m_lr - 2;
  e.rl_lo = -e.m_rl + 1; e.rl_hi = dw + e.m_rl - 2;              // the left pixels of the check lie in the tile: [0, dw)
  return e;
}

// the zones of a level become those of the next finer one (CorrelationView.cc:781-799)
inline void rescale_zones(std::vector<SearchZone>& zones, IBox const& next_size, IBox const& scale_search, IBox const& search) {
  for (SearchZone& z : zones) {
    z.region.scale(2);
    z.region.clip(next_size);
    z.range.scale(2);
    z.range.expand(2);
    z.range.clip(scale_search);
    if (z.range.empty()) z.range = IBox(0, 0, search.width(), search.height());
  }
}

}  // namespace vwgpu
