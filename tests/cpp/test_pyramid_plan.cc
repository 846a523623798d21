// The host plan of the pyramid correlator (visionworkbench_amd/csrc/pyramid_plan.h) on its own: level counts, the slice layout, the zone
// tasks of a level and the zone rescale.  A plain program: no device, no library; built with the address and undefined-behaviour sanitizers.
#include "pyramid_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace vwgpu;

static int failures = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { ++failures; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static vwgpu_pyramid_params params(int kx, int ky, int dx, int dy, int max_levels) {
  vwgpu_pyramid_params P{};
  P.kernel_x = kx; P.kernel_y = ky;
  P.search_min_x = 0; P.search_min_y = 0; P.search_max_x = dx; P.search_max_y = dy;
  P.max_pyramid_levels = max_levels;
  return P;
}

static void test_levels() {
  const int rows[][8] = {{1024, 1024, 11, 11, 128, 2, 5, 5}, {1024, 1024, 11, 11, 128, 2, 8, 6}, {96, 110, 7, 7, 17, 3, 2, 2},
                         {20, 20, 11, 11, 64, 64, 5, 0},     {150, 140, 7, 7, 25, 5, 3, 3},      {300, 200, 5, 5, 1, 1, 5, 0},
                         {300, 200, 5, 5, 61, 1, 5, 4},      {64, 64, 7, 7, 4, 4, 5, 1},         {64, 64, 7, 7, 8, 8, 5, 2}};
  for (auto const& r : rows) {
    const vwgpu_pyramid_params P = params(r[2], r[3], r[4], r[5], r[6]);
    const int L = pyramid_levels(&P, r[0], r[1]);
    if (L != r[7]) std::printf("levels(%d x %d, kernel %d x %d, search %d x %d, max %d) = %d, expected %d\n", r[0], r[1], r[2], r[3], r[4], r[5], r[6], L, r[7]);
    CHECK(L == r[7]);
  }
}

struct Buf { size_t off, bytes; };

static void test_layout() {
  const int shapes[][7] = {{1024, 1024, 11, 11, 128, 2, 5}, {96, 110, 7, 7, 17, 3, 2}, {150, 140, 7, 7, 25, 5, 3}};
  for (auto const& s : shapes)
    for (int filtered = 0; filtered < 2; ++filtered) {
      vwgpu_pyramid_params P = params(s[2], s[3], s[4], s[5], s[6]);
      P.search_min_x = -s[4] / 2; P.search_max_x = P.search_min_x + s[4];
      const IBox search(P.search_min_x, P.search_min_y, P.search_max_x, P.search_max_y);
      const int bw = s[0], bh = s[1], L = pyramid_levels(&P, bw, bh);
      const TileGeom g = tile_geom(37, 11, bw, bh, search, s[2] / 2, s[3] / 2, 1 << L);
      CHECK(g.lg.dx() == bw + 2 * (s[2] / 2) * (1 << L) && g.rg.dx() == g.lg.dx() + search.dx() && g.rmb.dx() == bw + search.dx());
      CHECK(g.rg.x0 == g.lg.x0 + search.x0 && g.rmb.y0 == g.bbox.y0 + search.y0 && g.rmb.dy() == bh + search.dy());
      const PyrLayout Y = pyr_layout(g, L, filtered != 0);
      CHECK(Y.L == L && Y.filtered == (filtered != 0));
      CHECK(Y.lpw[0] == g.lg.dx() && Y.lph[0] == g.lg.dy() && Y.rpw[0] == g.rg.dx() && Y.rph[0] == g.rg.dy());
      CHECK(Y.lmw[0] == bw && Y.lmh[0] == bh && Y.rmw[0] == g.rmb.dx() && Y.rmh[0] == g.rmb.dy());
      std::vector<Buf> bufs;
      const size_t nl = (size_t)Y.lpw[0] * Y.lph[0], nr = (size_t)Y.rpw[0] * Y.rph[0];
      bufs.push_back({Y.lmx, nl}); bufs.push_back({Y.rmx, nr});
      bufs.push_back({Y.d_acc, 4 * sizeof(double)}); bufs.push_back({Y.d_part, 2 * 2 * PYR_NB * sizeof(double)}); bufs.push_back({Y.d_cell, 8 * sizeof(int)});
      bufs.push_back({Y.d_cells, PYR_CS * (size_t)(L + 1) * sizeof(int)});
      bufs.push_back({Y.disp, (size_t)bw * bh * 12}); bufs.push_back({Y.disp2, (size_t)bw * bh * 12}); bufs.push_back({Y.padded, (size_t)(bw + 2) * (bh + 2) * 12});
      for (int i = 0; i <= L; ++i) {
        if (i > 0) {
          CHECK(Y.lpw[i] == 1 + (Y.lpw[i - 1] - 1) / 2 && Y.lph[i] == 1 + (Y.lph[i - 1] - 1) / 2);
          CHECK(Y.rpw[i] == 1 + (Y.rpw[i - 1] - 1) / 2 && Y.rph[i] == 1 + (Y.rph[i - 1] - 1) / 2);
          CHECK(Y.lmw[i] == 1 + (Y.lmw[i - 1] - 1) / 2 && Y.lmh[i] == 1 + (Y.lmh[i - 1] - 1) / 2);
          CHECK(Y.rmw[i] == 1 + (Y.rmw[i - 1] - 1) / 2 && Y.rmh[i] == 1 + (Y.rmh[i - 1] - 1) / 2);
        }
        bufs.push_back({Y.lp[i], (size_t)Y.lpw[i] * Y.lph[i] * 4}); bufs.push_back({Y.rp[i], (size_t)Y.rpw[i] * Y.rph[i] * 4});
        bufs.push_back({Y.lmp[i], (size_t)Y.lmw[i] * Y.lmh[i]}); bufs.push_back({Y.rmp[i], (size_t)Y.rmw[i] * Y.rmh[i]});
        if (filtered) { bufs.push_back({Y.lpf[i], (size_t)Y.lpw[i] * Y.lph[i] * 4}); bufs.push_back({Y.rpf[i], (size_t)Y.rpw[i] * Y.rph[i] * 4}); }
        else CHECK(Y.lpf[i] == Y.lp[i] && Y.rpf[i] == Y.rp[i]);
      }
      CHECK(Y.slice % 768 == 0);
      for (size_t a = 0; a < bufs.size(); ++a) {
        CHECK(bufs[a].off != 0 && bufs[a].off % 256 == 0);
        CHECK(bufs[a].off + bufs[a].bytes <= Y.slice);
        for (size_t b = a + 1; b < bufs.size(); ++b)
          CHECK(bufs[a].off + bufs[a].bytes <= bufs[b].off || bufs[b].off + bufs[b].bytes <= bufs[a].off);
      }
    }
}

// disjoint zones inside dw x dh: the cells of a jittered grid, each shrunk at random; some of them empty (in the region or in the range)
static std::vector<SearchZone> random_zones(std::mt19937& rng, int dw, int dh, int cols, int rows) {
  std::vector<SearchZone> zones;
  auto rnd = [&rng](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  for (int j = 0; j < rows; ++j)
    for (int i = 0; i < cols; ++i) {
      const int cx0 = dw * i / cols, cx1 = dw * (i + 1) / cols, cy0 = dh * j / rows, cy1 = dh * (j + 1) / rows;
      SearchZone z;
      const int x0 = rnd(cx0, cx1 - 1), y0 = rnd(cy0, cy1 - 1);
      z.region = IBox(x0, y0, rnd(x0 + 1, cx1), rnd(y0 + 1, cy1));
      const int rx = rnd(-9, 3), ry = rnd(-3, 1);
      z.range = IBox(rx, ry, rx + rnd(1, 12), ry + rnd(1, 4));
      const int kind = rnd(0, 9);
      if (kind == 0) z.region.x1 = z.region.x0;                  // an empty region
      if (kind == 1) z.range.y1 = z.range.y0;                    // an empty range
      zones.push_back(z);
    }
  return zones;
}

static void test_zone_tasks() {
  std::mt19937 rng(20240521u);
  const int dw = 301, dh = 187;
  const ZoneLevel g{6, 6, 3, 3, 7, 7, dw};
  const int diff_ul[2] = {40, 25};
  for (int lr_active = 0; lr_active < 2; ++lr_active)
    for (int with_ul = 0; with_ul < 2; ++with_ul) {
      const std::vector<SearchZone> zones = random_zones(rng, dw, dh, 20, 15);      // 300 zones
      const long long out_base = with_ul ? 0 : 5 * (long long)(dw * dh + 77);
      const int img = with_ul ? 0 : 5;
      ZoneTasks zt;
      std::vector<size_t> src;                      // the zone of every a task
      for (size_t k = 0; k < zones.size(); ++k) {
        const size_t before = zt.a.size();
        CHECK(zone_tasks(zones[k], g, lr_active != 0, true, out_base, img, with_ul ? diff_ul : nullptr, &zt) == ZONE_OK);
        if (zone_is_empty(zones[k])) CHECK(zt.a.size() == before);                     // empty zones produce nothing
        else { CHECK(zt.a.size() == before + 1); src.push_back(k); }
      }
      CHECK(zt.b.size() == (lr_active ? zt.a.size() : 0) && zt.c.size() == zt.b.size());
      size_t rl = 0;
      for (size_t i = 0; i < zt.a.size(); ++i) {
        const vwgpu_zone_task& a = zt.a[i];
        const SearchZone& z = zones[src[i]];
        // the output rectangle: inside the level, and the zone's own
        const long long rel = a.out_off - out_base;
        const int ox = (int)(rel % dw), oy = (int)(rel / dw);
        CHECK(rel >= 0 && ox == z.region.x0 && oy == z.region.y0 && a.zw == z.region.dx() && a.zh == z.region.dy());
        CHECK(ox >= 0 && oy >= 0 && ox + a.zw <= dw && oy + a.zh <= dh && a.out_stride == dw && a.img == img);
        CHECK(a.sx == z.range.dx() && a.sy == z.range.dy());
        CHECK(a.ax == z.region.x0 + g.rox - g.hkx && a.ay == z.region.y0 + g.roy - g.hky && a.bx == a.ax + z.range.x0 && a.by == a.ay + z.range.y0);
        CHECK(a.addx == (lr_active ? 0 : z.range.x0) && a.addy == (lr_active ? 0 : z.range.y0));
        for (size_t j = i + 1; j < zt.a.size(); ++j) {       // disjoint from every other zone's
          const vwgpu_zone_task& o = zt.a[j];
          const int px = (int)((o.out_off - out_base) % dw), py = (int)((o.out_off - out_base) / dw);
          CHECK(ox + a.zw <= px || px + o.zw <= ox || oy + a.zh <= py || py + o.zh <= oy);
        }
        if (lr_active) {
          const vwgpu_zone_task &b = zt.b[i], &c = zt.c[i];
          const int rlw = a.zw + 2 * g.hkx + a.sx - g.kx + 1, rlh = a.zh + 2 * g.hky + a.sy - g.ky + 1;
          CHECK(b.zw == rlw && b.zh == rlh && b.out_stride == rlw && (size_t)b.out_off == rl);      // running sums of rlw * rlh
          CHECK(b.ax == a.bx && b.ay == a.by && b.bx == a.ax - a.sx && b.by == a.ay - a.sy && b.sx == a.sx && b.sy == a.sy && b.addx == -a.sx && b.addy == -a.sy);
          CHECK(c.out_off == a.out_off && (size_t)c.ax == rl && c.bx == rlw && c.by == rlh && c.zw == a.zw && c.zh == a.zh && c.out_stride == dw);
          CHECK(c.addx == z.range.x0 && c.addy == z.range.y0 && b.img == img && c.img == img);
          CHECK(c.sx == (with_ul ? z.region.x0 + diff_ul[0] : 0) && c.sy == (with_ul ? z.region.y0 + diff_ul[1] : 0));
          rl += (size_t)rlw * rlh;
        }
      }
      CHECK(zt.rl == rl);
    }
  // a time budget may cut the list between a zone's two runs: the a task alone
  {
    ZoneTasks zt;
    const SearchZone z{IBox(3, 4, 20, 30), IBox(-2, 0, 5, 2)};
    CHECK(zone_tasks(z, g, true, false, 0, 0, nullptr, &zt) == ZONE_OK);
    CHECK(zt.a.size() == 1 && zt.b.empty() && zt.c.empty() && zt.rl == 0 && zt.a[0].addx == 0 && zt.a[0].addy == 0);
  }
  // the three limits
  {
    const ZoneLevel wide{0, 0, 0, 0, 1, 1, 65535 * 32 + 1};
    ZoneTasks zt;
    CHECK(zone_tasks(SearchZone{IBox(0, 0, 65535 * 32, 1), IBox(0, 0, 1, 1)}, wide, false, true, 0, 0, nullptr, &zt) == ZONE_OK && zt.a.size() == 1);
    CHECK(zone_tasks(SearchZone{IBox(0, 0, 65535 * 32 + 1, 1), IBox(0, 0, 1, 1)}, wide, false, true, 0, 0, nullptr, &zt) == ZONE_TOO_LARGE);
    CHECK(zone_tasks(SearchZone{IBox(0, 0, 1, 65535 * 32 + 1), IBox(0, 0, 1, 1)}, wide, false, true, 0, 0, nullptr, &zt) == ZONE_TOO_LARGE && zt.a.size() == 1);
  }
  {
    const ZoneLevel lv{0, 0, 0, 0, 1, 1, 100};
    const SearchZone z{IBox(7, 2, 9, 3), IBox(0, 0, 1, 1)};           // out_off = out_base + 207
    ZoneTasks zt;
    CHECK(zone_tasks(z, lv, false, true, (long long)INT32_MAX - 207, 3, nullptr, &zt) == ZONE_OK && zt.a.size() == 1 && zt.a[0].out_off == INT32_MAX);
    CHECK(zone_tasks(z, lv, false, true, (long long)INT32_MAX - 206, 3, nullptr, &zt) == ZONE_TABLES_TOO_LARGE && zt.a.size() == 1);
  }
  {
    const ZoneLevel lv{0, 0, 0, 0, 1, 1, 40000};
    const SearchZone z{IBox(0, 0, 32766, 32766), IBox(0, 0, 1, 1)};   // an R->L image of 32767^2 = 2^30 - 65535 pixels
    ZoneTasks zt;
    zt.rl = 65534;                                                     // the sum reaches INT32_MAX / 2 = 2^30 - 1: still fine
    CHECK(zone_tasks(z, lv, true, true, 0, 0, nullptr, &zt) == ZONE_OK && zt.rl == (size_t)INT32_MAX / 2);
    ZoneTasks zu;
    zu.rl = 65535;
    CHECK(zone_tasks(z, lv, true, true, 0, 0, nullptr, &zu) == ZONE_LR_TOO_LARGE);
  }
}

static void test_edge_margins() {
  vwgpu_pyramid_params P = params(7, 7, 20, 3, 3);
  P.filter_half_kernel = 3; P.consistency_threshold = 2.5f;
  // a tile whose right-mask crop starts 10 columns left of the right image (width 500) and is 120 wide, level 1, 50 columns
  EdgeMargins e = edge_margins(&P, false, false, 1, -10, 120, 500, 50);
  CHECK(e.m_lr == 11 && e.m_rl == 4 && e.lr_lo == 5 - 11 + 1 && e.lr_hi == 60 + 11 - 2 && e.rl_lo == -3 && e.rl_hi == 52);
  e = edge_margins(&P, true, false, 0, 450, 120, 500, 100);
  CHECK(e.m_lr == 7 && e.lr_lo == -6 && e.lr_hi == 50 + 7 - 2);
  CHECK(edge_margins(&P, true, true, 0, 450, 120, 500, 100).m_lr == 0 && edge_margins(&P, false, true, 1, 450, 120, 500, 100).m_lr == 11);
  P.filter_half_kernel = 0; P.consistency_threshold = -1.0f;
  e = edge_margins(&P, false, false, 1, 0, 120, 500, 50);
  CHECK(e.m_lr == 0 && e.m_rl == 0);
}

static void test_rescale() {
  const IBox search(-8, -1, 9, 2), next_size(0, 0, 101, 77), scale_search(0, 0, 17, 3);
  std::vector<SearchZone> zones;
  zones.push_back(SearchZone{IBox(10, 5, 60, 40), IBox(2, 0, 5, 1)});
  zones.push_back(SearchZone{IBox(0, 0, 10, 5), IBox(20, 4, 24, 6)});      // its range leaves the search after scaling: empty once clipped
  zones.push_back(SearchZone{IBox(3, 3, 4, 4), IBox()});                   // an empty range stays empty through scale / expand
  rescale_zones(zones, next_size, scale_search, search);
  CHECK(zones[0].region.same(IBox(20, 10, 101, 77)) && zones[0].range.same(IBox(2, 0, 12, 3)));
  CHECK(zones[1].region.same(IBox(0, 0, 20, 10)) && zones[1].range.same(IBox(0, 0, search.width(), search.height())));
  CHECK(zones[2].region.same(IBox(6, 6, 8, 8)) && zones[2].range.same(IBox(0, 0, 17, 3)));
}

int main() {
  test_levels();
  test_layout();
  test_zone_tasks();
  test_edge_margins();
  test_rescale();
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
