// corr_eval_ref.cc — CPU restatement of vw::stereo::CorrEval::prerasterize (src/vw/Stereo/CorrEval.cc:139-317) for the
// tests of corr_eval.hip (test infrastructure only).  Written from the reference's semantics, box by box as the reference
// runs: the box's right_box from its sampled valid pixels with BBox2i's grow / expand rules, real in-memory crops
// crop(edge_extend(image, nodata), box) of both images, calc_patches into patch arrays, then calc_ncc / calc_stddev on
// the patches.  The rows of a box are shared among `threads` threads (its pixels do not depend on each other).
// Defined where the reference is not (include/vwgpu.h): reads outside an empty right crop are nodata; a non-finite
// sampled valid disparity, a coordinate or box outside int32, sample_rate < 1 and a negative padding are errors.
#include <climits>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

namespace {

struct Px {
  float v;
  bool ok;
};

// crop(edge_extend(image, nodata), [x0, x0 + cw) x [y0, y0 + ch)) held in memory; nodata = {0, invalid}
struct Crop {
  long long x0 = 0, y0 = 0, cw = 0, ch = 0;
  std::vector<Px> px;
  Crop(const float* v, const uint8_t* m, int w, int h, long long bx0, long long by0, long long bw, long long bh)
      : x0(bx0), y0(by0), cw(bw > 0 ? bw : 0), ch(bh > 0 ? bh : 0), px((size_t)(cw * ch)) {
    for (long long y = 0; y < ch; ++y)
      for (long long x = 0; x < cw; ++x) {
        const long long gx = x0 + x, gy = y0 + y;
        Px p{0.f, false};
        if (gx >= 0 && gy >= 0 && gx < w && gy < h) {
          const size_t o = (size_t)(gy * w + gx);
          p = {v[o], m ? m[o] != 0 : true};
        }
        px[(size_t)(y * cw + x)] = p;
      }
  }
  bool contains(long long x, long long y) const { return x >= 0 && y >= 0 && x < cw && y < ch; }
  // ImageView access; the reference's round_to_int read of an empty crop is undefined, defined here as nodata
  Px at(long long x, long long y) const { return contains(x, y) ? px[(size_t)(y * cw + x)] : Px{0.f, false}; }
};

// math::impl::_floor (Math/Functions.h:74-81)
int32_t vw_floor(double val) {
  if (val < 0) {
    const int32_t iv = (int32_t)val;
    return (double)iv == val ? iv : iv - 1;
  }
  return (int32_t)val;
}

// interpolate(crop, BilinearInterpolation(), nodata) at (i, j): BilinearInterpolationImpl with PixelMask<float>
// (Interpolation.h:76-106): the integer shortcut on the doubles, float weights, children blended regardless of
// validity, validity ANDed
Px bilinear(const Crop& R, double i, double j) {
  const int32_t x = vw_floor(i), y = vw_floor(j);
  if (x == i && y == j) return R.at(x, y);
  const float normx = float(i) - float(x), normy = float(j) - float(y), norm1mx = 1 - normx, norm1my = 1 - normy;
  const Px a = R.at(x, y), b = R.at((long long)x + 1, y), c = R.at(x, (long long)y + 1), d = R.at((long long)x + 1, (long long)y + 1);
  float result = a.v * norm1mx;
  result += b.v * normx;
  result *= norm1my;
  float row = c.v * norm1mx;
  row += d.v * normx;
  result += row * normy;
  return {result, a.ok && b.ok && c.ok && d.ok};
}

struct Box {
  int x, y, w, h;
};

// calc_patches (CorrEval.cc:15-69); patches indexed [c * ky + r].  Returns false where the reference throws.
bool calc_patches(const Box& bbox, int kx, int ky, bool round_to_int, float dx, float dy, const Crop& L, const Crop& R,
                  int col, int row, Px* lp, Px* rp) {
  const int hx = kx / 2, hy = ky / 2;
  for (int c = 0; c < kx; ++c)
    for (int r = 0; r < ky; ++r) {
      long long lx = (long long)col + bbox.x + c - hx, ly = (long long)row + bbox.y + r - hy;
      double rx = double(lx) + double(dx), ry = double(ly) + double(dy);
      lx -= L.x0;
      ly -= L.y0;
      rx -= double(R.x0);
      ry -= double(R.y0);
      if (!L.contains(lx, ly)) return false;
      lp[c * ky + r] = L.at(lx, ly);
      rp[c * ky + r] = round_to_int ? R.at((int32_t)rx, (int32_t)ry) : bilinear(R, rx, ry);
    }
  return true;
}

double calc_ncc(const Px* lp, const Px* rp, int n) {
  double num = 0.0, den1 = 0.0, den2 = 0.0;
  for (int k = 0; k < n; ++k) {   // c outer, r inner; the reference's validity test always passes
    const double a = lp[k].v, b = rp[k].v;
    num += a * b;
    den1 += a * a;
    den2 += b * b;
  }
  if (den1 > 0.0 && den2 > 0.0) return num / std::sqrt(den1 * den2);
  return -1.0;
}

double calc_stddev(const Px* p, int n) {
  int num = 0;
  double mean = 0.0;
  for (int k = 0; k < n; ++k)
    if (p[k].ok) {
      num += 1;
      mean += p[k].v;
    }
  if (num == 0) return -1.0;
  mean /= num;
  double sum = 0.0;
  num = 0;
  for (int k = 0; k < n; ++k)
    if (p[k].ok) {
      num += 1;
      sum += (p[k].v - mean) * (p[k].v - mean);
    }
  if (num == 0) return -1.0;
  return std::sqrt(sum / num);
}

struct Call {
  const float *disp, *left, *right;
  const uint8_t *lv, *rv;
  int w, h, rw, rh, kx, ky, metric, rate;
  bool round_to_int;
  int pad;
  float* out;
};

// one prerasterize(bbox); returns 0 or an error code of cer_corr_eval
int prerasterize(const Call& k, const Box& bbox, int threads, long long* stats) {
  const int bw = bbox.w, bh = bbox.h;
  std::vector<float> ddx((size_t)bw * bh), ddy((size_t)bw * bh);
  std::vector<char> dv((size_t)bw * bh);
  for (int row = 0; row < bh; ++row)
    for (int col = 0; col < bw; ++col) {
      const float* d = k.disp + ((size_t)(bbox.y + row) * k.w + bbox.x + col) * 3;
      const size_t o = (size_t)row * bw + col;
      ddx[o] = k.round_to_int ? std::round(d[0]) : d[0];   // CorrEval.cc:145-151: every pixel, validity unchanged
      ddy[o] = k.round_to_int ? std::round(d[1]) : d[1];
      dv[o] = d[2] != 0.f;
    }
  const int32_t big = INT_MAX - 1;   // BBox2i() (Math/BBox.tcc:38-45)
  long long mn[2] = {big, big}, mx[2] = {-big, -big};
  for (int col = 0; col < bw; ++col)
    for (int row = 0; row < bh; ++row) {
      const size_t o = (size_t)row * bw + col;
      if (!dv[o] || col % k.rate != 0 || row % k.rate != 0) continue;
      if (!std::isfinite(ddx[o]) || !std::isfinite(ddy[o])) return 2;
      const double px = (double(bbox.x) + double(col)) + double(ddx[o]), py = (double(bbox.y) + double(row)) + double(ddy[o]);
      const double pts[2][2] = {{std::floor(px), std::floor(py)}, {std::ceil(px), std::ceil(py)}};
      for (const auto& p : pts) {
        if (p[0] < INT_MIN || p[0] > INT_MAX || p[1] < INT_MIN || p[1] > INT_MAX) return 3;
        for (int a = 0; a < 2; ++a) {   // BBox::grow (Math/BBox.tcc:82-97)
          if (p[a] > mx[a]) mx[a] = (long long)p[a];
          if (p[a] < mn[a]) mn[a] = (long long)p[a];
        }
      }
    }
  const bool grown = mn[0] <= mx[0];
  auto empty = [&]() { return mn[0] >= mx[0] || mn[1] >= mx[1]; };
  const bool curvature = k.metric >= 2;
  const long long ex[5][2] = {{k.kx / 2, k.ky / 2}, {1, 1}, {2, 2}, {k.pad, k.pad}, {curvature ? 1 : 0, curvature ? 1 : 0}};
  for (const auto& e : ex) {   // BBox::expand does nothing on an empty box (Math/BBox.tcc:228-246)
    if (empty()) break;
    mn[0] -= e[0]; mn[1] -= e[1]; mx[0] += e[0]; mx[1] += e[1];
  }
  if (mn[0] < INT_MIN || mn[1] < INT_MIN || mx[0] > INT_MAX || mx[1] > INT_MAX || mx[0] - mn[0] > INT_MAX ||
      mx[1] - mn[1] > INT_MAX)
    return 3;
  if (stats && grown && empty()) stats[3] += 1;
  const int hx = k.kx / 2, hy = k.ky / 2;
  const Crop L(k.left, k.lv, k.w, k.h, (long long)bbox.x - hx - k.pad, (long long)bbox.y - hy - k.pad,
               (long long)bw + 2 * (hx + k.pad), (long long)bh + 2 * (hy + k.pad));
  const Crop R(k.right, k.rv, k.rw, k.rh, mn[0], mn[1], mx[0] - mn[0], mx[1] - mn[1]);
  const int n = k.kx * k.ky;
  std::vector<long long> cnt((size_t)threads * 2, 0);
  std::vector<int> fail((size_t)threads, 0);
  auto work = [&](int t) {
    std::vector<Px> lp(n), rp(n), nl(n), nr(n);
    for (int row = t; row < bh; row += threads)
      for (int col = 0; col < bw; ++col) {
        float* o = k.out + ((size_t)(bbox.y + row) * k.w + bbox.x + col) * 2;
        o[0] = 0.f;   // the tile starts invalid (CorrEval.cc:239-241)
        o[1] = 0.f;
        const size_t q = (size_t)row * bw + col;
        if (!dv[q] || col % k.rate != 0 || row % k.rate != 0) continue;
        cnt[2 * t] += 1;
        const float dx = ddx[q], dy = ddy[q];
        if (!calc_patches(bbox, k.kx, k.ky, k.round_to_int, dx, dy, L, R, col, row, lp.data(), rp.data())) {
          fail[t] = 4;
          return;
        }
        bool valid = false;
        double value = 0.0;
        if (k.metric == 0) {
          value = calc_ncc(lp.data(), rp.data(), n);
          valid = value >= 0;
        } else if (k.metric == 1) {
          const double ls = calc_stddev(lp.data(), n), rs = calc_stddev(rp.data(), n);
          if (ls >= 0.0 && rs >= 0.0) {
            valid = true;
            value = (ls + rs) / 2.0;
          }
        } else {
          const double C = calc_ncc(lp.data(), rp.data(), n);
          if (C >= 0) {
            const float shifts[4][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}};
            double nbr[4];
            bool ok = true;
            for (int s = 0; s < 4 && ok; ++s) {
              const float sdx = dx + shifts[s][0], sdy = dy + shifts[s][1];   // Vector2f += Vector2f
              if (!calc_patches(bbox, k.kx, k.ky, k.round_to_int, sdx, sdy, L, R, col, row, nl.data(), nr.data())) {
                fail[t] = 4;
                return;
              }
              nbr[s] = calc_ncc(nl.data(), nr.data(), n);
              if (nbr[s] < 0) ok = false;
            }
            if (ok) {
              const double kxc = 2.0 * C - nbr[0] - nbr[1], kyc = 2.0 * C - nbr[2] - nbr[3];
              if (kxc > 0 && kyc > 0) {
                double sigma = std::sqrt(1.0 / kxc + 1.0 / kyc);
                if (k.metric == 3) {
                  double resid = 1.0 - C;
                  if (resid < 0) resid = 0;
                  sigma *= std::sqrt(resid);
                }
                valid = true;
                value = sigma;
              }
            }
          }
        }
        if (valid) {
          o[0] = (float)value;
          o[1] = 1.f;
          cnt[2 * t + 1] += 1;
        }
      }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; ++t) pool.emplace_back(work, t);
  work(0);
  for (auto& th : pool) th.join();
  for (int t = 0; t < threads; ++t) {
    if (fail[t]) return fail[t];
    if (stats) {
      stats[0] += cnt[2 * t];
      stats[1] += cnt[2 * t + 1];
    }
  }
  return 0;
}

}  // namespace

extern "C" {

// metric: 0 ncc, 1 stddev, 2 parabola_curvature, 3 cramer_rao.  Pixels outside the tiles are not written.
// Returns 0, 1 (argument: kernel, metric, sample_rate, padding), 2 (non-finite sampled valid disparity), 3 (coordinate or
// right box outside int32) or 4 (a patch leaves its left crop: the reference throws).  stats: 4 counters as vwgpu_corr_eval.
int cer_corr_eval(const float* disp, int w, int h, const float* left, const uint8_t* left_valid, const float* right,
                  const uint8_t* right_valid, int rw, int rh, int kx, int ky, int metric, int sample_rate, int round_to_int,
                  int prefilter_mode, float prefilter_kernel_width, const int* tiles, int ntiles, float* out, int threads,
                  long long* stats) {
  (void)prefilter_mode;
  if (kx <= 0 || ky <= 0 || kx % 2 != 1 || ky % 2 != 1) return 1;
  if (metric < 0 || metric > 3 || sample_rate < 1) return 1;
  if (!std::isfinite(prefilter_kernel_width) || std::ceil((double)prefilter_kernel_width) < -5.0 ||
      std::ceil((double)prefilter_kernel_width) > (double)(INT_MAX - 5))
    return 1;
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  const Call k{disp, left, right, left_valid, right_valid, w, h, rw, rh, kx, ky, metric, sample_rate, round_to_int != 0,
               (int)std::ceil(prefilter_kernel_width) + 5, out};
  for (int t = 0; t < ntiles; ++t) {
    const Box b{tiles[4 * t], tiles[4 * t + 1], tiles[4 * t + 2], tiles[4 * t + 3]};
    const int rc = prerasterize(k, b, threads < 1 ? 1 : threads, stats);
    if (rc) return rc;
    if (stats) stats[2] += 1;
  }
  return 0;
}

}  // extern "C"
