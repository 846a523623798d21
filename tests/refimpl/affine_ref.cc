// affine_ref.cc — TEST INFRASTRUCTURE ONLY: a sequential CPU restatement of
// vw::stereo::PyramidSubpixelView::prerasterize with SUBPIXEL_FAST_AFFINE (src/vw/Stereo/SubpixelView.cc:33-224)
// and of subpixel_optimized_affine_2d (src/vw/Stereo/Correlate.cc:848-1200), one tile at a time, statement order kept.
// The prefiltered crops come from the CPU parity oracle (vwo_prefilter_region, oracle/vw_oracle.h).
//
// Layouts: images row-major float; disparity w x h x {dx, dy, valid} float (valid != 0 is valid).
// Output: only the pixels of the tiles are written: refined {dx, dy, 1}, invalid {0, 0, 0}.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../oracle/vw_oracle.h"
#include "tile_range.h"

namespace {

struct DImg {  // PixelMask<Vector2f> image
  int w = 0, h = 0;
  std::vector<float> dx, dy;
  std::vector<uint8_t> v;
  void resize(int W, int H) { w = W; h = H; dx.assign((size_t)W * H, 0.f); dy.assign((size_t)W * H, 0.f); v.assign((size_t)W * H, 0); }
  size_t at(int x, int y) const { return (size_t)y * w + x; }
};

struct FImg {
  int w = 0, h = 0;
  std::vector<float> p;
  void resize(int W, int H) { w = W; h = H; p.assign((size_t)W * H, 0.f); }
  float at(int x, int y) const { return p[(size_t)y * w + x]; }
  float clamped(int x, int y) const {  // ConstantEdgeExtension
    x = x < 0 ? 0 : (x >= w ? w - 1 : x);
    y = y < 0 ? 0 : (y >= h ? h - 1 : y);
    return at(x, y);
  }
  float zero_ext(int x, int y) const { return (x < 0 || y < 0 || x >= w || y >= h) ? 0.f : at(x, y); }
};

// subsample(img, 2) (src/vw/Image/Manipulation.h:214-293): 1 + (n - 1) / 2 samples per axis, no smoothing.
FImg subsample2(const FImg& s) {
  FImg d;
  d.resize(1 + (s.w - 1) / 2, 1 + (s.h - 1) / 2);
  for (int y = 0; y < d.h; ++y)
    for (int x = 0; x < d.w; ++x) d.p[(size_t)y * d.w + x] = s.at(2 * x, 2 * y);
  return d;
}

// disparity_subsample (src/vw/Stereo/DisparityMap.h:1253-1324) over a ConstantEdgeExtension child.  The
// accumulator is double (AccumulatorType<float>); the first three terms convert the pixel before the product, the
// others multiply in float (int * PixelMask<Vector2f>) and then add to the double buffer.
DImg disparity_subsample(const DImg& s) {
  DImg d;
  d.resize(1 + (s.w - 1) / 2, 1 + (s.h - 1) / 2);
  auto idx = [&](int x, int y) {
    x = x < 0 ? 0 : (x >= s.w ? s.w - 1 : x);
    y = y < 0 ? 0 : (y >= s.h ? s.h - 1 : y);
    return s.at(x, y);
  };
  for (int j = 0; j < d.h; ++j)
    for (int i = 0; i < d.w; ++i) {
      const int ci = i << 1, cj = j << 1;
      double bx = 0, by = 0, count = 0;
      auto add_d = [&](int x, int y, int wgt) {  // buffer += wgt * bff_type(child)
        const size_t k = idx(x, y);
        if (!s.v[k]) return;
        count += wgt;
        bx += wgt * (double)s.dx[k];
        by += wgt * (double)s.dy[k];
      };
      auto add_f = [&](int x, int y, int wgt) {  // buffer += wgt * child  (float product)
        const size_t k = idx(x, y);
        if (!s.v[k]) return;
        count += wgt;
        bx += (double)((float)wgt * s.dx[k]);
        by += (double)((float)wgt * s.dy[k]);
      };
      add_d(ci, cj, 10);
      add_d(ci + 1, cj, 5);
      add_d(ci, cj + 1, 5);
      add_f(ci - 1, cj, 5);
      add_f(ci, cj - 1, 5);
      add_f(ci + 1, cj + 1, 2);
      add_f(ci - 1, cj - 1, 2);
      add_f(ci - 1, cj + 1, 2);
      add_f(ci + 1, cj - 1, 2);
      const size_t o = d.at(i, j);
      if (count > 0) {
        d.dx[o] = (float)(bx / (count * 2));
        d.dy[o] = (float)(by / (count * 2));
        d.v[o] = 1;
      }
    }
  return d;
}

// crop(disparity_upsample(edge_extend(d)), BBox2i(0, 0, W, H)) (SubpixelView.cc:183-189, DisparityMap.h:1326-1358).
DImg upsample_crop(const DImg& s, int W, int H) {
  DImg d;
  d.resize(W, H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int cx = x >> 1, cy = y >> 1;
      cx = cx >= s.w ? s.w - 1 : cx;
      cy = cy >= s.h ? s.h - 1 : cy;
      const size_t k = s.at(cx, cy), o = d.at(x, y);
      d.dx[o] = s.dx[k] * 2;
      d.dy[o] = s.dy[k] * 2;
      d.v[o] = s.v[k];
    }
  return d;
}

// derivative_filter(img, 1, 0) / (img, 0, 1): SeparableConvolutionView with the kernel {0.5, 0, -0.5} on one axis,
// ConstantEdgeExtension; correlate_1d_at_point sums k[2] * s(-1) + k[1] * s(0) + k[0] * s(+1) from 0 in float.
FImg derivative(const FImg& s, int ax) {
  FImg d;
  d.resize(s.w, s.h);
  for (int y = 0; y < s.h; ++y)
    for (int x = 0; x < s.w; ++x) {
      const float a = ax ? s.clamped(x, y - 1) : s.clamped(x - 1, y);
      const float b = s.at(x, y);
      const float c = ax ? s.clamped(x, y + 1) : s.clamped(x + 1, y);
      float r = 0.f;
      r += -0.5f * a;
      r += 0.0f * b;
      r += 0.5f * c;
      d.p[(size_t)y * s.w + x] = r;
    }
  return d;
}

// compute_spatial_weight_image (Correlate.cc:36-55).  two_sigma_sqr is formed in double and stored as float; the
// exponent is a float quotient, exp is evaluated in double and stored as float; the sum runs in float.
std::vector<float> weight_template(int kw, int kh) {
  const float two_sigma_sqr = 2.0 * std::pow(float(kw) / 5.0, 2.0);
  const int cx = kw / 2, cy = kh / 2;
  std::vector<float> w((size_t)kw * kh);
  float sum = 0.0f;
  for (int j = 0; j < kh; ++j)
    for (int i = 0; i < kw; ++i) {
      const float e = -1 * ((i - cx) * (i - cx) + (j - cy) * (j - cy)) / two_sigma_sqr;
      w[(size_t)j * kw + i] = (float)std::exp((double)e);
      sum += w[(size_t)j * kw + i];
    }
  for (auto& v : w) v /= sum;
  return w;
}

// BilinearInterpolation over ZeroEdgeExtension (src/vw/Image/Interpolation.h:76-106), float arithmetic, with the
// integer-pixel shortcut.
float bilinear_zero(const FImg& r, float xx, float yy) {
  const int x = (int)std::floor((double)xx), y = (int)std::floor((double)yy);
  if ((double)x == (double)xx && (double)y == (double)yy) return r.zero_ext(x, y);
  const float nx = xx - (float)x, ny = yy - (float)y, n1mx = 1 - nx, n1my = 1 - ny;
  float res = r.zero_ext(x, y) * n1mx;
  res += r.zero_ext(x + 1, y) * nx;
  res *= n1my;
  float row = r.zero_ext(x, y + 1) * n1mx;
  row += r.zero_ext(x + 1, y + 1) * nx;
  res += row * ny;
  return res;
}

// LAPACK reference SPOTRF2 (recursive, lower) on the n x n block at (o, o) of a 6 x 6 symmetric matrix;
// A(i, j) = a[i * 6 + j] with i >= j.  Returns 0 or the LAPACK info > 0.
int spotrf2(float* a, int o, int n) {
#define A_(i, j) a[(size_t)(i) * 6 + (j)]
  if (n == 1) {
    if (!(A_(o, o) > 0.0f)) return 1;  // A(1,1) <= 0 or NaN
    A_(o, o) = std::sqrt(A_(o, o));
    return 0;
  }
  const int n1 = n / 2, n2 = n - n1;
  int info = spotrf2(a, o, n1);
  if (info) return info;
  // STRSM('R', 'L', 'T', 'N', n2, n1, 1, A11, A21)
  for (int k = 0; k < n1; ++k) {
    const float t = 1.0f / A_(o + k, o + k);
    for (int i = 0; i < n2; ++i) A_(o + n1 + i, o + k) = t * A_(o + n1 + i, o + k);
    for (int j = k + 1; j < n1; ++j)
      if (A_(o + j, o + k) != 0.0f) {
        const float t2 = A_(o + j, o + k);
        for (int i = 0; i < n2; ++i) A_(o + n1 + i, o + j) = A_(o + n1 + i, o + j) - t2 * A_(o + n1 + i, o + k);
      }
  }
  // SSYRK('L', 'N', n2, n1, -1, A21, 1, A22)
  for (int j = 0; j < n2; ++j)
    for (int l = 0; l < n1; ++l)
      if (A_(o + n1 + j, o + l) != 0.0f) {
        const float t = -1.0f * A_(o + n1 + j, o + l);
        for (int i = j; i < n2; ++i) A_(o + n1 + i, o + n1 + j) = A_(o + n1 + i, o + n1 + j) + t * A_(o + n1 + i, o + l);
      }
  info = spotrf2(a, o + n1, n2);
  if (info) return info + n1;
  return 0;
}

// SPOSV('L', 6, 1): SPOTRF (= SPOTRF2 for n <= the block size) then SPOTRS; b is untouched when info > 0.
int sposv6(float* a, float* b) {
  const int info = spotrf2(a, 0, 6);
  if (info) return info;
  for (int k = 0; k < 6; ++k)  // STRSM('L', 'L', 'N', 'N')
    if (b[k] != 0.0f) {
      b[k] = b[k] / A_(k, k);
      for (int i = k + 1; i < 6; ++i) b[i] = b[i] - b[k] * A_(i, k);
    }
  for (int i = 5; i >= 0; --i) {  // STRSM('L', 'L', 'T', 'N')
    float t = b[i];
    for (int k = i + 1; k < 6; ++k) t = t - A_(k, i) * b[k];
    t = t / A_(i, i);
    b[i] = t;
  }
  return 0;
#undef A_
}

// norm_2 (src/vw/Math/Vector.h:1593-1604): float squares summed in double, the sum stored as float, sqrt in double.
double norm_2(const float* v, int n) {
  double r = 0.0;
  for (int i = 0; i < n; ++i) r += v[i] * v[i];
  return std::sqrt((double)(float)r);
}

// subpixel_optimized_affine_2d (Correlate.cc:848-1200).  inplace = 0 reads the validity of the window from the map
// as it was on entry (test-only switch: the reference always updates the map in place).
void affine_2d(DImg& D, const FImg& L, const FImg& R, int kw, int kh, int rx0, int ry0, int rx1, int ry1, int inplace,
               long long* iters) {
  const unsigned MAX_NUM_ITERATIONS = 10;
  const float max_translation = kw / 2;
  const int khh = kh / 2, khw = kw / 2, kern_pixels = kh * kw, min_good = kern_pixels / 2;
  const FImg Ix = derivative(L, 0), Iy = derivative(L, 1);
  const std::vector<float> tmpl = weight_template(kw, kh);
  const std::vector<uint8_t> v0 = D.v;
  const std::vector<uint8_t>& vref = inplace ? D.v : v0;
  std::vector<float> w((size_t)kw * kh);
  for (int y = std::max(ry0 - 1, khh); y < std::min(L.h - khh, ry1 + 1); ++y)
    for (int x = std::max(rx0 - 1, khw); x < std::min(L.w - khw, rx1 + 1); ++x) {
      const size_t p = D.at(x, y);
      if (!D.v[p]) continue;
      float d[6] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f};
      // adjust_weight_image (Correlate.cc:1393-1440)
      float sum = 0;
      int good = 0;
      for (int j = 0; j < kh; ++j)
        for (int i = 0; i < kw; ++i) {
          const size_t k = (size_t)j * kw + i;
          if (!vref[D.at(x - khw + i, y - khh + j)]) {
            w[k] = 0;
          } else {
            w[k] = tmpl[k];
            sum += w[k];
            ++good;
          }
        }
      for (auto& e : w) e /= sum;
      if (good < min_good) {
        D.v[p] = 0;
        continue;
      }
      for (unsigned iter = 0; iter < MAX_NUM_ITERATIONS; ++iter) {
        const float t2[2] = {d[2], d[5]};
        if (norm_2(t2, 2) > max_translation) break;
        if (iters) ++*iters;
        const float x_base = x + D.dx[p];
        const float y_base = y + D.dy[p];
        float rhs[36] = {0};
        float lhs[6] = {0};
        for (int jj = -khh; jj <= khh; ++jj) {
          const float xx_partial = x_base + d[1] * jj + d[2];
          const float yy_partial = y_base + d[4] * jj + d[5];
          for (int ii = -khw; ii <= khw; ++ii) {
            const float xx = d[0] * ii + xx_partial;
            const float yy = d[3] * ii + yy_partial;
            const float I_e_val = bilinear_zero(R, xx, yy) - L.at(x + ii, y + jj);
            const float weight = 1 * w[0];  // *w_ptr: w_ptr = w_row = w.origin() is never advanced (Correlate.cc:1002-1046)
            const float ix = Ix.at(x + ii, y + jj), iy = Iy.at(x + ii, y + jj);
            const float I_x_val = weight * ix, I_y_val = weight * iy;
            const float I_x_sqr = I_x_val * ix, I_y_sqr = I_y_val * iy, I_x_I_y = I_x_val * iy;
            const float IxIe = I_x_val * I_e_val, IyIe = I_y_val * I_e_val;
            lhs[0] -= ii * IxIe;
            lhs[1] -= jj * IxIe;
            lhs[2] -= IxIe;
            lhs[3] -= ii * IyIe;
            lhs[4] -= jj * IyIe;
            lhs[5] -= IyIe;
            const float m0 = ii * ii, m1 = ii * jj, m2 = jj * jj;
            rhs[0] += m0 * I_x_sqr;
            rhs[1] += m1 * I_x_sqr;
            rhs[2] += ii * I_x_sqr;
            rhs[7] += m2 * I_x_sqr;
            rhs[8] += jj * I_x_sqr;
            rhs[14] += I_x_sqr;
            rhs[3] += m0 * I_x_I_y;
            rhs[4] += m1 * I_x_I_y;
            rhs[5] += ii * I_x_I_y;
            rhs[10] += m2 * I_x_I_y;
            rhs[11] += jj * I_x_I_y;
            rhs[17] += I_x_I_y;
            rhs[21] += m0 * I_y_sqr;
            rhs[22] += m1 * I_y_sqr;
            rhs[23] += ii * I_y_sqr;
            rhs[28] += m2 * I_y_sqr;
            rhs[29] += jj * I_y_sqr;
            rhs[35] += I_y_sqr;
          }
        }
        // symmetric fill (Correlate.cc:1133-1145): the three upper entries that are not accumulated, then the lower triangle
        rhs[9] = rhs[4];    // rhs(1,3) = rhs(0,4)
        rhs[15] = rhs[5];   // rhs(2,3) = rhs(0,5)
        rhs[16] = rhs[11];  // rhs(2,4) = rhs(1,5)
        for (int r = 0; r < 6; ++r)
          for (int c = 0; c < r; ++c) rhs[r * 6 + c] = rhs[c * 6 + r];
        sposv6(rhs, lhs);  // info > 0: lhs stays the right-hand side and is still added
        for (int k = 0; k < 6; ++k) d[k] += lhs[k];
        float wl[6] = {lhs[0], lhs[1], lhs[2], lhs[3], lhs[4], lhs[5]};
        const int kqh = khh / 2, kqw = khw / 2;
        wl[0] *= kqw;
        wl[1] *= kqh;
        wl[3] *= kqw;
        wl[4] *= kqh;
        if (norm_2(wl, 6) < 0.05) break;
      }
      const float t2[2] = {d[2], d[5]};
      if (norm_2(t2, 2) > max_translation || std::isnan(d[2]) || std::isnan(d[5])) {
        D.v[p] = 0;
      } else {
        D.dx[p] += d[2];
        D.dy[p] += d[5];
      }
    }
}

}  // namespace

extern "C" {

// The range of one tile {x, y, w, h} (tile_range.h) as {min x, min y, max x, max y}.  Returns 0, -1 on bad arguments.
int afr_tile_range(const float* disp3, int w, int h, const int* tile, int* out4) {
  if (!disp3 || !tile || !out4 || w <= 0 || h <= 0) return -1;
  if (tile[2] <= 0 || tile[3] <= 0 || tile[0] < 0 || tile[1] < 0 || tile[0] + tile[2] > w || tile[1] + tile[3] > h) return -1;
  tile_disparity_range(disp3, w, tile, out4);
  return 0;
}

// One call = PyramidSubpixelView::prerasterize(bbox) for each of the ntiles boxes {x, y, w, h} (inside the left image),
// written into out3 (w x h x 3).  Returns 0, -1 on bad arguments, -2 for an algorithm other than FAST_AFFINE (1).
// stats (may be NULL): [0] += window-loop iterations run.
int afr_pyramid_subpixel(const float* disp3, int w, int h, const float* left, const float* right, int rw, int rh,
                         int mode, float width, int kx, int ky, int max_levels, int algorithm, const int* tiles,
                         int ntiles, float* out3, int inplace, long long* stats) {
  if (!disp3 || !left || !right || !out3 || w <= 0 || h <= 0 || rw <= 0 || rh <= 0) return -1;
  if (kx < 1 || ky < 1 || !(kx & 1) || !(ky & 1)) return -1;
  if (algorithm != 1) return -2;
  if (max_levels < 0) max_levels = 0;
  for (int t = 0; t < ntiles; ++t) {
    const int bx = tiles[4 * t], by = tiles[4 * t + 1], bw = tiles[4 * t + 2], bh = tiles[4 * t + 3];
    if (bw <= 0 || bh <= 0 || bx < 0 || by < 0 || bx + bw > w || by + bh > h) return -1;
  }
  for (int t = 0; t < ntiles; ++t) {
    const int bx = tiles[4 * t], by = tiles[4 * t + 1], bw = tiles[4 * t + 2], bh = tiles[4 * t + 3];
    // get_disparity_range over crop(disparity, bbox) (SubpixelView.cc:42): over the tile's valid pixels, zeros without any;
    // BBox2f -> BBox2i converts each corner with a C cast (tile_range.h).
    int rng[4];
    tile_disparity_range(disp3, w, tiles + 4 * t, rng);
    const int sminx = rng[0], sminy = rng[1], smaxx = rng[2], smaxy = rng[3];
    // crop boxes (SubpixelView.cc:46-63): both of the right box's size, grown by the full kernel size
    const int pw = bw + (smaxx - sminx) + 2 * kx, ph = bh + (smaxy - sminy) + 2 * ky;
    const int lx0 = bx - kx, ly0 = by - ky, rx0 = bx + sminx - kx, ry0 = by + sminy - ky;
    FImg L, R;
    L.resize(pw, ph);
    R.resize(pw, ph);
    if (vwo_prefilter_region(left, w, h, mode, width, lx0, ly0, pw, ph, L.p.data())) return -1;
    if (vwo_prefilter_region(right, rw, rh, mode, width, rx0, ry0, pw, ph, R.p.data())) return -1;
    // crop(edge_extend(disparity, ZeroEdgeExtension()), left_crop_bbox) - range.min (:88-95)
    DImg D;
    D.resize(pw, ph);
    for (int y = 0; y < ph; ++y)
      for (int x = 0; x < pw; ++x) {
        const int sx = lx0 + x, sy = ly0 + y;
        const size_t o = D.at(x, y);
        float vx = 0, vy = 0;
        uint8_t vv = 0;
        if (sx >= 0 && sy >= 0 && sx < w && sy < h) {
          const float* q = disp3 + ((size_t)sy * w + sx) * 3;
          vx = q[0];
          vy = q[1];
          vv = q[2] != 0.0f;
        }
        D.dx[o] = vx - (float)sminx;
        D.dy[o] = vy - (float)sminy;
        D.v[o] = vv;
      }
    // pyramid (:108-129): ROIs as {min, max} corners, halved by integer division
    std::vector<FImg> lp, rp;
    std::vector<int> roi;  // 4 per level
    DImg ds = D;
    for (int i = 0; i < max_levels; ++i) {
      if (i > 0) {
        lp.push_back(subsample2(lp.back()));
        rp.push_back(subsample2(rp.back()));
        ds = disparity_subsample(ds);
        const size_t b = roi.size() - 4;
        roi.insert(roi.end(), {roi[b] / 2, roi[b + 1] / 2, roi[b + 2] / 2, roi[b + 3] / 2});
      } else {
        lp.push_back(subsample2(L));
        rp.push_back(subsample2(R));
        ds = disparity_subsample(D);
        roi.insert(roi.end(), {kx / 2, ky / 2, (kx + bw) / 2, (ky + bh) / 2});
      }
    }
    for (int i = max_levels - 1; i >= 0; --i) {  // :133-190
      affine_2d(ds, lp[i], rp[i], kx, ky, roi[4 * i], roi[4 * i + 1], roi[4 * i + 2], roi[4 * i + 3], inplace, stats);
      const int W = i > 0 ? lp[i - 1].w : pw, H = i > 0 ? lp[i - 1].h : ph;
      ds = upsample_crop(ds, W, H);
    }
    affine_2d(ds, L, R, kx, ky, kx, ky, kx + bw, ky + bh, inplace, stats);  // final pass (:195-222)
    for (int y = by; y < by + bh; ++y)
      for (int x = bx; x < bx + bw; ++x) {
        const size_t k = ds.at(x - bx + kx, y - by + ky);
        float* o = out3 + ((size_t)y * w + x) * 3;
        if (ds.v[k]) {
          o[0] = ds.dx[k] + (float)sminx;
          o[1] = ds.dy[k] + (float)sminy;
          o[2] = 1.0f;
        } else {
          o[0] = o[1] = o[2] = 0.0f;
        }
      }
  }
  return 0;
}

}  // extern "C"
