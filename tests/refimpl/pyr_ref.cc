// pyr_ref.cc — TEST INFRASTRUCTURE ONLY: a sequential CPU restatement of vw::stereo::PyramidSubpixelView::prerasterize
// (src/vw/Stereo/SubpixelView.cc:33-224) with SUBPIXEL_LUCAS_KANADE (subpixel_optimized_LK_2d, Correlate.cc:1203-1391)
// and SUBPIXEL_BAYES_EM (subpixel_optimized_affine_2d_EM, Correlate.cc:500-845), statement order kept.  The pyramid
// helpers, the weight template, the bilinear interpolation, SPOSV and norm_2 come from the FAST_AFFINE restatement
// (affine_ref.cc, included); FAST_AFFINE itself is accepted too (algorithm 1 runs its affine_2d).
//
// exp: inside namespace vw only ::exp(double) is in scope (Math/Functions.h: `using ::exp;`), so `k * exp(e)` with float
// k and e is a double product of the host libm's double exp, rounded to float; this file spells the promotion out.
#include "affine_ref.cc"

namespace {

// SPOSV('L', 2, 1): SPOTRF2 (n1 = n2 = 1) then SPOTRS; b untouched when info > 0.  A(i, j) = a[i * 2 + j], i >= j.
int sposv2(float* a, float* b) {
  if (!(a[0] > 0.0f)) return 1;
  a[0] = std::sqrt(a[0]);
  {
    const float t = 1.0f / a[0];  // STRSM('R', 'L', 'T', 'N', 1, 1, 1, A11, A21)
    a[2] = t * a[2];
  }
  if (a[2] != 0.0f) {  // SSYRK('L', 'N', 1, 1, -1, A21, 1, A22)
    const float t = -1.0f * a[2];
    a[3] = a[3] + t * a[2];
  }
  if (!(a[3] > 0.0f)) return 2;
  a[3] = std::sqrt(a[3]);
  if (b[0] != 0.0f) {  // STRSM('L', 'L', 'N', 'N')
    b[0] = b[0] / a[0];
    b[1] = b[1] - b[0] * a[2];
  }
  if (b[1] != 0.0f) b[1] = b[1] / a[3];
  b[1] = b[1] / a[3];  // STRSM('L', 'L', 'T', 'N')
  {
    float t = b[0];
    t = t - a[2] * b[1];
    b[0] = t / a[0];
  }
  return 0;
}

// adjust_weight_image (Correlate.cc:1393-1440) into w; returns the number of good pixels
int adjust_weight(std::vector<float>& w, const std::vector<float>& tmpl, const std::vector<uint8_t>& vref, const DImg& D,
                  int x, int y, int kw, int kh) {
  float sum = 0;
  int good = 0;
  const int khw = kw / 2, khh = kh / 2;
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
  return good;
}

// subpixel_optimized_LK_2d (Correlate.cc:1203-1391).  inplace = 0 reads the window validity as on entry (test switch).
void lk_2d(DImg& D, const FImg& L, const FImg& R, int kw, int kh, int rx0, int ry0, int rx1, int ry1, int inplace,
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
      float d[2] = {0.0f, 0.0f};
      if (adjust_weight(w, tmpl, vref, D, x, y, kw, kh) < min_good) {
        D.v[p] = 0;
        continue;
      }
      for (unsigned iter = 0; iter < MAX_NUM_ITERATIONS; ++iter) {
        if (norm_2(d, 2) > max_translation) break;
        if (iters) ++*iters;
        const float x_base = x + D.dx[p];
        const float y_base = y + D.dy[p];
        float rhs[4] = {0, 0, 0, 0};
        float lhs[2] = {0, 0};
        for (int jj = -khh; jj <= khh; ++jj) {
          const float xx_partial = x_base + d[0];
          const float yy = y_base + jj + d[1];
          for (int ii = -khw; ii <= khw; ++ii) {
            const float xx = ii + xx_partial;
            const float interpreted_px = bilinear_zero(R, xx, yy);
            const float I_e_val = interpreted_px - L.at(x + ii, y + jj);
            const float robust_weight = 1;
            const float weight = robust_weight * w[0];  // *w_ptr: never advanced (Correlate.cc:1290-1330)
            const float ix = Ix.at(x + ii, y + jj), iy = Iy.at(x + ii, y + jj);
            const float I_x_val = weight * ix, I_y_val = weight * iy;
            const float I_x_sqr = I_x_val * ix, I_y_sqr = I_y_val * iy, I_x_I_y = I_x_val * iy;
            lhs[0] -= I_x_val * I_e_val;
            lhs[1] -= I_y_val * I_e_val;
            rhs[0] += I_x_sqr;
            rhs[1] += I_x_I_y;
            rhs[3] += I_y_sqr;
          }
        }
        rhs[2] = rhs[1];
        sposv2(rhs, lhs);
        d[0] += lhs[0];
        d[1] += lhs[1];
        if (norm_2(lhs, 2) < 0.05) break;
      }
      if (norm_2(d, 2) > max_translation || std::isnan(d[0]) || std::isnan(d[1])) {
        D.v[p] = 0;
      } else {
        D.dx[p] += d[0];
        D.dy[p] += d[1];
      }
    }
}

// subpixel_optimized_affine_2d_EM (Correlate.cc:500-845).  iters counts every pass over a window (EM passes included).
void em_2d(DImg& D, const FImg& L, const FImg& R, int kw, int kh, int rx0, int ry0, int rx1, int ry1, int inplace,
           long long* iters) {
  const unsigned M_MAX_EM_ITER = 2;
  const float max_translation = kw / 2;
  const int khh = kh / 2, khw = kw / 2, kern_pixels = kh * kw, weight_threshold = kern_pixels / 2;
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
      if (adjust_weight(w, tmpl, vref, D, x, y, kw, kh) < weight_threshold) {
        D.v[p] = 0;
        continue;
      }
      float curr_sum_I_e_val = 0.0;
      float prev_sum_I_e_val = 0.0;
      for (unsigned iter = 0; iter < 10; ++iter) {
        const float t2[2] = {d[2], d[5]};
        if (norm_2(t2, 2) > max_translation) break;
        const float x_base = x + D.dx[p];
        const float y_base = y + D.dy[p];
        float rhs[36] = {0};
        float lhs[6] = {0}, prev_lhs[6] = {0};
        const float var2_plane = 1e-3;
        float mean_noise = 0.0;
        const float var2_noise = 1e-2;
        float w_plane = 0.8;
        float w_noise = 0.2;
        float in_curr_sum_I_e_val = 0.0;
        float d_em[6];
        for (int k = 0; k < 6; ++k) d_em[k] = d[k];
        for (unsigned em_iter = 0; em_iter < M_MAX_EM_ITER; em_iter++) {
          const float noise_norm_factor = 1.0 / std::sqrt(2 * M_PI * var2_noise);
          const float plane_norm_factor = 1.0 / std::sqrt(2 * M_PI * var2_plane);
          std::fill(lhs, lhs + 6, 0.0f);
          std::fill(rhs, rhs + 36, 0.0f);
          in_curr_sum_I_e_val = 0.0;
          float mean_noise_tmp = 0.0;
          float sum_gamma_noise = 0.0;
          float sum_gamma_plane = 0.0;
          int skip = 0;
          if (iters) ++*iters;
          for (int jj = -khh; jj <= khh; ++jj) {
            const float xx_partial = x_base + d[1] * jj + d[2];
            const float yy_partial = y_base + d[4] * jj + d[5];
            const float delta_x_partial = d_em[1] * jj + d_em[2];
            const float delta_y_partial = d_em[4] * jj + d_em[5];
            for (int ii = -khw; ii <= khw; ++ii) {
              const float xx = d[0] * ii + xx_partial;
              const float yy = d[3] * ii + yy_partial;
              const float delta_x = d_em[0] * ii + delta_x_partial;
              const float delta_y = d_em[3] * ii + delta_y_partial;
              const float ix = Ix.at(x + ii, y + jj), iy = Iy.at(x + ii, y + jj);
              const float interpreted_px = bilinear_zero(R, xx, yy);
              const float I_e_val = interpreted_px - L.at(x + ii, y + jj);
              in_curr_sum_I_e_val += I_e_val;
              const float temp_plane = I_e_val - delta_x * ix - delta_y * iy;
              const float temp_noise = interpreted_px - mean_noise;
              const float plane_prob_exp = -1 * (temp_plane * temp_plane) / (2 * var2_plane);
              const float plane_prob =
                  (plane_prob_exp < -75) ? 0.0f : (float)((double)plane_norm_factor * std::exp((double)plane_prob_exp));
              const float noise_prob_exp = -1 * (temp_noise * temp_noise) / (2 * var2_noise);
              const float noise_prob =
                  (noise_prob_exp < -75) ? 0.0f : (float)((double)noise_norm_factor * std::exp((double)noise_prob_exp));
              const float sum = plane_prob * w_plane + noise_prob * w_noise;
              const float gamma_plane = plane_prob * w_plane / sum;
              const float gamma_noise = noise_prob * w_noise / sum;
              mean_noise_tmp += interpreted_px * gamma_noise;
              sum_gamma_plane += gamma_plane;
              sum_gamma_noise += gamma_noise;
              const float weight = gamma_plane * w[0];  // *w_ptr: never advanced (Correlate.cc:664-746)
              if (weight < 1e-26) {
                skip++;
                continue;
              }
              const float I_x_val = weight * ix, I_y_val = weight * iy;
              const float I_x_sqr = I_x_val * ix, I_y_sqr = I_y_val * iy, I_x_I_y = I_x_val * iy;
              lhs[0] -= ii * I_x_val * I_e_val;
              lhs[1] -= jj * I_x_val * I_e_val;
              lhs[2] -= I_x_val * I_e_val;
              lhs[3] -= ii * I_y_val * I_e_val;
              lhs[4] -= jj * I_y_val * I_e_val;
              lhs[5] -= I_y_val * I_e_val;
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
          if (skip == kern_pixels) break;
          rhs[9] = rhs[4];
          rhs[15] = rhs[5];
          rhs[16] = rhs[11];
          for (int r = 0; r < 6; ++r)
            for (int c = 0; c < r; ++c) rhs[r * 6 + c] = rhs[c * 6 + r];
          sposv6(rhs, lhs);
          mean_noise = mean_noise_tmp / sum_gamma_noise;
          w_plane = sum_gamma_plane / (float)(kern_pixels);
          w_noise = sum_gamma_noise / (float)(kern_pixels);
          float diff[6];
          for (int k = 0; k < 6; ++k) diff[k] = prev_lhs[k] - lhs[k];
          const float conv_error = norm_2(diff, 6);
          for (int k = 0; k < 6; ++k) d_em[k] = d[k] + lhs[k];
          if (in_curr_sum_I_e_val < 0) in_curr_sum_I_e_val = -in_curr_sum_I_e_val;
          curr_sum_I_e_val = in_curr_sum_I_e_val;
          for (int k = 0; k < 6; ++k) prev_lhs[k] = lhs[k];
          if ((conv_error < 1E-3) && (em_iter > 0)) break;
        }
        for (int k = 0; k < 6; ++k) d[k] += lhs[k];
        if (curr_sum_I_e_val < 0) curr_sum_I_e_val = -curr_sum_I_e_val;
        if ((prev_sum_I_e_val < curr_sum_I_e_val) && (iter > 0))
          break;
        else
          prev_sum_I_e_val = curr_sum_I_e_val;
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

typedef void (*refiner)(DImg&, const FImg&, const FImg&, int, int, int, int, int, int, int, long long*);

}  // namespace

extern "C" {

// As afr_pyramid_subpixel (affine_ref.cc) for algorithm 0 (LUCAS_KANADE), 1 (FAST_AFFINE) or 2 (BAYES_EM); -2 for others.
int pyr_pyramid_subpixel(const float* disp3, int w, int h, const float* left, const float* right, int rw, int rh, int mode,
                         float width, int kx, int ky, int max_levels, int algorithm, const int* tiles, int ntiles, float* out3,
                         int inplace, long long* stats) {
  if (!disp3 || !left || !right || !out3 || w <= 0 || h <= 0 || rw <= 0 || rh <= 0) return -1;
  if (kx < 1 || ky < 1 || !(kx & 1) || !(ky & 1)) return -1;
  if (algorithm < 0 || algorithm > 2) return -2;
  const refiner refine = algorithm == 0 ? lk_2d : algorithm == 1 ? affine_2d : em_2d;
  if (max_levels < 0) max_levels = 0;
  for (int t = 0; t < ntiles; ++t) {
    const int bx = tiles[4 * t], by = tiles[4 * t + 1], bw = tiles[4 * t + 2], bh = tiles[4 * t + 3];
    if (bw <= 0 || bh <= 0 || bx < 0 || by < 0 || bx + bw > w || by + bh > h) return -1;
  }
  for (int t = 0; t < ntiles; ++t) {
    const int bx = tiles[4 * t], by = tiles[4 * t + 1], bw = tiles[4 * t + 2], bh = tiles[4 * t + 3];
    // get_disparity_range (SubpixelView.cc:42) over the tile's valid pixels (tile_range.h)
    int rng[4];
    tile_disparity_range(disp3, w, tiles + 4 * t, rng);
    const int sminx = rng[0], sminy = rng[1], smaxx = rng[2], smaxy = rng[3];
    const int pw = bw + (smaxx - sminx) + 2 * kx, ph = bh + (smaxy - sminy) + 2 * ky;
    const int lx0 = bx - kx, ly0 = by - ky, rx0 = bx + sminx - kx, ry0 = by + sminy - ky;
    FImg L, R;
    L.resize(pw, ph);
    R.resize(pw, ph);
    if (vwo_prefilter_region(left, w, h, mode, width, lx0, ly0, pw, ph, L.p.data())) return -1;
    if (vwo_prefilter_region(right, rw, rh, mode, width, rx0, ry0, pw, ph, R.p.data())) return -1;
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
    std::vector<FImg> lp, rp;
    std::vector<int> roi;
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
    for (int i = max_levels - 1; i >= 0; --i) {
      refine(ds, lp[i], rp[i], kx, ky, roi[4 * i], roi[4 * i + 1], roi[4 * i + 2], roi[4 * i + 3], inplace, stats);
      const int W = i > 0 ? lp[i - 1].w : pw, H = i > 0 ? lp[i - 1].h : ph;
      ds = upsample_crop(ds, W, H);
    }
    refine(ds, L, R, kx, ky, kx, ky, kx + bw, ky + bh, inplace, stats);
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
