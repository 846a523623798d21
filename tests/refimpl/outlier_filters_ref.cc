// outlier_filters_ref.cc — CPU restatement (test infrastructure) of the local outlier filters of
// src/vw/Stereo/DisparityMap.h: rm_outliers_using_mean (:444-578), rm_outliers_using_stddev (:600-748),
// rm_outliers_using_plane (:769-927, DisparityMap.cc:37-118), their clean-up compositions (:580-598, :750-767, :929-947)
// and std_dev_image (:949-1014, DisparityMap.cc:24-34).  Dependency-free; built with -ffp-contract=off.
//
// Every filter is a per-pixel functor over the disparity with constant edge extension: a window of
// (2 half_h + 1) x (2 half_v + 1) pixels, rows outer, columns inner, every coordinate clamped on its own, read from the
// unmodified input.  An invalid centre is copied; a rejected pixel becomes {0, 0, 0}.  A clean-up composition evaluates
// the filter on (w + 2) x (h + 2) positions from (-1, -1) (the inner view is defined outside the image through its
// edge-extended child) and applies the thresh functor (1, 1, 3.0, 0.2) to that.
// Layouts: disparity (rows, cols, 3) int32 (type 0) or float32 (type 1) {dx, dy, valid != 0}; images (rows, cols) float32.
//
// The plane method's 3 x 3 solve is the specification of the project (the reference calls LAPACK gesv, whose bits are
// not pinned): unblocked LU with partial pivoting, column-wise search in which the first largest |a| wins, multipliers by
// the reciprocal of the pivot, rank-1 update, two triangular solves; an exactly zero pivot means unsolvable, and the
// pixel is kept.
// Outside the reference's contract: a NaN among the valid disparities of a mean window (std::sort; the centre is left
// unchanged here), int magnitudes |dx| + |dy| that overflow (taken modulo 2^32 here), and half_h > half_v in the stddev
// and plane methods (the reference's value buffer is (2 half_v + 1)^2; the evident result is computed here).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {

template <class F>
void for_rows(int rows, int threads, F f) {
  const int nt = std::max(1, std::min(threads, rows));
  std::vector<std::thread> pool;
  for (int t = 0; t < nt; ++t)
    pool.emplace_back([=] {
      for (int r = t; r < rows; r += nt) f(r, t);
    });
  for (auto& th : pool) th.join();
}

struct I32 {
  typedef int32_t word;
  static bool valid(const word* p) { return p[2] != 0; }
  static double magnitude(const word* p) {   // an int add in the reference
    const uint32_t a = p[0] < 0 ? 0u - (uint32_t)p[0] : (uint32_t)p[0], b = p[1] < 0 ? 0u - (uint32_t)p[1] : (uint32_t)p[1];
    return (double)(uint32_t)(a + b);
  }
  static double absdiff(word a, word b) { return std::fabs((double)(int32_t)((uint32_t)a - (uint32_t)b)); }
};
struct F32 {
  typedef float word;
  static bool valid(const word* p) { return p[2] != 0; }
  static double magnitude(const word* p) {   // a float add, then widened
    const float m = std::fabs(p[0]) + std::fabs(p[1]);
    return (double)m;
  }
  static double absdiff(word a, word b) { return (double)std::fabs(a - b); }
};

template <class T>
struct Image {
  const typename T::word* d;
  int w, h;
  const typename T::word* at(int x, int y) const {
    x = std::min(std::max(x, 0), w - 1);
    y = std::min(std::max(y, 0), h - 1);
    return d + ((size_t)y * w + x) * 3;
  }
};

struct Params {
  int hh, hv;
  double p0, p1;
  int skip;
};

// true: the (valid) pixel at (x, y) stays
template <class T>
bool mean_keep(const Image<T>& im, int x, int y, const Params& P) {
  std::vector<double> len;
  bool nan = false;
  for (int yk = -P.hv; yk <= P.hv; ++yk)
    for (int xk = -P.hh; xk <= P.hh; ++xk) {
      const auto* p = im.at(x + xk, y + yk);
      if (!T::valid(p)) continue;
      len.push_back(T::magnitude(p));
      nan = nan || std::isnan(len.back());
    }
  if (nan) return true;
  std::sort(len.begin(), len.end());
  double cutoff = 0.0;
  if (!len.empty()) cutoff = 2.0 * len[(int)(0.75 * len.size())];
  double mx = 0.0, my = 0.0;
  size_t matched = 0;
  for (int yk = -P.hv; yk <= P.hv; ++yk)
    for (int xk = -P.hh; xk <= P.hh; ++xk) {
      const auto* p = im.at(x + xk, y + yk);
      if (!T::valid(p)) continue;
      if (T::magnitude(p) > cutoff) {
        if (P.skip) continue;   // only this pixel
        break;                  // reference: the accessor no longer advances, the rest of the row is never read
      }
      mx += p[0];
      my += p[1];
      matched++;
    }
  const double limit = P.p0 * P.p0;
  double err = limit + 1.0;
  if (matched > 0) {
    mx = mx / (double)matched;
    my = my / (double)matched;
    const double tx = im.at(x, y)[0], ty = im.at(x, y)[1];
    err = (tx - mx) * (tx - mx) + (ty - my) * (ty - my);
  }
  return !(err > limit);
}

template <class T>
bool stddev_keep(const Image<T>& im, int x, int y, const Params& P) {
  std::vector<double> xs, ys;
  double mx = 0.0, my = 0.0;
  for (int yk = -P.hv; yk <= P.hv; ++yk)
    for (int xk = -P.hh; xk <= P.hh; ++xk) {
      const auto* p = im.at(x + xk, y + yk);
      if (!T::valid(p)) continue;
      xs.push_back(p[0]);
      ys.push_back(p[1]);
      mx += p[0];
      my += p[1];
    }
  const size_t n = xs.size();
  if (n == 0) return false;
  mx = mx / (double)n;
  my = my / (double)n;
  double sx = 0.0, sy = 0.0;
  for (size_t i = 0; i < n; ++i) {
    const double dx = xs[i] - mx, dy = ys[i] - my;
    sx += dx * dx;
    sy += dy * dy;
  }
  double sdx = std::sqrt(sx / (double)n), sdy = std::sqrt(sy / (double)n);
  if (sdx < P.p1) sdx = P.p1;
  if (sdy < P.p1) sdy = P.p1;
  const double ex = std::fabs((double)im.at(x, y)[0] - mx), ey = std::fabs((double)im.at(x, y)[1] - my);
  return !((ex > P.p0 * sdx) || (ey > P.p0 * sdy));
}

struct Pt {
  double x, y, z;
};

// A (3 x 3, row-major) x = b for two right-hand sides; false: an exactly zero pivot
bool solve3(double A[3][3], double b[3], double c[3]) {
  for (int j = 0; j < 3; ++j) {
    int p = j;
    double big = std::fabs(A[j][j]);
    for (int i = j + 1; i < 3; ++i)
      if (std::fabs(A[i][j]) > big) {
        big = std::fabs(A[i][j]);
        p = i;
      }
    if (p != j) {
      for (int k = 0; k < 3; ++k) std::swap(A[j][k], A[p][k]);
      std::swap(b[j], b[p]);
      std::swap(c[j], c[p]);
    }
    if (A[j][j] == 0.0) return false;
    const double r = 1.0 / A[j][j];
    for (int i = j + 1; i < 3; ++i) A[i][j] = A[i][j] * r;
    for (int k = j + 1; k < 3; ++k)
      for (int i = j + 1; i < 3; ++i) A[i][k] = A[i][k] - A[i][j] * A[j][k];
  }
  for (double* v : {b, c}) {
    for (int k = 0; k < 3; ++k)
      for (int i = k + 1; i < 3; ++i) v[i] = v[i] - v[k] * A[i][k];
    for (int k = 2; k >= 0; --k) {
      v[k] = v[k] / A[k][k];
      for (int i = k - 1; i >= 0; --i) v[i] = v[i] - v[k] * A[i][k];
    }
  }
  return true;
}

void normal_equations(const std::vector<Pt>& pts, double A[3][3], double b[3]) {
  for (int i = 0; i < 3; ++i) {
    b[i] = 0.0;
    for (int k = 0; k < 3; ++k) A[i][k] = 0.0;
  }
  for (const Pt& p : pts) {
    A[0][0] += p.x * p.x;
    A[0][1] += p.x * p.y;
    A[0][2] += p.x;
    A[1][0] += p.x * p.y;
    A[1][1] += p.y * p.y;
    A[1][2] += p.y;
    A[2][0] += p.x;
    A[2][1] += p.y;
    b[0] += p.x * p.z;
    b[1] += p.y * p.z;
    b[2] += p.z;
  }
  A[2][2] = (double)pts.size();
}

double plane_dist(const Pt& p, const double plane[3]) {
  const double a = plane[0], b = plane[1], c = -1.0, d = plane[2];
  const double num = std::fabs(a * p.x + b * p.y + c * p.z + d);
  const double den = std::sqrt(a * a + b * b + c * c);
  return num / den;
}

double plane_sigma(const std::vector<Pt>& pts, const double plane[3]) {
  double sum = 0.0;
  for (const Pt& p : pts) {
    const double d = plane_dist(p, plane);
    sum += d * d;
  }
  return std::sqrt(sum / (double)pts.size());
}

template <class T>
bool plane_keep(const Image<T>& im, int x, int y, const Params& P) {
  std::vector<Pt> px, py;
  for (int yk = -P.hv; yk <= P.hv; ++yk)
    for (int xk = -P.hh; xk <= P.hh; ++xk) {
      const auto* p = im.at(x + xk, y + yk);
      if (!T::valid(p)) continue;
      px.push_back(Pt{(double)xk, (double)yk, (double)p[0]});
      py.push_back(Pt{(double)xk, (double)yk, (double)p[1]});
    }
  if (px.empty()) return false;
  double A[3][3], B[3][3], fx[3], fy[3];
  normal_equations(px, A, fx);
  normal_equations(py, B, fy);   // the same matrix: offsets only
  if (!solve3(A, fx, fy)) return true;
  double sdx = plane_sigma(px, fx), sdy = plane_sigma(py, fy);
  if (sdx < P.p1) sdx = P.p1;
  if (sdy < P.p1) sdy = P.p1;
  const double ex = plane_dist(Pt{0.0, 0.0, (double)im.at(x, y)[0]}, fx);
  const double ey = plane_dist(Pt{0.0, 0.0, (double)im.at(x, y)[1]}, fy);
  return !((ex > P.p0 * sdx) || (ey > P.p0 * sdy));
}

// the filter's value at any integer position; returns 1 when it rejects
template <class T>
int filter_at(int method, const Image<T>& im, int x, int y, const Params& P, typename T::word* out) {
  const auto* c = im.at(x, y);
  out[0] = c[0];
  out[1] = c[1];
  out[2] = c[2];
  if (!T::valid(c)) return 0;
  const bool keep = method == 0 ? mean_keep(im, x, y, P) : method == 1 ? stddev_keep(im, x, y, P) : plane_keep(im, x, y, P);
  if (keep) return 0;
  out[0] = out[1] = out[2] = 0;
  return 1;
}

template <class T>
int run(int method, const typename T::word* in, int w, int h, const Params& P, int cleanup, typename T::word* out, int threads,
        long long* stats) {
  typedef typename T::word word;
  const Image<T> im{in, w, h};
  const int nt = std::max(1, threads);
  std::vector<long long> rej((size_t)nt, 0), rej2((size_t)nt, 0);
  if (!cleanup) {
    for_rows(h, nt, [&](int y, int t) {
      for (int x = 0; x < w; ++x) rej[t] += filter_at(method, im, x, y, P, out + ((size_t)y * w + x) * 3);
    });
  } else {
    const int pw = w + 2, ph = h + 2;
    std::vector<word> inner((size_t)pw * ph * 3);
    for_rows(ph, nt, [&](int j, int t) {
      for (int i = 0; i < pw; ++i) {
        const int r = filter_at(method, im, i - 1, j - 1, P, &inner[((size_t)j * pw + i) * 3]);
        if (i >= 1 && i <= w && j >= 1 && j <= h) rej[t] += r;
      }
    });
    for_rows(h, nt, [&](int y, int t) {
      for (int x = 0; x < w; ++x) {
        const word* c = &inner[((size_t)(y + 1) * pw + x + 1) * 3];
        word* o = out + ((size_t)y * w + x) * 3;
        o[0] = c[0];
        o[1] = c[1];
        o[2] = c[2];
        if (!T::valid(c)) continue;
        int matched = 0, total = 0;
        for (int yk = -1; yk <= 1; ++yk)
          for (int xk = -1; xk <= 1; ++xk) {
            const word* q = &inner[((size_t)(y + 1 + yk) * pw + x + 1 + xk) * 3];
            if (T::valid(q) && T::absdiff(c[0], q[0]) <= 3.0 && T::absdiff(c[1], q[1]) <= 3.0) matched++;
            total++;
          }
        if ((double)matched / (double)total < 0.2) {
          o[0] = o[1] = o[2] = 0;
          rej2[t] += 1;
        }
      }
    });
  }
  if (stats) {
    stats[0] = stats[1] = 0;
    for (int t = 0; t < nt; ++t) {
      stats[0] += rej[t];
      stats[1] += rej2[t];
    }
  }
  return 0;
}

}  // namespace

extern "C" {

// method 0 mean (p0 = max_mean_diff), 1 stddev, 2 plane (p0 = pixel_threshold, p1 = rejection_threshold); type 0 int32,
// 1 float32; semantics 0 reference, 1 skip.  Returns 0, or 1 for arguments the reference's constructors refuse.
int ofr_rm_outliers(int method, int type, const void* in, int w, int h, int half_h, int half_v, double p0, double p1, int cleanup,
                    int semantics, void* out, int threads, long long* stats) {
  if (method < 0 || method > 2 || type < 0 || type > 1 || !in || !out || w <= 0 || h <= 0 || half_h <= 0 || half_v <= 0) return 1;
  const Params P{half_h, half_v, p0, p1, semantics != 0};
  if (type == 0) return run<I32>(method, (const int32_t*)in, w, h, P, cleanup, (int32_t*)out, threads, stats);
  return run<F32>(method, (const float*)in, w, h, P, cleanup, (float*)out, threads, stats);
}

// edge 0 constant, 1 zero (vwgpu_edge)
int ofr_std_dev_image(const float* img, int w, int h, int kw, int kh, int edge, float* out, int threads) {
  if (!img || !out || w <= 0 || h <= 0 || kw <= 0 || kh <= 0) return 1;
  auto at = [=](int x, int y) -> float {
    if (edge == 1 && (x < 0 || y < 0 || x >= w || y >= h)) return 0.0f;
    return img[(size_t)std::min(std::max(y, 0), h - 1) * w + std::min(std::max(x, 0), w - 1)];
  };
  for_rows(h, std::max(1, threads), [&](int y, int) {
    for (int x = 0; x < w; ++x) {
      float sum = 0;
      for (int yk = -kh / 2; yk <= kh / 2; ++yk)
        for (int xk = -kw / 2; xk <= kw / 2; ++xk) sum += at(x + xk, y + yk);
      const float mean = sum / (kw * kh);
      sum = 0;
      for (int yk = -kh / 2; yk <= kh / 2; ++yk)
        for (int xk = -kw / 2; xk <= kw / 2; ++xk) {
          const float diff = at(x + xk, y + yk) - mean;
          sum += diff * diff;
        }
      out[(size_t)y * w + x] = sum / (kw * kh - 1);
    }
  });
  return 0;
}

}  // extern "C"
