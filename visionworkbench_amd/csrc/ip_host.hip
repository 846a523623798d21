// ip_host.hip — the host arithmetic that goes with ip_match.hip; no kernel, no context.  remove_duplicates
// (src/vw/InterestPoint/Matcher.cc:152-195), the three fitting functors of src/vw/Math/Geometry.h:50-351 and
// RandomSampleConsensus with HomogeneousL2NormErrorMetric<2> (src/vw/Math/RANSAC.h:77-100, :212-330).  The reference solves
// with LAPACK and its own Levenberg-Marquardt; here: the 2 x 2 polar factor in closed form, normal equations on centred points,
// an 8 x 8 elimination for the four-point DLT and a damped Gauss-Newton on Hartley-normalised points for the homography.
// include/vwgpu.h states the contract, tests/refimpl/ip_match_ref.py restates the fits with numpy, DESIGN §4.21.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "vwgpu_internal.h"

namespace {

// vwgpu_host_last_error(): every entry of this file clears it on the way in and sets it where it fails
std::string& ih_error_text() {
  static thread_local std::string text;
  return text;
}

int ih_fail(int status, const char* text) {
  ih_error_text() = text;
  return status;
}

struct ih_pt { double x, y; };
using ih_pts = std::vector<ih_pt>;

int ih_min_pairs(int kind) { return kind == VWGPU_FIT_HOMOGRAPHY ? 4 : 3; }

void ih_mul3(const double* a, const double* b, double* out) {
  double r[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[k * 3 + j];
      r[i * 3 + j] = s;
    }
  std::memcpy(out, r, sizeof r);
}

// Gaussian elimination with partial pivoting, A (n x n, row-major) x = b; both are overwritten
template <int N>
bool ih_solve(double* A, double* b, double* x) {
  for (int c = 0; c < N; ++c) {
    int piv = c;
    for (int r = c + 1; r < N; ++r)
      if (std::fabs(A[r * N + c]) > std::fabs(A[piv * N + c])) piv = r;
    if (A[piv * N + c] == 0 || !std::isfinite(A[piv * N + c])) return false;
    if (piv != c) {
      for (int k = 0; k < N; ++k) std::swap(A[c * N + k], A[piv * N + k]);
      std::swap(b[c], b[piv]);
    }
    for (int r = c + 1; r < N; ++r) {
      const double f = A[r * N + c] / A[c * N + c];
      for (int k = c; k < N; ++k) A[r * N + k] -= f * A[c * N + k];
      b[r] -= f * b[c];
    }
  }
  for (int r = N - 1; r >= 0; --r) {
    double s = b[r];
    for (int k = r + 1; k < N; ++k) s -= A[r * N + k] * x[k];
    x[r] = s / A[r * N + r];
  }
  for (int r = 0; r < N; ++r)
    if (!std::isfinite(x[r])) return false;
  return true;
}

ih_pt ih_mean(const ih_pts& p) {
  ih_pt m{0, 0};
  for (const ih_pt& q : p) { m.x += q.x; m.y += q.y; }
  m.x /= (double)p.size(); m.y /= (double)p.size();
  return m;
}

double ih_mean_dist(const ih_pts& p, ih_pt m) {
  double d = 0;
  for (const ih_pt& q : p) d += std::sqrt((q.x - m.x) * (q.x - m.x) + (q.y - m.y) * (q.y - m.y));
  return d / (double)p.size();
}

// SimilarityFittingFunctorN<2> (Geometry.h:305-347)
bool ih_similarity(const ih_pts& p1, const ih_pts& p2, double* H) {
  const ih_pt m1 = ih_mean(p1), m2 = ih_mean(p2);
  const double scale = ih_mean_dist(p2, m2) / ih_mean_dist(p1, m1);
  double a = 0, b = 0, c = 0, d = 0;   // sum (p1 - m1) (p2 - m2)^T
  for (size_t i = 0; i < p1.size(); ++i) {
    const double ax = p1[i].x - m1.x, ay = p1[i].y - m1.y, bx = p2[i].x - m2.x, by = p2[i].y - m2.y;
    a += ax * bx; b += ax * by; c += ay * bx; d += ay * by;
  }
  // U VT of the SVD is the orthogonal polar factor O of the 2 x 2 matrix: (M + cof M) normalised where det M >= 0, (M - cof M)
  // normalised (a reflection) where det M < 0; R = transpose(VT) transpose(U) = transpose(O)
  const double det = a * d - b * c;
  double o[4];
  if (det >= 0) {
    const double e = a + d, h = c - b, n = std::hypot(e, h);
    o[0] = e / n; o[1] = -h / n; o[2] = h / n; o[3] = e / n;
  } else {
    const double f = a - d, g = b + c, n = std::hypot(f, g);
    o[0] = f / n; o[1] = g / n; o[2] = g / n; o[3] = -f / n;
  }
  const double r[4] = {o[0], o[2], o[1], o[3]};
  H[0] = scale * r[0]; H[1] = scale * r[1]; H[2] = m2.x - (scale * r[0] * m1.x + scale * r[1] * m1.y);
  H[3] = scale * r[2]; H[4] = scale * r[3]; H[5] = m2.y - (scale * r[2] * m1.x + scale * r[3] * m1.y);
  H[6] = 0; H[7] = 0; H[8] = 1;
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(H[k])) return false;
  return true;
}

// AffineFittingFunctorN<2> (Geometry.h:222-270): least squares of p2 = A p1 + t
bool ih_affine(const ih_pts& p1, const ih_pts& p2, double* H) {
  const ih_pt m1 = ih_mean(p1), m2 = ih_mean(p2);
  double sxx = 0, sxy = 0, syy = 0, sxu = 0, syu = 0, sxv = 0, syv = 0;
  for (size_t i = 0; i < p1.size(); ++i) {
    const double x = p1[i].x - m1.x, y = p1[i].y - m1.y, u = p2[i].x - m2.x, v = p2[i].y - m2.y;
    sxx += x * x; sxy += x * y; syy += y * y;
    sxu += x * u; syu += y * u; sxv += x * v; syv += y * v;
  }
  const double det = sxx * syy - sxy * sxy;
  if (!(det > 0) || !std::isfinite(det)) return false;
  const double a = (syy * sxu - sxy * syu) / det, b = (sxx * syu - sxy * sxu) / det;
  const double c = (syy * sxv - sxy * syv) / det, d = (sxx * syv - sxy * sxv) / det;
  H[0] = a; H[1] = b; H[2] = m2.x - (a * m1.x + b * m1.y);
  H[3] = c; H[4] = d; H[5] = m2.y - (c * m1.x + d * m1.y);
  H[6] = 0; H[7] = 0; H[8] = 1;
  return true;
}

// NormSimilarity (Geometry.cc:66-88): {scale, tx, ty} of the matrix [s 0 -s tx; 0 s -s ty; 0 0 1]
struct ih_norm { double s, tx, ty; };
bool ih_norm_of(const ih_pts& p, ih_norm* n) {
  const ih_pt m = ih_mean(p);
  const double d = ih_mean_dist(p, m);
  n->s = std::sqrt(2.) / d; n->tx = m.x; n->ty = m.y;
  return std::isfinite(n->s);
}
void ih_norm_matrix(const ih_norm& n, double* S, double* Sinv) {
  const double s[9] = {n.s, 0, -n.s * n.tx, 0, n.s, -n.s * n.ty, 0, 0, 1};
  const double si[9] = {1 / n.s, 0, n.tx, 0, 1 / n.s, n.ty, 0, 0, 1};
  std::memcpy(S, s, sizeof s);
  std::memcpy(Sinv, si, sizeof si);
}
ih_pts ih_apply_norm(const ih_pts& p, const ih_norm& n) {
  ih_pts out(p.size());
  for (size_t i = 0; i < p.size(); ++i) out[i] = ih_pt{n.s * (p[i].x - n.tx), n.s * (p[i].y - n.ty)};
  return out;
}
bool ih_unit_corner(double* H) {
  const double w = H[8];
  if (w == 0 || !std::isfinite(w)) return false;
  for (int k = 0; k < 9; ++k) {
    H[k] /= w;
    if (!std::isfinite(H[k])) return false;
  }
  return true;
}

// the four-point branch of HomographyFittingFunctor (Geometry.h:136-147, BasicDLT Geometry.cc:90-122)
bool ih_dlt4(const ih_pt* p1, const ih_pt* p2, double* H) {
  const ih_pts in(p1, p1 + 4), out(p2, p2 + 4);
  ih_norm n1, n2;
  if (!ih_norm_of(in, &n1) || !ih_norm_of(out, &n2)) return false;
  const ih_pts x = ih_apply_norm(in, n1), y = ih_apply_norm(out, n2);
  // the rows of BasicDLT with the nullspace vector scaled to h8 = 1
  double A[64] = {0}, b[8], h[9];
  for (int i = 0; i < 4; ++i) {
    const double xi[3] = {x[i].x, x[i].y, 1.0};
    for (int j = 0; j < 3; ++j) {
      A[i * 8 + j + 3] = -xi[j];
      A[(i + 4) * 8 + j] = xi[j];
      if (j < 2) {
        A[i * 8 + j + 6] = y[i].y * xi[j];
        A[(i + 4) * 8 + j + 6] = -y[i].x * xi[j];
      }
    }
    b[i] = -y[i].y;
    b[i + 4] = y[i].x;
  }
  if (!ih_solve<8>(A, b, h)) return false;
  h[8] = 1;
  double S1[9], S1i[9], S2[9], S2i[9];
  ih_norm_matrix(n1, S1, S1i);
  ih_norm_matrix(n2, S2, S2i);
  ih_mul3(h, S1, H);
  ih_mul3(S2i, H, H);
  return ih_unit_corner(H);
}

double ih_homography_cost(const double* h, const ih_pts& x, const ih_pts& y) {
  double cost = 0;
  for (size_t i = 0; i < x.size(); ++i) {
    const double w = h[6] * x[i].x + h[7] * x[i].y + 1;
    const double ru = y[i].x - (h[0] * x[i].x + h[1] * x[i].y + h[2]) / w, rv = y[i].y - (h[3] * x[i].x + h[4] * x[i].y + h[5]) / w;
    cost += ru * ru + rv * rv;
  }
  return cost;
}

// the minimising branch (Geometry.h:149-190): sum |p2 - proj(H p1)|^2 over h0..h7 with h8 = 1.  A similarity of either side
// scales every residual alike, so the minimum is sought on Hartley-normalised points, where the normal equations are well scaled.
bool ih_homography(const ih_pts& p1, const ih_pts& p2, const double* seed, double* H) {
  if (p1.size() == 4) return ih_dlt4(p1.data(), p2.data(), H);
  double start[9];
  if (seed) std::memcpy(start, seed, sizeof start);
  else if (!ih_dlt4(p1.data(), p2.data(), start)) return false;
  ih_norm n1, n2;
  if (!ih_norm_of(p1, &n1) || !ih_norm_of(p2, &n2)) return false;
  const ih_pts x = ih_apply_norm(p1, n1), y = ih_apply_norm(p2, n2);
  double S1[9], S1i[9], S2[9], S2i[9], h[9];
  ih_norm_matrix(n1, S1, S1i);
  ih_norm_matrix(n2, S2, S2i);
  ih_mul3(start, S1i, h);
  ih_mul3(S2, h, h);
  if (!ih_unit_corner(h)) return false;
  double cost = ih_homography_cost(h, x, y), lambda = 1e-3;
  if (!std::isfinite(cost)) return false;
  for (int it = 0; it < 200 && cost > 0; ++it) {
    double A[64] = {0}, g[8] = {0};
    for (size_t i = 0; i < x.size(); ++i) {
      const double px = x[i].x, py = x[i].y;
      const double w = h[6] * px + h[7] * py + 1;
      const double u = (h[0] * px + h[1] * py + h[2]) / w, v = (h[3] * px + h[4] * py + h[5]) / w;
      const double ju[8] = {px / w, py / w, 1 / w, 0, 0, 0, -u * px / w, -u * py / w};
      const double jv[8] = {0, 0, 0, px / w, py / w, 1 / w, -v * px / w, -v * py / w};
      const double ru = y[i].x - u, rv = y[i].y - v;
      for (int r = 0; r < 8; ++r) {
        g[r] += ju[r] * ru + jv[r] * rv;
        for (int c = 0; c < 8; ++c) A[r * 8 + c] += ju[r] * ju[c] + jv[r] * jv[c];
      }
    }
    bool stepped = false, done = false;
    while (!stepped && lambda < 1e12) {
      double M[64], rhs[8], delta[8], trial[9];
      std::memcpy(M, A, sizeof M);
      std::memcpy(rhs, g, sizeof rhs);
      for (int r = 0; r < 8; ++r) M[r * 8 + r] += lambda * A[r * 8 + r];
      if (ih_solve<8>(M, rhs, delta)) {
        for (int r = 0; r < 8; ++r) trial[r] = h[r] + delta[r];
        trial[8] = 1;
        const double c = ih_homography_cost(trial, x, y);
        if (c < cost) {
          done = cost - c <= 1e-15 * cost;
          std::memcpy(h, trial, sizeof trial);
          cost = c;
          lambda = std::max(lambda * 0.1, 1e-12);
          stepped = true;
          continue;
        }
      }
      lambda *= 10;
    }
    if (!stepped || done) break;
  }
  ih_mul3(h, S1, H);
  ih_mul3(S2i, H, H);
  return ih_unit_corner(H);
}

bool ih_fit(int kind, const ih_pts& p1, const ih_pts& p2, const double* seed, double* H) {
  switch (kind) {
    case VWGPU_FIT_SIMILARITY: return ih_similarity(p1, p2, H);
    case VWGPU_FIT_AFFINE: return ih_affine(p1, p2, H);
    default: return ih_homography(p1, p2, seed, H);
  }
}

// HomogeneousL2NormErrorMetric<2> (RANSAC.h:77-100)
double ih_error(const double* H, ih_pt p1, ih_pt p2) {
  double r[3];
  for (int i = 0; i < 3; ++i) r[i] = H[i * 3] * p1.x + H[i * 3 + 1] * p1.y + H[i * 3 + 2] * 1.0;
  if (r[2] != 1) {
    const double w = r[2];
    for (int i = 0; i < 3; ++i) r[i] /= w;
  }
  const double dx = p2.x - r[0], dy = p2.y - r[1], dw = 1.0 - r[2];
  return std::sqrt(dx * dx + dy * dy + dw * dw);
}

bool ih_points(const double* p, long long n, ih_pts* out) {
  out->resize((size_t)n);
  for (long long i = 0; i < n; ++i) {
    if (!std::isfinite(p[2 * i]) || !std::isfinite(p[2 * i + 1])) return false;
    (*out)[(size_t)i] = ih_pt{p[2 * i], p[2 * i + 1]};
  }
  return true;
}

// attempt_ransac (RANSAC.h:246-330) over the caller's sample table
bool ih_attempt(int kind, const ih_pts& p1, const ih_pts& p2, const int32_t* samples, int iterations, double threshold, int min_inliers,
                double* best_H) {
  const int m = ih_min_pairs(kind);
  if (min_inliers < m) return false;
  double min_err = std::numeric_limits<double>::max();
  size_t num_inliers = 0;
  ih_pts try1, try2;
  for (int it = 0; it < iterations; ++it) {
    try1.resize(m); try2.resize(m);
    for (int i = 0; i < m; ++i) {
      try1[i] = p1[samples[(size_t)it * m + i]];
      try2[i] = p2[samples[(size_t)it * m + i]];
    }
    double H[9], H2[9];
    if (!ih_fit(kind, try1, try2, nullptr, H)) continue;
    try1.clear(); try2.clear();
    for (size_t i = 0; i < p1.size(); ++i)
      if (ih_error(H, p1[i], p2[i]) < threshold) {
        try1.push_back(p1[i]);
        try2.push_back(p2[i]);
      }
    if ((int)try1.size() < min_inliers) continue;
    if (!ih_fit(kind, try1, try2, H, H2)) continue;
    double err = 0.0;
    for (size_t i = 0; i < try1.size(); ++i) err += ih_error(H2, try1[i], try2[i]);
    err /= (double)try1.size();
    if (err < min_err) {
      min_err = err;
      std::memcpy(best_H, H2, sizeof H2);
      num_inliers = try1.size();
    }
  }
  return (long long)num_inliers >= min_inliers;
}

}  // namespace

extern "C" {

const char* vwgpu_host_last_error(void) { return ih_error_text().c_str(); }

int vwgpu_ip_remove_duplicates(const float* xy1, const float* xy2, long long n, uint8_t* keep, long long* n_kept) {
  ih_error_text().clear();
  if (n < 0 || (n > 0 && (!xy1 || !xy2 || !keep))) return ih_fail(VWGPU_ERR_ARGUMENT, "ip_remove_duplicates: null pointer or negative count");
  std::set<std::pair<float, float>> set1, set2;
  long long kept = 0;
  for (long long j = n - 1; j >= 0; --j) {   // the reverse order keeps the last repeated one
    const std::pair<float, float> a(xy1[2 * j], xy1[2 * j + 1]), b(xy2[2 * j], xy2[2 * j + 1]);
    keep[j] = 0;
    if (set1.find(a) != set1.end() || set2.find(b) != set2.end()) continue;
    set1.insert(a);
    set2.insert(b);
    keep[j] = 1;
    ++kept;
  }
  if (n_kept) *n_kept = kept;
  return VWGPU_OK;
}

int vwgpu_fit_transform(int kind, const double* p1, const double* p2, long long n, const double* seed, double* H) {
  ih_error_text().clear();
  if (!p1 || !p2 || !H) return ih_fail(VWGPU_ERR_ARGUMENT, "fit_transform: null pointer");
  if (kind < VWGPU_FIT_SIMILARITY || kind > VWGPU_FIT_HOMOGRAPHY) return ih_fail(VWGPU_ERR_ARGUMENT, "fit_transform: unknown kind");
  if (n < ih_min_pairs(kind)) return ih_fail(VWGPU_ERR_ARGUMENT, "fit_transform: insufficient data");
  ih_pts a, b;
  if (!ih_points(p1, n, &a) || !ih_points(p2, n, &b)) return ih_fail(VWGPU_ERR_ARGUMENT, "fit_transform: a coordinate is not finite");
  if (seed)
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(seed[k])) return ih_fail(VWGPU_ERR_ARGUMENT, "fit_transform: the seed is not finite");
  double out[9];
  if (!ih_fit(kind, a, b, seed, out)) return ih_fail(VWGPU_ERR_LOGIC, "fit_transform: degenerate point configuration");
  std::memcpy(H, out, sizeof out);
  return VWGPU_OK;
}

int vwgpu_ransac(int kind, const double* p1, const double* p2, long long n, const int32_t* samples, int iterations,
                 double inlier_threshold, int min_inliers, int reduce_if_no_fit, double* H, uint8_t* inlier_flags,
                 long long* num_inliers) {
  ih_error_text().clear();
  if (!p1 || !p2 || !samples || !H) return ih_fail(VWGPU_ERR_ARGUMENT, "ransac: null pointer");
  if (kind < VWGPU_FIT_SIMILARITY || kind > VWGPU_FIT_HOMOGRAPHY) return ih_fail(VWGPU_ERR_ARGUMENT, "ransac: unknown kind");
  const int m = ih_min_pairs(kind);
  if (n < m) return ih_fail(VWGPU_ERR_ARGUMENT, "RANSAC Error.  Not enough potential matches for this fitting functor.");
  if (iterations < 1) return ih_fail(VWGPU_ERR_ARGUMENT, "ransac: at least one iteration");
  if (min_inliers < m)
    return ih_fail(VWGPU_ERR_ARGUMENT, "RANSAC Error.  Number of requested inliers is less than min number of elements needed for fit.");
  if (std::isnan(inlier_threshold)) return ih_fail(VWGPU_ERR_ARGUMENT, "ransac: the threshold is NaN");
  for (int it = 0; it < iterations; ++it)
    for (int i = 0; i < m; ++i) {
      const int32_t s = samples[(size_t)it * m + i];
      if (s < 0 || s >= n) return ih_fail(VWGPU_ERR_ARGUMENT, "ransac: a sample index is out of range");
      for (int j = 0; j < i; ++j)
        if (samples[(size_t)it * m + j] == s) return ih_fail(VWGPU_ERR_ARGUMENT, "ransac: a sample row repeats an index");
    }
  ih_pts a, b;
  if (!ih_points(p1, n, &a) || !ih_points(p2, n, &b)) return ih_fail(VWGPU_ERR_ARGUMENT, "ransac: a coordinate is not finite");
  double best[9];
  bool success = false;
  for (int attempt = 0; attempt < 10; ++attempt) {   // RandomSampleConsensus::operator() (RANSAC.h:212-243)
    if ((success = ih_attempt(kind, a, b, samples, iterations, inlier_threshold, min_inliers, best))) break;
    if (!reduce_if_no_fit) break;
    min_inliers = int(min_inliers / 1.5);
    if (min_inliers < 2) break;
  }
  if (!success) return ih_fail(VWGPU_ERR_LOGIC, "RANSAC was unable to find a fit that matched the supplied data.");
  std::memcpy(H, best, sizeof best);
  long long count = 0;
  for (long long i = 0; i < n; ++i) {
    const bool in = ih_error(best, a[(size_t)i], b[(size_t)i]) < inlier_threshold;
    if (inlier_flags) inlier_flags[i] = in ? 1 : 0;
    count += in;
  }
  if (num_inliers) *num_inliers = count;
  return VWGPU_OK;
}

}  // extern "C"
