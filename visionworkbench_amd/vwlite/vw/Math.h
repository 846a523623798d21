// vw/Math.h — Vector2i/Vector2f and the half-open integer box BBox2i with the semantics of
// src/vw/Math/BBox.tcc:82-197,268-290; Matrix3x3 and HomographyTransform
// (src/vw/Math/Transform.h:365-389); math::Histogram (src/vw/Math/Statistics.h, Statistics.cc:34-104), the container that
// vw::histogram of vw/Image.h fills on the engine.
#ifndef VWLITE_MATH_H
#define VWLITE_MATH_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <ostream>
#include <vector>

#include "Core.h"

namespace vw {

template <class T, int N>
class Vector {
  T m[N];
public:
  Vector() { for (int i = 0; i < N; ++i) m[i] = T(); }
  Vector(T a, T b) { static_assert(N == 2, "2-vector ctor"); m[0] = a; m[1] = b; }
  Vector(T a, T b, T c) { static_assert(N == 3, "3-vector ctor"); m[0] = a; m[1] = b; m[2] = c; }
  template <class U> Vector(Vector<U, N> const& o) { for (int i = 0; i < N; ++i) m[i] = T(o[i]); }
  T& operator[](int i) { return m[i]; }
  T const& operator[](int i) const { return m[i]; }
  T& x() { return m[0]; }  T const& x() const { return m[0]; }
  T& y() { return m[1]; }  T const& y() const { return m[1]; }
  Vector& operator+=(Vector const& o) { for (int i = 0; i < N; ++i) m[i] += o.m[i]; return *this; }
  Vector& operator-=(Vector const& o) { for (int i = 0; i < N; ++i) m[i] -= o.m[i]; return *this; }
  bool operator==(Vector const& o) const { for (int i = 0; i < N; ++i) if (m[i] != o.m[i]) return false; return true; }
  bool operator!=(Vector const& o) const { return !(*this == o); }
};
template <class T, int N> Vector<T, N> operator+(Vector<T, N> a, Vector<T, N> const& b) { return a += b; }
template <class T, int N> Vector<T, N> operator-(Vector<T, N> a, Vector<T, N> const& b) { return a -= b; }
template <class T, int N> Vector<T, N> operator*(Vector<T, N> a, T s) { for (int i = 0; i < N; ++i) a[i] *= s; return a; }
template <class T, int N> Vector<T, N> operator*(T s, Vector<T, N> a) { for (int i = 0; i < N; ++i) a[i] = s * a[i]; return a; }
template <class T, int N> Vector<T, N> operator/(Vector<T, N> a, T s) { for (int i = 0; i < N; ++i) a[i] /= s; return a; }
template <class T, int N> T prod(Vector<T, N> const& v) { T p = 1; for (int i = 0; i < N; ++i) p *= v[i]; return p; }
template <class T, int N> std::ostream& operator<<(std::ostream& o, Vector<T, N> const& v) {
  o << "Vector" << N << "(";
  for (int i = 0; i < N; ++i) o << (i ? "," : "") << v[i];
  return o << ")";
}
typedef Vector<int32, 2> Vector2i;
typedef Vector<float, 2> Vector2f;
typedef Vector<double, 2> Vector2;
typedef Vector<double, 3> Vector3;

// Half-open box [min, max).  An empty box reports zero width/height/area (BBox.tcc:156-174).
class BBox2i {
  Vector2i m_min, m_max;
public:
  // default = empty, with the reference's +-(INT32_MAX - 1) corners (src/vw/Math/BBox.tcc:37-45)
  BBox2i() : m_min(0x7ffffffe, 0x7ffffffe), m_max(-0x7ffffffe, -0x7ffffffe) {}
  BBox2i(Vector2i const& mn, Vector2i const& mx) : m_min(mn), m_max(mx) {}
  BBox2i(int32 x, int32 y, int32 w, int32 h) : m_min(x, y), m_max(x + w, y + h) {}
  Vector2i& min() { return m_min; }  Vector2i const& min() const { return m_min; }
  Vector2i& max() { return m_max; }  Vector2i const& max() const { return m_max; }
  bool empty() const { return m_min[0] >= m_max[0] || m_min[1] >= m_max[1]; }
  int32 width() const { return empty() ? 0 : m_max[0] - m_min[0]; }
  int32 height() const { return empty() ? 0 : m_max[1] - m_min[1]; }
  int64 area() const { return (int64)width() * height(); }
  Vector2i size() const { return m_max - m_min; }
  void grow(Vector2i const& p) {            // include a point: max becomes p itself (BBox.tcc:82-92)
    for (int i = 0; i < 2; ++i) { if (p[i] > m_max[i]) m_max[i] = p[i]; if (p[i] < m_min[i]) m_min[i] = p[i]; }
  }
  void grow(BBox2i const& b) { if (!b.empty()) { grow(b.min()); grow(b.max()); } }
  void crop(BBox2i const& b) {              // intersect
    for (int i = 0; i < 2; ++i) { m_min[i] = std::max(m_min[i], b.m_min[i]); m_max[i] = std::min(m_max[i], b.m_max[i]); }
  }
  void expand(int32 n) { if (empty()) return; m_min -= Vector2i(n, n); m_max += Vector2i(n, n); }
  void contract(int32 n) { expand(-n); }
  bool contains(Vector2i const& p) const { return p[0] >= m_min[0] && p[0] < m_max[0] && p[1] >= m_min[1] && p[1] < m_max[1]; }
  bool contains(BBox2i const& b) const {
    return b.m_min[0] >= m_min[0] && b.m_min[1] >= m_min[1] && b.m_max[0] <= m_max[0] && b.m_max[1] <= m_max[1];
  }
  BBox2i& operator+=(Vector2i const& v) { if (!empty()) { m_min += v; m_max += v; } return *this; }
  BBox2i& operator-=(Vector2i const& v) { if (!empty()) { m_min -= v; m_max -= v; } return *this; }
  BBox2i& operator*=(int32 s) { if (!empty()) { m_min = m_min * s; m_max = m_max * s; } return *this; }
  BBox2i& operator/=(int32 s) { if (!empty()) { m_min = m_min / s; m_max = m_max / s; } return *this; }
  bool operator==(BBox2i const& o) const { return m_min == o.m_min && m_max == o.m_max; }
};
inline BBox2i operator+(BBox2i b, Vector2i const& v) { return b += v; }
inline BBox2i operator-(BBox2i b, Vector2i const& v) { return b -= v; }
inline BBox2i operator*(BBox2i b, int32 s) { return b *= s; }
inline BBox2i operator/(BBox2i b, int32 s) { return b /= s; }
inline std::ostream& operator<<(std::ostream& o, BBox2i const& b) {
  return o << "(" << b.min() << "-" << b.max() << ")";
}

// A row-major 3 x 3 double matrix, as much of vw::Matrix3x3 as a homography needs.
class Matrix3x3 {
  double m[9];
public:
  Matrix3x3() { for (int i = 0; i < 9; ++i) m[i] = 0.0; }
  void set_identity() { for (int i = 0; i < 9; ++i) m[i] = (i % 4 == 0) ? 1.0 : 0.0; }
  double& operator()(int r, int c) { return m[r * 3 + c]; }
  double const& operator()(int r, int c) const { return m[r * 3 + c]; }
  const double* data() const { return m; }
};
// The adjugate over the determinant.  The bits of the reference's inverse() (an LU solve) are not pinned.
inline Matrix3x3 inverse(Matrix3x3 const& h) {
  const double a = h(0, 0), b = h(0, 1), c = h(0, 2), d = h(1, 0), e = h(1, 1), f = h(1, 2), g = h(2, 0), i = h(2, 1), j = h(2, 2);
  const double det = a * (e * j - f * i) - b * (d * j - f * g) + c * (d * i - e * g);
  Matrix3x3 r;
  r(0, 0) = (e * j - f * i) / det; r(0, 1) = (c * i - b * j) / det; r(0, 2) = (b * f - c * e) / det;
  r(1, 0) = (f * g - d * j) / det; r(1, 1) = (a * j - c * g) / det; r(1, 2) = (c * d - a * f) / det;
  r(2, 0) = (d * i - e * g) / det; r(2, 1) = (b * g - a * i) / det; r(2, 2) = (a * e - b * d) / det;
  return r;
}

// HomographyTransform (src/vw/Math/Transform.h:369-389): forward applies H, reverse its inverse; w first, then the
// two quotients.
class HomographyTransform {
  Matrix3x3 m_H, m_H_inverse;
  static Vector2 apply(Matrix3x3 const& m, Vector2 const& p) {
    const double w = m(2, 0) * p[0] + m(2, 1) * p[1] + m(2, 2);
    return Vector2((m(0, 0) * p[0] + m(0, 1) * p[1] + m(0, 2)) / w, (m(1, 0) * p[0] + m(1, 1) * p[1] + m(1, 2)) / w);
  }
public:
  HomographyTransform(Matrix3x3 const& H) : m_H(H), m_H_inverse(inverse(H)) {}
  Vector2 forward(Vector2 const& p) const { return apply(m_H, p); }
  Vector2 reverse(Vector2 const& p) const { return apply(m_H_inverse, p); }
  Matrix3x3 const& matrix() const { return m_H; }
  Matrix3x3 const& inverse_matrix() const { return m_H_inverse; }
};

namespace math {
/// math::Histogram (src/vw/Math/Statistics.cc:34-104) with integer counts.  vw::histogram (vw/Image.h) fills it on the engine;
/// add_value is the host form of the same binning (saturate = true), a NaN bin argument is dropped.
class Histogram {
  int m_num_bins, m_max_bin;
  uint64_t m_num_values;
  double m_min_value, m_max_value, m_range, m_bin_width;
  std::vector<uint64_t> m_bin_values;
public:
  Histogram() : m_num_bins(0), m_max_bin(0), m_num_values(0), m_min_value(0), m_max_value(0), m_range(0), m_bin_width(0) {}
  Histogram(size_t num_bins, double min_value, double max_value) { initialize(num_bins, min_value, max_value); }
  void initialize(size_t num_bins, double min_value, double max_value) {
    if (num_bins == 0) vw_throw(ArgumentErr() << "Can't create a Histogram with zero bins!");
    m_num_bins = (int)num_bins; m_max_bin = (int)num_bins - 1; m_num_values = 0;
    m_min_value = min_value; m_max_value = max_value;
    m_range = max_value - min_value;
    m_bin_width = m_range / num_bins;
    m_bin_values.assign(num_bins, 0);
  }
  void add_value(double value) {
    const double r = std::round(m_max_bin * ((value - m_min_value) / m_range));
    if (r != r) return;
    m_bin_values[r < 0 ? 0 : r >= m_num_bins ? m_max_bin : (int)r] += 1;
    ++m_num_values;
  }
  void operator()(double value) { add_value(value); }
  /// The counts as the engine returns them: num_bins bins, then the total.
  void set_counts(const uint64_t* counts) {
    m_bin_values.assign(counts, counts + m_num_bins);
    m_num_values = counts[m_num_bins];
  }
  int get_num_bins() const { return m_num_bins; }
  uint64_t get_total_num_values() const { return m_num_values; }
  double get_bin_value(int i) const { return (double)m_bin_values[i]; }
  double get_bin_width() const { return m_bin_width; }
  double get_bin_center(int i) const { return m_min_value + i * m_bin_width + m_bin_width / 2.0; }
  double get_min_value() const { return m_min_value; }
  double get_max_value() const { return m_max_value; }
  const uint64_t* counts() const { return m_bin_values.data(); }
  size_t get_percentile(double percentile) const {
    if ((percentile < 0) || (percentile > 1.0)) vw_throw(ArgumentErr() << "get_histogram_percentile: illegal percentile request: " << percentile << "\n");
    const double sum = static_cast<double>(m_num_values);
    double running_percentile = 0;
    for (int i = 0; i < m_num_bins; ++i) {
      running_percentile += get_bin_value(i) / sum;
      if (running_percentile >= percentile) return i;
    }
    vw_throw(LogicErr() << "get_histogram_percentile: Illegal histogram encountered!");
    return 0;
  }
};
}  // namespace math

}  // namespace vw
#endif
