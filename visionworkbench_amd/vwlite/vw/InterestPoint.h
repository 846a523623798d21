// vw/InterestPoint.h — the matching half of the reference's InterestPoint module and the RANSAC alignment of vw::math on
// libvwgpu.so, under the reference's names.
//   vw::ip    InterestPoint, InterestPointList (src/vw/InterestPoint/InterestPoint.h:43-130), L2NormMetric, HammingMetric,
//             NullConstraint, ScaleOrientationConstraint, PositionConstraint, InterestPointMatcher, InterestPointMatcherSimple,
//             DefaultMatcher, remove_duplicates (src/vw/InterestPoint/Matcher.h), iplist_to_vectorlist, read / write
//             _binary_ip_file, read / write_binary_match_file (src/vw/InterestPoint/MatcherIO.cc:248-445)
//   vw::math  HomographyFittingFunctor, AffineFittingFunctor, SimilarityFittingFunctor (src/vw/Math/Geometry.h),
//             InterestPointErrorMetric, RandomSampleConsensus (src/vw/Math/RANSAC.h)
// The matchers search exactly where the reference's InterestPointMatcher asks FLANN (its flann_method argument is accepted
// and ignored); where its constraint fails the entry of the index list is size_t(-1) instead of missing.
//   vw::ip    also what tools/ipfind.cc runs without OpenCV (:328-339, :395-400): IntegralImage, OBALoGInterestOperator,
//             IntegralInterestPointDetector, IntegralAutoGainDetector, detect_interest_points, SGradDescriptorGenerator,
//             SGrad2DescriptorGenerator, describe_interest_points (further down)
#ifndef VWLITE_INTERESTPOINT_H
#define VWLITE_INTERESTPOINT_H

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
#include <list>
#include <map>
#include <string>
#include <vector>

#include "Engine.h"
#include "Image.h"
#include "Math.h"

namespace vw {
namespace ip {

/// The descriptor of a point: a vector of floats that takes the fixed-size vectors of vw/Math.h.
class Descriptor : public std::vector<float> {
public:
  Descriptor() {}
  explicit Descriptor(size_t n) : std::vector<float>(n) {}
  template <class T, int N> Descriptor(Vector<T, N> const& v) { *this = v; }
  template <class T, int N> Descriptor& operator=(Vector<T, N> const& v) {
    resize(N);
    for (int i = 0; i < N; ++i) (*this)[i] = float(v[i]);
    return *this;
  }
  void set_size(size_t n) { resize(n); }
  void set_all(float v) { assign(size(), v); }
};

struct InterestPoint {
  typedef Descriptor descriptor_type;
  InterestPoint(float x = 0, float y = 0, float scale = 1.0, float interest = 0.0, float ori = 0.0, bool pol = false, uint32 octave = 0,
                uint32 scale_lvl = 0)
      : x(x), y(y), scale(scale), ix(int32(x)), iy(int32(y)), orientation(ori), interest(interest), polarity(pol), octave(octave),
        scale_lvl(scale_lvl) {}
  float x, y;
  float scale;
  int32 ix, iy;
  float orientation;
  float interest;
  bool polarity;
  uint32 octave, scale_lvl;
  descriptor_type descriptor;
  size_t size() const { return descriptor.size(); }
  float operator[](int index) { return descriptor[index]; }
  bool operator<(InterestPoint const& other) const { return other.interest < interest; }
};
typedef std::list<InterestPoint> InterestPointList;

inline std::vector<Vector3> iplist_to_vectorlist(std::vector<InterestPoint> const& iplist) {
  std::vector<Vector3> result(iplist.size());
  for (size_t i = 0; i < iplist.size(); ++i) result[i] = Vector3(iplist[i].x, iplist[i].y, 1);
  return result;
}

struct L2NormMetric { static const int vwgpu_metric = VWGPU_IP_METRIC_L2; };
struct HammingMetric { static const int vwgpu_metric = VWGPU_IP_METRIC_HAMMING; };

class NullConstraint {
public:
  static const int vwgpu_constraint = VWGPU_IP_CONSTRAINT_NONE;
  void bounds(double* b) const { b[0] = b[1] = b[2] = b[3] = 0; }
};
class ScaleOrientationConstraint {
public:
  static const int vwgpu_constraint = VWGPU_IP_CONSTRAINT_SCALE_ORIENTATION;
  double scale_ratio_min, scale_ratio_max, ori_diff_min, ori_diff_max;
  ScaleOrientationConstraint(double srmin = 0.9, double srmax = 1.1, double odmin = -0.1, double odmax = 0.1)
      : scale_ratio_min(srmin), scale_ratio_max(srmax), ori_diff_min(odmin), ori_diff_max(odmax) {}
  void bounds(double* b) const { b[0] = scale_ratio_min; b[1] = scale_ratio_max; b[2] = ori_diff_min; b[3] = ori_diff_max; }
};
class PositionConstraint {
public:
  static const int vwgpu_constraint = VWGPU_IP_CONSTRAINT_POSITION;
  double min_x, max_x, min_y, max_y;
  PositionConstraint(double _min_x = -10.0, double _max_x = 10.0, double _min_y = -10.0, double _max_y = 10.0)
      : min_x(_min_x), max_x(_max_x), min_y(_min_y), max_y(_max_y) {}
  void bounds(double* b) const { b[0] = min_x; b[1] = max_x; b[2] = min_y; b[3] = max_y; }
};

namespace detail {
// the status of an entry that takes no context, as the reference's exception
inline void check_host(int rc) {
  if (rc == VWGPU_OK) return;
  std::string msg = vwgpu_host_last_error();
  if (msg.empty()) msg = vwgpu_strerror(rc);
  if (rc == VWGPU_ERR_ARGUMENT) vw_throw(ArgumentErr() << msg);
  vw_throw(LogicErr() << msg);
}
// the lists as the library takes them; Hamming descriptors as bytes, as the reference's static_cast<uint8> makes them
struct Packed {
  std::vector<float> f;
  std::vector<uint8> b, pol;
  std::vector<float> attr;
  int n = 0, k = 0;
  const void* data(int metric) const { return metric == VWGPU_IP_METRIC_HAMMING ? (const void*)b.data() : (const void*)f.data(); }
};
template <class ListT>
Packed pack(ListT const& ips, int metric) {
  Packed p;
  p.n = (int)ips.size();
  p.k = p.n ? (int)ips.begin()->descriptor.size() : 0;
  for (InterestPoint const& ip : ips) {
    VW_ASSERT((int)ip.descriptor.size() == p.k, ArgumentErr() << "interest point descriptors differ in length");
    for (float v : ip.descriptor) {
      if (metric == VWGPU_IP_METRIC_HAMMING) {
        VW_ASSERT(v >= 0 && v <= 255 && v == float(uint8(v)), ArgumentErr() << "HammingMetric: a descriptor value is no byte");
        p.b.push_back(uint8(v));
      } else {
        p.f.push_back(v);
      }
    }
    p.pol.push_back(ip.polarity ? 1 : 0);
    const float a[4] = {ip.x, ip.y, ip.scale, ip.orientation};
    p.attr.insert(p.attr.end(), a, a + 4);
  }
  return p;
}
template <class ListT, class ConstraintT>
std::vector<int32> match(ListT const& ip1, ListT const& ip2, int metric, int mode, double threshold, ConstraintT const& constraint,
                         bool bidirectional) {
  const Packed a = pack(ip1, metric), b = pack(ip2, metric);
  std::vector<int32> index(a.n, -1);
  if (!a.n || !b.n) return index;
  VW_ASSERT(a.k == b.k, ArgumentErr() << "interest point descriptors differ in length");
  vwgpu_ip_match_params P;
  P.metric = metric; P.mode = mode; P.threshold = threshold;
  P.constraint = ConstraintT::vwgpu_constraint; P.bidirectional = bidirectional ? 1 : 0;
  constraint.bounds(P.bounds);
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_ip_match(ctx, a.data(metric), a.n, 0, b.data(metric), b.n, 0, a.k, a.pol.data(), b.pol.data(), a.attr.data(),
                                    b.attr.data(), &P, index.data(), nullptr, nullptr));
  return index;
}
template <class ListT, class MatchListT>
void pairs(ListT const& ip1, ListT const& ip2, std::vector<int32> const& index, MatchListT& matched_ip1, MatchListT& matched_ip2) {
  matched_ip1.clear();
  matched_ip2.clear();
  typename ListT::const_iterator it = ip1.begin();
  for (size_t i = 0; i < index.size(); ++i, ++it) {
    if (index[i] < 0) continue;
    typename ListT::const_iterator other = ip2.begin();
    std::advance(other, index[i]);
    matched_ip1.push_back(*it);
    matched_ip2.push_back(*other);
  }
}
}  // namespace detail

/// InterestPointMatcher (Matcher.h:156-202): the two nearest candidates by an exact search, the constraint on the nearest,
/// a match when dist0 < threshold * dist1.
template <class MetricT, class ConstraintT>
class InterestPointMatcher {
  ConstraintT m_constraint;
  double m_threshold;
  bool m_bidirectional;
public:
  InterestPointMatcher(std::string const& /*flann_method*/, double threshold = 0.5, MetricT = MetricT(), ConstraintT constraint = ConstraintT(),
                       bool bidirectional = false)
      : m_constraint(constraint), m_threshold(threshold), m_bidirectional(bidirectional) {}
  /// index_list[i] is the match of ip1[i] in ip2, or size_t(-1).
  template <class ListT, class IndexListT>
  void operator()(ListT const& ip1, ListT const& ip2, IndexListT& index_list) const {
    index_list.clear();
    if (!ip1.size() || !ip2.size()) return;
    for (int32 j : detail::match(ip1, ip2, MetricT::vwgpu_metric, VWGPU_IP_MODE_KNN, m_threshold, m_constraint, m_bidirectional))
      index_list.push_back(j < 0 ? (size_t)(-1) : (size_t)j);
  }
  template <class ListT, class MatchListT>
  void operator()(ListT const& ip1, ListT const& ip2, MatchListT& matched_ip1, MatchListT& matched_ip2) const {
    detail::pairs(ip1, ip2, detail::match(ip1, ip2, MetricT::vwgpu_metric, VWGPU_IP_MODE_KNN, m_threshold, m_constraint, m_bidirectional),
                  matched_ip1, matched_ip2);
  }
};

/// InterestPointMatcherSimple (Matcher.h:207-225): brute force over the points of equal polarity.
template <class MetricT, class ConstraintT>
class InterestPointMatcherSimple {
  ConstraintT m_constraint;
  double m_threshold;
public:
  InterestPointMatcherSimple(double threshold = 0.5, MetricT = MetricT(), ConstraintT constraint = ConstraintT())
      : m_constraint(constraint), m_threshold(threshold) {}
  template <class ListT, class MatchListT>
  void operator()(ListT const& ip1, ListT const& ip2, MatchListT& matched_ip1, MatchListT& matched_ip2) const {
    detail::pairs(ip1, ip2, detail::match(ip1, ip2, MetricT::vwgpu_metric, VWGPU_IP_MODE_SIMPLE, m_threshold, m_constraint, false), matched_ip1,
                  matched_ip2);
  }
};

typedef InterestPointMatcher<L2NormMetric, NullConstraint> DefaultMatcher;

inline void remove_duplicates(std::vector<InterestPoint>& ip1, std::vector<InterestPoint>& ip2) {
  VW_ASSERT(ip1.size() == ip2.size(), ArgumentErr() << "Input vectors are not the same size.");
  std::vector<float> a, b;
  for (size_t i = 0; i < ip1.size(); ++i) {
    a.push_back(ip1[i].x); a.push_back(ip1[i].y);
    b.push_back(ip2[i].x); b.push_back(ip2[i].y);
  }
  std::vector<uint8> keep(ip1.size());
  detail::check_host(vwgpu_ip_remove_duplicates(a.data(), b.data(), (long long)ip1.size(), keep.data(), nullptr));
  std::vector<InterestPoint> f1, f2;
  for (size_t i = 0; i < keep.size(); ++i)
    if (keep[i]) {
      f1.push_back(ip1[i]);
      f2.push_back(ip2[i]);
    }
  ip1.swap(f1);
  ip2.swap(f2);
}

// ---- files: the layout of MatcherIO.cc:248-445, little-endian ---------------------------------------------------------------
// A list is a uint64 count and its records; a record is a packed head of 45 bytes — float x, y; int32 ix, iy; float orientation,
// scale, interest; uint8 polarity; uint32 octave, scale_lvl; uint64 descriptor length — and that many floats.  A match file has
// two counts, then the records of list 1, then those of list 2.

namespace detail {
const size_t RECORD_HEAD = 45;

template <class T> void put(std::string& out, T v) { out.append(reinterpret_cast<const char*>(&v), sizeof(T)); }
template <class T> T get(const char*& at) {
  T v;
  std::memcpy(&v, at, sizeof(T));
  at += sizeof(T);
  return v;
}

template <class IterT>
std::string records(IterT begin, IterT end) {
  std::string out;
  for (IterT it = begin; it != end; ++it) {
    InterestPoint const& p = *it;
    put<float>(out, p.x); put<float>(out, p.y);
    put<int32>(out, p.ix); put<int32>(out, p.iy);
    put<float>(out, p.orientation); put<float>(out, p.scale); put<float>(out, p.interest);
    put<uint8>(out, p.polarity ? 1 : 0);
    put<uint32>(out, p.octave); put<uint32>(out, p.scale_lvl);
    put<uint64>(out, (uint64)p.descriptor.size());
    if (!p.descriptor.empty()) out.append(reinterpret_cast<const char*>(p.descriptor.data()), p.descriptor.size() * sizeof(float));
  }
  return out;
}

inline void save(std::string const& name, std::string const& bytes) {
  std::ofstream f(name.c_str(), std::ios::binary | std::ios::trunc);
  f.write(bytes.data(), (std::streamsize)bytes.size());
  f.close();
  if (!f) vw_throw(IOErr() << "Failed to write \"" << name << "\".");
}

// the whole file, or false where it cannot be opened
inline bool load(std::string const& name, std::string& bytes) {
  std::ifstream f(name.c_str(), std::ios::binary);
  if (!f.is_open()) return false;
  bytes.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
  return true;
}

// `count` records from `at`; a file that ends inside a record is refused
inline void parse_records(std::string const& name, const char*& at, const char* end, uint64 count, std::vector<InterestPoint>& out) {
  for (uint64 i = 0; i < count; ++i) {
    if ((size_t)(end - at) < RECORD_HEAD) vw_throw(IOErr() << "Failed to read interest point from file \"" << name << "\".");
    InterestPoint p;
    p.x = get<float>(at); p.y = get<float>(at);
    p.ix = get<int32>(at); p.iy = get<int32>(at);
    p.orientation = get<float>(at); p.scale = get<float>(at); p.interest = get<float>(at);
    p.polarity = get<uint8>(at) != 0;
    p.octave = get<uint32>(at); p.scale_lvl = get<uint32>(at);
    const uint64 len = get<uint64>(at);
    if (len > (uint64)(end - at) / sizeof(float)) vw_throw(IOErr() << "Failed to read interest point from file \"" << name << "\".");
    p.descriptor = Descriptor((size_t)len);
    if (len) std::memcpy(p.descriptor.data(), at, (size_t)len * sizeof(float));
    at += (size_t)len * sizeof(float);
    out.push_back(p);
  }
}
}  // namespace detail

inline void write_binary_ip_file(std::string ip_file, InterestPointList ip) {
  std::string bytes;
  detail::put<uint64>(bytes, (uint64)ip.size());
  detail::save(ip_file, bytes + detail::records(ip.begin(), ip.end()));
}

inline std::vector<InterestPoint> read_binary_ip_file(std::string ip_file) {
  std::string bytes;
  if (!detail::load(ip_file, bytes)) vw_throw(IOErr() << "Failed to open \"" << ip_file << "\" as VWIP file.");
  std::vector<InterestPoint> result;
  if (bytes.size() < sizeof(uint64)) return result;      // an empty file is an empty list, as in the reference
  const char *at = bytes.data(), *end = at + bytes.size();
  const uint64 count = detail::get<uint64>(at);
  detail::parse_records(ip_file, at, end, count, result);
  return result;
}

inline void write_binary_match_file(std::string match_file, std::vector<InterestPoint> const& ip1, std::vector<InterestPoint> const& ip2) {
  if (ip1.size() != ip2.size()) vw_throw(IOErr() << "The vectors of matching interest points must have the same size.\n");
  std::string bytes;
  detail::put<uint64>(bytes, (uint64)ip1.size());
  detail::put<uint64>(bytes, (uint64)ip2.size());
  detail::save(match_file, bytes + detail::records(ip1.begin(), ip1.end()) + detail::records(ip2.begin(), ip2.end()));
}

inline void read_binary_match_file(std::string match_file, std::vector<InterestPoint>& ip1, std::vector<InterestPoint>& ip2) {
  ip1.clear();
  ip2.clear();
  std::string bytes;
  if (!detail::load(match_file, bytes) || bytes.size() < 2 * sizeof(uint64)) return;      // a match file may be missing: nothing is written for no matches
  const char *at = bytes.data(), *end = at + bytes.size();
  const uint64 n1 = detail::get<uint64>(at), n2 = detail::get<uint64>(at);
  if (n1 != n2) vw_throw(IOErr() << "The vectors of matching interest points must have the same size.\n");
  detail::parse_records(match_file, at, end, n1, ip1);
  detail::parse_records(match_file, at, end, n2, ip2);
}

/// read_match_file / write_match_file (MatcherIO.cc): the binary form; the text form is not part of vwlite.
inline void read_match_file(std::string match_file, std::vector<InterestPoint>& ip1, std::vector<InterestPoint>& ip2, bool matches_as_txt = false) {
  if (matches_as_txt) vw_throw(NoImplErr() << "read_match_file: text match files are not implemented");
  read_binary_match_file(match_file, ip1, ip2);
}
inline void write_match_file(std::string match_file, std::vector<InterestPoint> const& ip1, std::vector<InterestPoint> const& ip2,
                             bool matches_as_txt = false) {
  if (matches_as_txt) vw_throw(NoImplErr() << "write_match_file: text match files are not implemented");
  write_binary_match_file(match_file, ip1, ip2);
}

// ---- detection and description: what tools/ipfind.cc runs without OpenCV --------------------------------------------------
// IntegralImage (IntegralImage.h:43-91), OBALoGInterestOperator (IntegralInterestOperator.h:67-159), IntegralInterestPointDetector
// and IntegralAutoGainDetector (IntegralDetector.h:40-97), detect_interest_points (DetectorBase.h:302-328),
// SGradDescriptorGenerator (Descriptor.h:120-132), SGrad2DescriptorGenerator (IntegralDescriptor.h:76-179),
// describe_interest_points (Descriptor.h:324-354).  The tile loops, the per-tile counts and the crops are host logic here; the
// pixels go through vwgpu_ip_detect and vwgpu_ip_describe.  describe_interest_points keeps the list's order where the
// reference's std::partition reorders it.

namespace detail {
inline float gray_of(float v) { return v; }
template <class T> float gray_of(PixelGray<T> const& p) { return float(p.v()); }
template <class T> float gray_of(T const& v) { return float(v); }
/// the view as dense floats (the detectors and generators take float pixels: pixel_cast<float> in ipfind.cc)
template <class ViewT>
ImageView<float> float_image(ImageViewBase<ViewT> const& view) {
  ImageView<float> img(view.impl().cols(), view.impl().rows());
  for (int32 r = 0; r < img.rows(); ++r)
    for (int32 c = 0; c < img.cols(); ++c) img(c, r) = gray_of(view.impl()(c, r));
  return img;
}
inline ImageView<float> float_image(ImageView<float> const& view) { return view; }

const int IP_TILE_SIZE = 1024;      // vw_settings().default_tile_size(), never below 1024 (DetectorBase.h:308-310)

/// One vwgpu_ip_detect call over `tiles` (rows x, y, w, h); repeated with the capacity its counts ask for when a segment is too small.
inline InterestPointList detect_tiles(ImageView<float> const& img, vwgpu_ip_detect_params const& P, std::vector<int> const& tiles,
                                      std::vector<int> const& desired) {
  const int n = (int)desired.size();
  InterestPointList out;
  if (!n || img.cols() < 1 || img.rows() < 1) return out;
  int capacity = 0;
  for (int i = 0; i < n; ++i) {
    const int limit = desired[i] > 0 ? desired[i] : P.max_points;
    if (limit <= 0) { capacity = 4096; break; }
    capacity = std::max(capacity, limit);
  }
  std::vector<int> stats(3 * (size_t)n);
  vwgpu_ctx* ctx = engine::thread_context();
  for (;;) {
    const size_t words = (size_t)n * capacity;
    std::vector<float> x(words), y(words), ori(words), scale(words), interest(words);
    std::vector<int32> ix(words), iy(words);
    vwgpu_ip_points pts = {x.data(), y.data(), ix.data(), iy.data(), ori.data(), scale.data(), interest.data()};
    const int rc = vwgpu_ip_detect(ctx, img.data(), img.cols(), img.rows(), img.cols(), tiles.data(), n, &P, desired.data(), capacity, &pts,
                                   stats.data());
    if (rc == VWGPU_ERR_CAPACITY) {
      for (int i = 0; i < n; ++i) capacity = std::max(capacity, stats[3 * i + 2]);
      continue;
    }
    engine::check(ctx, rc);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < stats[3 * i + 2]; ++k) {
        const size_t at = (size_t)i * capacity + k;
        InterestPoint p(x[at], y[at], scale[at], interest[at], ori[at]);
        p.ix = ix[at]; p.iy = iy[at];
        out.push_back(p);
      }
    return out;
  }
}
inline InterestPointList detect_whole(ImageView<float> const& img, vwgpu_ip_detect_params const& P, int desired_num_ip) {
  const int tile[4] = {0, 0, img.cols(), img.rows()};
  return detect_tiles(img, P, std::vector<int>(tile, tile + 4), std::vector<int>(1, desired_num_ip));
}
}  // namespace detail

/// IntegralImage(source): (cols + 1) x (rows + 1) floats in the reference's summation order.
template <class ViewT>
ImageView<float> IntegralImage(ImageViewBase<ViewT> const& source) {
  const ImageView<float> img = detail::float_image(source.impl());
  ImageView<float> integral(img.cols() + 1, img.rows() + 1);
  if (img.cols() < 1 || img.rows() < 1) return integral;
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_integral_image(ctx, img.data(), img.cols(), img.rows(), img.cols(), integral.data(), integral.cols()));
  return integral;
}

class OBALoGInterestOperator {
  double m_threshold;
public:
  OBALoGInterestOperator(double threshold = 0.05) : m_threshold(threshold) {}
  double threshold() const { return m_threshold; }
};

/// "obalog": a fixed threshold, the list sorted by interest whenever a limit is set, every point oriented; as in the reference a
/// point lies one pixel right and down of its extremum.
class IntegralInterestPointDetector {
  OBALoGInterestOperator m_interest;
  int m_scales, m_max_points;
public:
  static const int IP_DEFAULT_SCALES = 8;
  IntegralInterestPointDetector(int max_points = 1000, int num_scales = IP_DEFAULT_SCALES)
      : m_interest(OBALoGInterestOperator()), m_scales(num_scales), m_max_points(max_points) {}
  IntegralInterestPointDetector(OBALoGInterestOperator const& interest, int max_points = 1000)
      : m_interest(interest), m_scales(IP_DEFAULT_SCALES), m_max_points(max_points) {}
  IntegralInterestPointDetector(OBALoGInterestOperator const& interest, int scales, int max_points)
      : m_interest(interest), m_scales(scales), m_max_points(max_points) {}
  vwgpu_ip_detect_params params() const {
    vwgpu_ip_detect_params P = {VWGPU_IP_DETECTOR_OBALOG, m_scales, m_interest.threshold(), m_max_points, 0};
    return P;
  }
  template <class ViewT>
  InterestPointList process_image(ImageViewBase<ViewT> const& image, int desired_num_ip = 0) const {
    return detail::detect_whole(detail::float_image(image.impl()), params(), desired_num_ip);
  }
};

/// "iagd": the threshold is 0.1 % of each interest plane's range; no orientation.
class IntegralAutoGainDetector {
  int m_scales, m_max_points;
public:
  static const int IP_DEFAULT_SCALES = 8;
  IntegralAutoGainDetector(size_t max_points = 200, size_t scales = IP_DEFAULT_SCALES) : m_scales((int)scales), m_max_points((int)max_points) {}
  vwgpu_ip_detect_params params() const {
    vwgpu_ip_detect_params P = {VWGPU_IP_DETECTOR_IAGD, m_scales, 0.0, m_max_points, 0};
    return P;
  }
  template <class ViewT>
  InterestPointList process_image(ImageViewBase<ViewT> const& image, int desired_num_ip = 0) const {
    return detail::detect_whole(detail::float_image(image.impl()), params(), desired_num_ip);
  }
};

/// Every 1024 x 1024 tile is an independent crop; the points are shifted by the tile's origin and appended in tile order; a
/// tile is asked for ceil(area / 1024^2 * desired_num_ip) points, kept within [1, desired_num_ip].  One library call.
template <class ViewT, class DetectorT>
InterestPointList detect_interest_points(ImageViewBase<ViewT> const& view, DetectorT& detector, int desired_num_ip = 0) {
  const ImageView<float> img = detail::float_image(view.impl());
  const int tile_size = detail::IP_TILE_SIZE;
  std::vector<int> tiles, desired;
  for (int y = 0; y < img.rows(); y += tile_size)
    for (int x = 0; x < img.cols(); x += tile_size) {
      const int w = std::min(tile_size, img.cols() - x), h = std::min(tile_size, img.rows() - y);
      const int t[4] = {x, y, w, h};
      tiles.insert(tiles.end(), t, t + 4);
      int num_ip = 0;
      if (desired_num_ip > 0) {
        const double expected_area = (double)tile_size * tile_size, area = (double)w * h;
        num_ip = (int)std::ceil(area / expected_area * static_cast<double>(desired_num_ip));
        if (num_ip < 1) num_ip = 1;
        if (num_ip > desired_num_ip) num_ip = desired_num_ip;
      }
      desired.push_back(num_ip);
    }
  return detail::detect_tiles(img, detector.params(), tiles, desired);
}

namespace detail {
/// The crop InterestPointDescriptionTask rasterises (Descriptor.h:261-277): the union of reverse_bbox of every point's support
/// square under its affine map, expanded by 1.  It may leave the image.
inline void description_crop(std::vector<InterestPoint*> const& pts, int support_size, int* crop) {
  const float half_size = ((float)(support_size - 1)) / 2.0f;
  bool first = true;
  int lo[2] = {0, 0}, hi[2] = {0, 0};
  for (const InterestPoint* it : pts) {
    const float scaling = 1.0f / it->scale;
    const double c = std::cos((double)(-it->orientation)), s = std::sin((double)(-it->orientation));
    const double sc = scaling, x = it->x, y = it->y;
    const double ma = sc * c, mb = -sc * s, mc = sc * s, md = sc * c;
    const double mx = sc * (s * y - c * x) + (double)half_size, my = -sc * (s * x + c * y) + (double)half_size;
    const double det = ma * md - mb * mc;
    const double ai = md / det, bi = -mb / det, ci = -mc / det, di = ma / det;
    double bmin[2] = {0, 0}, bmax[2] = {0, 0};
    const int corner[4][2] = {{0, 0}, {support_size - 1, 0}, {0, support_size - 1}, {support_size - 1, support_size - 1}};
    for (int k = 0; k < 4; ++k) {
      const double qx = corner[k][0] - mx, qy = corner[k][1] - my;
      const double r[2] = {ai * qx + bi * qy, ci * qx + di * qy};
      for (int d = 0; d < 2; ++d) {
        if (k == 0 || r[d] < bmin[d]) bmin[d] = r[d];
        if (k == 0 || r[d] > bmax[d]) bmax[d] = r[d];
      }
    }
    for (int d = 0; d < 2; ++d) {      // grow_bbox_to_int (BBox.tcc:368-389), then the union
      const int a0 = (int)std::floor(bmin[d]), a1 = (int)std::floor(bmax[d]) + 1;
      if (first || a0 < lo[d]) lo[d] = a0;
      if (first || a1 > hi[d]) hi[d] = a1;
    }
    first = false;
  }
  crop[0] = lo[0] - 1; crop[1] = lo[1] - 1; crop[2] = hi[0] - lo[0] + 2; crop[3] = hi[1] - lo[1] + 2;
}
inline void describe_on_crop(ImageView<float> const& img, const int* crop, std::vector<InterestPoint*> const& pts, int kind, int k) {
  const int n = (int)pts.size();
  if (!n) return;
  std::vector<float> x(n), y(n), scale(n), ori(n), desc((size_t)n * k);
  for (int i = 0; i < n; ++i) { x[i] = pts[i]->x; y[i] = pts[i]->y; scale[i] = pts[i]->scale; ori[i] = pts[i]->orientation; }
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_ip_describe(ctx, img.data(), img.cols(), img.rows(), img.cols(), crop, n, x.data(), y.data(), scale.data(),
                                       ori.data(), kind, desc.data(), k));
  for (int i = 0; i < n; ++i) {
    pts[i]->descriptor.set_size(k);
    std::copy(desc.begin() + (size_t)i * k, desc.begin() + (size_t)(i + 1) * k, pts[i]->descriptor.begin());
  }
}
template <int KIND, int SUPPORT, int SIZE>
struct DescriptorGenerator {
  static const int vwgpu_descriptor = KIND;
  int support_size() { return SUPPORT; }
  int descriptor_size() { return SIZE; }
  /// The generator on the image it is given: operator()(image, points).
  template <class ViewT>
  void operator()(ImageViewBase<ViewT> const& image, InterestPointList& points) {
    const ImageView<float> img = float_image(image.impl());
    std::vector<InterestPoint*> pts;
    for (InterestPoint& p : points) pts.push_back(&p);
    const int crop[4] = {0, 0, img.cols(), img.rows()};
    describe_on_crop(img, crop, pts, KIND, SIZE);
  }
};
}  // namespace detail

struct SGradDescriptorGenerator : detail::DescriptorGenerator<VWGPU_IP_DESCRIPTOR_SGRAD, 42, 180> {};
struct SGrad2DescriptorGenerator : detail::DescriptorGenerator<VWGPU_IP_DESCRIPTOR_SGRAD2, 41, 128> {};

/// The points are grouped by the 1024 x 1024 tile that holds them (their truncated x, y); every group is described on its own
/// crop.  A point outside the image belongs to no tile: ArgumentErr (the reference leaves it undescribed).
template <class ViewT, class DescriptorT>
void describe_interest_points(ImageViewBase<ViewT> const& view, DescriptorT& descriptor, InterestPointList& list) {
  const ImageView<float> img = detail::float_image(view.impl());
  const int tile_size = detail::IP_TILE_SIZE, across = (img.cols() + tile_size - 1) / tile_size;
  std::map<int, std::vector<InterestPoint*>> groups;
  for (InterestPoint& p : list) {
    const int tx = int32(p.x), ty = int32(p.y);
    VW_ASSERT(tx >= 0 && ty >= 0 && tx < img.cols() && ty < img.rows(), ArgumentErr() << "describe_interest_points: a point lies outside the image");
    groups[(ty / tile_size) * across + tx / tile_size].push_back(&p);
  }
  for (auto& g : groups) {
    int crop[4];
    detail::description_crop(g.second, descriptor.support_size(), crop);
    detail::describe_on_crop(img, crop, g.second, DescriptorT::vwgpu_descriptor, descriptor.descriptor_size());
  }
}

}  // namespace ip

namespace math {

namespace detail {
template <class ContainerT>
std::vector<double> flatten(std::vector<ContainerT> const& p) {
  std::vector<double> out;
  out.reserve(2 * p.size());
  for (ContainerT const& v : p) {
    out.push_back(v[0]);
    out.push_back(v[1]);
  }
  return out;
}
template <int KIND, int MIN>
struct FittingFunctor {
  typedef Matrix3x3 result_type;
  static const int vwgpu_kind = KIND;
  template <class ContainerT> size_t min_elements_needed_for_fit(ContainerT const&) const { return MIN; }
  template <class ContainerT>
  Matrix3x3 operator()(std::vector<ContainerT> const& p1, std::vector<ContainerT> const& p2, const Matrix3x3* seed = nullptr) const {
    VW_ASSERT(p1.size() == p2.size(), ArgumentErr() << "Cannot compute the transformation.  p1 and p2 are not the same size.");
    const std::vector<double> a = flatten(p1), b = flatten(p2);
    double H[9];
    ip::detail::check_host(vwgpu_fit_transform(KIND, a.data(), b.data(), (long long)p1.size(), seed ? seed->data() : nullptr, H));
    Matrix3x3 out;
    for (int i = 0; i < 9; ++i) out(i / 3, i % 3) = H[i];
    return out;
  }
  template <class ContainerT>
  Matrix3x3 operator()(std::vector<ContainerT> const& p1, std::vector<ContainerT> const& p2, Matrix3x3 const& seed) const {
    return (*this)(p1, p2, &seed);
  }
};
}  // namespace detail

typedef detail::FittingFunctor<VWGPU_FIT_HOMOGRAPHY, 4> HomographyFittingFunctor;
typedef detail::FittingFunctor<VWGPU_FIT_AFFINE, 3> AffineFittingFunctor;
typedef detail::FittingFunctor<VWGPU_FIT_SIMILARITY, 3> SimilarityFittingFunctor;

/// HomogeneousL2NormErrorMetric<2> (RANSAC.h:77-100).
struct InterestPointErrorMetric {
  template <class ContainerT>
  double operator()(Matrix3x3 const& H, ContainerT const& p1, ContainerT const& p2) const {
    double r[3];
    for (int i = 0; i < 3; ++i) r[i] = H(i, 0) * p1[0] + H(i, 1) * p1[1] + H(i, 2) * 1.0;
    if (r[2] != 1) {
      const double w = r[2];
      for (int i = 0; i < 3; ++i) r[i] /= w;
    }
    const double dx = p2[0] - r[0], dy = p2[1] - r[1], dw = 1.0 - r[2];
    return std::sqrt(dx * dx + dy * dy + dw * dw);
  }
};

VWLITE_EXCEPTION(RANSACErr, Exception);

/// RandomSampleConsensus (RANSAC.h:109-332) for the three functors above and InterestPointErrorMetric.  The sample table is
/// drawn with the reference's formula from rand() (:144-148), for every iteration before the first; the search is
/// vwgpu_ransac's.
template <class FittingFuncT, class ErrorFuncT>
class RandomSampleConsensus {
  ErrorFuncT m_error_func;
  int m_num_iterations;
  double m_inlier_threshold;
  int m_min_num_output_inliers;
  bool m_reduce_min_num_output_inliers_if_no_fit;

  // One row of the sample table: n distinct indices below `count`, each drawn as int(rand() / (RAND_MAX + 1.0) * count)
  // (RANSAC.h:144-148) and drawn again while it repeats an earlier one of the row.
  static void draw_row(int count, int32* row, int n) {
    VW_ASSERT(count >= n, ArgumentErr() << "Not enough samples (" << n << " / " << count << ")\n");
    for (int filled = 0; filled < n;) {
      const int32 pick = int(std::rand() / (RAND_MAX + 1.0) * count);
      if (std::find(row, row + filled, pick) == row + filled) row[filled++] = pick;
    }
  }
  template <class ContainerT1, class ContainerT2>
  bool is_inlier(Matrix3x3 const& H, ContainerT1 const& a, ContainerT2 const& b) const { return m_error_func(H, a, b) < m_inlier_threshold; }

public:
  RandomSampleConsensus(FittingFuncT const& /*fitting_func*/, ErrorFuncT const& error_func, int num_iterations, double inlier_threshold,
                        int min_num_output_inliers, bool reduce_min_num_output_inliers_if_no_fit = false, int /*num_threads*/ = 1)
      : m_error_func(error_func), m_num_iterations(num_iterations), m_inlier_threshold(inlier_threshold),
        m_min_num_output_inliers(min_num_output_inliers),
        m_reduce_min_num_output_inliers_if_no_fit(reduce_min_num_output_inliers_if_no_fit) {}

  /// The pairs whose error under H is below the threshold, as two lists.
  template <class ContainerT1, class ContainerT2>
  void inliers(Matrix3x3 const& H, std::vector<ContainerT1> const& p1, std::vector<ContainerT2> const& p2, std::vector<ContainerT1>& inliers1,
               std::vector<ContainerT2>& inliers2) const {
    std::vector<ContainerT1> kept1;
    std::vector<ContainerT2> kept2;
    for (size_t i : inlier_indices(H, p1, p2)) {
      kept1.push_back(p1[i]);
      kept2.push_back(p2[i]);
    }
    inliers1.swap(kept1);
    inliers2.swap(kept2);
  }

  /// Their positions in the lists.
  template <class ContainerT1, class ContainerT2>
  std::vector<size_t> inlier_indices(Matrix3x3 const& H, std::vector<ContainerT1> const& p1, std::vector<ContainerT2> const& p2) const {
    std::vector<size_t> where;
    const size_t n = std::min(p1.size(), p2.size());
    for (size_t i = 0; i < n; ++i)
      if (is_inlier(H, p1[i], p2[i])) where.push_back(i);
    return where;
  }

  template <class ContainerT1, class ContainerT2>
  Matrix3x3 operator()(std::vector<ContainerT1> const& p1, std::vector<ContainerT2> const& p2) {
    VW_ASSERT(!p1.empty(), RANSACErr() << "RANSAC Error.  Insufficient data.\n");
    VW_ASSERT(p1.size() == p2.size(), RANSACErr() << "RANSAC Error.  Data vectors are not the same size.");
    const int m = (int)FittingFuncT().min_elements_needed_for_fit(p1[0]);
    VW_ASSERT((int)p1.size() >= m, RANSACErr() << "RANSAC Error.  Not enough potential matches for this fitting functor. (" << p1.size() << "/"
                                               << m << ")\n");
    std::vector<int32> samples((size_t)m_num_iterations * m);
    for (int it = 0; it < m_num_iterations; ++it) draw_row((int)p1.size(), &samples[(size_t)it * m], m);
    const std::vector<double> a = detail::flatten(p1), b = detail::flatten(p2);
    double H[9];
    const int rc = vwgpu_ransac(FittingFuncT::vwgpu_kind, a.data(), b.data(), (long long)p1.size(), samples.data(), m_num_iterations,
                                m_inlier_threshold, m_min_num_output_inliers, m_reduce_min_num_output_inliers_if_no_fit ? 1 : 0, H, nullptr,
                                nullptr);
    if (rc != VWGPU_OK) vw_throw(RANSACErr() << vwgpu_host_last_error());
    Matrix3x3 out;
    for (int i = 0; i < 9; ++i) out(i / 3, i % 3) = H[i];
    return out;
  }
};

}  // namespace math
}  // namespace vw
#endif
