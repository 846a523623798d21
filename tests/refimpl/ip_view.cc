// ip_view.cc — the C++ surface of vw::ip matching and the RANSAC alignment (vwlite vw/InterestPoint.h), as a reference user
// would call it.
//   ip_view pairs.match list1.vwip list2.vwip expected.bin image.bin cols rows prefix
//       list1.vwip, list2.vwip  two point lists whose ix is the point's row number
//       expected.bin            int32: n1, then n1 indices for DefaultMatcher (-1 = none), then n1 for InterestPointMatcherSimple
//       pairs.match             matched pairs, aligned as tools/correlate.cc:153-164 does
//       image.bin               cols x rows floats, the "right image" that is warped by the alignment
//   Writes prefix.meta (doubles: the 9 words of the alignment, the number of pairs, the number of inlier indices, then the
//   inlier indices) and prefix.aligned (cols x rows floats).
// Exit status: 0 done, 1 any error, 3 a matcher disagrees with expected.bin.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <vw/InterestPoint.h>
#include <vw/Transform.h>

namespace {
using namespace vw;

template <class T>
bool read_raw(std::string const& path, std::vector<T>& data) {
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  data.resize((size_t)bytes / sizeof(T));
  const size_t got = std::fread(data.data(), sizeof(T), data.size(), f);
  std::fclose(f);
  return got == data.size();
}
template <class T>
bool write_raw(std::string const& path, const T* data, size_t n) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const size_t put = std::fwrite(data, sizeof(T), n, f);
  return std::fclose(f) == 0 && put == n;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 9) {
    std::fprintf(stderr, "usage: %s pairs.match list1.vwip list2.vwip expected.bin image.bin cols rows prefix\n", argv[0]);
    return 2;
  }
  try {
    const std::string match_file = argv[1], prefix = argv[8];
    const int cols = std::atoi(argv[6]), rows = std::atoi(argv[7]);

    // the matchers
    std::vector<ip::InterestPoint> ip1 = ip::read_binary_ip_file(argv[2]), ip2 = ip::read_binary_ip_file(argv[3]);
    std::vector<int32> expected;
    if (!read_raw(argv[4], expected) || expected.empty() || expected[0] != (int32)ip1.size() || expected.size() != 1 + 2 * ip1.size()) return 1;
    const size_t n1 = ip1.size();
    std::vector<size_t> matched_indexes;
    ip::DefaultMatcher matcher("kmeans");
    matcher(ip1, ip2, matched_indexes);
    if (matched_indexes.size() != n1) return 3;
    for (size_t i = 0; i < n1; ++i)
      if (matched_indexes[i] != (expected[1 + i] < 0 ? (size_t)(-1) : (size_t)expected[1 + i])) {
        std::fprintf(stderr, "ip_view: DefaultMatcher point %zu: %zd, expected %d\n", i, (ssize_t)matched_indexes[i], expected[1 + i]);
        return 3;
      }
    std::vector<ip::InterestPoint> matched_ip1, matched_ip2, knn_ip1, knn_ip2;
    matcher(ip1, ip2, knn_ip1, knn_ip2);
    ip::InterestPointMatcherSimple<ip::L2NormMetric, ip::NullConstraint> simple(0.5);
    simple(ip1, ip2, matched_ip1, matched_ip2);
    std::vector<int32> got(n1, -1), got_knn(n1, -1);
    for (size_t i = 0; i < matched_ip1.size(); ++i) got[matched_ip1[i].ix] = matched_ip2[i].ix;
    for (size_t i = 0; i < knn_ip1.size(); ++i) got_knn[knn_ip1[i].ix] = knn_ip2[i].ix;
    for (size_t i = 0; i < n1; ++i)
      if (got[i] != expected[1 + n1 + i] || got_knn[i] != expected[1 + i]) {
        std::fprintf(stderr, "ip_view: point %zu: simple %d (expected %d), pair-list %d (expected %d)\n", i, got[i], expected[1 + n1 + i],
                     got_knn[i], expected[1 + i]);
        return 3;
      }
    ip::remove_duplicates(matched_ip1, matched_ip2);
    if (matched_ip1.size() != matched_ip2.size()) return 1;

    // tools/correlate.cc:153-164
    Matrix3x3 alignment;
    std::vector<ip::InterestPoint> pair_ip1, pair_ip2;
    bool matches_as_txt = false;
    ip::read_match_file(match_file, pair_ip1, pair_ip2, matches_as_txt);
    std::vector<Vector3> ransac_ip1 = ip::iplist_to_vectorlist(pair_ip1);
    std::vector<Vector3> ransac_ip2 = ip::iplist_to_vectorlist(pair_ip2);
    vw::math::RandomSampleConsensus<vw::math::HomographyFittingFunctor, vw::math::InterestPointErrorMetric>
        ransac( vw::math::HomographyFittingFunctor(), vw::math::InterestPointErrorMetric(), 100, 30, ransac_ip1.size()/2, true );
    alignment = ransac( ransac_ip2, ransac_ip1 );

    ImageView<float> right_image(cols, rows);
    std::vector<float> pixels;
    if (!read_raw(argv[5], pixels) || pixels.size() != (size_t)cols * rows) return 1;
    for (size_t i = 0; i < pixels.size(); ++i) right_image.data()[i] = pixels[i];
    ImageView<float> aligned = transform(right_image, HomographyTransform(alignment));

    std::vector<size_t> inl = ransac.inlier_indices(alignment, ransac_ip2, ransac_ip1);
    std::vector<double> meta;
    for (int i = 0; i < 9; ++i) meta.push_back(alignment(i / 3, i % 3));
    meta.push_back((double)ransac_ip1.size());
    meta.push_back((double)inl.size());
    for (size_t i : inl) meta.push_back((double)i);
    if (!write_raw(prefix + ".meta", meta.data(), meta.size()) || !write_raw(prefix + ".aligned", aligned.data(), (size_t)cols * rows)) return 1;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "ip_view: %s\n", e.what());
    return 1;
  }
  std::printf("ip_view ok\n");
  return 0;
}
