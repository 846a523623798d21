// ip_match_ref.cc — CPU restatement of the interest-point matchers (test infrastructure only): the literal serial loops of
// InterestPointMatcherSimple (src/vw/InterestPoint/Matcher.h:461-494), the index-list call of InterestPointMatcher
// (:331-381) with a brute-force two-nearest search where the reference asks FLANN, L2NormMetric and HammingMetric
// (Matcher.cc:34-102), the two constraints (:119-147) and remove_duplicates (:152-195).  Built with -ffp-contract=off:
// every float operation is rounded on its own.  Written from the reference's text, independently of ip_match.hip.
#include <cmath>
#include <cstdint>
#include <limits>
#include <set>
#include <utility>
#include <vector>

namespace {

float l2(const float* a, const float* b, int k, float maxdist) {
  float dist = 0.0;
  for (int i = 0; i < k; i++) {
    dist += (a[i] - b[i]) * (a[i] - b[i]);
    if (dist > maxdist) break;
  }
  return dist;
}

int bits(uint64_t v) {
  int n = 0;
  for (; v; v &= v - 1) ++n;
  return n;
}

// units of 8 bytes, then 4, then 1, each count added to the float as HammingMetric does
float hamming(const uint8_t* a, const uint8_t* b, int k, float maxdist) {
  float dist = 0.0;
  int d = k;
  const int num_64 = d / 8;
  d -= num_64 * 8;
  const int num_32 = d / 4;
  int i = 0;
  for (int i64 = 0; i64 < num_64; ++i64) {
    uint64_t x = 0, y = 0;
    for (int b8 = 0; b8 < 8; ++b8) {
      x |= (uint64_t)a[i + b8] << (8 * b8);
      y |= (uint64_t)b[i + b8] << (8 * b8);
    }
    i += 8;
    dist += static_cast<float>(bits(x ^ y));
    if (dist > maxdist) return dist;
  }
  for (int i32 = 0; i32 < num_32; ++i32) {
    uint32_t x = 0, y = 0;
    for (int b4 = 0; b4 < 4; ++b4) {
      x |= (uint32_t)a[i + b4] << (8 * b4);
      y |= (uint32_t)b[i + b4] << (8 * b4);
    }
    i += 4;
    dist += static_cast<float>(bits(x ^ y));
    if (dist > maxdist) return dist;
  }
  for (; i < k; ++i) dist += static_cast<float>(bits((uint8_t)(a[i] ^ b[i])));
  return dist;
}

struct Lists {
  int metric;
  const void *d1, *d2;
  long long s1, s2;
  int k;
  float distance(long long i, long long j) const {
    const float big = std::numeric_limits<float>::max();
    if (metric == 0) return l2((const float*)d1 + i * s1, (const float*)d2 + j * s2, k, big);
    return hamming((const uint8_t*)d1 + i * s1, (const uint8_t*)d2 + j * s2, k, big);
  }
};

// ConstraintT::operator()(baseline_ip, test_ip); an attribute row is {x, y, scale, orientation}
bool constraint(int kind, const double* c, const float* baseline, const float* test) {
  if (kind == 1) {
    double sr = test[2] / baseline[2];
    double od = test[3] - baseline[3];
    if (od < -M_PI) od += M_PI * 2;
    else if (od > M_PI) od -= M_PI * 2;
    return sr >= c[0] && sr <= c[1] && od >= c[2] && od <= c[3];
  }
  if (kind == 2) {
    double dx = test[0] - baseline[0];
    double dy = test[1] - baseline[1];
    return dx >= c[0] && dx <= c[1] && dy >= c[2] && dy <= c[3];
  }
  return true;
}

}  // namespace

extern "C" {

float ipr_l2(const float* a, const float* b, int k) { return l2(a, b, k, std::numeric_limits<float>::max()); }
double ipr_l2_double(const float* a, const float* b, int k) {
  double dist = 0.0;
  for (int i = 0; i < k; i++) dist += ((double)a[i] - (double)b[i]) * ((double)a[i] - (double)b[i]);
  return dist;
}
float ipr_hamming(const uint8_t* a, const uint8_t* b, int k) { return hamming(a, b, k, std::numeric_limits<float>::max()); }
int ipr_constraint(int kind, const double* bounds, const float* baseline, const float* test) {
  return constraint(kind, bounds, baseline, test) ? 1 : 0;
}

// mode 0: InterestPointMatcherSimple; mode 1: InterestPointMatcher with an exact search (ties to the lowest index; the
// entry of a point whose constraint fails is -1).  dist: the two picks as floats, +inf where a pick is missing.
void ipr_match(int metric, int mode, const void* d1, int n1, long long s1, const void* d2, int n2, long long s2, int k,
               const uint8_t* pol1, const uint8_t* pol2, const float* attr1, const float* attr2, double threshold, int ckind,
               const double* bounds, int bidirectional, int32_t* index, float* dist, long long* stats) {
  const Lists L{metric, d1, d2, s1, s2, k};
  const float inf = std::numeric_limits<float>::infinity();
  long long matched = 0;
  for (int i = 0; i < n1; i++) {
    double first_pick = 1e100, second_pick = 1e100;
    int match = -1;
    for (int j = 0; j < n2; j++) {
      if (mode == 0 && pol1 && pol1[i] != pol2[j]) continue;
      double distance = L.distance(i, j);
      if (distance < first_pick) {
        match = j;
        second_pick = first_pick;
        first_pick = distance;
      } else if (distance < second_pick) {
        second_pick = distance;
      }
    }
    if (dist) {
      dist[2 * i] = first_pick == 1e100 ? inf : (float)first_pick;
      dist[2 * i + 1] = second_pick == 1e100 ? inf : (float)second_pick;
    }
    if (mode == 0) {
      if (first_pick > threshold * second_pick) match = -1;
    } else if (second_pick == 1e100) {
      match = -1;   // fewer than two neighbours
    } else {
      const float *q = attr1 ? attr1 + 4 * (long long)i : nullptr, *nb = attr2 ? attr2 + 4 * (long long)match : nullptr;
      bool ok = true;
      if (ckind != 0) ok = bidirectional ? (constraint(ckind, bounds, q, nb) && constraint(ckind, bounds, nb, q)) : constraint(ckind, bounds, nb, q);
      if (ok) {
        double dist0 = first_pick, dist1 = second_pick;
        if (!(dist0 < threshold * dist1)) match = -1;
      } else {
        match = -1;
      }
    }
    index[i] = match;
    matched += match >= 0;
  }
  if (stats) {
    stats[0] = matched;
    stats[1] = n1;
  }
}

// keep[j] = 1 for the pairs remove_duplicates keeps; returns their number
long long ipr_remove_duplicates(const float* xy1, const float* xy2, long long n, uint8_t* keep) {
  std::set<std::pair<float, float>> ip1_set, ip2_set;
  long long kept = 0;
  for (long long i = 0; i < n; i++) {
    long long j = n - i - 1;
    keep[j] = 0;
    std::pair<float, float> ip1_pair(xy1[2 * j], xy1[2 * j + 1]);
    std::pair<float, float> ip2_pair(xy2[2 * j], xy2[2 * j + 1]);
    if (ip1_set.find(ip1_pair) != ip1_set.end() || ip2_set.find(ip2_pair) != ip2_set.end()) continue;
    ip1_set.insert(ip1_pair);
    ip2_set.insert(ip2_pair);
    keep[j] = 1;
    ++kept;
  }
  return kept;
}

}  // extern "C"
