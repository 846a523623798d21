// ip_atan2.h — one atan2f for the host and the device.  The orientation of IntegralInterestPointDetector
// (src/vw/InterestPoint/IntegralDetector.cc:37-104) sorts 113 angles into slices by comparing them with the slice edges, so an
// angle that differs by one ulp between two libraries moves a sample in or out of a slice and the orientation jumps.  As
// em_exp.h does for exp, this form uses IEEE double additions, multiplications and divisions only, which round the same
// everywhere (no contraction: -ffp-contract=off), and rounds the result to float once.  ip_detect.hip runs it in the kernel,
// tests/refimpl/ip_detect_ref.cc in the restatement.
//
// Method: q = min(|y|, |x|) / max(|y|, |x|) in [0, 1]; c = the nearest multiple of 1/8; t = (q - c) / (1 + q c), |t| <= 1/16;
// atan q = atan c + (t - t^3/3 + t^5/5 - ... - t^15/15), the series' remainder below 16^-17 / 17 = 2e-22; then the octant.
// The double result is within a few 1e-16 of atan2, so its float rounding is the correctly rounded atan2f except where the
// true value lies that close to the middle of two floats.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define IPA_HD __host__ __device__ inline
#else
#define IPA_HD inline
#endif

IPA_HD double ipa_atan_unit(double q) {   // atan q for 0 <= q <= 1
  const double at[9] = {0.0, 0.12435499454676144, 0.24497866312686414, 0.35877067027057225, 0.4636476090008061,
                        0.5585993153435624, 0.6435011087932844, 0.7188299996216245, 0.7853981633974483};   // atan(k / 8)
  const int k = (int)(q * 8.0 + 0.5);
  const double c = k * 0.125;
  const double t = (q - c) / (1.0 + q * c);
  const double z = t * t;
  double p = -1.0 / 15.0;
  p = p * z + 1.0 / 13.0;
  p = p * z - 1.0 / 11.0;
  p = p * z + 1.0 / 9.0;
  p = p * z - 1.0 / 7.0;
  p = p * z + 1.0 / 5.0;
  p = p * z - 1.0 / 3.0;
  p = p * z;
  return at[k] + (t + t * p);
}

IPA_HD float ipa_atan2f(float yf, float xf) {
  const double pi = 3.141592653589793, pi_2 = 1.5707963267948966, pi_4 = 0.7853981633974483, pi3_4 = 2.356194490192345;
  if (yf != yf || xf != xf) return yf + xf;
  const double y = yf, x = xf;
  const bool yneg = std::signbit(yf), xneg = std::signbit(xf);
  const double ay = yneg ? -y : y, ax = xneg ? -x : x;
  const double inf = HUGE_VAL;
  double r;
  if (ay == 0.0) r = xneg ? pi : 0.0;
  else if (ax == 0.0) r = pi_2;
  else if (ax == inf) r = ay == inf ? (xneg ? pi3_4 : pi_4) : (xneg ? pi : 0.0);
  else if (ay == inf) r = pi_2;
  else {
    r = ay > ax ? pi_2 - ipa_atan_unit(ax / ay) : ipa_atan_unit(ay / ax);
    if (xneg) r = pi - r;
  }
  return (float)(yneg ? -r : r);
}
