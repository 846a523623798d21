// em_exp.h — the probability of subpixel_optimized_affine_2d_EM (src/vw/Stereo/Correlate.cc:711-714), bit for bit:
//
//   float p = k * exp(e);        // k a float constant, e a float exponent in [-75, 0]
//
// Inside namespace vw only ::exp(double) is in scope (Math/Functions.h: `using ::exp;`), so the reference evaluates
// (float)((double)k * exp((double)e)): a double product of the libm's double exp, rounded once to float.  expf (or a
// float product) differs from that at about 5 % of the inputs, so this restates it:
//   - common path: a double exp of relative error below 2^-48 (Cody-Waite reduction, degree-11 Taylor polynomial),
//     the double product, and the float rounding of it, taken when the product lies more than EMX_GUARD double ulps from
//     the midpoint of two floats (the correctly rounded float of k * e^e is then certain);
//   - otherwise: k * e^e in double-double (about 2^-100 relative) and its correctly rounded float;
//   - the libm (glibc 2.35) form is the correctly rounded float of k * e^e at every float e in [-75, 0] except one input
//     per constant, where its double product falls exactly on a float midpoint: those two are listed.
// The exhaustive test (tests/test_pyramid_subpixel_lk_em_gpu.py) compares every float in [-75, 0], -0.0 and NaN against
// the host libm for both constants.  NaN in, NaN out.  Arguments below -75 are the caller's (the reference returns 0).
//
// __host__ __device__ with the same operations on both sides (fma, rint and IEEE double arithmetic only), built with
// -ffp-contract=off, so a host build of this header computes what the kernel computes.
#ifndef VWGPU_EM_EXP_H
#define VWGPU_EM_EXP_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EMX_HD __host__ __device__ inline
#else
#define EMX_HD inline
#endif

// plane_norm_factor / noise_norm_factor: 1.0 / sqrt(2 * M_PI * var2) in double stored to float, var2 = 1e-3f / 1e-2f
// (Correlate.cc:634-635; the variances are never updated)
#define EMX_PLANE_NORM_BITS 0x4149d9c1u   // 12.6156626f
#define EMX_NOISE_NORM_BITS 0x407f52b4u   // 3.9894228f
#define EMX_GUARD 2048                    // double ulps around a float midpoint that take the double-double path

namespace emx {

EMX_HD uint64_t dbits(double d) { return __builtin_bit_cast(uint64_t, d); }
EMX_HD uint32_t fbits(float f) { return __builtin_bit_cast(uint32_t, f); }
EMX_HD float bitsf(uint32_t b) { return __builtin_bit_cast(float, b); }
EMX_HD double pow2(int n) { return __builtin_bit_cast(double, (uint64_t)(int64_t)(n + 1023) << 52); }   // normal range only

// ln 2 = L1 + L2 + L3; L1 has 38 significant bits, so n * L1 is exact for |n| < 2^15
constexpr double LN2_1 = 0x1.62e42fefa4000p-1, LN2_2 = -0x1.8432a1b0e2634p-43, LN2_3 = 0x1.f97b57a079a19p-103;
constexpr double INV_LN2 = 0x1.71547652b82fep+0;

struct dd { double hi, lo; };
EMX_HD dd fast_two_sum(double a, double b) { const double s = a + b; return {s, b - (s - a)}; }
EMX_HD dd two_sum(double a, double b) {
  const double s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
EMX_HD dd two_prod(double a, double b) { const double p = a * b; return {p, fma(a, b, -p)}; }
EMX_HD dd mul(dd a, dd b) {
  dd p = two_prod(a.hi, b.hi);
  p.lo = p.lo + (a.hi * b.lo + a.lo * b.hi);
  return fast_two_sum(p.hi, p.lo);
}
EMX_HD dd div_small(dd a, double d) {                 // a / d, d a small positive integer
  const double q1 = a.hi / d;
  const dd p = two_prod(q1, d);
  const double r = ((a.hi - p.hi) - p.lo) + a.lo;
  return fast_two_sum(q1, r / d);
}

// x - n ln 2 in double-double; x a float value, n = rint(x / ln 2)
EMX_HD dd reduce(double x, double n) {
  const double r0 = fma(-n, LN2_1, x);                // exact: |r0| < 0.35 and its bits lie above 2^-40
  const dd p = two_prod(n, LN2_2);
  dd s = two_sum(r0, -p.hi);
  s.lo = s.lo - p.lo - n * LN2_3;
  return fast_two_sum(s.hi, s.lo);
}

// the correctly rounded float of k * e^x (x a float in [-75, 0]), from k * e^x in double-double
__attribute__((noinline)) EMX_HD float slow(double k, double x) {
  const double n = rint(x * INV_LN2);
  const dd r = reduce(x, n);
  dd s = {1.0, 0.0};                                  // e^r = 1 + r (1 + r/2 (1 + r/3 (...))), |r| <= 0.35: 2^-120
  for (int j = 24; j >= 1; --j) {
    const dd t = div_small(mul(r, s), (double)j);
    s = two_sum(1.0, t.hi);
    s = fast_two_sum(s.hi, s.lo + t.lo);
  }
  dd v = two_prod(s.hi, k);
  v = fast_two_sum(v.hi, v.lo + s.lo * k);
  const double sc = pow2((int)n);
  const double hi = v.hi * sc, lo = v.lo * sc;        // exact scalings (normal results)
  float f = (float)hi;
  if ((dbits(hi) & 0x1fffffffu) == 0x10000000u && lo != 0.0) {   // hi is a float midpoint: the tail decides
    const double fd = (double)f;
    if (lo > 0.0 && fd < hi) f = bitsf(fbits(f) + 1);
    else if (lo < 0.0 && fd > hi) f = bitsf(fbits(f) - 1);
  }
  return f;
}

}  // namespace emx

// (float)((double)k * exp((double)e)) as the host libm (glibc 2.35) gives it, for e in [-75, 0] or NaN; k is one of the
// two EM constants (any other k gets the correctly rounded float of k * e^e).
EMX_HD float em_scaled_exp(float k, float e) {
  if (e != e) return e + k;
  const double x = (double)e, kd = (double)k;
  const double n = rint(x * emx::INV_LN2);
  double r = fma(-n, emx::LN2_1, x);
  r = fma(-n, emx::LN2_2, r);
  double p = 0x1.ae64567f544e4p-26;                   // Taylor coefficients 1/j!, j = 11 .. 0
  p = fma(p, r, 0x1.27e4fb7789f5cp-22);
  p = fma(p, r, 0x1.71de3a556c734p-19);
  p = fma(p, r, 0x1.a01a01a01a01ap-16);
  p = fma(p, r, 0x1.a01a01a01a01ap-13);
  p = fma(p, r, 0x1.6c16c16c16c17p-10);
  p = fma(p, r, 0x1.1111111111111p-7);
  p = fma(p, r, 0x1.5555555555555p-5);
  p = fma(p, r, 0x1.5555555555555p-3);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  const double prod = kd * (p * emx::pow2((int)n));
  const int64_t m = (int64_t)(emx::dbits(prod) & 0x1fffffffu) - 0x10000000;
  if (m > EMX_GUARD || m < -EMX_GUARD) return (float)prod;
  const uint32_t kb = emx::fbits(k), eb = emx::fbits(e);
  if (kb == EMX_PLANE_NORM_BITS && eb == 0xb48e0bb1u) return emx::bitsf(0x4149d9beu);   // libm: product on a midpoint
  if (kb == EMX_NOISE_NORM_BITS && eb == 0xb85a7556u) return emx::bitsf(0x407f4f4cu);
  return emx::slow(kd, x);
}

#endif
