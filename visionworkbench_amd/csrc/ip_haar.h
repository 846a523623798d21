// ip_haar.h — the float-coordinate Haar wavelets of src/vw/InterestPoint/IntegralImage.h:215-281 on the bilinear view of an
// integral image with constant edge extension (image_sample.h), as the orientation of IntegralInterestPointDetector
// (ip_detect.hip) and SGrad2DescriptorGenerator (ip_describe.hip) call them: the horizontal and the vertical response at one
// position, which share their four corner taps.  size / 2 is taken in double and stored in float, the corner coordinates are
// float sums, every accumulation is a float operation in the reference's order.
#pragma once
#include "image_sample.h"

__device__ inline float iph_tap(const is_src& s, float x, float y) {
  bool valid;
  return is_sample<VWGPU_TRANSFORM_INTERP_BILINEAR, false>(s, (double)x, (double)y, valid);
}
__device__ inline void iph_haar(const is_src& s, double x, double y, float size, float* hres, float* vres) {
  const float half_size = (float)((double)size / 2.0);
  const float top = (float)y - half_size, left = (float)x - half_size;
  const float tl = iph_tap(s, left, top), tr = iph_tap(s, left + size, top);
  const float bl = iph_tap(s, left, top + size), br = iph_tap(s, left + size, top + size);
  float r = -tl;
  r += 2 * iph_tap(s, left + half_size, top);
  r -= tr;
  r += bl;
  r -= 2 * iph_tap(s, left + half_size, top + size);
  r += br;
  *hres = r;
  r = -tl;
  r += tr;
  r += 2 * iph_tap(s, left, top + half_size);
  r -= 2 * iph_tap(s, left + size, top + half_size);
  r -= bl;
  r += br;
  *vres = r;
}
