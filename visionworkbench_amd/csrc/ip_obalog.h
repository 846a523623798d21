// ip_obalog.h — the numbers that define the OBALoG interest operator (Optimized Box Approximation of the Laplacian of
// Gaussian; src/vw/InterestPoint/IntegralInterestOperator.cc:28-61): for each of eight scales the sigma of the Laplacian it
// approximates and six centred boxes {width, height, weight} summed over the integral image.  The reference carries two
// more rows that are placeholders (3 x 3 boxes, weights +-1) whose Harris test reads outside the image; they are not here,
// and scales beyond 8 are refused.  This is the only place the numbers are entered: ip_detect.hip reads them on the device,
// tests/refimpl/ip_detect_ref.cc in the restatement.
#pragma once

#if defined(__HIPCC__)
#define IPO_HD __host__ __device__ inline
#else
#define IPO_HD inline
#endif

enum { IPO_SCALES = 8, IPO_BOXES = 6 };

IPO_HD double ipo_sigma(int scale) {
  const double sigma[IPO_SCALES] = {1.2, 1.5, 1.875, 2.34375, 2.9296875, 3.662109, 4.577636, 5.722046};
  return sigma[scale];
}

struct ipo_box { int w, h; double weight; };

IPO_HD ipo_box ipo_box_of(int scale, int b) {
  const int bw[IPO_SCALES][IPO_BOXES] = {
    {11, 7, 5, 3, 3, 1},      {13, 9, 7, 5, 3, 1},      {17, 11, 9, 5, 5, 3},     {21, 13, 11, 7, 7, 3},
    {27, 17, 13, 9, 9, 5},    {33, 21, 17, 11, 11, 5},  {41, 27, 21, 13, 13, 7},  {51, 33, 27, 17, 17, 7}};
  const int bh[IPO_SCALES][IPO_BOXES] = {
    {11, 5, 7, 3, 1, 3},      {13, 7, 9, 1, 3, 5},      {17, 9, 11, 5, 3, 5},     {21, 11, 13, 3, 7, 7},
    {27, 13, 17, 5, 9, 9},    {33, 17, 21, 5, 11, 11},  {41, 21, 27, 7, 13, 13},  {51, 27, 33, 7, 17, 17}};
  const double wt[IPO_SCALES][IPO_BOXES] = {
    {0.0006179999909, 0.008283999749, 0.008283999749, -0.03556599841, -0.05576400086, -0.05576400086},
    {0.0002659999882, 0.004889999982, 0.004889999982, -0.0221420005, -0.0488499999, -0.0221420005},
    {0.0002659424644, 0.003207367443, 0.003207367443, -0.001847865087, -0.022190776, -0.022190776},
    {0.000218920823, 0.002005755751, 0.002005755751, -0.01499466244, -0.0008247125278, -0.01499466244},
    {0.0001030362087, 0.00137811946, 0.00137811946, -0.009606413672, 0.002226325845, -0.009606413672},
    {7.198028372e-05, 0.0008259398524, 0.0008259398524, -0.006072390568, -1.177469443e-06, -0.006072390568},
    {3.803569417e-05, 0.0005251058097, 0.0005251058097, -0.003885340628, 0.0002823550512, -0.003885340628},
    {2.892054582e-05, 0.0003287680581, 0.0003287680581, -0.002447736656, -0.0002717150913, -0.002447736656}};
  return ipo_box{bw[scale][b], bh[scale][b], wt[scale][b]};
}

// half of the largest box side: the filter is zero within this many pixels of the border (BoxFilter.h:91-98, :109-111)
IPO_HD int ipo_pixel_buffer(int scale) {
  int m = 0;
  for (int b = 0; b < IPO_BOXES; ++b) {
    const ipo_box x = ipo_box_of(scale, b);
    if (m < x.w) m = x.w;
    if (m < x.h) m = x.h;
  }
  return m >> 1;
}
