// vw/Stereo.h — vw::stereo entry points of the block-matching hot path with the reference's signatures,
// implemented on libvwgpu.so (include/vwgpu.h).  Header-only; link with -lvwgpu.
//
//   calc_disparity               src/vw/Stereo/Correlation.h:50-57   (impl Correlation.cc:330-375)
//   fast_box_sum                 src/vw/Stereo/Algorithms.h:41-129
//   cross_corr_consistency_check src/vw/Stereo/Correlate.h:52-58     (impl Correlate.cc:1441-1502)
//   correlate                    legacy single-level entry, signature recovered from
//                                src/vw/Stereo/tests/TestCorrelationView.cxx:79-82,213-215
//   pyramid_correlate            src/vw/Stereo/CorrelationView.h:195-230 (PyramidCorrelationView :35-190, BM algorithm)
//   parabola_subpixel            src/vw/Stereo/ParabolaSubpixelView.h:112-117
//   PyramidSubpixelView, lk_subpixel, affine_subpixel, bayes_em_subpixel
//                                src/vw/Stereo/SubpixelView.h:28-134 (SUBPIXEL_PHASE: NoImplErr)
//   phase_subpixel               src/vw/Stereo/SubpixelView.h:136-144 (vwgpu_phase_subpixel)
//   CorrEval, corr_eval          src/vw/Stereo/CorrEval.h:56-128 (vwgpu_corr_eval)
//   disparity_median_filter, disparity_neighbor_filter, texture_measure, texture_preserving_disparity_filter
//                                src/vw/Stereo/Algorithms.h:132-281, Algorithms.cc:26-110 (vwgpu_disparity_median_filter ...)
//   prefilter_image              src/vw/Stereo/PreFilter.h:76-95
//   rm_outliers_using_thresh / disparity_cleanup_using_thresh / disparity_mask
//                                src/vw/Stereo/DisparityMap.h:387-441, 236-253
//   rm_outliers_using_mean / _stddev / _plane, disparity_cleanup_using_mean / _stddev, disparity_clean_using_plane,
//   std_dev_image                src/vw/Stereo/DisparityMap.h:444-1014, DisparityMap.cc:24-118 (vwgpu_rm_outliers,
//                                vwgpu_std_dev_image)
//   get_disparity_range, missing_pixel_image, disparity_range_mask, transform_disparities (both overloads),
//   DisparityTransform, intersect_mask_and_data, disparity_subsample, disparity_upsample
//                                src/vw/Stereo/DisparityMap.h:48-87, 255-300, 1016-1057, 1164-1358
//   StereoModel, StereoView / stereo_triangulate, UniverseRadiusFunc (with the cameras of vw/Camera.h)
//                                src/vw/Stereo/StereoModel.{h,cc}, StereoView.h
//   SearchParam, subdivide_regions, calc_seconds_per_op   src/vw/Stereo/Correlation.h:66-122
//   SemiGlobalMatcher, calc_disparity_sgm                 src/vw/Stereo/SGM.h:75-157,360-375
// Errors: the C ABI's status codes become the reference's exception types (src/vw/Core/Exception.h:225-253).
// Threading: one engine context per (host thread x GPU), created lazily — the reference calls these functions
// concurrently from its tile threads (src/vw/Image/ImageIO.h:228-251).
#ifndef VWLITE_STEREO_H
#define VWLITE_STEREO_H

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "Camera.h"
#include "Engine.h"
#include "Filter.h"
#include "Image.h"
#include "vwgpu.h"

namespace vw {
namespace stereo {

enum CostFunctionType {                  // src/vw/Stereo/CostFunctions.h:143-149
  ABSOLUTE_DIFFERENCE, SQUARED_DIFFERENCE, CROSS_CORRELATION, CENSUS_TRANSFORM, TERNARY_CENSUS_TRANSFORM
};
enum PrefilterModeType { PREFILTER_NONE = 0, PREFILTER_MEANSUB = 1, PREFILTER_LOG = 2 };   // PrefilterEnum.h:24-28

enum CorrelationAlgorithm {              // src/vw/Stereo/CorrelationAlgorithms.h:29-35
  VW_CORRELATION_BM = 0, VW_CORRELATION_SGM = 1, VW_CORRELATION_MGM = 2, VW_CORRELATION_FINAL_MGM = 3, VW_CORRELATION_OTHER = 4
};

namespace detail {
using engine::thread_context;
using engine::check;
}  // namespace detail

/// calc_disparity — same signature and semantics as the reference (Correlation.h:50-57).
inline ImageView<PixelMask<Vector2i>>
calc_disparity(CostFunctionType cost_type,
               ImageViewRef<PixelGray<float>> const& left_in,
               ImageViewRef<PixelGray<float>> const& right_in,
               BBox2i const& left_region,     // valid region in the left image
               Vector2i const& search_volume, // max disparity to search in the right image
               Vector2i const& kernel_size) {
  // The reference's sanity checks (Correlation.cc:341-351); the engine repeats the rest behind the ABI.
  VW_ASSERT(left_region.min().x() >= 0 && left_region.min().y() >= 0 &&
            left_region.max().x() <= left_in.cols() && left_region.max().y() <= left_in.rows(),
            ArgumentErr() << "calc_disparity: Region not inside left image.");
  BBox2i right_region = left_region;
  right_region.max() += search_volume - Vector2i(1, 1);                          // Correlation.cc:356-357
  const int32 lw = left_region.width(), lh = left_region.height();
  const int32 rw = right_region.width(), rh = right_region.height();

  // Rasterise the two crops (Correlation.cc:358-359).  A handle that wraps a plain ImageView is used in place.
  ImageView<PixelGray<float>> lbuf, rbuf;
  int32 ls = 0, rs = 0;
  const PixelGray<float>* lp = left_in.plain_data(ls);
  const PixelGray<float>* rp = right_in.plain_data(rs);
  if (lp) lp += (size_t)left_region.min().y() * ls + left_region.min().x();
  else { lbuf = crop(left_in, left_region); lp = lbuf.data(); ls = lw; }
  if (rp && right_region.max().x() <= right_in.cols() && right_region.max().y() <= right_in.rows())
    rp += (size_t)right_region.min().y() * rs + right_region.min().x();
  else { rbuf = crop(right_in, right_region); rp = rbuf.data(); rs = rw; }

  const int32 ow = lw - kernel_size[0] + 1, oh = lh - kernel_size[1] + 1;
  ImageView<PixelMask<Vector2i>> out(ow > 0 ? ow : 0, oh > 0 ? oh : 0);
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_calc_disparity(ctx, (int)cost_type,
                                          reinterpret_cast<const float*>(lp), lw, lh, ls,
                                          reinterpret_cast<const float*>(rp), rw, rh, rs,
                                          kernel_size[0], kernel_size[1], search_volume[0], search_volume[1],
                                          reinterpret_cast<int32_t*>(out.data()), 0));
  return out;
}

/// cross_corr_consistency_check — in place on l2r, as the reference (Correlate.h:52-58).
inline void cross_corr_consistency_check(ImageView<PixelMask<Vector2i>> const& l2r,
                                         ImageView<PixelMask<Vector2i>> const& r2l,
                                         float cross_corr_threshold, bool /*verbose*/ = false) {
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_cross_corr_consistency_check(ctx, reinterpret_cast<int32_t*>(l2r.data()), l2r.cols(), l2r.rows(), 0,
                                                        reinterpret_cast<const int32_t*>(r2l.data()), r2l.cols(), r2l.rows(), 0,
                                                        cross_corr_threshold));
}

/// fast_box_sum<AccumulatorType>(image, kernel) — Algorithms.h:41-43.  The engine forms the sums in float64 in the
/// reference's running-sum order (the only accumulator the reference's callers use is double, CostFunctions.h:55-57);
/// other accumulator types receive the rounded float64 sums.
template <class AccumulatorType, class ViewT>
ImageView<AccumulatorType> fast_box_sum(ImageViewBase<ViewT> const& image, Vector2i const& kernel) {
  VW_ASSERT(kernel[0] % 2 == 1 && kernel[1] % 2 == 1, ArgumentErr() << "fast_box_sum: Kernel input not sized with odd values.");
  ImageView<PixelGray<float>> in = pixel_cast<PixelGray<float>>(image.impl());
  VW_ASSERT(in.cols() >= kernel[0] && in.rows() >= kernel[1], ArgumentErr() << "fast_box_sum: Image is not big enough for kernel.");
  const int32 ow = in.cols() - kernel[0] + 1, oh = in.rows() - kernel[1] + 1;
  ImageView<double> sums(ow, oh);
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_fast_box_sum(ctx, reinterpret_cast<const float*>(in.data()), in.cols(), in.rows(), 0, kernel[0], kernel[1],
                                        sums.data(), 0));
  ImageView<AccumulatorType> out(ow, oh);
  for (int32 r = 0; r < oh; ++r) for (int32 c = 0; c < ow; ++c) out(c, r) = AccumulatorType(sums(c, r));
  return out;
}

/// Legacy correlate(): prefilter -> calc_disparity over the whole left image -> optional R->L run + L/R check.
/// search_volume is a BBox2i of signed disparities, max() INCLUSIVE as the legacy view took it (its own test searches
/// BBox2i(1,1,1,1) and expects valid (1,1) answers, TestCorrelationView.cxx:46,64-66); the result holds signed disparities
/// (offset by search_volume.min()), like the legacy view did.  The overload taking a prefilter object follows below.
inline ImageView<PixelMask<Vector2i>>
correlate(ImageView<PixelGray<float>> const& left, ImageView<PixelGray<float>> const& right,
          BBox2i const& search_volume, Vector2i const& kernel_size,
          CostFunctionType cost_type = ABSOLUTE_DIFFERENCE, float consistency_threshold = -1) {
  const Vector2i half(kernel_size[0] / 2, kernel_size[1] / 2);
  const Vector2i s = search_volume.size() + Vector2i(1, 1);
  // Pad so that every pixel of `left` gets a disparity: windows are centred (edge-extended with zeros like the
  // legacy CorrelationView) and the right crop is shifted by search_volume.min().
  const int32 W = left.cols(), H = left.rows();
  ImageView<PixelGray<float>> lpad = crop(edge_extend(left, ZeroEdgeExtension()), -half[0], -half[1], W + 2 * half[0], H + 2 * half[1]);
  ImageView<PixelGray<float>> rpad = crop(edge_extend(right, ZeroEdgeExtension()),
                                         -half[0] + search_volume.min().x(), -half[1] + search_volume.min().y(),
                                         W + 2 * half[0] + s[0] - 1, H + 2 * half[1] + s[1] - 1);
  ImageView<PixelMask<Vector2i>> l2r = calc_disparity(cost_type, lpad, rpad, bounding_box(lpad), s, kernel_size);
  if (consistency_threshold >= 0) {
    // R->L: search the left image around each right pixel over the mirrored range.
    ImageView<PixelGray<float>> rp2 = crop(edge_extend(right, ZeroEdgeExtension()), -half[0], -half[1], W + 2 * half[0], H + 2 * half[1]);
    ImageView<PixelGray<float>> lp2 = crop(edge_extend(left, ZeroEdgeExtension()),
                                          -half[0] - search_volume.max().x(), -half[1] - search_volume.max().y(),
                                          W + 2 * half[0] + s[0] - 1, H + 2 * half[1] + s[1] - 1);
    ImageView<PixelMask<Vector2i>> r2l = calc_disparity(cost_type, rp2, lp2, bounding_box(rp2), s, kernel_size);
    const Vector2i lmin = search_volume.min(), rmin(-search_volume.max().x(), -search_volume.max().y());
    for (int32 r = 0; r < H; ++r) for (int32 c = 0; c < W; ++c) { l2r(c, r).child() += lmin; r2l(c, r).child() += rmin; }
    cross_corr_consistency_check(l2r, r2l, consistency_threshold);
    return l2r;
  }
  for (int32 r = 0; r < H; ++r) for (int32 c = 0; c < W; ++c) l2r(c, r).child() += search_volume.min();
  return l2r;
}

/// prefilter_image — rasterised (PreFilter.h:76-95).
inline ImageView<PixelGray<float>>
prefilter_image(ImageView<PixelGray<float>> const& image, PrefilterModeType prefilter_mode, float prefilter_width) {
  ImageView<PixelGray<float>> out(image.cols(), image.rows());
  if (image.cols() == 0 || image.rows() == 0) return out;
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_prefilter_image(ctx, reinterpret_cast<const float*>(image.data()), image.cols(), image.rows(), 0,
                                           (int)prefilter_mode, prefilter_width, reinterpret_cast<float*>(out.data()), 0));
  return out;
}

/// The prefilter objects of PreFilter.h:40-73; filter() returns the rasterised image (zero outside, like ConstantEdgeExtension
/// views do once rasterised over the image's own box).
struct NullOperation {
  ImageView<PixelGray<float>> filter(ImageView<PixelGray<float>> const& image) const { return prefilter_image(image, PREFILTER_NONE, 0.0f); }
};
struct LaplacianOfGaussian {
  float kernel_width;
  explicit LaplacianOfGaussian(float size) : kernel_width(size) {}
  ImageView<PixelGray<float>> filter(ImageView<PixelGray<float>> const& image) const { return prefilter_image(image, PREFILTER_LOG, kernel_width); }
};
struct SubtractedMean {
  float kernel_width;
  explicit SubtractedMean(float size) : kernel_width(size) {}
  ImageView<PixelGray<float>> filter(ImageView<PixelGray<float>> const& image) const { return prefilter_image(image, PREFILTER_MEANSUB, kernel_width); }
};

/// Legacy correlate() with a prefilter object (TestCorrelationView.cxx:79-84 call shape).
template <class PreFilterT>
inline ImageView<PixelMask<Vector2i>>
correlate(ImageView<PixelGray<float>> const& left, ImageView<PixelGray<float>> const& right, PreFilterT const& prefilter,
          BBox2i const& search_volume, Vector2i const& kernel_size,
          CostFunctionType cost_type = ABSOLUTE_DIFFERENCE, float consistency_threshold = -1) {
  return correlate(prefilter.filter(left), prefilter.filter(right), search_volume, kernel_size, cost_type, consistency_threshold);
}

/// parabola_subpixel — the rasterised ParabolaSubpixelView (ParabolaSubpixelView.h:112-117).
inline ImageView<PixelMask<Vector2f>>
parabola_subpixel(ImageViewRef<PixelMask<Vector2f>> const& disparity,
                  ImageViewRef<PixelGray<float>> const& left_image, ImageViewRef<PixelGray<float>> const& right_image,
                  PrefilterModeType prefilter_mode, float prefilter_width, Vector2i const& kernel_size) {
  VW_ASSERT(disparity.cols() == left_image.cols() && disparity.rows() == left_image.rows(),
            ArgumentErr() << "SubpixelView: Disparity image must match left image.");   // ParabolaSubpixelView.h:67-69
  ImageView<PixelMask<Vector2f>> d = disparity, out(disparity.cols(), disparity.rows());
  ImageView<PixelGray<float>> l = left_image, r = right_image;
  if (d.cols() == 0 || d.rows() == 0) return out;
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_parabola_subpixel(ctx, reinterpret_cast<const float*>(d.data()), d.cols(), d.rows(), 0,
                                             reinterpret_cast<const float*>(l.data()), 0,
                                             reinterpret_cast<const float*>(r.data()), r.cols(), r.rows(), 0,
                                             (int)prefilter_mode, prefilter_width, kernel_size[0], kernel_size[1],
                                             reinterpret_cast<float*>(out.data()), 0));
  return out;
}

namespace detail {
inline ImageView<PixelMask<Vector2i>> disparity_filter(ImageView<PixelMask<Vector2i>> const& d, int32 hh, int32 hv,
                                                       double pthr, double rthr, int cleanup) {
  ImageView<PixelMask<Vector2i>> out(d.cols(), d.rows());
  if (d.cols() == 0 || d.rows() == 0) return out;
  vwgpu_ctx* ctx = thread_context();
  check(ctx, vwgpu_disparity_filter(ctx, reinterpret_cast<const int32_t*>(d.data()), d.cols(), d.rows(), hh, hv, pthr, rthr, cleanup,
                                    reinterpret_cast<int32_t*>(out.data())));
  return out;
}
}  // namespace detail

/// rm_outliers_using_thresh — rasterised over the whole image (DisparityMap.h:403-414).
template <class ViewT>
ImageView<PixelMask<Vector2i>> rm_outliers_using_thresh(ImageViewBase<ViewT> const& disparity_map, int32 half_h_kernel, int32 half_v_kernel,
                                                        double pixel_threshold, double rejection_threshold) {
  VW_ASSERT(half_h_kernel > 0 && half_v_kernel > 0, ArgumentErr() << "RmOutliersFunc: half kernel sizes must be non-zero.");
  ImageView<PixelMask<Vector2i>> d = disparity_map.impl();
  return detail::disparity_filter(d, half_h_kernel, half_v_kernel, pixel_threshold, rejection_threshold, 0);
}
/// disparity_cleanup_using_thresh — two passes, the second with (1,1,3.0,0.20) (DisparityMap.h:422-441).
template <class ViewT>
ImageView<PixelMask<Vector2i>> disparity_cleanup_using_thresh(ImageViewBase<ViewT> const& disparity_map, int32 h_half_kernel, int32 v_half_kernel,
                                                              double pixel_threshold, double rejection_threshold) {
  VW_ASSERT(h_half_kernel > 0 && v_half_kernel > 0, ArgumentErr() << "RmOutliersFunc: half kernel sizes must be non-zero.");
  ImageView<PixelMask<Vector2i>> d = disparity_map.impl();
  return detail::disparity_filter(d, h_half_kernel, v_half_kernel, pixel_threshold, rejection_threshold, 1);
}
/// disparity_mask — rasterised (DisparityMap.h:236-253); masks are uint8 images, 0 = no data.
template <class ViewT, class M1, class M2>
ImageView<PixelMask<Vector2i>> disparity_mask(ImageViewBase<ViewT> const& disparity_map, ImageViewBase<M1> const& left_mask,
                                              ImageViewBase<M2> const& right_mask) {
  ImageView<PixelMask<Vector2i>> d = copy(disparity_map.impl());
  ImageView<uint8> m1 = left_mask.impl(), m2 = right_mask.impl();
  VW_ASSERT(d.cols() == m1.cols() && d.rows() == m1.rows(), ArgumentErr() << "disparity_mask: input and left mask are not same dimensions.");
  if (d.cols() == 0 || d.rows() == 0) return d;
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_disparity_mask(ctx, reinterpret_cast<int32_t*>(d.data()), d.cols(), d.rows(), m1.data(), m2.data(), m2.cols(), m2.rows()));
  return d;
}

/// SearchParam / subdivide_regions — the zone scheduler (Correlation.h:66-91,118-122).
struct SearchParam : public std::pair<BBox2i, BBox2i> {
  SearchParam(BBox2i const& image_region, BBox2i const& disparity_range) : std::pair<BBox2i, BBox2i>(image_region, disparity_range) {}
  BBox2i& image_region() { return this->first; }            BBox2i const& image_region() const { return this->first; }
  BBox2i& disparity_range() { return this->second; }        BBox2i const& disparity_range() const { return this->second; }
  double search_volume() const {
    return (double)first.width() * (double)first.height() * (double)second.width() * (double)second.height();
  }
};
struct SearchParamLessThan {
  bool operator()(SearchParam const& A, SearchParam const& B) const { return A.search_volume() < B.search_volume(); }
};
inline bool subdivide_regions(ImageView<PixelMask<Vector2i>> const& disparity, BBox2i const& current_bbox,
                              std::vector<SearchParam>& list, Vector2i const& kernel_size, int32 /*fail_count*/ = 0) {
  // the engine scheduler works on a whole image: hand it the crop and shift the zones back
  ImageView<PixelMask<Vector2i>> d = crop(disparity, current_bbox);
  if (d.cols() == 0 || d.rows() == 0) return true;
  std::vector<int32_t> zones(8 * 1024);
  int n = vwgpu_subdivide_regions(reinterpret_cast<const int32_t*>(d.data()), d.cols(), d.rows(), kernel_size[0], kernel_size[1],
                                  zones.data(), (int)zones.size() / 8);
  if (n > (int)zones.size() / 8) {
    zones.resize((size_t)n * 8);
    n = vwgpu_subdivide_regions(reinterpret_cast<const int32_t*>(d.data()), d.cols(), d.rows(), kernel_size[0], kernel_size[1], zones.data(), n);
  }
  VW_ASSERT(n >= 0, ArgumentErr() << "subdivide_regions: bad arguments");
  for (int i = 0; i < n; ++i) {
    const int32_t* z = &zones[(size_t)i * 8];
    list.push_back(SearchParam(BBox2i(Vector2i(z[0], z[1]) + current_bbox.min(), Vector2i(z[2], z[3]) + current_bbox.min()),
                               BBox2i(Vector2i(z[4], z[5]), Vector2i(z[6], z[7]))));
  }
  return true;
}

/// calc_seconds_per_op (Correlation.cc:382-436): time a fake calc_disparity and divide by region x search volume.
/// The reference grows the problem until one call takes a second; on the GPU that would need tens of GB, so the
/// loop stops at 20 ms or 2048^2 — the figure only feeds pyramid_correlate's corr_timeout estimate.
inline double calc_seconds_per_op(CostFunctionType cost_type, Vector2i const& kernel_size) {
  double elapsed = -1.0, seconds_per_op = -1.0;
  int lsize = 100;
  while (elapsed < 0.02 && lsize < 2048) {
    lsize = (int)std::ceil(lsize * 1.2) + std::max(kernel_size[0], kernel_size[1]);
    ImageView<PixelGray<float>> fake_left(lsize, lsize), fake_right(lsize + lsize / 5, lsize + lsize / 5);
    for (int row = 0; row < fake_left.rows(); ++row) for (int col = 0; col < fake_left.cols(); ++col) fake_left(col, row) = float(col % 2 + 2 * (row % 5));
    for (int row = 0; row < fake_right.rows(); ++row) for (int col = 0; col < fake_right.cols(); ++col) fake_right(col, row) = float(3 * (col % 7) + row % 3);
    const Vector2i search(std::max(lsize / 5, 1), std::max(lsize / 5, 1));
    calc_disparity(cost_type, fake_left, fake_right, bounding_box(fake_left), search, kernel_size);   // warm-up (allocations)
    const auto t0 = std::chrono::steady_clock::now();
    calc_disparity(cost_type, fake_left, fake_right, bounding_box(fake_left), search, kernel_size);
    elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    seconds_per_op = elapsed / ((double)lsize * lsize * search[0] * search[1]);
  }
  return seconds_per_op;
}

/// SemiGlobalMatcher — the slice of the reference's class (SGM.h:75-352) that callers of calc_disparity_sgm touch: the
/// sub-pixel mode enum and create_disparity_view_subpixel on the matcher handed back through matcher_ptr.  The engine
/// computes the sub-pixel view in the same pass (the accumulation buffers live in HBM only during the call).
class SemiGlobalMatcher {
public:
  typedef ImageView<PixelMask<Vector2i>> DisparityImage;
  enum SgmSubpixelMode { SUBPIXEL_NONE = 0, SUBPIXEL_PARABOLA = 1, SUBPIXEL_LINEAR = 2, SUBPIXEL_POLY4 = 3,
                         SUBPIXEL_COSINE = 4, SUBPIXEL_LC_BLEND = 5 };
  /// SGM.h:157 — valid for the integer disparity this matcher produced.
  ImageView<PixelMask<Vector2f>> create_disparity_view_subpixel(DisparityImage const& integer_disparity) const {
    VW_ASSERT(integer_disparity.cols() == m_subpixel.cols() && integer_disparity.rows() == m_subpixel.rows(),
              ArgumentErr() << "create_disparity_view_subpixel: not the disparity this matcher produced.");
    ImageView<PixelMask<Vector2f>> out = copy(m_subpixel);
    for (int32 r = 0; r < out.rows(); ++r)
      for (int32 c = 0; c < out.cols(); ++c)
        if (!is_valid(integer_disparity(c, r))) {          // SGM.cc:1523-1527
          out(c, r) = PixelMask<Vector2f>(Vector2f(float(integer_disparity(c, r)[0]), float(integer_disparity(c, r)[1])));
          out(c, r).invalidate();
        }
    return out;
  }
  ImageView<PixelMask<Vector2f>> m_subpixel;   // filled by calc_disparity_sgm
};

/// Opt-in to the code the reference keeps behind a throw: with the flag set, calc_disparity_sgm with ABSOLUTE_DIFFERENCE /
/// SQUARED_DIFFERENCE runs fill_costs_block's mean-abs-difference cost (SGM.cc:1651-1738, p1 = 3, p2 = 250) instead of throwing
/// NoImplErr like compute_disparity_costs (SGM.cc:1887-1892).  Process wide, off by default; not part of the reference's API.
inline bool& sgm_allow_block_cost() { static bool flag = false; return flag; }

/// calc_disparity_sgm — the reference's signature (SGM.h:360-375); std::shared_ptr stands in for boost::shared_ptr.
inline ImageView<PixelMask<Vector2i>>
calc_disparity_sgm(CostFunctionType cost_type,
                   ImageView<PixelGray<float>> const& left_in, ImageView<PixelGray<float>> const& right_in,
                   BBox2i const& left_region, Vector2i const& search_volume, Vector2i const& kernel_size,
                   bool const use_mgm, SemiGlobalMatcher::SgmSubpixelMode const& subpixel_mode,
                   Vector2i const search_buffer, size_t const memory_limit_mb,
                   std::shared_ptr<SemiGlobalMatcher>& matcher_ptr,
                   ImageView<uint8> const* left_mask_ptr = 0, ImageView<uint8> const* right_mask_ptr = 0,
                   SemiGlobalMatcher::DisparityImage const* prev_disparity = 0) {
  VW_ASSERT(kernel_size[0] % 2 == 1 && kernel_size[1] % 2 == 1, ArgumentErr() << "calc_disparity_sgm: Kernel input not sized with odd values.");
  VW_ASSERT(kernel_size[0] <= left_region.width() && kernel_size[1] <= left_region.height(),
            ArgumentErr() << "calc_disparity_sgm: Kernel size too large of active region.");
  VW_ASSERT(left_region.min().x() >= 0 && left_region.min().y() >= 0 && left_region.max().x() <= left_in.cols() &&
            left_region.max().y() <= left_in.rows(), ArgumentErr() << "calc_disparity_sgm: Region not inside left image.");
  BBox2i right_region = left_region;
  right_region.max() += search_volume;                               // inclusive search volume (SGM.cc:186-191)
  ImageView<PixelGray<float>> l = crop(left_in, left_region);
  ImageView<PixelGray<float>> r = crop(edge_extend(right_in, ConstantEdgeExtension()), right_region);
  vwgpu_sgm_params p = vwgpu_sgm_params();
  p.cost_type = (int)cost_type; p.use_mgm = use_mgm ? 1 : 0; p.kernel_size = kernel_size[0]; p.subpixel_mode = (int)subpixel_mode;
  p.search_buffer_x = search_buffer[0]; p.search_buffer_y = search_buffer[1]; p.memory_limit_mb = memory_limit_mb;
  p.p1 = 0; p.p2 = 0; p.ternary_census_threshold = 5; p.num_threads = 1;
  p.allow_block_cost = sgm_allow_block_cost() ? 1 : 0;
  const size_t cap = (size_t)l.cols() * l.rows();
  std::vector<int32_t> disp(cap * 3);
  std::vector<float> sub(cap * 3);
  int ow = 0, oh = 0;
  vwgpu_ctx* ctx = detail::thread_context();
  try {
    detail::check(ctx, vwgpu_calc_disparity_sgm(ctx, &p, reinterpret_cast<const float*>(l.data()), l.cols(), l.rows(), 0,
                                                reinterpret_cast<const float*>(r.data()), r.cols(), r.rows(), 0, search_volume[0], search_volume[1],
                                                left_mask_ptr ? left_mask_ptr->data() : 0, left_mask_ptr ? left_mask_ptr->cols() : 0, left_mask_ptr ? left_mask_ptr->rows() : 0,
                                                right_mask_ptr ? right_mask_ptr->data() : 0, right_mask_ptr ? right_mask_ptr->cols() : 0, right_mask_ptr ? right_mask_ptr->rows() : 0,
                                                prev_disparity ? reinterpret_cast<const int32_t*>(prev_disparity->data()) : 0,
                                                prev_disparity ? prev_disparity->cols() : 0, prev_disparity ? prev_disparity->rows() : 0,
                                                disp.data(), sub.data(), cap, &ow, &oh));
  } catch (NoImplErr const&) {
    throw;                                                           // MAD cost / census size: as the reference's NoImplErr
  } catch (std::exception const& e) {                                // SGM.cc:221-226
    vw_throw(ArgumentErr() << "Failed to compute the correlation. See the online documentation (next_steps.html) for how to "
                           << "handle failures.\nDetailed error message: " << e.what() << "\n");
  }
  ImageView<PixelMask<Vector2i>> out(ow, oh);
  matcher_ptr.reset(new SemiGlobalMatcher());
  matcher_ptr->m_subpixel.set_size(ow, oh);
  std::memcpy(static_cast<void*>(out.data()), disp.data(), (size_t)ow * oh * 12);
  std::memcpy(static_cast<void*>(matcher_ptr->m_subpixel.data()), sub.data(), (size_t)ow * oh * 12);
  return out;
}

/// PyramidCorrelationView — lazy like the reference's (CorrelationView.h:35-190): nothing runs until a tile is
/// requested through prerasterize(bbox) / rasterize, and every tile is independent (CorrelationView.cc:273-886).
class PyramidCorrelationView : public ImageViewBase<PyramidCorrelationView> {
  // Type-erased handles, as in the reference (CorrelationView.h:38-45): nothing is rasterised until a tile is requested,
  // and then only the window that tile can touch (CorrelationView.cc:89-97) — the sources may be file-backed views.
  ImageViewRef<PixelGray<float>> m_left, m_right;
  ImageViewRef<uint8> m_left_mask, m_right_mask;
  vwgpu_pyramid_params m_p;
  int m_collar_size;                                      ///< Expand the size of the image for each tile before correlating
  ImageView<PixelMask<float>>* m_lr_disp_diff;            ///< L-R / R-L discrepancy output (CorrelationView.h:84), or NULL
  Vector2i m_region_ul;
public:
  typedef PixelMask<Vector2f> pixel_type;
  typedef pixel_type result_type;
  typedef CropView<ImageView<pixel_type>> prerasterize_type;

  PyramidCorrelationView(ImageViewRef<PixelGray<float>> const& left, ImageViewRef<PixelGray<float>> const& right,
                         ImageViewRef<uint8> const& left_mask, ImageViewRef<uint8> const& right_mask, vwgpu_pyramid_params const& p,
                         int collar_size = 0, ImageView<PixelMask<float>>* lr_disp_diff = NULL, Vector2i const& region_ul = Vector2i(0, 0))
      : m_left(left), m_right(right), m_left_mask(left_mask), m_right_mask(right_mask), m_p(p), m_collar_size(collar_size),
        m_lr_disp_diff(lr_disp_diff), m_region_ul(region_ul) {
    if (m_lr_disp_diff) {                                 // the tile threads write disjoint pixels of the caller's image
      m_p.lr_disp_diff = reinterpret_cast<float*>(m_lr_disp_diff->data());
      m_p.lr_disp_diff_cols = m_lr_disp_diff->cols(); m_p.lr_disp_diff_rows = m_lr_disp_diff->rows(); m_p.lr_disp_diff_stride = 0;
      m_p.region_ul_x = region_ul[0]; m_p.region_ul_y = region_ul[1];
    }
    VW_ASSERT(left_mask.cols() == left.cols() && left_mask.rows() == left.rows() &&
              right_mask.cols() == right.cols() && right_mask.rows() == right.rows(),
              ArgumentErr() << "PyramidCorrelationView: masks must match their images.");
  }
  int32 cols() const { return m_left.cols(); }
  int32 rows() const { return m_left.rows(); }
  int32 planes() const { return 1; }
  pixel_type operator()(int32 /*i*/, int32 /*j*/, int32 /*p*/ = 0) const {
    vw_throw(NoImplErr() << "PyramidCorrelationView::operator()(....) has not been implemented.");   // CorrelationView.h:166-171
    return pixel_type();
  }
  /// One tile; the returned image is indexed from the tile's own origin (0,0) = bbox.min().
  ImageView<pixel_type> correlate_tile(BBox2i const& bbox) const {
    ImageView<pixel_type> out(bbox.width(), bbox.height());
    if (bbox.empty()) return out;
    vwgpu_ctx* ctx = detail::thread_context();
    int32 ls = 0, rs = 0, lms = 0, rms = 0;
    const PixelGray<float>* lp = m_left.plain_data(ls);
    const PixelGray<float>* rp = m_right.plain_data(rs);
    const uint8* lmp = m_left_mask.plain_data(lms);
    const uint8* rmp = m_right_mask.plain_data(rms);
    if (lp && rp && lmp && rmp) {                  // plain in-memory images: used in place (the engine ships the window)
      detail::check(ctx, vwgpu_pyramid_correlate(ctx, reinterpret_cast<const float*>(lp), m_left.cols(), m_left.rows(), ls,
                                                 reinterpret_cast<const float*>(rp), m_right.cols(), m_right.rows(), rs,
                                                 lmp, lms, rmp, rms, &m_p,
                                                 bbox.min().x(), bbox.min().y(), bbox.width(), bbox.height(),
                                                 reinterpret_cast<float*>(out.data()), 0));
      return out;
    }
    // lazy sources: rasterise the tile's window only.  Window = tile grown by the pyramid padding half_kernel * 2^levels,
    // twice the search extent (the SGM branch's R->L runs) and the search range, cut at the image borders; all four
    // rasters share its origin, so the engine sees a smaller pair in which the tile sits at bbox - origin.
    const int64 up = int64(1) << std::max(0, std::min<int>(m_p.max_pyramid_levels, 12));
    const int64 sdx = std::max(0, m_p.search_max_x - m_p.search_min_x), sdy = std::max(0, m_p.search_max_y - m_p.search_min_y);
    const int64 padx = (m_p.kernel_x / 2) * up + 2 * sdx + 8, pady = (m_p.kernel_y / 2) * up + 2 * sdy + 8;
    const int64 wx0 = std::max<int64>(0, bbox.min().x() - padx + std::min(m_p.search_min_x, 0));
    const int64 wy0 = std::max<int64>(0, bbox.min().y() - pady + std::min(m_p.search_min_y, 0));
    const int64 wx1 = int64(bbox.max().x()) + padx + std::max(m_p.search_max_x, 0);
    const int64 wy1 = int64(bbox.max().y()) + pady + std::max(m_p.search_max_y, 0);
    const int32 ox = (int32)std::min<int64>(wx0, std::min(m_left.cols(), m_right.cols()));
    const int32 oy = (int32)std::min<int64>(wy0, std::min(m_left.rows(), m_right.rows()));
    const BBox2i lwin(ox, oy, (int32)(std::min<int64>(wx1, m_left.cols()) - ox), (int32)(std::min<int64>(wy1, m_left.rows()) - oy));
    const BBox2i rwin(ox, oy, (int32)(std::min<int64>(wx1, m_right.cols()) - ox), (int32)(std::min<int64>(wy1, m_right.rows()) - oy));
    VW_ASSERT(!lwin.empty() && !rwin.empty(), ArgumentErr() << "PyramidCorrelationView: the tile lies outside the images.");
    ImageView<PixelGray<float>> l = m_left.prerasterize(lwin), r = m_right.prerasterize(rwin);
    ImageView<uint8> lm = m_left_mask.prerasterize(lwin), rm = m_right_mask.prerasterize(rwin);
    vwgpu_pyramid_params p = m_p;
    p.region_ul_x -= ox; p.region_ul_y -= oy;
    detail::check(ctx, vwgpu_pyramid_correlate(ctx, reinterpret_cast<const float*>(l.data()), l.cols(), l.rows(), 0,
                                               reinterpret_cast<const float*>(r.data()), r.cols(), r.rows(), 0,
                                               lm.data(), 0, rm.data(), 0, &p,
                                               bbox.min().x() - ox, bbox.min().y() - oy, bbox.width(), bbox.height(),
                                               reinterpret_cast<float*>(out.data()), 0));
    return out;
  }
  /// Several tiles in one engine call (vwgpu_pyramid_correlate_batch, include/vwgpu.h): runs of equal-sized tiles go through the pyramid
  /// level loop together — every launch serves the group, one host round trip per level.  Tile i of the result is what correlate_tile(boxes[i])
  /// returns.  The reference hands tiles to its threads one by one (ImageIO.h:228-251); block_write_image below hands this view a run of
  /// blocks of a block row at a time (group_size()).
  std::vector<ImageView<pixel_type>> correlate_tiles(std::vector<BBox2i> const& boxes) const {
    const int n = (int)boxes.size();
    std::vector<ImageView<pixel_type>> out((size_t)n);
    if (n == 0) return out;
    std::vector<int> bx((size_t)n), by((size_t)n), bw((size_t)n), bh((size_t)n);
    std::vector<float*> ptr((size_t)n);
    BBox2i all;
    for (int i = 0; i < n; ++i) {
      VW_ASSERT(!boxes[i].empty(), ArgumentErr() << "PyramidCorrelationView: empty tile in a group.");
      out[i].set_size(boxes[i].width(), boxes[i].height());
      bx[i] = boxes[i].min().x(); by[i] = boxes[i].min().y(); bw[i] = boxes[i].width(); bh[i] = boxes[i].height();
      ptr[i] = reinterpret_cast<float*>(out[i].data());
      all.grow(boxes[i]);
    }
    vwgpu_ctx* ctx = detail::thread_context();
    int32 ls = 0, rs = 0, lms = 0, rms = 0;
    const PixelGray<float>* lp = m_left.plain_data(ls);
    const PixelGray<float>* rp = m_right.plain_data(rs);
    const uint8* lmp = m_left_mask.plain_data(lms);
    const uint8* rmp = m_right_mask.plain_data(rms);
    if (lp && rp && lmp && rmp) {
      detail::check(ctx, vwgpu_pyramid_correlate_batch(ctx, reinterpret_cast<const float*>(lp), m_left.cols(), m_left.rows(), ls,
                                                       reinterpret_cast<const float*>(rp), m_right.cols(), m_right.rows(), rs, lmp, lms, rmp, rms, &m_p,
                                                       n, bx.data(), by.data(), bw.data(), bh.data(), ptr.data(), NULL));
      return out;
    }
    // lazy sources: one window for the group (the union of the tiles grown as in correlate_tile)
    const int64 up = int64(1) << std::max(0, std::min<int>(m_p.max_pyramid_levels, 12));
    const int64 sdx = std::max(0, m_p.search_max_x - m_p.search_min_x), sdy = std::max(0, m_p.search_max_y - m_p.search_min_y);
    const int64 padx = (m_p.kernel_x / 2) * up + 2 * sdx + 8, pady = (m_p.kernel_y / 2) * up + 2 * sdy + 8;
    const int64 wx0 = std::max<int64>(0, all.min().x() - padx + std::min(m_p.search_min_x, 0));
    const int64 wy0 = std::max<int64>(0, all.min().y() - pady + std::min(m_p.search_min_y, 0));
    const int64 wx1 = int64(all.max().x()) + padx + std::max(m_p.search_max_x, 0);
    const int64 wy1 = int64(all.max().y()) + pady + std::max(m_p.search_max_y, 0);
    const int32 ox = (int32)std::min<int64>(wx0, std::min(m_left.cols(), m_right.cols()));
    const int32 oy = (int32)std::min<int64>(wy0, std::min(m_left.rows(), m_right.rows()));
    const BBox2i lwin(ox, oy, (int32)(std::min<int64>(wx1, m_left.cols()) - ox), (int32)(std::min<int64>(wy1, m_left.rows()) - oy));
    const BBox2i rwin(ox, oy, (int32)(std::min<int64>(wx1, m_right.cols()) - ox), (int32)(std::min<int64>(wy1, m_right.rows()) - oy));
    VW_ASSERT(!lwin.empty() && !rwin.empty(), ArgumentErr() << "PyramidCorrelationView: the tiles lie outside the images.");
    ImageView<PixelGray<float>> l = m_left.prerasterize(lwin), r = m_right.prerasterize(rwin);
    ImageView<uint8> lm = m_left_mask.prerasterize(lwin), rm = m_right_mask.prerasterize(rwin);
    vwgpu_pyramid_params p = m_p;
    p.region_ul_x -= ox; p.region_ul_y -= oy;
    for (int i = 0; i < n; ++i) { bx[i] -= ox; by[i] -= oy; }
    detail::check(ctx, vwgpu_pyramid_correlate_batch(ctx, reinterpret_cast<const float*>(l.data()), l.cols(), l.rows(), 0,
                                                     reinterpret_cast<const float*>(r.data()), r.cols(), r.rows(), 0, lm.data(), 0, rm.data(), 0, &p,
                                                     n, bx.data(), by.data(), bw.data(), bh.data(), ptr.data(), NULL));
    return out;
  }
  /// How many blocks of a block row block_write_image hands over at a time (rasterize_group).
  int32 group_size() const { return 8; }
  /// rasterize() for a run of blocks: collars as in rasterize (CorrelationView.h:123-133), the tiles correlated as one group.
  template <class DestT> void rasterize_group(std::vector<DestT> const& dests, std::vector<BBox2i> const& boxes) const {
    std::vector<BBox2i> proc(boxes);
    if (m_collar_size > 0) for (BBox2i& b : proc) b.expand(m_collar_size);
    std::vector<ImageView<pixel_type>> tiles = correlate_tiles(proc);
    for (size_t i = 0; i < boxes.size(); ++i)
      vw::rasterize(prerasterize_type(tiles[i], -proc[i].min().x(), -proc[i].min().y(), cols(), rows()), dests[i], boxes[i]);
  }
  /// CorrelationView.cc:876-885: the tile wrapped so that GLOBAL pixel coordinates inside bbox address it.
  prerasterize_type prerasterize(BBox2i const& bbox) const {
    return prerasterize_type(correlate_tile(bbox), -bbox.min().x(), -bbox.min().y(), cols(), rows());
  }
  /// CorrelationView.h:123-133: the tile is correlated over the collared box and its centre is kept.
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const {
    BBox2i proc_bbox = bbox;
    if (m_collar_size > 0) proc_bbox.expand(m_collar_size);
    vw::rasterize(prerasterize(proc_bbox), dest, bbox);
  }
};

namespace detail {
// A plain ImageView<PixelGray<float>> is wrapped as it is (the engine then reads it in place); anything else goes through a
// lazy pixel_cast.
inline ImageViewRef<PixelGray<float>> gray_float_ref(ImageView<PixelGray<float>> const& v) { return ImageViewRef<PixelGray<float>>(v); }
template <class ViewT> ImageViewRef<PixelGray<float>> gray_float_ref(ImageViewBase<ViewT> const& v) {
  return ImageViewRef<PixelGray<float>>(pixel_cast<PixelGray<float>>(v.impl()));
}
inline ImageViewRef<uint8> mask_ref(ImageView<uint8> const& v) { return ImageViewRef<uint8>(v); }
template <class ViewT> ImageViewRef<uint8> mask_ref(ImageViewBase<ViewT> const& v) { return ImageViewRef<uint8>(pixel_cast<uint8>(v.impl())); }
}  // namespace detail

/// pyramid_correlate — the reference's argument list (CorrelationView.h:195-230), verbatim; the image / mask arguments
/// accept any view (the reference takes ImageViewRef handles, which convert from any view as well).  All four algorithms
/// are implemented (VW_CORRELATION_MGM: use_mgm at every level, _FINAL_MGM: at level 0 only).  write_debug_images is
/// accepted and ignored (the reference's debug dumps are TIFF files written next to the process).
template <class Image1T, class Image2T, class Mask1T, class Mask2T>
PyramidCorrelationView
pyramid_correlate(ImageViewBase<Image1T> const& left, ImageViewBase<Image2T> const& right,
                  ImageViewBase<Mask1T> const& left_mask, ImageViewBase<Mask2T> const& right_mask,
                  PrefilterModeType prefilter_mode, float prefilter_width,
                  BBox2i const& search_region, Vector2i const& kernel_size, CostFunctionType cost_type,
                  int corr_timeout, double seconds_per_op, float consistency_threshold, int min_consistency_level,
                  int filter_half_kernel, int32 max_pyramid_levels,
                  CorrelationAlgorithm algorithm = VW_CORRELATION_BM, int collar_size = 0,
                  SemiGlobalMatcher::SgmSubpixelMode sgm_subpixel_mode = SemiGlobalMatcher::SUBPIXEL_LC_BLEND,
                  Vector2i sgm_search_buffer = Vector2i(2, 2), size_t memory_limit_mb = 6000, int blob_filter_area = 0,
                  ImageView<PixelMask<float>>* lr_disp_diff = NULL, Vector2i const& region_ul = Vector2i(0, 0),
                  bool write_debug_images = false) {
  (void)write_debug_images;
  vwgpu_pyramid_params p = vwgpu_pyramid_params();   // lr_disp_diff is wired by the view's constructor
  p.prefilter_mode = (int)prefilter_mode; p.prefilter_width = prefilter_width;
  p.search_min_x = search_region.min().x(); p.search_min_y = search_region.min().y();
  p.search_max_x = search_region.max().x(); p.search_max_y = search_region.max().y();
  p.kernel_x = kernel_size[0]; p.kernel_y = kernel_size[1];
  p.cost_type = (int)cost_type; p.corr_timeout = corr_timeout; p.seconds_per_op = seconds_per_op;
  p.consistency_threshold = consistency_threshold; p.min_consistency_level = min_consistency_level;
  p.filter_half_kernel = filter_half_kernel; p.max_pyramid_levels = max_pyramid_levels;
  p.algorithm = (int)algorithm; p.blob_filter_area = blob_filter_area;
  p.sgm_subpixel_mode = (int)sgm_subpixel_mode; p.sgm_search_buffer_x = sgm_search_buffer[0]; p.sgm_search_buffer_y = sgm_search_buffer[1];
  p.memory_limit_mb = memory_limit_mb; p.sgm_num_threads = 1;
  return PyramidCorrelationView(detail::gray_float_ref(left.impl()), detail::gray_float_ref(right.impl()),
                                detail::mask_ref(left_mask.impl()), detail::mask_ref(right_mask.impl()), p, collar_size, lr_disp_diff, region_ul);
}

enum PyramidSubpixelView_Algorithm {     // src/vw/Stereo/SubpixelView.h:28-33
  SUBPIXEL_LUCAS_KANADE = 0, SUBPIXEL_FAST_AFFINE = 1, SUBPIXEL_BAYES_EM = 2, SUBPIXEL_PHASE = 3
};

/// PyramidSubpixelView (src/vw/Stereo/SubpixelView.h:36-108): lazy; rasterize(dest, bbox) runs one
/// prerasterize(bbox) of the reference (SubpixelView.cc:33-224) on the engine (vwgpu_pyramid_subpixel).  The result of a
/// pixel depends on the tile it is rasterised in, as in the reference.  SUBPIXEL_LUCAS_KANADE, SUBPIXEL_FAST_AFFINE and
/// SUBPIXEL_BAYES_EM are implemented; the engine reports SUBPIXEL_PHASE as NoImplErr through this constructor: phase
/// refinement is reached through phase_subpixel(...), which takes the accuracy argument (vwgpu_phase_subpixel).
class PyramidSubpixelView : public ImageViewBase<PyramidSubpixelView> {
  ImageViewRef<PixelMask<Vector2f>> m_disparity_map;
  ImageViewRef<PixelGray<float>> m_left_image, m_right_image;
  Vector2i m_kernel_size;
  int32 m_max_pyramid_levels;
  PyramidSubpixelView_Algorithm m_algorithm;
  PrefilterModeType m_prefilter_mode;
  float m_prefilter_width;
  bool m_phase_entry = false;        // built by phase_subpixel: vwgpu_phase_subpixel with m_phase_accuracy
  int32 m_phase_accuracy = 20;
  friend PyramidSubpixelView phase_subpixel(ImageViewRef<PixelMask<Vector2f>> const&, ImageViewRef<PixelGray<float>> const&,
                                            ImageViewRef<PixelGray<float>> const&, PrefilterModeType, float, Vector2i const&,
                                            int, int);
public:
  typedef PixelMask<Vector2f> pixel_type;
  typedef pixel_type result_type;
  typedef CropView<ImageView<pixel_type>> prerasterize_type;

  PyramidSubpixelView(ImageViewRef<PixelMask<Vector2f>> const& disparity_map, ImageViewRef<PixelGray<float>> const& left_image,
                      ImageViewRef<PixelGray<float>> const& right_image, PrefilterModeType prefilter_mode, float prefilter_width,
                      Vector2i const& kernel_size, int32 max_pyramid_levels, PyramidSubpixelView_Algorithm algorithm)
      : m_disparity_map(disparity_map), m_left_image(left_image), m_right_image(right_image), m_kernel_size(kernel_size),
        m_max_pyramid_levels(max_pyramid_levels < 0 ? 0 : max_pyramid_levels), m_algorithm(algorithm),
        m_prefilter_mode(prefilter_mode), m_prefilter_width(prefilter_width) {
    VW_ASSERT(m_disparity_map.cols() == m_left_image.cols() && m_disparity_map.rows() == m_left_image.rows(),
              ArgumentErr() << "PyramidSubpixelView::PyramidSubpixelView(): Disparity image must match left image.\n");
  }
  int32 cols() const { return m_left_image.cols(); }
  int32 rows() const { return m_left_image.rows(); }
  int32 planes() const { return 1; }
  pixel_type operator()(int32 /*i*/, int32 /*j*/, int32 /*p*/ = 0) const {
    vw_throw(NoImplErr() << "PyramidSubpixelView::operator() is not yet implemented.");   // SubpixelView.h:93-96
    return pixel_type();
  }
  /// The tile at bbox, indexed from the tile's own origin.  The operands are rasterised whole (the tile's patch depends on
  /// its disparity range), and the engine writes into an image of the full size of which the tile is copied out.
  ImageView<pixel_type> refine_tile(BBox2i const& bbox) const {
    ImageView<pixel_type> tile(bbox.width(), bbox.height());
    if (bbox.empty()) return tile;
    const BBox2i all(0, 0, cols(), rows()), rall(0, 0, m_right_image.cols(), m_right_image.rows());
    ImageView<pixel_type> d = m_disparity_map.prerasterize(all), full(cols(), rows());
    ImageView<PixelGray<float>> l = m_left_image.prerasterize(all), r = m_right_image.prerasterize(rall);
    const int box[4] = {bbox.min().x(), bbox.min().y(), bbox.width(), bbox.height()};
    vwgpu_ctx* ctx = detail::thread_context();
    if (m_phase_entry)
      detail::check(ctx, vwgpu_phase_subpixel(ctx, reinterpret_cast<const float*>(d.data()), d.cols(), d.rows(), 0,
                                              reinterpret_cast<const float*>(l.data()), 0,
                                              reinterpret_cast<const float*>(r.data()), r.cols(), r.rows(), 0,
                                              (int)m_prefilter_mode, m_prefilter_width, m_kernel_size[0], m_kernel_size[1],
                                              m_max_pyramid_levels, m_phase_accuracy, box, 1,
                                              reinterpret_cast<float*>(full.data()), 0, NULL));
    else
      detail::check(ctx, vwgpu_pyramid_subpixel(ctx, reinterpret_cast<const float*>(d.data()), d.cols(), d.rows(), 0,
                                                reinterpret_cast<const float*>(l.data()), 0,
                                                reinterpret_cast<const float*>(r.data()), r.cols(), r.rows(), 0,
                                                (int)m_prefilter_mode, m_prefilter_width, m_kernel_size[0], m_kernel_size[1],
                                                m_max_pyramid_levels, (int)m_algorithm, box, 1,
                                                reinterpret_cast<float*>(full.data()), 0, NULL));
    for (int32 y = 0; y < bbox.height(); ++y)
      for (int32 x = 0; x < bbox.width(); ++x) tile(x, y) = full(bbox.min().x() + x, bbox.min().y() + y);
    return tile;
  }
  prerasterize_type prerasterize(BBox2i const& bbox) const {
    return prerasterize_type(refine_tile(bbox), -bbox.min().x(), -bbox.min().y(), cols(), rows());
  }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const {
    ImageView<pixel_type> t = refine_tile(bbox);
    for (int32 y = 0; y < bbox.height(); ++y)
      for (int32 x = 0; x < bbox.width(); ++x) dest(x, y) = t(x, y);
  }
};

/// lk_subpixel (src/vw/Stereo/SubpixelView.h:111-117).
inline PyramidSubpixelView
lk_subpixel(ImageViewRef<PixelMask<Vector2f>> const& disparity_map, ImageViewRef<PixelGray<float>> const& left_image,
            ImageViewRef<PixelGray<float>> const& right_image, PrefilterModeType prefilter_mode, float prefilter_width,
            Vector2i const& kernel_size, int max_pyramid_levels = 2) {
  return PyramidSubpixelView(disparity_map, left_image, right_image, prefilter_mode, prefilter_width, kernel_size,
                             max_pyramid_levels, SUBPIXEL_LUCAS_KANADE);
}

/// bayes_em_subpixel (src/vw/Stereo/SubpixelView.h:127-133).
inline PyramidSubpixelView
bayes_em_subpixel(ImageViewRef<PixelMask<Vector2f>> const& disparity_map, ImageViewRef<PixelGray<float>> const& left_image,
                  ImageViewRef<PixelGray<float>> const& right_image, PrefilterModeType prefilter_mode, float prefilter_width,
                  Vector2i const& kernel_size, int max_pyramid_levels = 2) {
  return PyramidSubpixelView(disparity_map, left_image, right_image, prefilter_mode, prefilter_width, kernel_size,
                             max_pyramid_levels, SUBPIXEL_BAYES_EM);
}

/// affine_subpixel (src/vw/Stereo/SubpixelView.h:120-126, SubpixelView.cc:242-254).
inline PyramidSubpixelView
affine_subpixel(ImageViewRef<PixelMask<Vector2f>> const& disparity_map, ImageViewRef<PixelGray<float>> const& left_image,
                ImageViewRef<PixelGray<float>> const& right_image, PrefilterModeType prefilter_mode, float prefilter_width,
                Vector2i const& kernel_size, int max_pyramid_levels = 2) {
  return PyramidSubpixelView(disparity_map, left_image, right_image, prefilter_mode, prefilter_width, kernel_size,
                             max_pyramid_levels, SUBPIXEL_FAST_AFFINE);
}

/// phase_subpixel (src/vw/Stereo/SubpixelView.h:136-144, SubpixelView.cc:275-289): PyramidSubpixelView with SUBPIXEL_PHASE
/// and the phase accuracy, rasterised through vwgpu_phase_subpixel (kernels up to 41 x 41, accuracy up to 64).
inline PyramidSubpixelView
phase_subpixel(ImageViewRef<PixelMask<Vector2f>> const& disparity_map, ImageViewRef<PixelGray<float>> const& left_image,
               ImageViewRef<PixelGray<float>> const& right_image, PrefilterModeType prefilter_mode, float prefilter_width,
               Vector2i const& kernel_size, int max_pyramid_levels = 0, int phase_subpixel_accuracy = 20) {
  PyramidSubpixelView v(disparity_map, left_image, right_image, prefilter_mode, prefilter_width, kernel_size,
                        max_pyramid_levels, SUBPIXEL_PHASE);
  v.m_phase_entry = true;
  v.m_phase_accuracy = phase_subpixel_accuracy;
  return v;
}

/// CorrEval (src/vw/Stereo/CorrEval.h:56-115): lazy; prerasterize(bbox) is one vwgpu_corr_eval call with the one box
/// (CorrEval.cc:139-317).  The result of a pixel depends on the tile it is rasterised in, as in the reference (the right
/// crop is built per tile, and only pixels whose column and row inside the tile are multiples of sample_rate are
/// evaluated).  Kernels up to 63 x 63 (NoImplErr above).
static_assert(sizeof(PixelMask<float>) == 8, "PixelMask<float> is the engine's {value, valid} pair");
class CorrEval : public ImageViewBase<CorrEval> {
  ImageViewRef<PixelMask<float>> m_left, m_right;
  ImageViewRef<PixelMask<Vector2f>> m_disp;
  Vector2i m_kernel_size;
  std::string m_metric;
  int m_sample_rate;
  bool m_round_to_int;
  int m_prefilter_mode;
  float m_prefilter_kernel_width;
public:
  typedef PixelMask<float> pixel_type;
  typedef PixelMask<float> result_type;
  typedef CropView<ImageView<pixel_type>> prerasterize_type;

  CorrEval(ImageViewRef<PixelMask<float>> left, ImageViewRef<PixelMask<float>> right, ImageViewRef<PixelMask<Vector2f>> disp,
           Vector2i const& kernel_size, std::string const& metric, int sample_rate, bool round_to_int, int prefilter_mode = 0,
           float prefilter_kernel_width = 0.0)
      : m_left(left), m_right(right), m_disp(disp), m_kernel_size(kernel_size), m_metric(metric), m_sample_rate(sample_rate),
        m_round_to_int(round_to_int), m_prefilter_mode(prefilter_mode), m_prefilter_kernel_width(prefilter_kernel_width) {
    VW_ASSERT(m_left.cols() == m_disp.cols() && m_left.rows() == m_disp.rows(),
              ArgumentErr() << "CorrEval: Left image and disparity must have the same dimensions.\n");
    VW_ASSERT(m_kernel_size[0] > 0 && m_kernel_size[0] % 2 == 1 && m_kernel_size[1] > 0 && m_kernel_size[1] % 2 == 1,
              ArgumentErr() << "CorrEval: The kernel dimensions must be positive and odd.\n");
    VW_ASSERT(metric_code() >= 0, ArgumentErr() << "CorrEval: Invalid metric: " << m_metric << ".\n");
  }
  int metric_code() const {
    return m_metric == "ncc" ? VWGPU_CORR_EVAL_NCC : m_metric == "stddev" ? VWGPU_CORR_EVAL_STDDEV
         : m_metric == "parabola_curvature" ? VWGPU_CORR_EVAL_PARABOLA_CURVATURE
         : m_metric == "cramer_rao" ? VWGPU_CORR_EVAL_CRAMER_RAO : -1;
  }
  int32 cols() const { return m_left.cols(); }
  int32 rows() const { return m_left.rows(); }
  int32 planes() const { return 1; }
  pixel_type operator()(int32 /*i*/, int32 /*j*/, int32 /*p*/ = 0) const {
    vw_throw(NoImplErr() << "CorrEval::operator() is not implemented.");   // CorrEval.h:103-106
    return pixel_type();
  }
  /// The tile at bbox, indexed from the tile's own origin.  The operands are rasterised whole (the right crop depends on
  /// the tile's disparities), and the engine writes into an image of the full size of which the tile is copied out.
  ImageView<pixel_type> evaluate_tile(BBox2i const& bbox) const {
    ImageView<pixel_type> tile(bbox.width(), bbox.height());
    if (bbox.empty()) return tile;
    const BBox2i all(0, 0, cols(), rows()), rall(0, 0, m_right.cols(), m_right.rows());
    ImageView<PixelMask<Vector2f>> d = m_disp.prerasterize(all);
    ImageView<pixel_type> l = m_left.prerasterize(all), r = m_right.prerasterize(rall), full(cols(), rows());
    std::vector<float> lv((size_t)l.cols() * l.rows()), rv((size_t)r.cols() * r.rows());
    std::vector<uint8_t> lm(lv.size()), rm(rv.size());
    for (int32 y = 0; y < l.rows(); ++y)
      for (int32 x = 0; x < l.cols(); ++x) {
        lv[(size_t)y * l.cols() + x] = l(x, y).child();
        lm[(size_t)y * l.cols() + x] = is_valid(l(x, y)) ? 1 : 0;
      }
    for (int32 y = 0; y < r.rows(); ++y)
      for (int32 x = 0; x < r.cols(); ++x) {
        rv[(size_t)y * r.cols() + x] = r(x, y).child();
        rm[(size_t)y * r.cols() + x] = is_valid(r(x, y)) ? 1 : 0;
      }
    const int box[4] = {bbox.min().x(), bbox.min().y(), bbox.width(), bbox.height()};
    vwgpu_ctx* ctx = detail::thread_context();
    detail::check(ctx, vwgpu_corr_eval(ctx, reinterpret_cast<const float*>(d.data()), d.cols(), d.rows(), 0, lv.data(), lm.data(), 0,
                                       rv.data(), rm.data(), r.cols(), r.rows(), 0, m_kernel_size[0], m_kernel_size[1],
                                       metric_code(), m_sample_rate, m_round_to_int ? 1 : 0, m_prefilter_mode,
                                       m_prefilter_kernel_width, box, 1, reinterpret_cast<float*>(full.data()), 0, NULL));
    for (int32 y = 0; y < bbox.height(); ++y)
      for (int32 x = 0; x < bbox.width(); ++x) tile(x, y) = full(bbox.min().x() + x, bbox.min().y() + y);
    return tile;
  }
  prerasterize_type prerasterize(BBox2i const& bbox) const {
    return prerasterize_type(evaluate_tile(bbox), -bbox.min().x(), -bbox.min().y(), cols(), rows());
  }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const {
    ImageView<pixel_type> t = evaluate_tile(bbox);
    for (int32 y = 0; y < bbox.height(); ++y)
      for (int32 x = 0; x < bbox.width(); ++x) dest(x, y) = t(x, y);
  }
};

/// corr_eval (src/vw/Stereo/CorrEval.h:117-128).
inline CorrEval corr_eval(ImageViewRef<PixelMask<float>> left, ImageViewRef<PixelMask<float>> right,
                          ImageViewRef<PixelMask<Vector2f>> disp, Vector2i const& kernel_size, std::string const& metric,
                          int sample_rate, bool round_to_int, int prefilter_mode = 0, float prefilter_kernel_width = 0.0) {
  return CorrEval(left, right, disp, kernel_size, metric, sample_rate, round_to_int, prefilter_mode, prefilter_kernel_width);
}

// ---- the disparity post-filters of Stereo/Algorithms.h -------------------------------------------------------------
// The reference's three disparity filters start with `disparity_out = disparity_in`, a shallow copy, and then filter in
// place in raster order (include/vwgpu.h, vwgpu_filter_semantics).  By default these functions do the same: the engine
// filters disparity_in's buffer in place and disparity_out shares it afterwards.  snapshot = true filters every pixel
// from the unmodified input into a fresh image and leaves disparity_in alone.
namespace detail {
static_assert(sizeof(PixelMask<Vector2f>) == 12 && sizeof(PixelMask<Vector2i>) == 12, "{dx, dy, valid} pixels");
// call(in, out, box): the engine entry on one whole-image box
template <class PixelT, class CallT>
void post_filter(ImageView<PixelT> const& disparity_in, ImageView<PixelT>& disparity_out, bool snapshot, CallT call) {
  if (disparity_in.cols() == 0 || disparity_in.rows() == 0) {
    disparity_out = disparity_in;
    return;
  }
  const int box[4] = {0, 0, disparity_in.cols(), disparity_in.rows()};
  if (!snapshot) {
    call(disparity_in.data(), disparity_in.data(), box, (int)VWGPU_FILTER_REFERENCE);
    disparity_out = disparity_in;
    return;
  }
  ImageView<PixelT> fresh(disparity_in.cols(), disparity_in.rows());
  call(disparity_in.data(), fresh.data(), box, (int)VWGPU_FILTER_SNAPSHOT);
  disparity_out = fresh;
}
}  // namespace detail

/// disparity_median_filter (Algorithms.h:132-135, Algorithms.cc:26-67); kernel sizes up to 31 (NoImplErr above).
inline void disparity_median_filter(ImageView<PixelMask<Vector2f>> const& disparity_in,
                                    ImageView<PixelMask<Vector2f>>& disparity_out, int kernel_size, bool snapshot = false) {
  detail::post_filter(disparity_in, disparity_out, snapshot,
                      [&](PixelMask<Vector2f>* in, PixelMask<Vector2f>* out, const int* box, int semantics) {
    vwgpu_ctx* ctx = detail::thread_context();
    detail::check(ctx, vwgpu_disparity_median_filter(ctx, reinterpret_cast<const float*>(in), box[2], box[3], 0, kernel_size,
                                                     semantics, box, 1, reinterpret_cast<float*>(out), 0, NULL));
  });
}

/// disparity_neighbor_filter (Algorithms.h:137-139, Algorithms.cc:69-110).
inline void disparity_neighbor_filter(ImageView<PixelMask<Vector2i>> const& disparity_in,
                                      ImageView<PixelMask<Vector2i>>& disparity_out, bool snapshot = false) {
  detail::post_filter(disparity_in, disparity_out, snapshot,
                      [&](PixelMask<Vector2i>* in, PixelMask<Vector2i>* out, const int* box, int semantics) {
    vwgpu_ctx* ctx = detail::thread_context();
    detail::check(ctx, vwgpu_disparity_neighbor_filter(ctx, reinterpret_cast<const int32_t*>(in), box[2], box[3], 0, semantics,
                                                       box, 1, reinterpret_cast<int32_t*>(out), 0, NULL));
  });
}

/// texture_measure (Algorithms.h:144-209) of a plain float image (masked inputs: not implemented); kernel sizes up to 31.
template <class ImageT>
inline void texture_measure(ImageViewBase<ImageT> const& input_image, ImageView<float>& output_image, int kernel_size = 9,
                            double gradient_weight = 0.5, double stddev_weight = 0.5) {
  ImageView<float> in = pixel_cast<float>(input_image.impl());
  output_image.set_size(in.cols(), in.rows());
  if (in.cols() == 0 || in.rows() == 0) return;
  const int box[4] = {0, 0, in.cols(), in.rows()};
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_texture_measure(ctx, in.data(), in.cols(), in.rows(), 0, kernel_size, gradient_weight, stddev_weight,
                                           box, 1, output_image.data(), 0, NULL));
}

/// texture_preserving_disparity_filter<float> (Algorithms.h:215-281); max_kernel_size up to 31 (NoImplErr above).
inline void texture_preserving_disparity_filter(ImageView<PixelMask<Vector2f>> const& disparity_in,
                                                ImageView<PixelMask<Vector2f>>& disparity_out,
                                                ImageView<float> const& texture_image, float texture_max = 0.15,
                                                int max_kernel_size = 11, bool snapshot = false) {
  VW_ASSERT(texture_image.cols() == disparity_in.cols() && texture_image.rows() == disparity_in.rows(),
            ArgumentErr() << "texture_preserving_disparity_filter: texture image and disparity must have the same dimensions.");
  detail::post_filter(disparity_in, disparity_out, snapshot,
                      [&](PixelMask<Vector2f>* in, PixelMask<Vector2f>* out, const int* box, int semantics) {
    vwgpu_ctx* ctx = detail::thread_context();
    detail::check(ctx, vwgpu_texture_preserving_disparity_filter(ctx, reinterpret_cast<const float*>(in), box[2], box[3], 0,
                                                                 texture_image.data(), 0, texture_max, max_kernel_size,
                                                                 semantics, box, 1, reinterpret_cast<float*>(out), 0, NULL));
  });
}

// ---- the local outlier filters of Stereo/DisparityMap.h and std_dev_image ------------------------------------------
// Rasterised over the whole image, on PixelMask<Vector2i> and PixelMask<Vector2f> disparities (include/vwgpu.h,
// vwgpu_rm_outliers).  Half kernel sizes up to 15 (NoImplErr above).  reference_loop = false selects
// VWGPU_OUTLIER_SKIP for the mean method.
namespace detail {
inline int disparity_type_code(PixelMask<Vector2i> const*) { return VWGPU_DISPARITY_I32; }
inline int disparity_type_code(PixelMask<Vector2f> const*) { return VWGPU_DISPARITY_F32; }
template <class PixelT>
ImageView<PixelT> rm_outliers(ImageView<PixelT> const& d, int method, int32 hh, int32 hv, double p0, double p1, int cleanup,
                              int semantics) {
  VW_ASSERT(hh > 0 && hv > 0, ArgumentErr() << (method == VWGPU_OUTLIER_MEAN ? "RmOutliersUsingMeanFunc" : "RmOutliersFunc")
                                            << ": half kernel sizes must be non-zero.");
  ImageView<PixelT> out(d.cols(), d.rows());
  if (d.cols() == 0 || d.rows() == 0) return out;
  vwgpu_ctx* ctx = thread_context();
  check(ctx, vwgpu_rm_outliers(ctx, method, disparity_type_code(d.data()), d.data(), d.cols(), d.rows(), 0, hh, hv, p0, p1, cleanup,
                               semantics, out.data(), 0, NULL));
  return out;
}
}  // namespace detail

/// rm_outliers_using_mean (DisparityMap.h:567-578).
template <class PixelT>
ImageView<PixelT> rm_outliers_using_mean(ImageView<PixelT> const& disparity_map, int32 half_h_kernel, int32 half_v_kernel,
                                         double max_mean_diff, bool reference_loop = true) {
  return detail::rm_outliers(disparity_map, VWGPU_OUTLIER_MEAN, half_h_kernel, half_v_kernel, max_mean_diff, 0.0, 0,
                             reference_loop ? VWGPU_OUTLIER_REFERENCE : VWGPU_OUTLIER_SKIP);
}
/// disparity_cleanup_using_mean (DisparityMap.h:580-598).
template <class PixelT>
ImageView<PixelT> disparity_cleanup_using_mean(ImageView<PixelT> const& disparity_map, int32 h_half_kernel, int32 v_half_kernel,
                                               double max_mean_diff, bool reference_loop = true) {
  return detail::rm_outliers(disparity_map, VWGPU_OUTLIER_MEAN, h_half_kernel, v_half_kernel, max_mean_diff, 0.0, 1,
                             reference_loop ? VWGPU_OUTLIER_REFERENCE : VWGPU_OUTLIER_SKIP);
}
/// rm_outliers_using_stddev (DisparityMap.h:737-748).
template <class PixelT>
ImageView<PixelT> rm_outliers_using_stddev(ImageView<PixelT> const& disparity_map, int32 half_h_kernel, int32 half_v_kernel,
                                           double pixel_threshold, double rejection_threshold) {
  return detail::rm_outliers(disparity_map, VWGPU_OUTLIER_STDDEV, half_h_kernel, half_v_kernel, pixel_threshold,
                             rejection_threshold, 0, VWGPU_OUTLIER_REFERENCE);
}
/// disparity_cleanup_using_stddev (DisparityMap.h:750-767).
template <class PixelT>
ImageView<PixelT> disparity_cleanup_using_stddev(ImageView<PixelT> const& disparity_map, int32 h_half_kernel, int32 v_half_kernel,
                                                 double pixel_threshold, double rejection_threshold) {
  return detail::rm_outliers(disparity_map, VWGPU_OUTLIER_STDDEV, h_half_kernel, v_half_kernel, pixel_threshold,
                             rejection_threshold, 1, VWGPU_OUTLIER_REFERENCE);
}
/// rm_outliers_using_plane (DisparityMap.h:916-927).
template <class PixelT>
ImageView<PixelT> rm_outliers_using_plane(ImageView<PixelT> const& disparity_map, int32 half_h_kernel, int32 half_v_kernel,
                                          double pixel_threshold, double rejection_threshold) {
  return detail::rm_outliers(disparity_map, VWGPU_OUTLIER_PLANE, half_h_kernel, half_v_kernel, pixel_threshold,
                             rejection_threshold, 0, VWGPU_OUTLIER_REFERENCE);
}
/// disparity_clean_using_plane (DisparityMap.h:929-947; the reference's spelling).
template <class PixelT>
ImageView<PixelT> disparity_clean_using_plane(ImageView<PixelT> const& disparity_map, int32 h_half_kernel, int32 v_half_kernel,
                                              double pixel_threshold, double rejection_threshold) {
  return detail::rm_outliers(disparity_map, VWGPU_OUTLIER_PLANE, h_half_kernel, v_half_kernel, pixel_threshold,
                             rejection_threshold, 1, VWGPU_OUTLIER_REFERENCE);
}

/// std_dev_image (DisparityMap.h:998-1014) of a plain float image; kernel sizes up to 31 (NoImplErr above).
template <class EdgeT>
ImageView<float> std_dev_image(ImageView<float> const& image, int32 kernel_width, int32 kernel_height, EdgeT edge) {
  VW_ASSERT(kernel_width > 0 && kernel_height > 0, ArgumentErr() << "StdDevImageFunc: kernel sizes must be non-zero.");
  ImageView<float> out(image.cols(), image.rows());
  if (image.cols() == 0 || image.rows() == 0) return out;
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_std_dev_image(ctx, image.data(), image.cols(), image.rows(), 0, kernel_width, kernel_height,
                                         vw::detail::edge_code(edge), out.data(), 0));
  return out;
}
inline ImageView<float> std_dev_image(ImageView<float> const& image, int32 kernel_width, int32 kernel_height) {
  return std_dev_image(image, kernel_width, kernel_height, ZeroEdgeExtension());
}

// ---- the rest of Stereo/DisparityMap.h: range, masks, transforms, resampling ---------------------------------------
// Each function rasterises its argument, calls the engine on the whole image (include/vwgpu.h) and returns the result
// as an ImageView, which takes part in the block protocol like the other filter results.  Both disparity pixel types.

/// The (min, max) corners of get_disparity_range's BBox2f.
struct BBox2f {
  Vector2f m_min, m_max;
  BBox2f() {}
  BBox2f(Vector2f const& mn, Vector2f const& mx) : m_min(mn), m_max(mx) {}
  Vector2f const& min() const { return m_min; }
  Vector2f const& max() const { return m_max; }
};

/// get_disparity_range (DisparityMap.h:48-66): over the valid pixels, BBox2f(0, 0, 0, 0) when there is none.
template <class ViewT>
BBox2f get_disparity_range(ImageViewBase<ViewT> const& disparity_map) {
  ImageView<typename ViewT::pixel_type> d = disparity_map.impl();
  if (d.cols() == 0 || d.rows() == 0) return BBox2f();
  float r[4] = {0, 0, 0, 0};
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_get_disparity_range(ctx, detail::disparity_type_code(d.data()), d.data(), d.cols(), d.rows(), 0, r));
  return BBox2f(Vector2f(r[0], r[1]), Vector2f(r[2], r[3]));
}

/// PixelRGB<uint8> of missing_pixel_image.
struct PixelRGB8 {
  uint8 r, g, b;
  bool operator==(PixelRGB8 const& o) const { return r == o.r && g == o.g && b == o.b; }
};
/// missing_pixel_image (DisparityMap.h:68-87).
template <class ViewT>
ImageView<PixelRGB8> missing_pixel_image(ImageViewBase<ViewT> const& image) {
  ImageView<typename ViewT::pixel_type> d = image.impl();
  ImageView<PixelRGB8> out(d.cols(), d.rows());
  if (d.cols() == 0 || d.rows() == 0) return out;
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_missing_pixel_image(ctx, detail::disparity_type_code(d.data()), d.data(), d.cols(), d.rows(), 0,
                                               reinterpret_cast<unsigned char*>(out.data()), 0));
  return out;
}

/// disparity_range_mask (DisparityMap.h:255-300); reference_bounds = false compares the lower bound of y with min[1]
/// instead of the reference's min[0] (:279).
template <class ViewT>
ImageView<typename ViewT::pixel_type> disparity_range_mask(ImageViewBase<ViewT> const& disparity_map,
                                                           typename ViewT::pixel_type const& min,
                                                           typename ViewT::pixel_type const& max, bool reference_bounds = true) {
  ImageView<typename ViewT::pixel_type> d = disparity_map.impl(), out(d.cols(), d.rows());
  if (d.cols() == 0 || d.rows() == 0) return out;
  const double mn[2] = {(double)min[0], (double)min[1]}, mx[2] = {(double)max[0], (double)max[1]};
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_disparity_range_mask(ctx, detail::disparity_type_code(d.data()), d.data(), d.cols(), d.rows(), 0, 0, 0, mn, mx,
                                                reference_bounds ? VWGPU_RANGE_MASK_REFERENCE : VWGPU_RANGE_MASK_FIXED, out.data(), 0,
                                                NULL));
  return out;
}

namespace detail {
template <class PixelT>
ImageView<PixelT> transform_disparities(ImageView<PixelT> const& d, Matrix3x3 const& applied, int mode, int32 x0, int32 y0) {
  ImageView<PixelT> out(d.cols(), d.rows());
  if (d.cols() == 0 || d.rows() == 0) return out;
  vwgpu_ctx* ctx = thread_context();
  check(ctx, vwgpu_transform_disparities(ctx, disparity_type_code(d.data()), d.data(), d.cols(), d.rows(), 0, x0, y0, applied.data(), mode,
                                         out.data(), 0));
  return out;
}
}  // namespace detail

/// transform_disparities(disparity_map, HomographyTransform(H)) (DisparityMap.h:1046-1057): the functor calls
/// transform.reverse(), so inverse(H) is applied.
template <class ViewT>
ImageView<typename ViewT::pixel_type> transform_disparities(ImageViewBase<ViewT> const& disparity_map,
                                                            HomographyTransform const& transform) {
  ImageView<typename ViewT::pixel_type> d = disparity_map.impl();
  return detail::transform_disparities(d, transform.inverse_matrix(), VWGPU_TRANSFORM_FUNCTOR, 0, 0);
}
/// transform_disparities(do_round, subregion, T, disparity) (DisparityMap.h:1190-1224).
template <class DispT>
ImageView<typename DispT::pixel_type> transform_disparities(bool do_round, BBox2i subregion, Matrix3x3 const& T,
                                                            DispT const& disparity) {
  VW_ASSERT(subregion.width() == disparity.cols() && subregion.height() == disparity.rows(),
            ArgumentErr() << "transform_disparities: The sizes of subregion and disparity don't match.\n");
  ImageView<typename DispT::pixel_type> d = disparity;
  return detail::transform_disparities(d, T, do_round ? VWGPU_TRANSFORM_SUBREGION_ROUND : VWGPU_TRANSFORM_SUBREGION,
                                       subregion.min().x(), subregion.min().y());
}

/// intersect_mask_and_data (DisparityMap.h:1226-1249).
template <class ViewT, class MaskViewT>
ImageView<typename ViewT::pixel_type> intersect_mask_and_data(ImageViewBase<ViewT> const& view, ImageViewBase<MaskViewT> const& mask_view) {
  ImageView<typename ViewT::pixel_type> d = view.impl(), m = mask_view.impl(), out(d.cols(), d.rows());
  VW_ASSERT(d.cols() == m.cols() && d.rows() == m.rows(), ArgumentErr() << "intersect_mask_and_data: the images differ in size.");
  if (d.cols() == 0 || d.rows() == 0) return out;
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_intersect_mask_and_data(ctx, detail::disparity_type_code(d.data()), d.data(), 0, m.data(), 0, d.cols(), d.rows(),
                                                   out.data(), 0));
  return out;
}

/// disparity_subsample (DisparityMap.h:1318-1322).
template <class ViewT>
ImageView<typename ViewT::pixel_type> disparity_subsample(ImageViewBase<ViewT> const& view) {
  ImageView<typename ViewT::pixel_type> d = view.impl();
  if (d.cols() == 0 || d.rows() == 0) return ImageView<typename ViewT::pixel_type>();
  ImageView<typename ViewT::pixel_type> out(1 + (d.cols() - 1) / 2, 1 + (d.rows() - 1) / 2);
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_disparity_subsample(ctx, detail::disparity_type_code(d.data()), d.data(), d.cols(), d.rows(), 0, out.data(), 0));
  return out;
}
/// disparity_upsample (DisparityMap.h:1354-1358).
template <class ViewT>
ImageView<typename ViewT::pixel_type> disparity_upsample(ImageViewBase<ViewT> const& view) {
  ImageView<typename ViewT::pixel_type> d = view.impl(), out(d.cols() * 2, d.rows() * 2);
  if (d.cols() == 0 || d.rows() == 0) return out;
  vwgpu_ctx* ctx = detail::thread_context();
  detail::check(ctx, vwgpu_disparity_upsample(ctx, detail::disparity_type_code(d.data()), d.data(), d.cols(), d.rows(), 0, out.data(), 0));
  return out;
}

/// DisparityTransform (DisparityMap.h:1164-1187): transform(right_image, DisparityTransform(disparity)) projects the
/// right image into the perspective of the left.
class DisparityTransform {
  ImageView<PixelMask<Vector2f>> m_offset_image;
public:
  template <class DisparityT>
  DisparityTransform(ImageViewBase<DisparityT> const& offset_image) : m_offset_image(offset_image.impl()) {}
  ImageView<PixelMask<Vector2f>> const& offset_image() const { return m_offset_image; }
  /// nearest pixel of the zero-extended offset image (Image/Interpolation.h:221-224, Math/Functions.h:48-51)
  Vector2 reverse(Vector2 const& p) const {
    const int32 x = p.x() < 0 ? int32(p.x() - 0.5) : int32(p.x() + 0.5), y = p.y() < 0 ? int32(p.y() - 0.5) : int32(p.y() + 0.5);
    if (x < 0 || y < 0 || x >= m_offset_image.cols() || y >= m_offset_image.rows() || !is_valid(m_offset_image(x, y)))
      return Vector2(-1, p.y());
    return Vector2(p.x() + m_offset_image(x, y).child()[0], p.y() + m_offset_image(x, y).child()[1]);
  }
};

// ---- Stereo/StereoModel.{h,cc} and Stereo/StereoView.h: triangulation and the universe radius -----------------------

namespace detail {
// the pixel forms DispHelper accepts (StereoView.h:37-53): channel type and layout of a disparity pixel type
template <class PixelT> struct disparity_form;
template <> struct disparity_form<PixelMask<Vector2f>> { enum { type = VWGPU_DISPARITY_F32, layout = VWGPU_DISPARITY_LAYOUT_DXDYV }; };
template <> struct disparity_form<PixelMask<Vector2i>> { enum { type = VWGPU_DISPARITY_I32, layout = VWGPU_DISPARITY_LAYOUT_DXDYV }; };
template <> struct disparity_form<Vector2f> { enum { type = VWGPU_DISPARITY_F32, layout = VWGPU_DISPARITY_LAYOUT_DXDY }; };
template <> struct disparity_form<Vector2i> { enum { type = VWGPU_DISPARITY_I32, layout = VWGPU_DISPARITY_LAYOUT_DXDY }; };
template <> struct disparity_form<PixelMask<float>> { enum { type = VWGPU_DISPARITY_F32, layout = VWGPU_DISPARITY_LAYOUT_DV }; };
template <> struct disparity_form<PixelMask<int32>> { enum { type = VWGPU_DISPARITY_I32, layout = VWGPU_DISPARITY_LAYOUT_DV }; };
template <> struct disparity_form<float> { enum { type = VWGPU_DISPARITY_F32, layout = VWGPU_DISPARITY_LAYOUT_D }; };
template <> struct disparity_form<int32> { enum { type = VWGPU_DISPARITY_I32, layout = VWGPU_DISPARITY_LAYOUT_D }; };
static_assert(sizeof(Vector3) == 24 && sizeof(PixelMask<float>) == 8 && sizeof(Vector2f) == 8, "pixel layouts of the triangulation entries");
}  // namespace detail

/// StereoModel(camera1, camera2, angle_tol) for two cameras (StereoModel.h).  The cameras are vw::camera models of
/// vw/Camera.h; like the reference, the model keeps pointers to them.
class StereoModel {
  camera::CameraModel const* m_cam1;
  camera::CameraModel const* m_cam2;
  double m_angle_tol;
public:
  StereoModel(camera::CameraModel const* camera_model1, camera::CameraModel const* camera_model2, double angle_tol = 0.0)
      : m_cam1(camera_model1), m_cam2(camera_model2), m_angle_tol(angle_tol) {}
  camera::CameraModel const* camera1() const { return m_cam1; }
  camera::CameraModel const* camera2() const { return m_cam2; }
  double angle_tol() const { return m_angle_tol; }

  /// One box of a disparity image on the engine: w x h pixels at `disp` whose pixel (0, 0) is image pixel (x0, y0).
  template <class PixelT>
  void triangulate(PixelT const* disp, int32 w, int32 h, ptrdiff_t dstride, int32 x0, int32 y0, int semantics, Vector3* xyz, double* error,
                   vwgpu_triangulate_stats* stats = NULL) const {
    vwgpu_ctx* ctx = detail::thread_context();
    detail::check(ctx, vwgpu_stereo_triangulate(ctx, detail::disparity_form<PixelT>::type, disp, w, h, dstride, x0, y0, &m_cam1->descriptor(),
                                                &m_cam2->descriptor(), m_angle_tol, semantics | detail::disparity_form<PixelT>::layout,
                                                reinterpret_cast<double*>(xyz), 0, error, 0, NULL, 0, stats));
  }

  /// operator()(disparity_map, error) (StereoModel.cc:254-309): the point image and the ray-intersection error; the right
  /// pixel is x + dx with x an int32 and dx a float.  The statistics the reference prints are returned through stats.
  template <class PixelT>
  ImageView<Vector3> operator()(ImageView<PixelT> const& disparity_map, ImageView<double>& error,
                                vwgpu_triangulate_stats* stats = NULL) const {
    ImageView<Vector3> xyz(disparity_map.cols(), disparity_map.rows());
    error.set_size(disparity_map.cols(), disparity_map.rows());
    if (disparity_map.cols() == 0 || disparity_map.rows() == 0) return xyz;
    triangulate(disparity_map.data(), disparity_map.cols(), disparity_map.rows(), 0, 0, 0, VWGPU_TRIANGULATE_MODEL, xyz.data(), error.data(),
                stats);
    return xyz;
  }

  /// convergence_angle (StereoModel.cc:174-177) for every pixel pair of a disparity image; 0 at invalid pixels.
  template <class PixelT>
  ImageView<double> convergence_angle(ImageView<PixelT> const& disparity_map, int semantics = VWGPU_TRIANGULATE_MODEL) const {
    ImageView<double> out(disparity_map.cols(), disparity_map.rows());
    if (disparity_map.cols() == 0 || disparity_map.rows() == 0) return out;
    vwgpu_ctx* ctx = detail::thread_context();
    detail::check(ctx, vwgpu_convergence_angle(ctx, detail::disparity_form<PixelT>::type, disparity_map.data(), disparity_map.cols(),
                                               disparity_map.rows(), 0, 0, 0, &m_cam1->descriptor(), &m_cam2->descriptor(),
                                               semantics | detail::disparity_form<PixelT>::layout, out.data(), 0));
    return out;
  }
};

/// StereoView (StereoView.h:56-123): a lazy ImageView<Vector3>-style view of a disparity image.  rasterize() hands each
/// box to the engine with the box's origin as x0, y0, so any tiling gives the pixels of the whole image.  error() of the
/// reference has no definition behind it (StereoModelHelper is declared nowhere); the error of this project is
/// StereoModel's scalar error, through error_image().
template <class DisparityImageT>
class StereoView : public ImageViewBase<StereoView<DisparityImageT>> {
  typedef typename DisparityImageT::pixel_type dpixel_type;
  ImageView<dpixel_type> m_disparity_map;
  StereoModel m_stereo_model;
public:
  typedef Vector3 pixel_type;
  typedef ImageView<Vector3> prerasterize_type;
  StereoView(DisparityImageT const& disparity_map, camera::CameraModel const* camera_model1, camera::CameraModel const* camera_model2)
      : m_disparity_map(disparity_map), m_stereo_model(camera_model1, camera_model2) {}
  StereoView(DisparityImageT const& disparity_map, StereoModel const& stereo_model)
      : m_disparity_map(disparity_map), m_stereo_model(stereo_model) {}
  int32 cols() const { return m_disparity_map.cols(); }
  int32 rows() const { return m_disparity_map.rows(); }
  int32 planes() const { return 1; }
  ImageView<dpixel_type> const& disparity_map() const { return m_disparity_map; }

  /// the box as an image of its own
  ImageView<Vector3> box(BBox2i const& bbox, ImageView<double>* error = NULL) const {
    ImageView<Vector3> out(bbox.width(), bbox.height());
    if (error) error->set_size(bbox.width(), bbox.height());
    if (bbox.empty()) return out;
    VW_ASSERT(bounding_box(m_disparity_map).contains(bbox), ArgumentErr() << "StereoView: the box leaves the disparity image.");
    m_stereo_model.triangulate(&m_disparity_map(bbox.min().x(), bbox.min().y()), bbox.width(), bbox.height(), m_disparity_map.cols(),
                               bbox.min().x(), bbox.min().y(), VWGPU_TRIANGULATE_VIEW, out.data(), error ? error->data() : NULL);
    return out;
  }
  Vector3 operator()(int32 i, int32 j) const { return box(BBox2i(i, j, 1, 1))(0, 0); }
  ImageView<double> error_image() const {
    ImageView<double> e;
    box(bounding_box(m_disparity_map), &e);
    return e;
  }
  prerasterize_type prerasterize(BBox2i const& bbox) const { return box(bbox); }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const {
    vw::rasterize(box(bbox), dest, BBox2i(0, 0, bbox.width(), bbox.height()));
  }
};

/// stereo_triangulate(disparity, camera1, camera2) (StereoView.h:125-130).
template <class ImageT>
StereoView<ImageT> stereo_triangulate(ImageViewBase<ImageT> const& v, camera::CameraModel const* camera1, camera::CameraModel const* camera2) {
  return StereoView<ImageT>(v.impl(), camera1, camera2);
}

/// UniverseRadiusFunc (StereoView.h:139-222) applied to a whole point image of Vector<double, 3 | 4 | 6> pixels: the
/// functor keeps the reference's shared counters, operator() filters an image on the engine.
class UniverseRadiusFunc {
  struct UniverseRadiusState { int64 rejected_points, total_points; };
  Vector3 m_origin;
  double m_near_radius, m_far_radius;
  std::shared_ptr<UniverseRadiusState> m_state;
public:
  UniverseRadiusFunc(Vector3 universe_origin, double near_radius = 0, double far_radius = std::numeric_limits<double>::max())
      : m_origin(universe_origin), m_near_radius(near_radius), m_far_radius(far_radius), m_state(new UniverseRadiusState()) {
    VW_ASSERT(m_near_radius >= 0 && m_far_radius >= 0, ArgumentErr() << "UniverseRadius: radii must be >= 0.");
    VW_ASSERT(m_near_radius <= m_far_radius, ArgumentErr() << "UniverseRadius: near radius must be <= far radius.");
    m_state->rejected_points = m_state->total_points = 0;
  }
  double near_radius() const { return m_near_radius; }
  double far_radius() const { return m_far_radius; }
  int64 rejected_points() const { return m_state->rejected_points; }
  int64 total_points() const { return m_state->total_points; }

  template <int N>
  ImageView<Vector<double, N>> operator()(ImageView<Vector<double, N>> const& points) const {
    static_assert(N == 3 || N == 4 || N == 6, "UniverseRadiusFunc: points, points with error, points with the error vector");
    ImageView<Vector<double, N>> out(points.cols(), points.rows());
    if (points.cols() == 0 || points.rows() == 0) return out;
    const double origin[3] = {m_origin[0], m_origin[1], m_origin[2]};
    long long counts[2] = {0, 0};
    vwgpu_ctx* ctx = detail::thread_context();
    detail::check(ctx, vwgpu_universe_radius(ctx, reinterpret_cast<const double*>(points.data()), N, points.cols(), points.rows(), 0, origin,
                                             m_near_radius, m_far_radius, reinterpret_cast<double*>(out.data()), 0, counts));
    m_state->total_points += counts[0];
    m_state->rejected_points += counts[1];
    return out;
  }
};

}  // namespace stereo

/// transform(image, DisparityTransform) (src/vw/Image/Transform.h: ZeroEdgeExtension, BilinearInterpolation) on a float
/// or PixelGray<float> image, rasterised over the image's own size.
template <class ViewT>
ImageView<typename ViewT::pixel_type> transform(ImageViewBase<ViewT> const& image, stereo::DisparityTransform const& tx) {
  static_assert(sizeof(typename ViewT::pixel_type) == sizeof(float), "transform(image, DisparityTransform): one float per pixel");
  ImageView<typename ViewT::pixel_type> r = image.impl(), out(r.cols(), r.rows());
  ImageView<PixelMask<Vector2f>> const& d = tx.offset_image();
  if (r.cols() == 0 || r.rows() == 0) return out;
  VW_ASSERT(d.cols() > 0 && d.rows() > 0, ArgumentErr() << "DisparityTransform: empty disparity image.");
  vwgpu_ctx* ctx = stereo::detail::thread_context();
  stereo::detail::check(ctx, vwgpu_disparity_warp(ctx, reinterpret_cast<const float*>(r.data()), r.cols(), r.rows(), 0,
                                                  reinterpret_cast<const float*>(d.data()), d.cols(), d.rows(), 0,
                                                  reinterpret_cast<float*>(out.data()), 0));
  return out;
}

}  // namespace vw
#endif
