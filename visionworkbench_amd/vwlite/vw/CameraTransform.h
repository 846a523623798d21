// vw/CameraTransform.h — resampling an image from one camera into another at the same centre
// (src/vw/Camera/CameraTransform.h:43-225): CameraTransform<Src, Dst>, camera_transform(image, src, dst[, size][, edge,
// interp]), linearize_camera_transform(image, src[, edge, interp]) and resize_epipolar_cameras_to_fit (src/vw/Camera/EpipolarUtils.cc:37-76) over compute_transformed_bbox_fast
// (src/vw/Image/Transform.h:272-315).  The view is lazy: rasterize(dest, bbox) is one vwgpu_camera_transform call with the
// box's origin as x0, y0, so any tiling gives the pixels of the whole image; points go through
// vwgpu_camera_transform_points.  Pixel types: float, PixelGray<float> and PixelMask<float>; bilinear interpolation only.
#ifndef VWLITE_CAMERATRANSFORM_H
#define VWLITE_CAMERATRANSFORM_H

#include <limits>
#include <vector>

#include "Camera.h"
#include "Engine.h"
#include "Image.h"

namespace vw {

struct BilinearInterpolation {};
/// ValueEdgeExtension<PixelT>(value) (src/vw/Image/EdgeExtension.h): pixels outside the image are `value`.
template <class PixelT>
struct ValueEdgeExtension {
  PixelT value;
  explicit ValueEdgeExtension(PixelT v) : value(v) {}
};

namespace camera {

namespace detail {
// how a pixel type splits into the float plane and the validity the engine takes
template <class PixelT> struct transform_pixel;
template <> struct transform_pixel<float> {
  enum { masked = 0 };
  static float value(float p) { return p; }
  static bool valid(float) { return true; }
  static float make(float v, bool) { return v; }
};
template <> struct transform_pixel<PixelGray<float>> {
  enum { masked = 0 };
  static float value(PixelGray<float> const& p) { return p.v(); }
  static bool valid(PixelGray<float> const&) { return true; }
  static PixelGray<float> make(float v, bool) { return PixelGray<float>(v); }
};
template <> struct transform_pixel<PixelMask<float>> {
  enum { masked = 1 };
  static float value(PixelMask<float> const& p) { return p.child(); }
  static bool valid(PixelMask<float> const& p) { return p.valid() != 0; }
  static PixelMask<float> make(float v, bool ok) { PixelMask<float> p(v); if (!ok) p.invalidate(); return p; }
};
}  // namespace detail

/// CameraTransform<SrcCameraT, DstCameraT>(src, dst) (CameraTransform.h:43-79).  Single points and arrays of points are
/// transformed on the engine; a point whose projection fails the pinhole's check throws LogicErr, as the reference
/// throws PointToPixelErr, and so do cameras whose centres differ.
template <class SrcCameraT, class DstCameraT>
class CameraTransform {
  SrcCameraT m_src_camera;
  DstCameraT m_dst_camera;
  void run(int direction, Vector2 const* in, size_t n, Vector2* out) const {
    if (n == 0) return;
    CameraModel const& to = direction == VWGPU_CAMERA_TRANSFORM_FORWARD ? static_cast<CameraModel const&>(m_dst_camera)
                                                                        : static_cast<CameraModel const&>(m_src_camera);
    vwgpu_ctx* ctx = engine::thread_context();
    engine::check(ctx, vwgpu_camera_transform_points(ctx, &m_src_camera.descriptor(), m_src_camera.camera_matrix(), &m_dst_camera.descriptor(),
                                                     m_dst_camera.camera_matrix(), direction, to.do_point_to_pixel_check() ? 1 : 0,
                                                     reinterpret_cast<const double*>(in), (long long)n, reinterpret_cast<double*>(out), NULL));
  }
public:
  CameraTransform(SrcCameraT const& src_camera, DstCameraT const& dst_camera) : m_src_camera(src_camera), m_dst_camera(dst_camera) {}
  SrcCameraT const& src_camera() const { return m_src_camera; }
  DstCameraT const& dst_camera() const { return m_dst_camera; }
  Vector2 reverse(Vector2 const& p) const { Vector2 q; run(VWGPU_CAMERA_TRANSFORM_REVERSE, &p, 1, &q); return q; }
  Vector2 forward(Vector2 const& p) const { Vector2 q; run(VWGPU_CAMERA_TRANSFORM_FORWARD, &p, 1, &q); return q; }
  std::vector<Vector2> reverse(std::vector<Vector2> const& p) const {
    std::vector<Vector2> q(p.size());
    run(VWGPU_CAMERA_TRANSFORM_REVERSE, p.data(), p.size(), q.data());
    return q;
  }
  std::vector<Vector2> forward(std::vector<Vector2> const& p) const {
    std::vector<Vector2> q(p.size());
    run(VWGPU_CAMERA_TRANSFORM_FORWARD, p.data(), p.size(), q.data());
    return q;
  }
};

/// The view camera_transform returns: TransformView<InterpolationView<EdgeExtensionView<ImageT, EdgeT>, Bilinear>, CameraTransform>.
template <class ImageT, class SrcCameraT, class DstCameraT>
class CameraTransformView : public ImageViewBase<CameraTransformView<ImageT, SrcCameraT, DstCameraT>> {
public:
  typedef typename ImageT::pixel_type pixel_type;
  typedef ImageView<pixel_type> prerasterize_type;
private:
  typedef detail::transform_pixel<pixel_type> px;
  SrcCameraT m_src_camera;
  DstCameraT m_dst_camera;
  int32 m_cols, m_rows, m_src_cols, m_src_rows;
  std::vector<float> m_plane;
  std::vector<uint8> m_mask;
  float m_edge_value;
  bool m_edge_valid;
public:
  CameraTransformView(ImageT const& image, SrcCameraT const& src, DstCameraT const& dst, Vector2i size, pixel_type const& edge)
      : m_src_camera(src), m_dst_camera(dst), m_cols(size[0]), m_rows(size[1]), m_src_cols(image.cols()), m_src_rows(image.rows()),
        m_plane((size_t)image.cols() * image.rows()), m_mask(px::masked ? m_plane.size() : 0), m_edge_value(px::value(edge)),
        m_edge_valid(px::masked && px::valid(edge)) {
    ImageView<pixel_type> src_image = image.prerasterize(bounding_box(image));
    for (int32 r = 0; r < m_src_rows; ++r)
      for (int32 c = 0; c < m_src_cols; ++c) {
        const size_t i = (size_t)r * m_src_cols + c;
        m_plane[i] = px::value(src_image(c, r));
        if (px::masked) m_mask[i] = px::valid(src_image(c, r)) ? 255 : 0;
      }
  }
  int32 cols() const { return m_cols; }
  int32 rows() const { return m_rows; }
  int32 planes() const { return 1; }
  SrcCameraT const& src_camera() const { return m_src_camera; }
  DstCameraT const& dst_camera() const { return m_dst_camera; }

  /// the box as an image of its own; it may leave [0, cols) x [0, rows), like any TransformView
  ImageView<pixel_type> box(BBox2i const& bbox) const {
    ImageView<pixel_type> out(bbox.width(), bbox.height());
    if (bbox.empty()) return out;
    const size_t n = (size_t)bbox.width() * bbox.height();
    std::vector<float> plane(n);
    std::vector<uint8> mask(px::masked ? n : 0);
    vwgpu_ctx* ctx = engine::thread_context();
    engine::check(ctx, vwgpu_camera_transform(ctx, m_plane.data(), m_src_cols, m_src_rows, 0, px::masked ? m_mask.data() : NULL, 0,
                                              &m_src_camera.descriptor(), m_src_camera.camera_matrix(), &m_dst_camera.descriptor(),
                                              m_dst_camera.camera_matrix(), bbox.width(), bbox.height(), bbox.min().x(), bbox.min().y(),
                                              m_edge_value, m_edge_valid ? 1 : 0, m_src_camera.do_point_to_pixel_check() ? 1 : 0, plane.data(), 0,
                                              px::masked ? mask.data() : NULL, 0, NULL));
    for (size_t i = 0; i < n; ++i) out.data()[i] = px::make(plane[i], px::masked ? mask[i] != 0 : true);
    return out;
  }
  pixel_type operator()(int32 i, int32 j) const { return box(BBox2i(i, j, 1, 1))(0, 0); }
  prerasterize_type prerasterize(BBox2i const& bbox) const { return box(bbox); }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const {
    vw::rasterize(box(bbox), dest, BBox2i(0, 0, bbox.width(), bbox.height()));
  }
};

/// camera_transform(image, src, dst, size, edge, interp) (CameraTransform.h:125-131)
template <class ImageT, class SrcCameraT, class DstCameraT>
CameraTransformView<ImageT, SrcCameraT, DstCameraT> camera_transform(ImageViewBase<ImageT> const& image, SrcCameraT const& src_camera,
                                                                     DstCameraT const& dst_camera, Vector2i size,
                                                                     ValueEdgeExtension<typename ImageT::pixel_type> const& edge_func,
                                                                     BilinearInterpolation const& = BilinearInterpolation()) {
  return CameraTransformView<ImageT, SrcCameraT, DstCameraT>(image.impl(), src_camera, dst_camera, size, edge_func.value);
}
/// ... with the image's own size (:135-141)
template <class ImageT, class SrcCameraT, class DstCameraT>
CameraTransformView<ImageT, SrcCameraT, DstCameraT> camera_transform(ImageViewBase<ImageT> const& image, SrcCameraT const& src_camera,
                                                                     DstCameraT const& dst_camera,
                                                                     ValueEdgeExtension<typename ImageT::pixel_type> const& edge_func,
                                                                     BilinearInterpolation const& = BilinearInterpolation()) {
  return camera_transform(image, src_camera, dst_camera, Vector2i(image.impl().cols(), image.impl().rows()), edge_func);
}
/// ... with ZeroEdgeExtension and bilinear interpolation, with and without a size (:155-172)
template <class ImageT, class SrcCameraT, class DstCameraT>
CameraTransformView<ImageT, SrcCameraT, DstCameraT> camera_transform(ImageViewBase<ImageT> const& image, SrcCameraT const& src_camera,
                                                                     DstCameraT const& dst_camera, Vector2i size) {
  typedef typename ImageT::pixel_type pixel_type;
  return CameraTransformView<ImageT, SrcCameraT, DstCameraT>(image.impl(), src_camera, dst_camera, size, pixel_type());
}
template <class ImageT, class SrcCameraT, class DstCameraT>
CameraTransformView<ImageT, SrcCameraT, DstCameraT> camera_transform(ImageViewBase<ImageT> const& image, SrcCameraT const& src_camera,
                                                                     DstCameraT const& dst_camera) {
  return camera_transform(image, src_camera, dst_camera, Vector2i(image.impl().cols(), image.impl().rows()));
}

/// linearize_camera_transform(image, src_camera[, edge][, interp]) (CameraTransform.h:185-225): the image of a CAHVORModel or
/// CAHVOREModel as its own linearisation at the image's size sees it; view.dst_camera() is the CAHVModel that goes with it.
template <class ImageT, class SrcCameraT>
CameraTransformView<ImageT, SrcCameraT, typename SrcCameraT::linearized_type>
linearize_camera_transform(ImageViewBase<ImageT> const& image, SrcCameraT const& src_camera,
                           ValueEdgeExtension<typename ImageT::pixel_type> const& edge_func, BilinearInterpolation const& = BilinearInterpolation()) {
  const Vector2i size(image.impl().cols(), image.impl().rows());
  return camera_transform(image, src_camera, linearize_camera(src_camera, size, size), size, edge_func);
}
template <class ImageT, class SrcCameraT>
CameraTransformView<ImageT, SrcCameraT, typename SrcCameraT::linearized_type> linearize_camera_transform(ImageViewBase<ImageT> const& image,
                                                                                                         SrcCameraT const& src_camera) {
  const Vector2i size(image.impl().cols(), image.impl().rows());
  return camera_transform(image, src_camera, linearize_camera(src_camera, size, size), size);
}

/// compute_transformed_bbox_fast(roi, transform) (Image/Transform.h:272-315): min and max of the BBox2f grown by the
/// forward-transformed perimeter of roi (a coordinate is compared in double and stored rounded to float, BBox.tcc:82-97).
template <class TransformT>
void compute_transformed_bbox_fast(BBox2i const& image_roi, TransformT const& transform_func, Vector2f& box_min, Vector2f& box_max) {
  std::vector<Vector2> pts;
  for (int32 x = image_roi.min()[0]; x < image_roi.max()[0]; ++x) pts.push_back(Vector2(x, image_roi.min()[1]));
  for (int32 x = image_roi.min()[0]; x < image_roi.max()[0]; ++x) pts.push_back(Vector2(x, image_roi.max()[1] - 1));
  for (int32 y = image_roi.min()[1]; y < image_roi.max()[1]; ++y) pts.push_back(Vector2(image_roi.min()[0], y));
  for (int32 y = image_roi.min()[1]; y < image_roi.max()[1]; ++y) pts.push_back(Vector2(image_roi.max()[0] - 1, y));
  const std::vector<Vector2> out = transform_func.forward(pts);
  const float big = std::numeric_limits<float>::max();
  box_min = Vector2f(big, big);
  box_max = Vector2f(-big, -big);
  for (size_t k = 0; k < out.size(); ++k)
    for (int i = 0; i < 2; ++i) {
      if (out[k][i] > box_max[i]) box_max[i] = float(out[k][i]);
      if (out[k][i] < box_min[i]) box_min[i] = float(out[k][i]);
    }
}

/// resize_epipolar_cameras_to_fit (EpipolarUtils.cc:37-76), with the reference's signature.
inline void resize_epipolar_cameras_to_fit(PinholeModel const& cam1, PinholeModel const& cam2, PinholeModel& epi_cam1, PinholeModel& epi_cam2,
                                           BBox2i const& roi1, BBox2i const& roi2, Vector2i& epi_size1, Vector2i& epi_size2) {
  Vector2f min1, max1, min2, max2;
  compute_transformed_bbox_fast(roi1, CameraTransform<PinholeModel, PinholeModel>(cam1, epi_cam1), min1, max1);
  compute_transformed_bbox_fast(roi2, CameraTransform<PinholeModel, PinholeModel>(cam2, epi_cam2), min2, max2);
  const double min_col = std::min((double)min1[0], (double)min2[0]), min_row = std::min((double)min1[1], (double)min2[1]);
  const Vector2 point_offset = epi_cam1.point_offset();
  const Vector2 center_adjust = Vector2(min_col, min_row) * epi_cam1.pixel_pitch();
  epi_cam1.set_point_offset(point_offset - center_adjust);
  epi_cam2.set_point_offset(point_offset - center_adjust);
  compute_transformed_bbox_fast(roi1, CameraTransform<PinholeModel, PinholeModel>(cam1, epi_cam1), min1, max1);
  compute_transformed_bbox_fast(roi2, CameraTransform<PinholeModel, PinholeModel>(cam2, epi_cam2), min2, max2);
  epi_size1 = Vector2i(max1);   // Vector2i from a float vector: truncation
  epi_size2 = Vector2i(max2);
}

}  // namespace camera
}  // namespace vw
#endif
