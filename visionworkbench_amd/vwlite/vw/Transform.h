// vw/Transform.h — vw::transform on libvwgpu.so: the closed-form map functors of src/vw/Math/Transform.h:231-500
// (IdentityTransform, TranslateTransform, ResampleTransform, LinearTransform, AffineTransform, RotateTransform,
// InverseTransform, CompositionTransform, compose), TransformView (src/vw/Image/Transform.h:335-387), and the free functions
// transform, transform_nodata, resample, resize, translate and rotate (:485-843) with the reference's defaults, over
// BilinearInterpolation, BicubicInterpolation and NearestPixelInterpolation (src/vw/Image/Interpolation.h) and the edge
// extensions of src/vw/Image/EdgeExtension.h.  HomographyTransform is the one of vw/Math.h.  The view is lazy:
// rasterize(dest, bbox) is one vwgpu_transform_image call with the box's origin as x0, y0, so any tiling gives the pixels
// of the whole image; single points go through vwgpu_transform_points.  Pixel types: float, PixelGray<float> and
// PixelMask<float>.  A chain holds at most four maps, and LinearEdgeExtension of a masked image is NoImplErr.
#ifndef VWLITE_TRANSFORM_H
#define VWLITE_TRANSFORM_H

#include <cmath>
#include <vector>

#include "CameraTransform.h"
#include "Engine.h"
#include "Filter.h"
#include "Image.h"
#include "Math.h"

namespace vw {

// the tags that Image.h (Zero, Constant) and CameraTransform.h (Value, Bilinear) do not have yet
struct BicubicInterpolation {};
struct NearestPixelInterpolation {};
struct PeriodicEdgeExtension {};
struct CylindricalEdgeExtension {};
struct ReflectEdgeExtension {};
struct LinearEdgeExtension {};

namespace detail {
inline int interp_code(NearestPixelInterpolation) { return VWGPU_TRANSFORM_INTERP_NEAREST; }
inline int interp_code(BilinearInterpolation) { return VWGPU_TRANSFORM_INTERP_BILINEAR; }
inline int interp_code(BicubicInterpolation) { return VWGPU_TRANSFORM_INTERP_BICUBIC; }

// an edge tag as the words of vwgpu_transform_params
template <class PixelT> struct transform_edge {
  int code;
  float value;
  bool valid;
  transform_edge(ZeroEdgeExtension) : code(VWGPU_TRANSFORM_EDGE_ZERO), value(0), valid(false) {}
  transform_edge(ConstantEdgeExtension) : code(VWGPU_TRANSFORM_EDGE_CONSTANT), value(0), valid(false) {}
  transform_edge(PeriodicEdgeExtension) : code(VWGPU_TRANSFORM_EDGE_PERIODIC), value(0), valid(false) {}
  transform_edge(CylindricalEdgeExtension) : code(VWGPU_TRANSFORM_EDGE_CYLINDRICAL), value(0), valid(false) {}
  transform_edge(ReflectEdgeExtension) : code(VWGPU_TRANSFORM_EDGE_REFLECT), value(0), valid(false) {}
  transform_edge(LinearEdgeExtension) : code(VWGPU_TRANSFORM_EDGE_LINEAR), value(0), valid(false) {}
  transform_edge(ValueEdgeExtension<PixelT> const& e)
      : code(VWGPU_TRANSFORM_EDGE_VALUE), value(camera::detail::transform_pixel<PixelT>::value(e.value)),
        valid(camera::detail::transform_pixel<PixelT>::masked && camera::detail::transform_pixel<PixelT>::valid(e.value)) {}
};

// the chain of descriptors of a functor, in the order reverse() applies them
typedef std::vector<vwgpu_transform> transform_chain;
inline transform_chain chain_of(HomographyTransform const& h) {
  vwgpu_transform t = vwgpu_transform();
  t.kind = VWGPU_TRANSFORM_HOMOGRAPHY;
  for (int i = 0; i < 9; ++i) {
    t.fwd[i] = h.matrix().data()[i];
    t.rev[i] = h.inverse_matrix().data()[i];
  }
  return transform_chain(1, t);
}
template <class TxT> transform_chain chain_of(TxT const& tx) { return tx.descriptors(); }

inline Vector2 transform_point(transform_chain const& chain, int direction, Vector2 const& p) {
  VW_ASSERT(chain.size() >= 1 && chain.size() <= 4, ArgumentErr() << "transform: a chain has 1 to 4 maps");
  Vector2 q;
  const int rc = vwgpu_transform_points(chain.data(), (int)chain.size(), direction, reinterpret_cast<const double*>(&p), 1,
                                        reinterpret_cast<double*>(&q));
  VW_ASSERT(rc == VWGPU_OK, ArgumentErr() << "transform: the engine refused the chain");
  return q;
}

// what the functors share: one descriptor, forward and reverse through the engine's host entry
class TransformFunctor {
protected:
  vwgpu_transform m_desc;
  TransformFunctor() : m_desc() {}
  void make(int kind, const double* params, int n) {
    VW_ASSERT(vwgpu_transform_make(kind, params, n, &m_desc) == VWGPU_OK,
              ArgumentErr() << "transform: a singular matrix, a parameter that is not finite or a resample factor of 0");
  }
public:
  transform_chain descriptors() const { return transform_chain(1, m_desc); }
  Vector2 forward(Vector2 const& p) const { return transform_point(descriptors(), VWGPU_TRANSFORM_FORWARD, p); }
  Vector2 reverse(Vector2 const& p) const { return transform_point(descriptors(), VWGPU_TRANSFORM_REVERSE, p); }
};
}  // namespace detail

/// A 2 x 2 double matrix, row-major: as much of vw::Matrix2x2 as the functors need.
class Matrix2x2 {
  double m[4];
public:
  Matrix2x2() { m[0] = m[1] = m[2] = m[3] = 0.0; }
  Matrix2x2(double a, double b, double c, double d) { m[0] = a; m[1] = b; m[2] = c; m[3] = d; }
  double& operator()(int r, int c) { return m[r * 2 + c]; }
  double const& operator()(int r, int c) const { return m[r * 2 + c]; }
};

/// IdentityTransform (Math/Transform.h:231-237)
class IdentityTransform : public detail::TransformFunctor {
public:
  IdentityTransform() { make(VWGPU_TRANSFORM_IDENTITY, NULL, 0); }
};
/// TranslateTransform(x, y) (:267-288)
class TranslateTransform : public detail::TransformFunctor {
public:
  TranslateTransform(double x_translation, double y_translation) {
    const double p[2] = {x_translation, y_translation};
    make(VWGPU_TRANSFORM_TRANSLATE, p, 2);
  }
  explicit TranslateTransform(Vector2 const& v) {
    const double p[2] = {v[0], v[1]};
    make(VWGPU_TRANSFORM_TRANSLATE, p, 2);
  }
};
/// ResampleTransform(x_scaling, y_scaling) (:242-263)
class ResampleTransform : public detail::TransformFunctor {
public:
  ResampleTransform(double x_scaling, double y_scaling) {
    const double p[2] = {x_scaling, y_scaling};
    make(VWGPU_TRANSFORM_RESAMPLE, p, 2);
  }
  explicit ResampleTransform(Vector2 const& v) {
    const double p[2] = {v[0], v[1]};
    make(VWGPU_TRANSFORM_RESAMPLE, p, 2);
  }
};
/// AffineTransform(matrix, offset) (:310-341)
class AffineTransform : public detail::TransformFunctor {
protected:
  AffineTransform() {}
public:
  AffineTransform(Matrix2x2 const& matrix, Vector2 const& offset) {
    const double p[6] = {matrix(0, 0), matrix(0, 1), matrix(1, 0), matrix(1, 1), offset[0], offset[1]};
    make(VWGPU_TRANSFORM_AFFINE, p, 6);
  }
};
/// LinearTransform(matrix) (:292-307): the affine map with the offset 0
class LinearTransform : public AffineTransform {
public:
  explicit LinearTransform(Matrix2x2 const& matrix) : AffineTransform(matrix, Vector2()) {}
};
/// RotateTransform(theta, translate) (:349-363)
class RotateTransform : public AffineTransform {
public:
  RotateTransform(double theta, Vector2 const& translate) {
    VW_ASSERT(vwgpu_transform_rotate(theta, translate[0], translate[1], &m_desc) == VWGPU_OK,
              ArgumentErr() << "RotateTransform: a parameter is not finite");
  }
};

/// InverseTransform<TxT>(tx) (:394-411): forward and reverse change places
template <class TxT>
class InverseTransform {
  detail::transform_chain m_chain;
public:
  explicit InverseTransform(TxT const& tx) {
    const detail::transform_chain c = detail::chain_of(tx);
    for (size_t k = c.size(); k-- > 0;) {
      vwgpu_transform inv;
      VW_ASSERT(vwgpu_transform_invert(&c[k], &inv) == VWGPU_OK, ArgumentErr() << "InverseTransform: the engine refused a descriptor");
      m_chain.push_back(inv);
    }
  }
  detail::transform_chain descriptors() const { return m_chain; }
  Vector2 forward(Vector2 const& p) const { return detail::transform_point(m_chain, VWGPU_TRANSFORM_FORWARD, p); }
  Vector2 reverse(Vector2 const& p) const { return detail::transform_point(m_chain, VWGPU_TRANSFORM_REVERSE, p); }
};

/// CompositionTransform<Tx1T, Tx2T>(tx1, tx2) (:429-453): forward is tx1.forward(tx2.forward(p)), reverse tx2.reverse(tx1.reverse(p))
template <class Tx1T, class Tx2T>
class CompositionTransform {
  detail::transform_chain m_chain;
public:
  CompositionTransform(Tx1T const& tx1, Tx2T const& tx2) : m_chain(detail::chain_of(tx1)) {
    const detail::transform_chain c = detail::chain_of(tx2);
    m_chain.insert(m_chain.end(), c.begin(), c.end());
  }
  detail::transform_chain descriptors() const { return m_chain; }
  Vector2 forward(Vector2 const& p) const { return detail::transform_point(m_chain, VWGPU_TRANSFORM_FORWARD, p); }
  Vector2 reverse(Vector2 const& p) const { return detail::transform_point(m_chain, VWGPU_TRANSFORM_REVERSE, p); }
};
/// compose(tx1, tx2[, tx3[, tx4]]) (:455-483)
template <class Tx1T, class Tx2T>
CompositionTransform<Tx1T, Tx2T> compose(Tx1T const& tx1, Tx2T const& tx2) { return CompositionTransform<Tx1T, Tx2T>(tx1, tx2); }
template <class Tx1T, class Tx2T, class Tx3T>
CompositionTransform<Tx1T, CompositionTransform<Tx2T, Tx3T>> compose(Tx1T const& tx1, Tx2T const& tx2, Tx3T const& tx3) {
  return CompositionTransform<Tx1T, CompositionTransform<Tx2T, Tx3T>>(tx1, compose(tx2, tx3));
}
template <class Tx1T, class Tx2T, class Tx3T, class Tx4T>
CompositionTransform<Tx1T, CompositionTransform<Tx2T, CompositionTransform<Tx3T, Tx4T>>> compose(Tx1T const& tx1, Tx2T const& tx2, Tx3T const& tx3,
                                                                                                 Tx4T const& tx4) {
  return CompositionTransform<Tx1T, CompositionTransform<Tx2T, CompositionTransform<Tx3T, Tx4T>>>(tx1, compose(tx2, tx3, tx4));
}

/// TransformView<ImageT, TransformT> (Image/Transform.h:335-387) over interpolate(image, interp, edge), and with a nodata
/// pixel TransformViewNoData (:401-437).
template <class ImageT, class TransformT>
class TransformView : public ImageViewBase<TransformView<ImageT, TransformT>> {
public:
  typedef typename ImageT::pixel_type pixel_type;
  typedef ImageView<pixel_type> prerasterize_type;
private:
  typedef camera::detail::transform_pixel<pixel_type> px;
  TransformT m_mapper;
  detail::transform_chain m_chain;
  int32 m_cols, m_rows, m_x0, m_y0, m_src_cols, m_src_rows;
  std::vector<float> m_plane;
  std::vector<uint8> m_mask;
  vwgpu_transform_params m_params;
public:
  template <class EdgeT, class InterpT>
  TransformView(ImageT const& image, TransformT const& mapper, int32 width, int32 height, EdgeT const& edge, InterpT const& interp)
      : m_mapper(mapper), m_chain(detail::chain_of(mapper)), m_cols(width), m_rows(height), m_x0(0), m_y0(0), m_src_cols(image.cols()), m_src_rows(image.rows()),
        m_plane((size_t)image.cols() * image.rows()), m_mask(px::masked ? m_plane.size() : 0), m_params() {
    const detail::transform_edge<pixel_type> e(edge);
    m_params.interp = detail::interp_code(interp);
    m_params.edge = e.code;
    m_params.edge_value = e.value;
    m_params.edge_valid = e.valid ? 1 : 0;
    ImageView<pixel_type> src_image = image.prerasterize(bounding_box(image));
    for (int32 r = 0; r < m_src_rows; ++r)
      for (int32 c = 0; c < m_src_cols; ++c) {
        const size_t i = (size_t)r * m_src_cols + c;
        m_plane[i] = px::value(src_image(c, r));
        if (px::masked) m_mask[i] = px::valid(src_image(c, r)) ? 255 : 0;
      }
  }
  /// transform_nodata: the pixel where reverse(p) comes closer to the border than the interpolation's pixel_buffer allows
  void set_nodata(pixel_type const& nodata_val) {
    m_params.nodata = 1;
    m_params.nodata_value = px::value(nodata_val);
    m_params.nodata_valid = px::masked && px::valid(nodata_val) ? 1 : 0;
  }
  /// crop(view, bbox) (the box is in the transformed space and may leave the view): still one engine call per rasterised box,
  /// where a CropView would ask for the pixels one by one
  TransformView cropped(BBox2i const& bbox) const {
    TransformView v(*this);
    v.m_x0 += bbox.min().x();
    v.m_y0 += bbox.min().y();
    v.m_cols = bbox.width();
    v.m_rows = bbox.height();
    return v;
  }
  int32 cols() const { return m_cols; }
  int32 rows() const { return m_rows; }
  int32 planes() const { return 1; }
  TransformT const& transform() const { return m_mapper; }

  /// the box (in the view's own coordinates) as an image of its own; it may leave [0, cols) x [0, rows), like the reference's view
  ImageView<pixel_type> box(BBox2i const& bbox) const {
    ImageView<pixel_type> out(bbox.width(), bbox.height());
    if (bbox.empty()) return out;
    VW_ASSERT(m_chain.size() >= 1 && m_chain.size() <= 4, ArgumentErr() << "transform: a chain has 1 to 4 maps");
    const size_t n = (size_t)bbox.width() * bbox.height();
    std::vector<float> plane(n);
    std::vector<uint8> mask(px::masked ? n : 0);
    vwgpu_ctx* ctx = engine::thread_context();
    engine::check(ctx, vwgpu_transform_image(ctx, m_plane.data(), m_src_cols, m_src_rows, 0, px::masked ? m_mask.data() : NULL, 0, m_chain.data(),
                                             (int)m_chain.size(), &m_params, bbox.width(), bbox.height(), m_x0 + bbox.min().x(), m_y0 + bbox.min().y(),
                                             plane.data(), 0, px::masked ? mask.data() : NULL, 0));
    for (size_t i = 0; i < n; ++i) out.data()[i] = px::make(plane[i], px::masked ? mask[i] != 0 : true);
    return out;
  }
  pixel_type operator()(int32 i, int32 j) const { return box(BBox2i(i, j, 1, 1))(0, 0); }
  prerasterize_type prerasterize(BBox2i const& bbox) const { return box(bbox); }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const {
    vw::rasterize(box(bbox), dest, BBox2i(0, 0, bbox.width(), bbox.height()));
  }
};

// ---- transform (Image/Transform.h:485-601): Zero, bilinear by default ----------------------------------------------------
template <class ImageT, class TransformT, class EdgeT, class InterpT>
TransformView<ImageT, TransformT> transform(ImageViewBase<ImageT> const& v, TransformT const& tx, int32 width, int32 height, EdgeT const& edge,
                                            InterpT const& interp) {
  return TransformView<ImageT, TransformT>(v.impl(), tx, width, height, edge, interp);
}
template <class ImageT, class TransformT, class EdgeT>
TransformView<ImageT, TransformT> transform(ImageViewBase<ImageT> const& v, TransformT const& tx, int32 width, int32 height, EdgeT const& edge) {
  return transform(v, tx, width, height, edge, BilinearInterpolation());
}
template <class ImageT, class TransformT>
TransformView<ImageT, TransformT> transform(ImageViewBase<ImageT> const& v, TransformT const& tx, int32 width, int32 height) {
  return transform(v, tx, width, height, ZeroEdgeExtension(), BilinearInterpolation());
}
/// ... with the image's own size (:485-514)
template <class ImageT, class TransformT, class EdgeT, class InterpT>
TransformView<ImageT, TransformT> transform(ImageViewBase<ImageT> const& v, TransformT const& tx, EdgeT const& edge, InterpT const& interp) {
  return transform(v, tx, v.impl().cols(), v.impl().rows(), edge, interp);
}
template <class ImageT, class TransformT, class EdgeT>
TransformView<ImageT, TransformT> transform(ImageViewBase<ImageT> const& v, TransformT const& tx, EdgeT const& edge) {
  return transform(v, tx, v.impl().cols(), v.impl().rows(), edge, BilinearInterpolation());
}
template <class ImageT, class TransformT>
TransformView<ImageT, TransformT> transform(ImageViewBase<ImageT> const& v, TransformT const& tx) {
  return transform(v, tx, v.impl().cols(), v.impl().rows(), ZeroEdgeExtension(), BilinearInterpolation());
}
/// ... cropped to a box of the transformed space (:565-601; the reference's CropView<TransformView>)
template <class ImageT, class TransformT, class EdgeT, class InterpT>
TransformView<ImageT, TransformT> transform(ImageViewBase<ImageT> const& v, TransformT const& tx, BBox2i const& bbox, EdgeT const& edge,
                                                      InterpT const& interp) {
  return transform(v, tx, edge, interp).cropped(bbox);
}
template <class ImageT, class TransformT, class EdgeT>
TransformView<ImageT, TransformT> transform(ImageViewBase<ImageT> const& v, TransformT const& tx, BBox2i const& bbox, EdgeT const& edge) {
  return transform(v, tx, edge, BilinearInterpolation()).cropped(bbox);
}
template <class ImageT, class TransformT>
TransformView<ImageT, TransformT> transform(ImageViewBase<ImageT> const& v, TransformT const& tx, BBox2i const& bbox) {
  return transform(v, tx, ZeroEdgeExtension(), BilinearInterpolation()).cropped(bbox);
}
/// transform_nodata(v, tx, width, height, edge, interp, nodata_val) (:606-618)
template <class ImageT, class TransformT, class EdgeT, class InterpT>
TransformView<ImageT, TransformT> transform_nodata(ImageViewBase<ImageT> const& v, TransformT const& tx, int32 width, int32 height,
                                                   EdgeT const& edge, InterpT const& interp, typename ImageT::pixel_type nodata_val) {
  TransformView<ImageT, TransformT> view(v.impl(), tx, width, height, edge, interp);
  view.set_nodata(nodata_val);
  return view;
}

// ---- resample (:624-709): Constant, bilinear by default; size int(.5 + cols * f) --------------------------------------
template <class ImageT, class EdgeT, class InterpT>
TransformView<ImageT, ResampleTransform> resample(ImageViewBase<ImageT> const& v, double x_scale_factor, double y_scale_factor, EdgeT const& edge,
                                                  InterpT const& interp) {
  return transform(v, ResampleTransform(x_scale_factor, y_scale_factor), int(.5 + (v.impl().cols() * x_scale_factor)),
                   int(.5 + (v.impl().rows() * y_scale_factor)), edge, interp);
}
template <class ImageT, class EdgeT>
TransformView<ImageT, ResampleTransform> resample(ImageViewBase<ImageT> const& v, double x_scale_factor, double y_scale_factor, EdgeT const& edge) {
  return resample(v, x_scale_factor, y_scale_factor, edge, BilinearInterpolation());
}
template <class ImageT>
TransformView<ImageT, ResampleTransform> resample(ImageViewBase<ImageT> const& v, double x_scale_factor, double y_scale_factor) {
  return resample(v, x_scale_factor, y_scale_factor, ConstantEdgeExtension(), BilinearInterpolation());
}
template <class ImageT, class EdgeT, class InterpT>
TransformView<ImageT, ResampleTransform> resample(ImageViewBase<ImageT> const& v, double scale_factor, int32 output_width, int32 output_height,
                                                  EdgeT const& edge, InterpT const& interp) {
  return transform(v, ResampleTransform(scale_factor, scale_factor), output_width, output_height, edge, interp);
}
template <class ImageT>
TransformView<ImageT, ResampleTransform> resample(ImageViewBase<ImageT> const& v, double scale_factor) {
  return resample(v, scale_factor, scale_factor, ConstantEdgeExtension(), BilinearInterpolation());
}

// ---- resize (:716-747): the factors are out / (double) cols ----------------------------------------------------------------
template <class ImageT, class EdgeT, class InterpT>
TransformView<ImageT, ResampleTransform> resize(ImageViewBase<ImageT> const& v, int32 output_width, int32 output_height, EdgeT const& edge,
                                                InterpT const& interp) {
  return transform(v, ResampleTransform(output_width / (double)v.impl().cols(), output_height / (double)v.impl().rows()), output_width,
                   output_height, edge, interp);
}
template <class ImageT, class EdgeT>
TransformView<ImageT, ResampleTransform> resize(ImageViewBase<ImageT> const& v, int32 output_width, int32 output_height, EdgeT const& edge) {
  return resize(v, output_width, output_height, edge, BilinearInterpolation());
}
template <class ImageT>
TransformView<ImageT, ResampleTransform> resize(ImageViewBase<ImageT> const& v, int32 output_width, int32 output_height) {
  return resize(v, output_width, output_height, ConstantEdgeExtension(), BilinearInterpolation());
}

// ---- translate (:754-809): Zero, bilinear by default.  The reference's overload for int32 offsets is an EdgeExtensionView
// shifted by (-x, -y): the same pixels, since every interpolation returns the pixel itself at an integer position. ----------
template <class ImageT, class EdgeT, class InterpT>
TransformView<ImageT, TranslateTransform> translate(ImageViewBase<ImageT> const& v, double x_offset, double y_offset, EdgeT const& edge,
                                                    InterpT const& interp) {
  return transform(v, TranslateTransform(x_offset, y_offset), v.impl().cols(), v.impl().rows(), edge, interp);
}
template <class ImageT, class EdgeT>
TransformView<ImageT, TranslateTransform> translate(ImageViewBase<ImageT> const& v, double x_offset, double y_offset, EdgeT const& edge) {
  return translate(v, x_offset, y_offset, edge, BilinearInterpolation());
}
template <class ImageT>
TransformView<ImageT, TranslateTransform> translate(ImageViewBase<ImageT> const& v, double x_offset, double y_offset) {
  return translate(v, x_offset, y_offset, ZeroEdgeExtension(), BilinearInterpolation());
}
template <class ImageT, class EdgeT>
TransformView<ImageT, TranslateTransform> translate(ImageViewBase<ImageT> const& im, int32 x_offset, int32 y_offset, EdgeT const& edge) {
  return translate(im, (double)x_offset, (double)y_offset, edge, NearestPixelInterpolation());
}
template <class ImageT>
TransformView<ImageT, TranslateTransform> translate(ImageViewBase<ImageT> const& im, int32 x_offset, int32 y_offset) {
  return translate(im, (double)x_offset, (double)y_offset, ZeroEdgeExtension(), NearestPixelInterpolation());
}

// ---- rotate (:817-843) ------------------------------------------------------------------------------------------------------
template <class ImageT, class EdgeT, class InterpT>
TransformView<ImageT, RotateTransform> rotate(ImageViewBase<ImageT> const& v, double theta, Vector2 translate, EdgeT const& edge,
                                              InterpT const& interp) {
  return transform(v, RotateTransform(theta, translate), edge, interp);
}
template <class ImageT, class EdgeT>
TransformView<ImageT, RotateTransform> rotate(ImageViewBase<ImageT> const& v, double theta, Vector2 translate, EdgeT const& edge) {
  return transform(v, RotateTransform(theta, translate), edge, BilinearInterpolation());
}
template <class ImageT>
TransformView<ImageT, RotateTransform> rotate(ImageViewBase<ImageT> const& v, double theta, Vector2 translate = Vector2()) {
  return transform(v, RotateTransform(theta, translate), ZeroEdgeExtension(), BilinearInterpolation());
}

}  // namespace vw
#endif
