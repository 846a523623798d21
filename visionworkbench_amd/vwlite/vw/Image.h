// vw/Image.h — the operator surface of Vision Workbench's Image module that the stereo hot path uses,
// boost-free and header-only: ImageView<T> storage, the CRTP lazy-view protocol, crop / edge_extend views,
// ImageViewRef<T> type erasure, PixelGray<T> and PixelMask<T>.
//
// Protocol kept from the reference:
//   every view derives from ImageViewBase<Impl> (src/vw/Image/ImageViewBase.h:57-122) and offers cols/rows/planes,
//   operator()(col,row), prerasterize(bbox) and rasterize(dest,bbox); nothing is computed until a view is assigned
//   to an ImageView<T> (src/vw/Image/ImageView.h:113-119,136-141); ImageViewRef<T> erases the view type behind
//   virtual calls (src/vw/Image/ImageViewRef.h:189-267).
// Layouts are the reference's: ImageView is row-major contiguous and zero-initialised (ImageView.h:209-239),
// PixelMask<Vector2i> is {int32,int32,int32 valid in {0,INT32_MAX}} (src/vw/Image/PixelMask.h:48-120).
//
// Hole filling on the engine (include/vwgpu.h), with the reference's signatures, eager like every
// other engine wrapper:
//   grassfire                                      src/vw/Image/Grassfire.h:43-55
//   BlobIndexThreaded (constructor, num_blobs, blob_bbox, wipe_big_blobs), get_blob_sizes, invert_mask
//                                                  src/vw/Image/BlobIndex.h:385-500, :507-615
//   applyErodeView                                 src/vw/Image/ErodeView.h:157-162
//   inpaint, fill_holes_grass, fill_nodata_with_avg   src/vw/Image/InpaintView.h:231-237, :307-311, :381-387
//
// Image statistics and intensity scaling on the engine, on float, PixelGray<float> and
// PixelMask<float> images:
//   find_image_min_max, min_max_channel_values, sum_of_channel_values, mean_channel_value, stddev_channel_value,
//   median_channel_value                           src/vw/Image/Statistics.h:98-186
//   histogram, otsu_threshold (both overloads), percentile_scale_convert, u8_convert   src/vw/Image/ImageThresh.h:53-286
//   clamp, normalize, threshold                    src/vw/Image/Algorithms.h:50-61, :171-188, :210-, AutoNormalize.h:33-86
#ifndef VWLITE_IMAGE_H
#define VWLITE_IMAGE_H

#include <algorithm>
#include <atomic>
#include <cmath>
#include <exception>
#include <limits>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "Engine.h"
#include "Math.h"

namespace vw {

// ---- pixel types -------------------------------------------------------------------------------------------
template <class ChannelT>
class PixelGray {
  ChannelT m_v;
public:
  typedef ChannelT channel_type;
  PixelGray() : m_v() {}
  PixelGray(ChannelT v) : m_v(v) {}
  template <class U> explicit PixelGray(PixelGray<U> const& o) : m_v(ChannelT(o.v())) {}
  ChannelT& v() { return m_v; }  ChannelT const& v() const { return m_v; }
  operator ChannelT() const { return m_v; }
  ChannelT& operator[](int) { return m_v; }  ChannelT const& operator[](int) const { return m_v; }
};

template <class T> struct CompoundChannelType { typedef T type; };
template <class T> struct CompoundChannelType<PixelGray<T>> { typedef T type; };
template <class T, int N> struct CompoundChannelType<Vector<T, N>> { typedef T type; };

// ChannelRange (src/vw/Image/PixelTypeInfo.h:85-118): integer max = numeric max, float max = 1.0.
template <class T> struct ChannelRange {
  static T max() { return std::is_floating_point<T>::value ? T(1) : std::numeric_limits<T>::max(); }
  static T min() { return T(); }
};

template <class ChildT>
class PixelMask {
public:
  typedef typename CompoundChannelType<ChildT>::type channel_type;
private:
  ChildT m_child;
  channel_type m_valid;
public:
  PixelMask() : m_child(), m_valid(ChannelRange<channel_type>::min()) {}          // invalid by default (:58-61)
  PixelMask(ChildT const& c) : m_child(c), m_valid(ChannelRange<channel_type>::max()) {}
  PixelMask(channel_type a0, channel_type a1) : m_valid(ChannelRange<channel_type>::max()) { m_child[0] = a0; m_child[1] = a1; }
  template <class U> PixelMask(PixelMask<U> const& o)
      : m_child(ChildT(o.child())), m_valid(o.valid() ? ChannelRange<channel_type>::max() : ChannelRange<channel_type>::min()) {}
  channel_type valid() const { return m_valid; }
  void invalidate() { m_valid = ChannelRange<channel_type>::min(); }
  void validate() { m_valid = ChannelRange<channel_type>::max(); }
  ChildT& child() { return m_child; }  ChildT const& child() const { return m_child; }
  channel_type& operator[](int i) { return m_child[i]; }
  channel_type const& operator[](int i) const { return m_child[i]; }
};
template <class T> bool is_valid(PixelMask<T> const& p) { return p.valid() != 0; }
template <class T> bool is_valid(T const&) { return true; }
template <class T> void invalidate(PixelMask<T>& p) { p.invalidate(); }
template <class T> void validate(PixelMask<T>& p) { p.validate(); }
static_assert(sizeof(PixelMask<Vector2i>) == 12, "PixelMask<Vector2i> must keep the reference's 12-byte layout");
static_assert(sizeof(PixelMask<Vector2f>) == 12, "PixelMask<Vector2f> must keep the reference's 12-byte layout");
static_assert(sizeof(PixelGray<float>) == 4, "PixelGray<float> is one float");

// ---- view protocol -----------------------------------------------------------------------------------------
template <class ImplT>
struct ImageViewBase {
  ImplT& impl() { return static_cast<ImplT&>(*this); }
  ImplT const& impl() const { return static_cast<ImplT const&>(*this); }
  int32 get_cols() const { return impl().cols(); }
  int32 get_rows() const { return impl().rows(); }
};

template <class ViewT> BBox2i bounding_box(ImageViewBase<ViewT> const& v) {
  return BBox2i(0, 0, v.impl().cols(), v.impl().rows());
}

// Default rasterisation: walk the source pixel by pixel (src/vw/Image/ImageViewBase.h:282-316).
template <class SrcT, class DestT>
void rasterize(SrcT const& src, DestT const& dest, BBox2i const& bbox) {
  for (int32 r = 0; r < bbox.height(); ++r)
    for (int32 c = 0; c < bbox.width(); ++c)
      dest(c, r) = typename DestT::pixel_type(src(c + bbox.min().x(), r + bbox.min().y()));
}

template <class PixelT>
class ImageView : public ImageViewBase<ImageView<PixelT>> {
  std::shared_ptr<std::vector<PixelT>> m_data;   // shared, shallow-copied by value (ImageView.h:72-75,98-103)
  int32 m_cols, m_rows;
public:
  typedef PixelT pixel_type;
  typedef ImageView prerasterize_type;
  ImageView() : m_cols(0), m_rows(0) {}
  ImageView(int32 cols, int32 rows) { set_size(cols, rows); }
  template <class ViewT> ImageView(ImageViewBase<ViewT> const& view) {          // rasterising ctor (:113-119)
    set_size(view.impl().cols(), view.impl().rows());
    view.impl().rasterize(*this, BBox2i(0, 0, m_cols, m_rows));
  }
  template <class ViewT> ImageView& operator=(ImageViewBase<ViewT> const& view) {  // (:136-141)
    set_size(view.impl().cols(), view.impl().rows());
    view.impl().rasterize(*this, BBox2i(0, 0, m_cols, m_rows));
    return *this;
  }
  void set_size(int32 cols, int32 rows) {
    VW_ASSERT(cols >= 0 && rows >= 0, ArgumentErr() << "Cannot allocate image with negative pixel count.");
    m_cols = cols; m_rows = rows;
    m_data = std::make_shared<std::vector<PixelT>>((size_t)cols * rows);          // zero / default initialised
  }
  int32 cols() const { return m_cols; }
  int32 rows() const { return m_rows; }
  int32 planes() const { return 1; }
  PixelT* data() const { return m_data ? m_data->data() : nullptr; }
  PixelT& operator()(int32 c, int32 r) const { return (*m_data)[(size_t)r * m_cols + c]; }
  prerasterize_type prerasterize(BBox2i const&) const { return *this; }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const { vw::rasterize(*this, dest, bbox); }
};

// crop(view, bbox): lazy window; negative / out-of-range origins are legal when the child is edge-extended
// (src/vw/Image/Manipulation.h:82-147).
template <class ChildT>
class CropView : public ImageViewBase<CropView<ChildT>> {
  ChildT m_child; int32 m_x, m_y, m_w, m_h;
public:
  typedef typename ChildT::pixel_type pixel_type;
  typedef ImageView<pixel_type> prerasterize_type;
  CropView(ChildT const& c, int32 x, int32 y, int32 w, int32 h) : m_child(c), m_x(x), m_y(y), m_w(w), m_h(h) {}
  int32 cols() const { return m_w; }  int32 rows() const { return m_h; }  int32 planes() const { return 1; }
  // l-value when the child yields references (crop(image, ...) = ... ; src/vw/Image/Manipulation.h:122-133)
  decltype(auto) operator()(int32 c, int32 r) const { return m_child(c + m_x, r + m_y); }
  prerasterize_type prerasterize(BBox2i const& b) const { ImageView<pixel_type> o(b.width(), b.height()); rasterize(o, b); return o; }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const { vw::rasterize(*this, dest, bbox); }
};
template <class ViewT> CropView<ViewT> crop(ImageViewBase<ViewT> const& v, int32 x, int32 y, int32 w, int32 h) {
  return CropView<ViewT>(v.impl(), x, y, w, h);
}
template <class ViewT> CropView<ViewT> crop(ImageViewBase<ViewT> const& v, BBox2i const& b) {
  return CropView<ViewT>(v.impl(), b.min().x(), b.min().y(), b.width(), b.height());
}

// Edge extension (src/vw/Image/EdgeExtension.h): Constant = clamp to the nearest edge pixel, Zero = 0 outside.
struct ConstantEdgeExtension {
  template <class V> typename V::pixel_type operator()(V const& v, int32 c, int32 r) const {
    c = c < 0 ? 0 : (c >= v.cols() ? v.cols() - 1 : c);
    r = r < 0 ? 0 : (r >= v.rows() ? v.rows() - 1 : r);
    return v(c, r);
  }
};
struct ZeroEdgeExtension {
  template <class V> typename V::pixel_type operator()(V const& v, int32 c, int32 r) const {
    if (c < 0 || r < 0 || c >= v.cols() || r >= v.rows()) return typename V::pixel_type();
    return v(c, r);
  }
};
template <class ChildT, class ExtT>
class EdgeExtensionView : public ImageViewBase<EdgeExtensionView<ChildT, ExtT>> {
  ChildT m_child; ExtT m_ext;
public:
  typedef typename ChildT::pixel_type pixel_type;
  typedef ImageView<pixel_type> prerasterize_type;
  EdgeExtensionView(ChildT const& c, ExtT e = ExtT()) : m_child(c), m_ext(e) {}
  int32 cols() const { return m_child.cols(); }  int32 rows() const { return m_child.rows(); }  int32 planes() const { return 1; }
  pixel_type operator()(int32 c, int32 r) const { return m_ext(m_child, c, r); }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const { vw::rasterize(*this, dest, bbox); }
};
template <class ViewT, class ExtT> EdgeExtensionView<ViewT, ExtT> edge_extend(ImageViewBase<ViewT> const& v, ExtT e) {
  return EdgeExtensionView<ViewT, ExtT>(v.impl(), e);
}
template <class ViewT> EdgeExtensionView<ViewT, ConstantEdgeExtension> edge_extend(ImageViewBase<ViewT> const& v) {
  return EdgeExtensionView<ViewT, ConstantEdgeExtension>(v.impl());
}

// constant_view(value, cols, rows) / constant_view(value, like_view): a view with the same value everywhere
// (src/vw/Image/Algorithms.h ConstantView) — e.g. an all-valid mask without allocating one.
template <class PixelT>
class ConstantView : public ImageViewBase<ConstantView<PixelT>> {
  PixelT m_value;
  int32 m_cols, m_rows;
public:
  typedef PixelT pixel_type;
  typedef PixelT result_type;
  typedef ConstantView prerasterize_type;
  ConstantView(PixelT const& value, int32 cols, int32 rows) : m_value(value), m_cols(cols), m_rows(rows) {}
  int32 cols() const { return m_cols; }  int32 rows() const { return m_rows; }  int32 planes() const { return 1; }
  result_type operator()(int32, int32) const { return m_value; }
  prerasterize_type prerasterize(BBox2i const&) const { return *this; }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const {
    for (int32 r = 0; r < bbox.height(); ++r) for (int32 c = 0; c < bbox.width(); ++c) dest(c, r) = m_value;
  }
};
template <class PixelT> ConstantView<PixelT> constant_view(PixelT const& value, int32 cols, int32 rows) { return ConstantView<PixelT>(value, cols, rows); }
template <class PixelT, class ViewT> ConstantView<PixelT> constant_view(PixelT const& value, ImageViewBase<ViewT> const& like) {
  return ConstantView<PixelT>(value, like.impl().cols(), like.impl().rows());
}

// pixel_cast<DestPixelT>(view): lazy per-pixel conversion.
template <class ChildT, class DestPixelT>
class PixelCastView : public ImageViewBase<PixelCastView<ChildT, DestPixelT>> {
  ChildT m_child;
public:
  typedef DestPixelT pixel_type;
  PixelCastView(ChildT const& c) : m_child(c) {}
  int32 cols() const { return m_child.cols(); }  int32 rows() const { return m_child.rows(); }  int32 planes() const { return 1; }
  pixel_type operator()(int32 c, int32 r) const { return pixel_type(m_child(c, r)); }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const { vw::rasterize(*this, dest, bbox); }
};
template <class DestPixelT, class ViewT> PixelCastView<ViewT, DestPixelT> pixel_cast(ImageViewBase<ViewT> const& v) {
  return PixelCastView<ViewT, DestPixelT>(v.impl());
}

// ImageViewRef<PixelT>: type-erased view handle (src/vw/Image/ImageViewRef.h:189-267).
template <class PixelT>
class ImageViewRef : public ImageViewBase<ImageViewRef<PixelT>> {
  struct Base {
    virtual ~Base() {}
    virtual int32 cols() const = 0;
    virtual int32 rows() const = 0;
    virtual PixelT at(int32 c, int32 r) const = 0;
    virtual void raster(ImageView<PixelT> const& dest, BBox2i const& bbox) const = 0;
    virtual const PixelT* plain(int32& stride) const = 0;   // non-null when the view is a plain ImageView
  };
  template <class ViewT> struct Impl : Base {
    ViewT v;
    Impl(ViewT const& view) : v(view) {}
    int32 cols() const override { return v.cols(); }
    int32 rows() const override { return v.rows(); }
    PixelT at(int32 c, int32 r) const override { return PixelT(v(c, r)); }
    void raster(ImageView<PixelT> const& dest, BBox2i const& bbox) const override { v.rasterize(dest, bbox); }
    const PixelT* plain(int32& stride) const override { return plain_of(v, stride); }
    static const PixelT* plain_of(ImageView<PixelT> const& iv, int32& stride) { stride = iv.cols(); return iv.data(); }
    template <class Other> static const PixelT* plain_of(Other const&, int32&) { return nullptr; }
  };
  std::shared_ptr<Base> m_view;
public:
  typedef PixelT pixel_type;
  typedef ImageView<PixelT> prerasterize_type;
  ImageViewRef() {}
  template <class ViewT> ImageViewRef(ImageViewBase<ViewT> const& view) : m_view(new Impl<ViewT>(view.impl())) {}
  int32 cols() const { return m_view->cols(); }
  int32 rows() const { return m_view->rows(); }
  int32 planes() const { return 1; }
  PixelT operator()(int32 c, int32 r) const { return m_view->at(c, r); }
  prerasterize_type prerasterize(BBox2i const& b) const { ImageView<PixelT> o(b.width(), b.height()); m_view->raster(o, b); return o; }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const {
    ImageView<PixelT> tmp(bbox.width(), bbox.height());
    m_view->raster(tmp, bbox);
    vw::rasterize(tmp, dest, BBox2i(0, 0, bbox.width(), bbox.height()));
  }
  void rasterize(ImageView<PixelT> const& dest, BBox2i const& bbox) const { m_view->raster(dest, bbox); }
  // Engine fast path: direct pointer when the handle wraps a plain ImageView (no copy).
  const PixelT* plain_data(int32& stride) const { return m_view->plain(stride); }
};

// block_rasterize(view, block_size, num_threads): rasterise the child view block by block from a pool of threads
// (src/vw/Image/BlockRasterize.h:43-176 without the cache; block walk of src/vw/Image/BlockProcessor.h:63-176: blocks are
// aligned to multiples of block_size counted from the image origin, cropped to the requested bbox, handed out in raster order).
// Each worker calls child.rasterize(crop(dest, block - offset), block); with the engine's views every worker thread owns
// its own GPU context, so several tiles are in flight on the device at once.
template <class ImageT>
class BlockRasterizeView : public ImageViewBase<BlockRasterizeView<ImageT>> {
  std::shared_ptr<ImageT> m_child;
  Vector2i m_block_size;
  int32 m_num_threads;
  static int32 round_down(int32 val, int32 mod) { return val + ((val >= 0) ? (-(val % mod)) : (((-val - 1) % mod) - mod + 1)); }
public:
  typedef typename ImageT::pixel_type pixel_type;
  typedef pixel_type result_type;
  typedef ImageView<pixel_type> prerasterize_type;
  BlockRasterizeView(ImageT const& image, Vector2i const& block_size, int32 num_threads = 0)
      : m_child(new ImageT(image)), m_block_size(block_size), m_num_threads(num_threads) {
    if (m_block_size.x() <= 0 || m_block_size.y() <= 0) m_block_size = Vector2i(1024, 1024);
    if (m_num_threads <= 0) {
      const unsigned hc = std::thread::hardware_concurrency();
      m_num_threads = (int32)(hc == 0 ? 1 : (hc > 8 ? 8 : hc));
    }
  }
  int32 cols() const { return m_child->cols(); }
  int32 rows() const { return m_child->rows(); }
  int32 planes() const { return 1; }
  ImageT const& child() const { return *m_child; }
  result_type operator()(int32 x, int32 y) const { return (*m_child)(x, y); }
  prerasterize_type prerasterize(BBox2i const& b) const { ImageView<pixel_type> o(b.width(), b.height()); rasterize(o, b); return o; }
  template <class DestT> void rasterize(DestT const& dest, BBox2i const& bbox) const {
    if (bbox.empty()) return;
    const int32 bx0 = round_down(bbox.min().x(), m_block_size.x()), by0 = round_down(bbox.min().y(), m_block_size.y());
    const int32 nbx = (bbox.max().x() - bx0 + m_block_size.x() - 1) / m_block_size.x();
    const int32 nby = (bbox.max().y() - by0 + m_block_size.y() - 1) / m_block_size.y();
    std::atomic<int32> next(0);
    std::exception_ptr error;
    std::mutex error_mutex;
    auto worker = [&](int32 index) {
      engine::thread_worker_index() = index;      // the engine wrappers bind worker w to GPU w % ndev (vw/Engine.h)
      try {
        for (;;) {
          const int32 i = next.fetch_add(1);
          if (i >= nbx * nby) return;
          BBox2i block(bx0 + (i % nbx) * m_block_size.x(), by0 + (i / nbx) * m_block_size.y(), m_block_size.x(), m_block_size.y());
          block.crop(bbox);
          if (block.empty()) continue;
          m_child->rasterize(crop(dest, block - bbox.min()), block);
        }
      } catch (...) {
        std::lock_guard<std::mutex> lock(error_mutex);
        if (!error) error = std::current_exception();
        next.store(nbx * nby);
      }
    };
    const int32 nt = std::min<int32>(m_num_threads, nbx * nby);
    if (nt <= 1) worker(engine::thread_worker_index());
    else {
      std::vector<std::thread> pool;
      for (int32 t = 0; t < nt; ++t) pool.emplace_back(worker, t);
      for (std::thread& t : pool) t.join();
    }
    if (error) std::rethrow_exception(error);
  }
};
template <class ImageT>
BlockRasterizeView<ImageT> block_rasterize(ImageViewBase<ImageT> const& image, Vector2i const& block_size, int32 num_threads = 0) {
  return BlockRasterizeView<ImageT>(image.impl(), block_size, num_threads);
}

template <class ViewT, class ValT> void fill(ImageViewBase<ViewT> const& v, ValT const& val) {
  for (int32 r = 0; r < v.impl().rows(); ++r)
    for (int32 c = 0; c < v.impl().cols(); ++c) v.impl()(c, r) = typename ViewT::pixel_type(val);
}
template <class ViewT> ImageView<typename ViewT::pixel_type> copy(ImageViewBase<ViewT> const& v) {
  ImageView<typename ViewT::pixel_type> o(v.impl().cols(), v.impl().rows());
  v.impl().rasterize(o, BBox2i(0, 0, o.cols(), o.rows()));
  return o;
}

// ---- hole filling on the engine ------------------------------------------------------------------------------
namespace detail {
template <class PixelT> struct masked_kind;      // the vwgpu_pixel_kind of a pixel type the engine takes as it is stored
template <> struct masked_kind<uint8> { static const int value = VWGPU_PIXEL_MASK_U8; };
template <> struct masked_kind<PixelMask<float>> { static const int value = VWGPU_PIXEL_MASKED_F32; };
template <> struct masked_kind<PixelMask<Vector2i>> { static const int value = VWGPU_PIXEL_DISPARITY_I32; };
template <> struct masked_kind<PixelMask<Vector2f>> { static const int value = VWGPU_PIXEL_DISPARITY_F32; };
static_assert(sizeof(PixelMask<float>) == 8, "PixelMask<float> is {value, valid}");
template <class T> struct grassfire_type;
template <> struct grassfire_type<uint8> { static const int value = VWGPU_GRASSFIRE_U8; };
template <> struct grassfire_type<int32> { static const int value = VWGPU_GRASSFIRE_I32; };
template <> struct grassfire_type<float> { static const int value = VWGPU_GRASSFIRE_F32; };
template <> struct grassfire_type<PixelGray<float>> { static const int value = VWGPU_GRASSFIRE_F32; };
}  // namespace detail

/// grassfire(src, dst, ignore_borders) (Grassfire.h:43-45).
template <class SourceT, class OutputT>
void grassfire(ImageViewBase<SourceT> const& src, ImageView<OutputT>& dst, bool ignore_borders = false) {
  ImageView<typename SourceT::pixel_type> in = src.impl();
  dst.set_size(in.cols(), in.rows());
  if (in.cols() == 0 || in.rows() == 0) return;
  ImageView<int32> d(in.cols(), in.rows());
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_grassfire(ctx, detail::grassfire_type<typename SourceT::pixel_type>::value, in.data(), in.cols(), in.rows(), 0,
                                     ignore_borders ? 1 : 0, d.data(), 0));
  for (int32 r = 0; r < d.rows(); ++r)
    for (int32 c = 0; c < d.cols(); ++c) dst(c, r) = OutputT(d(c, r));
}
/// Without a destination: a new ImageView<int32> (Grassfire.h:48-55).
template <class SourceT>
ImageView<int32> grassfire(ImageViewBase<SourceT> const& src, bool ignore_borders = false) {
  ImageView<int32> result;
  grassfire(src, result, ignore_borders);
  return result;
}

/// invert_mask(view): valid pixels become invalid and invalid ones valid (PixelMask.h); values are kept.
template <class ViewT>
ImageView<typename ViewT::pixel_type> invert_mask(ImageViewBase<ViewT> const& view) {
  ImageView<typename ViewT::pixel_type> in = view.impl(), out(in.cols(), in.rows());
  for (int32 r = 0; r < in.rows(); ++r)
    for (int32 c = 0; c < in.cols(); ++c) {
      out(c, r) = in(c, r);
      if (is_valid(in(c, r))) out(c, r).invalidate(); else out(c, r).validate();
    }
  return out;
}

/// BlobIndexThreaded (BlobIndex.h:385-500) over the whole image as one tile: the 8-connected blobs of the valid pixels in the
/// reference's order.  tile_size and num_threads are accepted and ignored (the blob order of several tiles is not reproduced).
class BlobIndexThreaded {
  ImageView<uint8> m_mask;
  int32 m_max_area;
  std::vector<BBox2i> m_blob_bbox;
  ImageView<int32> m_labels;
  std::vector<int32> m_table;
  void index(int wipe) {
    m_labels.set_size(m_mask.cols(), m_mask.rows());
    m_table.clear();
    m_blob_bbox.clear();
    if (m_mask.cols() == 0 || m_mask.rows() == 0) return;
    vwgpu_ctx* ctx = engine::thread_context();
    int count = 0;
    engine::check(ctx, vwgpu_blob_index(ctx, VWGPU_PIXEL_MASK_U8, m_mask.data(), m_mask.cols(), m_mask.rows(), 0, 0, m_max_area, wipe, nullptr, 0,
                                        nullptr, 0, &count));
    m_table.resize((size_t)5 * std::max(count, 1));
    engine::check(ctx, vwgpu_blob_index(ctx, VWGPU_PIXEL_MASK_U8, m_mask.data(), m_mask.cols(), m_mask.rows(), 0, 0, m_max_area, wipe,
                                        m_labels.data(), 0, m_table.data(), count, &count));
    m_table.resize((size_t)5 * count);
    for (int k = 0; k < count; ++k)
      m_blob_bbox.push_back(BBox2i(m_table[5 * k], m_table[5 * k + 1], m_table[5 * k + 2] - m_table[5 * k], m_table[5 * k + 3] - m_table[5 * k + 1]));
  }
public:
  template <class SourceT>
  BlobIndexThreaded(ImageViewBase<SourceT> const& src, int32 const& max_area = 0, int32 const& /*tile_size*/ = 0, int32 const& /*num_threads*/ = 0)
      : m_max_area(max_area) {
    ImageView<typename SourceT::pixel_type> in = src.impl();
    m_mask.set_size(in.cols(), in.rows());
    for (int32 r = 0; r < in.rows(); ++r)
      for (int32 c = 0; c < in.cols(); ++c) m_mask(c, r) = is_valid(in(c, r)) ? 255 : 0;
    index(0);
  }
  /// Wipe blobs whose bounding box is wider or taller than max_size (BlobIndex.h:457-477).
  void wipe_big_blobs(int max_size) {
    if (max_size > 0) { index(max_size); return; }
    m_table.clear();
    m_blob_bbox.clear();
    fill(m_labels, 0);
  }
  uint32 num_blobs() const { return (uint32)m_blob_bbox.size(); }
  BBox2i const& blob_bbox(uint32 const& index) const { return m_blob_bbox[index]; }
  int32 blob_size(uint32 const& index) const { return m_table[5 * (size_t)index + 4]; }
  // the engine's form of the selection: 1-based blob numbers per pixel, {min.x, min.y, max.x, max.y, size} per blob
  ImageView<int32> const& labels() const { return m_labels; }
  std::vector<int32> const& table() const { return m_table; }
};

/// get_blob_sizes(image, expand_size, size_limit) (BlobIndex.h:611-615) with the image as one tile.
template <class ImageT>
ImageView<uint32> get_blob_sizes(ImageViewBase<ImageT> const& image, int /*expand_size*/, uint32 size_limit) {
  ImageView<typename ImageT::pixel_type> in = image.impl();
  ImageView<uint32> out(in.cols(), in.rows());
  if (in.cols() == 0 || in.rows() == 0) return out;
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_blob_sizes(ctx, detail::masked_kind<typename ImageT::pixel_type>::value, in.data(), in.cols(), in.rows(), 0, size_limit,
                                      out.data(), 0));
  return out;
}

/// applyErodeView(src, bindex) (ErodeView.h:157-162, :199-221): a pixel inside a listed blob becomes the default pixel.
template <class SourceT>
ImageView<typename SourceT::pixel_type> applyErodeView(ImageViewBase<SourceT> const& src, BlobIndexThreaded const& bindex) {
  typedef typename SourceT::pixel_type pixel_type;
  ImageView<pixel_type> in = src.impl(), out(in.cols(), in.rows());
  VW_ASSERT(in.cols() == bindex.labels().cols() && in.rows() == bindex.labels().rows(), ArgumentErr() << "applyErodeView: the blob index belongs to another image.");
  for (int32 r = 0; r < in.rows(); ++r)
    for (int32 c = 0; c < in.cols(); ++c) out(c, r) = bindex.labels()(c, r) ? pixel_type() : in(c, r);
  return out;
}

/// inpaint(src, bindex, use_grassfire, default_inpaint_val) (InpaintView.h:231-237), rasterised over the whole image.
template <class SourceT>
ImageView<typename SourceT::pixel_type> inpaint(ImageViewBase<SourceT> const& src, BlobIndexThreaded const& bindex, bool use_grassfire,
                                                typename SourceT::pixel_type default_inpaint_val) {
  typedef typename SourceT::pixel_type pixel_type;
  ImageView<pixel_type> in = src.impl(), out(in.cols(), in.rows());
  if (in.cols() == 0 || in.rows() == 0) return out;
  VW_ASSERT(in.cols() == bindex.labels().cols() && in.rows() == bindex.labels().rows(), ArgumentErr() << "inpaint: the blob index belongs to another image.");
  for (uint32 k = 0; k < bindex.num_blobs(); ++k)
    VW_ASSERT(bindex.blob_bbox(k).width() <= VWGPU_HOLE_FILL_MAX_LEN && bindex.blob_bbox(k).height() <= VWGPU_HOLE_FILL_MAX_LEN,
              NoImplErr() << "inpaint: a blob wider or taller than " << VWGPU_HOLE_FILL_MAX_LEN << " pixels.");
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_inpaint(ctx, detail::masked_kind<pixel_type>::value, in.data(), in.cols(), in.rows(), 0, bindex.labels().data(), 0,
                                   bindex.table().data(), (int)bindex.num_blobs(), use_grassfire ? 1 : 0,
                                   reinterpret_cast<const float*>(&default_inpaint_val), VWGPU_HOLE_EDGE_REFERENCE, VWGPU_HOLE_FILL_MAX_LEN,
                                   out.data(), 0));
  return out;
}

/// fill_holes_grass(img, hole_fill_len) (InpaintView.h:307-311), rasterised in one call over the whole image.
template <class ImageT>
ImageView<typename ImageT::pixel_type> fill_holes_grass(ImageViewBase<ImageT> const& img, int hole_fill_len) {
  ImageView<typename ImageT::pixel_type> in = img.impl(), out(in.cols(), in.rows());
  if (in.cols() == 0 || in.rows() == 0) return out;
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_fill_holes_grass(ctx, detail::masked_kind<typename ImageT::pixel_type>::value, in.data(), in.cols(), in.rows(), 0,
                                            hole_fill_len, VWGPU_HOLE_EDGE_REFERENCE, out.data(), 0));
  return out;
}

/// fill_nodata_with_avg(img, kernel_size) (InpaintView.h:381-387) on PixelMask<float>.
template <class ImgT>
ImageView<PixelMask<float>> fill_nodata_with_avg(ImageViewBase<ImgT> const& img, int kernel_size) {
  VW_ASSERT((kernel_size % 2 == 1) && (kernel_size > 0), ArgumentErr() << "Expecting odd and positive kernel size.");
  ImageView<PixelMask<float>> in = img.impl(), out(in.cols(), in.rows());
  if (in.cols() == 0 || in.rows() == 0) return out;
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_fill_nodata_with_avg(ctx, reinterpret_cast<const float*>(in.data()), in.cols(), in.rows(), 0, kernel_size,
                                                reinterpret_cast<float*>(out.data()), 0));
  return out;
}

// ---- image statistics and intensity scaling on the engine ----------------------------------------------------------
namespace detail {
/// A single-channel float image as the engine takes it: the values and, for PixelMask<float>, the validity as uint8.
struct GrayOperand {
  ImageView<float> values;
  ImageView<uint8> mask;
  bool masked = false;
  const uint8* mask_ptr() const { return masked ? mask.data() : nullptr; }
  int32 cols() const { return values.cols(); }
  int32 rows() const { return values.rows(); }
};
inline float gray_value(float p) { return p; }
inline float gray_value(PixelGray<float> const& p) { return p.v(); }
template <class PixelT> struct gray_pixel { static const bool masked = false; static float value(PixelT const& p) { return gray_value(p); } };
template <class ChildT> struct gray_pixel<PixelMask<ChildT>> {
  static const bool masked = true;
  static float value(PixelMask<ChildT> const& p) { return gray_value(p.child()); }
};
template <class ViewT>
GrayOperand gray_operand(ImageViewBase<ViewT> const& view) {
  typedef typename ViewT::pixel_type pixel_type;
  ImageView<pixel_type> in = view.impl();
  GrayOperand g;
  g.values.set_size(in.cols(), in.rows());
  g.masked = gray_pixel<pixel_type>::masked;
  if (g.masked) g.mask.set_size(in.cols(), in.rows());
  for (int32 r = 0; r < in.rows(); ++r)
    for (int32 c = 0; c < in.cols(); ++c) {
      g.values(c, r) = gray_pixel<pixel_type>::value(in(c, r));
      if (g.masked) g.mask(c, r) = is_valid(in(c, r)) ? 1 : 0;
    }
  return g;
}
/// The values of `out` under the validity of `like` (UnaryCompoundFunctor carries the validity over, PixelMask.h:514-523).
inline void gray_store(float v, float const&, float& dst) { dst = v; }
inline void gray_store(float v, PixelGray<float> const&, PixelGray<float>& dst) { dst = PixelGray<float>(v); }
template <class ChildT> void gray_store(float v, PixelMask<ChildT> const& like, PixelMask<ChildT>& dst) {
  ChildT c;
  gray_store(v, like.child(), c);
  dst = PixelMask<ChildT>(c);
  if (!is_valid(like)) dst.invalidate();
}
template <class ViewT>
ImageView<typename ViewT::pixel_type> rescaled(ImageViewBase<ViewT> const& view, int mode, const double* params) {
  typedef typename ViewT::pixel_type pixel_type;
  ImageView<pixel_type> in = view.impl(), out(in.cols(), in.rows());
  if (in.cols() == 0 || in.rows() == 0) return out;
  GrayOperand g = gray_operand(in);
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_image_rescale(ctx, g.values.data(), g.cols(), g.rows(), 0, mode, params, VWGPU_PIXEL_F32, g.values.data(), 0));
  for (int32 r = 0; r < in.rows(); ++r)
    for (int32 c = 0; c < in.cols(); ++c) gray_store(g.values(c, r), in(c, r), out(c, r));
  return out;
}
inline void moments_of(GrayOperand const& g, double* m) {
  m[0] = m[1] = m[2] = 0;
  if (g.cols() == 0 || g.rows() == 0) return;
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_image_moments(ctx, g.values.data(), g.cols(), g.rows(), 0, g.mask_ptr(), 0, 0, 0, m));
}
}  // namespace detail

/// find_image_min_max(view, min_val, max_val) (Statistics.h:113-127).
template <class ViewT>
void find_image_min_max(ImageViewBase<ViewT> const& view, double& min_val, double& max_val) {
  max_val = -std::numeric_limits<double>::max();
  min_val = -max_val;
  detail::GrayOperand g = detail::gray_operand(view);
  if (g.cols() == 0 || g.rows() == 0) return;
  vwgpu_ctx* ctx = engine::thread_context();
  vwgpu_image_range r;
  engine::check(ctx, vwgpu_image_min_max(ctx, g.values.data(), g.cols(), g.rows(), 0, g.mask_ptr(), 0, 0, 0, VWGPU_MIN_MAX_FIND, &r));
  min_val = r.min; max_val = r.max;
}
/// min_max_channel_values(view, min, max) (Statistics.h:98-108): ArgumentErr without a valid sample.
template <class ViewT>
void min_max_channel_values(ImageViewBase<ViewT> const& view, float& min, float& max) {
  detail::GrayOperand g = detail::gray_operand(view);
  VW_ASSERT(g.cols() > 0 && g.rows() > 0, ArgumentErr() << "MinMaxAccumulator: no valid samples");
  vwgpu_ctx* ctx = engine::thread_context();
  vwgpu_image_range r;
  engine::check(ctx, vwgpu_image_min_max(ctx, g.values.data(), g.cols(), g.rows(), 0, g.mask_ptr(), 0, 0, 0, VWGPU_MIN_MAX_ACCUM, &r));
  min = (float)r.min; max = (float)r.max;
}
/// sum_of_channel_values (Statistics.h:129-137), mean_channel_value (:139-148), stddev_channel_value (:166-172).
template <class ViewT> double sum_of_channel_values(ImageViewBase<ViewT> const& view) {
  double m[3];
  detail::moments_of(detail::gray_operand(view), m);
  return m[1];
}
template <class ViewT> double mean_channel_value(ImageViewBase<ViewT> const& view) {
  double m[3], r = 0;
  detail::moments_of(detail::gray_operand(view), m);
  VW_ASSERT(vwgpu_moments_mean(m, &r) == VWGPU_OK, ArgumentErr() << "MeanAccumulator: no valid samples");
  return r;
}
template <class ViewT> double stddev_channel_value(ImageViewBase<ViewT> const& view) {
  double m[3], r = 0;
  detail::moments_of(detail::gray_operand(view), m);
  VW_ASSERT(vwgpu_moments_stddev(m, &r) == VWGPU_OK, ArgumentErr() << "StdDevAccumulator(): no valid samples.");
  return r;
}
/// median_channel_value (Statistics.h:179-186): an exact selection on the engine, nothing is sorted.
template <class ViewT> double median_channel_value(ImageViewBase<ViewT> const& view) {
  detail::GrayOperand g = detail::gray_operand(view);
  VW_ASSERT(g.cols() > 0 && g.rows() > 0, ArgumentErr() << "median: no valid samples.");
  vwgpu_ctx* ctx = engine::thread_context();
  double r = 0;
  engine::check(ctx, vwgpu_image_order_statistic(ctx, g.values.data(), g.cols(), g.rows(), 0, g.mask_ptr(), 0, VWGPU_ORDER_MEDIAN, 0.0, &r));
  return r;
}

/// histogram(view, num_bins, min_val, max_val, hist) (ImageThresh.h:53-73).
template <class ViewT>
void histogram(ImageViewBase<ViewT> const& view, int num_bins, double min_val, double max_val, math::Histogram& hist) {
  VW_ASSERT(num_bins > 0, ArgumentErr() << "histogram: number of input bins must be positive");
  if (max_val == min_val) max_val = min_val + 1.0;
  hist.initialize(num_bins, min_val, max_val);
  detail::GrayOperand g = detail::gray_operand(view);
  if (g.cols() == 0 || g.rows() == 0) return;
  vwgpu_ctx* ctx = engine::thread_context();
  std::vector<uint64_t> counts((size_t)num_bins + 2);
  engine::check(ctx, vwgpu_image_histogram(ctx, g.values.data(), g.cols(), g.rows(), 0, g.mask_ptr(), 0, 0, 0, num_bins, min_val, max_val, 0,
                                           counts.data(), nullptr));
  hist.set_counts(counts.data());
}

/// otsu_threshold(view) (ImageThresh.h:80-145) and otsu_threshold(view, num_sample_rows, num_sample_cols, num_bins) (:151-239).
template <class ViewT> double otsu_threshold(ImageViewBase<ViewT> const& view) {
  detail::GrayOperand g = detail::gray_operand(view);
  if (g.cols() == 0 || g.rows() == 0) return 0.0;
  vwgpu_ctx* ctx = engine::thread_context();
  double t = 0;
  engine::check(ctx, vwgpu_otsu_threshold(ctx, g.values.data(), g.cols(), g.rows(), 0, g.mask_ptr(), 0, 0, 0, 256, 1, &t));
  return t;
}
template <class ViewT> double otsu_threshold(ImageViewBase<ViewT> const& view, int num_sample_rows, int num_sample_cols, int num_bins) {
  detail::GrayOperand g = detail::gray_operand(view);
  if (g.cols() == 0 || g.rows() == 0) return 0.0;
  vwgpu_ctx* ctx = engine::thread_context();
  double t = 0;
  engine::check(ctx, vwgpu_otsu_threshold(ctx, g.values.data(), g.cols(), g.rows(), 0, g.mask_ptr(), 0, num_sample_cols, num_sample_rows,
                                          num_bins, 2, &t));
  return t;
}

/// percentile_scale_convert(input_image, output_image, low_percentile, high_percentile, num_bins) (ImageThresh.h:243-270).
template <class ViewT>
void percentile_scale_convert(ImageViewBase<ViewT> const& input_image, ImageView<uint8>& output_image, double low_percentile = 0.02,
                              double high_percentile = 0.98, int num_bins = 256) {
  detail::GrayOperand g = detail::gray_operand(input_image);
  output_image.set_size(g.cols(), g.rows());
  if (g.cols() == 0 || g.rows() == 0) return;
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_percentile_scale_convert(ctx, g.values.data(), g.cols(), g.rows(), 0, g.mask_ptr(), 0, low_percentile,
                                                    high_percentile, num_bins, VWGPU_PIXEL_U8, output_image.data(), 0, nullptr));
}
/// u8_convert(input_image, output_image) (ImageThresh.h:274-286).
template <class ViewT>
void u8_convert(ImageViewBase<ViewT> const& input_image, ImageView<PixelGray<uint8>>& output_image) {
  static_assert(sizeof(PixelGray<uint8>) == 1, "PixelGray<uint8> is one byte");
  detail::GrayOperand g = detail::gray_operand(input_image);
  output_image.set_size(g.cols(), g.rows());
  if (g.cols() == 0 || g.rows() == 0) return;
  vwgpu_ctx* ctx = engine::thread_context();
  engine::check(ctx, vwgpu_u8_convert(ctx, g.values.data(), g.cols(), g.rows(), 0, g.mask_ptr(), 0, VWGPU_PIXEL_U8,
                                      reinterpret_cast<uint8*>(output_image.data()), 0, nullptr));
}

/// clamp(image, low, high) (Algorithms.h:50-61), threshold(image, thresh, low, high) (:210-), normalize(image, old_low, old_high,
/// new_low, new_high) (:171-188), normalize(image, low, high) and normalize(image) (AutoNormalize.h:33-86); rasterised at once.
template <class ViewT>
ImageView<typename ViewT::pixel_type> clamp(ImageViewBase<ViewT> const& image, double low, double high) {
  const double p[2] = {low, high};
  return detail::rescaled(image, VWGPU_RESCALE_CLAMP, p);
}
template <class ViewT>
ImageView<typename ViewT::pixel_type> threshold(ImageViewBase<ViewT> const& image, double thresh = 0.0, double low = 0.0, double high = 1.0) {
  const double p[3] = {thresh, low, high};
  return detail::rescaled(image, VWGPU_RESCALE_THRESHOLD, p);
}
template <class ViewT>
ImageView<typename ViewT::pixel_type> normalize(ImageViewBase<ViewT> const& image, double old_low, double old_high, double new_low,
                                                double new_high) {
  const double p[4] = {old_low, old_high, new_low, new_high};
  return detail::rescaled(image, VWGPU_RESCALE_NORMALIZE, p);
}
template <class ViewT>
ImageView<typename ViewT::pixel_type> normalize(ImageViewBase<ViewT> const& image, double low, double high) {
  float old_min, old_max;
  min_max_channel_values(image, old_min, old_max);
  return normalize(image, old_min, old_max, low, high);
}
template <class ViewT>
ImageView<typename ViewT::pixel_type> normalize(ImageViewBase<ViewT> const& image) { return normalize(image, 0.0, 1.0); }

}  // namespace vw
#endif
