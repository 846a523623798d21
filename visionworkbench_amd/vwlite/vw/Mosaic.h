// vw/Mosaic.h — vw::mosaic::ImageComposite (src/vw/Mosaic/ImageComposite.h) over the engine's vwgpu_composite entries
// (include/vwgpu.h), with the reference's names:
//   ImageComposite<PixelT>::insert / prepare / generate_patch / operator()       :249-279
//   set_draft_mode / set_fill_holes / cols / rows / bbox / source_data_bbox       :261-272
// PixelT is PixelGrayA<float> or PixelRGBA<float> (premultiplied alpha, alpha last), in draft mode also float or
// PixelGray<float>.  Every inserted image is copied to the device.  Not here: the cache, reuse_masks, sparse_check,
// integer pixels, QuadTreeGenerator.
#ifndef VWLITE_VW_MOSAIC_H
#define VWLITE_VW_MOSAIC_H

#include "Engine.h"
#include "Image.h"
#include "Math.h"

namespace vw {

// As much of the reference's PixelGrayA and PixelRGBA (src/vw/Image/PixelTypes.h) as the composite needs: plain channels, alpha last.
template <class ChannelT>
struct PixelGrayA {
  ChannelT m_ch[2];
  PixelGrayA() : m_ch{ChannelT(), ChannelT()} {}
  PixelGrayA(ChannelT v, ChannelT a) : m_ch{v, a} {}
  ChannelT& v() { return m_ch[0]; }  ChannelT const& v() const { return m_ch[0]; }
  ChannelT& a() { return m_ch[1]; }  ChannelT const& a() const { return m_ch[1]; }
  ChannelT& operator[](int i) { return m_ch[i]; }  ChannelT const& operator[](int i) const { return m_ch[i]; }
  bool operator==(PixelGrayA const& o) const { return m_ch[0] == o.m_ch[0] && m_ch[1] == o.m_ch[1]; }
};
template <class ChannelT>
struct PixelRGBA {
  ChannelT m_ch[4];
  PixelRGBA() : m_ch{ChannelT(), ChannelT(), ChannelT(), ChannelT()} {}
  PixelRGBA(ChannelT r, ChannelT g, ChannelT b, ChannelT a) : m_ch{r, g, b, a} {}
  ChannelT& r() { return m_ch[0]; }  ChannelT const& r() const { return m_ch[0]; }
  ChannelT& g() { return m_ch[1]; }  ChannelT const& g() const { return m_ch[1]; }
  ChannelT& b() { return m_ch[2]; }  ChannelT const& b() const { return m_ch[2]; }
  ChannelT& a() { return m_ch[3]; }  ChannelT const& a() const { return m_ch[3]; }
  ChannelT& operator[](int i) { return m_ch[i]; }  ChannelT const& operator[](int i) const { return m_ch[i]; }
  bool operator==(PixelRGBA const& o) const {
    return m_ch[0] == o.m_ch[0] && m_ch[1] == o.m_ch[1] && m_ch[2] == o.m_ch[2] && m_ch[3] == o.m_ch[3];
  }
};
static_assert(sizeof(PixelGrayA<float>) == 8 && sizeof(PixelRGBA<float>) == 16, "interleaved floats, alpha last");

namespace mosaic {

namespace detail {
template <class PixelT> struct composite_channels;
template <> struct composite_channels<float> { static const int value = 1; };
template <> struct composite_channels<PixelGray<float>> { static const int value = 1; };
template <> struct composite_channels<PixelGrayA<float>> { static const int value = 2; };
template <> struct composite_channels<PixelRGBA<float>> { static const int value = 4; };
}  // namespace detail

template <class PixelT>
class ImageComposite {
  vwgpu_composite* m_c;
  BBox2i m_view, m_data;
  bool m_draft, m_fill;

  ImageComposite(ImageComposite const&);              // the composite owns device memory: no copies
  ImageComposite& operator=(ImageComposite const&);

  void read_boxes() {
    int b[4];
    if (vwgpu_composite_bbox(m_c, 0, b) == VWGPU_OK) m_data = BBox2i(Vector2i(b[0], b[1]), Vector2i(b[2], b[3]));
    if (vwgpu_composite_bbox(m_c, 1, b) == VWGPU_OK) m_view = BBox2i(Vector2i(b[0], b[1]), Vector2i(b[2], b[3]));
  }

public:
  typedef PixelT pixel_type;
  typedef PixelT result_type;

  ImageComposite() : m_c(nullptr), m_draft(false), m_fill(false) {
    vwgpu_ctx* ctx = engine::thread_context();
    engine::check(ctx, vwgpu_composite_create(ctx, &m_c));
  }
  ~ImageComposite() { vwgpu_composite_destroy(m_c); }

  template <class ViewT>
  void insert(ImageViewBase<ViewT> const& image, int x, int y) {
    ImageView<PixelT> in = image.impl();
    vwgpu_ctx* ctx = engine::thread_context();
    engine::check(ctx, vwgpu_composite_insert(ctx, m_c, reinterpret_cast<const float*>(in.data()), in.cols(), in.rows(), 0,
                                              detail::composite_channels<PixelT>::value, x, y));
    read_boxes();
  }

  void set_draft_mode(bool draft_mode) { m_draft = draft_mode; }
  void set_fill_holes(bool fill_holes) {
    m_fill = fill_holes;
    vwgpu_ctx* ctx = engine::thread_context();
    engine::check(ctx, vwgpu_composite_set_fill_holes(ctx, m_c, m_fill ? 1 : 0));
  }

  void prepare() { prepare_impl(nullptr); }
  void prepare(BBox2i const& total_bbox) {
    const int box[4] = {total_bbox.min()[0], total_bbox.min()[1], total_bbox.max()[0], total_bbox.max()[1]};
    prepare_impl(box);
  }

  /// Generate a section of the output image (:255-258).
  ImageView<PixelT> generate_patch(BBox2i const& patch_bbox) const {
    ImageView<PixelT> out(patch_bbox.width(), patch_bbox.height());
    vwgpu_ctx* ctx = engine::thread_context();
    engine::check(ctx, vwgpu_composite_set_draft_mode(ctx, m_c, m_draft ? 1 : 0));
    engine::check(ctx, vwgpu_composite_generate_patch(ctx, m_c, patch_bbox.min()[0], patch_bbox.min()[1], patch_bbox.width(), patch_bbox.height(),
                                                      reinterpret_cast<float*>(out.data()), 0));
    return out;
  }

  int32 cols() const { return vwgpu_composite_cols(m_c); }
  int32 rows() const { return vwgpu_composite_rows(m_c); }
  int32 planes() const { return 1; }
  int32 levels() const { return vwgpu_composite_levels(m_c); }

  BBox2i const& bbox() const { return m_data; }
  BBox2i const& source_data_bbox() const { return m_view; }

  /// One pixel: the 1 x 1 patch (:274-279).
  pixel_type operator()(int x, int y, int /*p*/ = 0) const { return generate_patch(BBox2i(x, y, 1, 1))(0, 0); }

private:
  void prepare_impl(const int* box) {
    vwgpu_ctx* ctx = engine::thread_context();
    engine::check(ctx, vwgpu_composite_set_draft_mode(ctx, m_c, m_draft ? 1 : 0));
    engine::check(ctx, vwgpu_composite_prepare(ctx, m_c, box));
    read_boxes();
  }
};

}  // namespace mosaic
}  // namespace vw

#endif  // VWLITE_VW_MOSAIC_H
