// mosaic.hip — vw::mosaic::ImageComposite (src/vw/Mosaic/ImageComposite.h) for float pixels with premultiplied alpha:
// grassfire-weighted masks (:331-369), the Burt-Adelson pyramid of every image (:373-408), blend_patch (:468-567) and
// draft_patch (:573-590), every image device resident.  DESIGN.md section 4.24; tests/refimpl/mosaic_ref.cc restates it.
//
// What the reference rasterises one view at a time is fused per output pixel:
//   mo_mask_kernel      a pixel of image p against a table of the overlapping images' grassfire planes
//   mo_reduce_kernel    PositionedImage::reduce(): zero pad, [.25 .5 .25] x [.25 .5 .25], subsample, constant extend
//   mo_laplace_kernel   unpremultiply, expand the level below, subtract, multiply by the mask
//   mo_collapse_kernel  one level of blend_patch: the sums over the images in insertion order inside the thread (no atomics),
//                       the safe quotient, plus the expanded level above
//   mo_trim_kernel      the division by alpha (fill_holes) or the trim to the largest source alpha
//   mo_draft_kernel     draft_patch: the overlay in insertion order
// Every float operation is rounded on its own (-ffp-contract=off) in the reference's order.  The unpremultiplied images
// are never stored: the Gaussian chain stays premultiplied and its readers divide on load.
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "image_sample.h"
#include "vwgpu_internal.h"

namespace {

struct mo_box {
  int x0, y0, x1, y1;
  int w() const { return x1 - x0; }
  int h() const { return y1 - y0; }
  bool empty() const { return x0 >= x1 || y0 >= y1; }                                                   // BBox.tcc:156-160
  bool intersects(const mo_box& b) const { return !(x0 >= b.x1 || x1 <= b.x0 || y0 >= b.y1 || y1 <= b.y0); }   // :142-151
};

// ---- pixels -----------------------------------------------------------------------------------------------------------
template <int C> struct mo_px { float v[C]; };
typedef float mo_f2 __attribute__((ext_vector_type(2), aligned(4)));   // one 8- / 16-byte access at 4-byte alignment
typedef float mo_f4 __attribute__((ext_vector_type(4), aligned(4)));

template <int C> __device__ __forceinline__ mo_px<C> mo_load(const float* p);
template <> __device__ __forceinline__ mo_px<1> mo_load<1>(const float* p) { return mo_px<1>{{p[0]}}; }
template <> __device__ __forceinline__ mo_px<2> mo_load<2>(const float* p) {
  const mo_f2 q = *reinterpret_cast<const mo_f2*>(p);
  return mo_px<2>{{q.x, q.y}};
}
template <> __device__ __forceinline__ mo_px<4> mo_load<4>(const float* p) {
  const mo_f4 q = *reinterpret_cast<const mo_f4*>(p);
  return mo_px<4>{{q.x, q.y, q.z, q.w}};
}
template <int C> __device__ __forceinline__ void mo_store(float* p, const mo_px<C>& v);
template <> __device__ __forceinline__ void mo_store<1>(float* p, const mo_px<1>& v) { p[0] = v.v[0]; }
template <> __device__ __forceinline__ void mo_store<2>(float* p, const mo_px<2>& v) {
  mo_f2 q; q.x = v.v[0]; q.y = v.v[1];
  *reinterpret_cast<mo_f2*>(p) = q;
}
template <> __device__ __forceinline__ void mo_store<4>(float* p, const mo_px<4>& v) {
  mo_f4 q; q.x = v.v[0]; q.y = v.v[1]; q.z = v.v[2]; q.w = v.v[3];
  *reinterpret_cast<mo_f4*>(p) = q;
}
template <int C> __device__ __forceinline__ mo_px<C> mo_zero() {
  mo_px<C> r;
#pragma unroll
  for (int c = 0; c < C; ++c) r.v[c] = 0.0f;
  return r;
}
// pixel / scalar with ArgArgSafeQuotientFunctor (src/vw/Core/Functors.h:415-421, :454-460)
template <int C> __device__ __forceinline__ mo_px<C> mo_safe_div(const mo_px<C>& p, float d) {
  if (d == 0.0f) return mo_zero<C>();
  mo_px<C> r;
#pragma unroll
  for (int c = 0; c < C; ++c) r.v[c] = p.v[c] / d;
  return r;
}
// pixel (x, y) of a dense image of w columns; UNPRE: image /= select_alpha_channel(image) on load (:92-94)
template <int C, bool UNPRE> __device__ __forceinline__ mo_px<C> mo_at(const float* img, int w, int x, int y) {
  const mo_px<C> p = mo_load<C>(img + ((long long)y * w + x) * C);
  return UNPRE ? mo_safe_div<C>(p, p.v[C - 1]) : p;
}

// pixel (X, Y) of resample(img, 2): ResampleTransform::reverse, BilinearInterpolation over ConstantEdgeExtension
// (src/vw/Image/Transform.h:702-709); 0 <= X < 2 w, 0 <= Y < 2 h
template <int C, bool UNPRE> __device__ __forceinline__ mo_px<C> mo_expand(const float* img, int w, int h, int X, int Y) {
  const double qx = X / 2.0, qy = Y / 2.0;
  const int xi = (int)floor(qx), yi = (int)floor(qy);
  if ((double)xi == qx && (double)yi == qy) return mo_at<C, UNPRE>(img, w, xi, yi);
  const float normx = (float)qx - (float)xi, normy = (float)qy - (float)yi;
  const int xa = is_clamp(xi, w), xb = is_clamp(xi + 1, w), ya = is_clamp(yi, h), yb = is_clamp(yi + 1, h);
  const mo_px<C> t00 = mo_at<C, UNPRE>(img, w, xa, ya), t10 = mo_at<C, UNPRE>(img, w, xb, ya);
  const mo_px<C> t01 = mo_at<C, UNPRE>(img, w, xa, yb), t11 = mo_at<C, UNPRE>(img, w, xb, yb);
  mo_px<C> r;
#pragma unroll
  for (int c = 0; c < C; ++c) r.v[c] = is_bilinear_mix(t00.v[c], t10.v[c], t01.v[c], t11.v[c], normx, normy);
  return r;
}

const dim3 mo_block(64, 4);
dim3 mo_grid(int w, int h) { return dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)); }

// ---- masks (generate_masks, :331-369) -----------------------------------------------------------------------------------
template <int C> __global__ void mo_alpha_kernel(const float* __restrict__ src, int w, int h, float* __restrict__ alpha) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  alpha[(long long)y * w + x] = src[((long long)y * w + x) * C + (C - 1)];
}

constexpr int MO_MASK_TAB = 8;
struct mo_mask_entry { const int32_t* g; int ox, oy, w, h, later, pad; };
struct mo_mask_tab { int n, first; mo_mask_entry e[MO_MASK_TAB]; };
// mask = 1 where the grassfire of image p is positive and no other image beats it: a larger distance, or an equal one in an image
// inserted later (:354-356, then threshold()).  first == 0: a further table of the same image, the mask only loses pixels.
__global__ void mo_mask_kernel(const int32_t* __restrict__ g, int w, int h, mo_mask_tab t, float* __restrict__ mask) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  const long long at = (long long)y * w + x;
  const int gp = g[at];
  bool keep = t.first ? gp > 0 : mask[at] != 0.0f;
  for (int k = 0; k < t.n; ++k) {
    const mo_mask_entry& e = t.e[k];
    const int i = x - e.ox, j = y - e.oy;
    if (i < 0 || j < 0 || i >= e.w || j >= e.h) continue;
    const int gq = e.g[(long long)j * e.w + i];
    if (gq > gp || (gq == gp && e.later)) keep = false;
  }
  mask[at] = keep ? 1.0f : 0.0f;
}

// ---- PositionedImage::reduce() (:68-90) -----------------------------------------------------------------------------------
struct mo_reduce_args {
  const float* src; int w, h;     // the image
  int left, top, pw, ph;          // the zero-padded view: pixel (X, Y) is src(X - left, Y - top), zero outside either
  int sw, sh;                     // the subsampled raster, 1 + (pw - 1) / 2
  float* dst; int nw, nh;         // new_bbox's size
};
template <int C, bool UNPRE> __device__ __forceinline__ mo_px<C> mo_padded(const mo_reduce_args& a, int X, int Y) {
  const int x = X - a.left, y = Y - a.top;
  if (X < 0 || Y < 0 || X >= a.pw || Y >= a.ph || x < 0 || y < 0 || x >= a.w || y >= a.h) return mo_zero<C>();
  return mo_at<C, UNPRE>(a.src, a.w, x, y);
}
// correlate_1d_at_point (src/vw/Image/Convolution.h:53-64) along x, then along y: from zero, one product added at a time
template <int C, bool UNPRE> __global__ void mo_reduce_kernel(mo_reduce_args a) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
  if (i >= a.nw || j >= a.nh) return;
  const int X = 2 * min(i, a.sw - 1), Y = 2 * min(j, a.sh - 1);   // ConstantEdgeExtension of the subsampled raster
  const float k[3] = {0.25f, 0.5f, 0.25f};
  mo_px<C> acc = mo_zero<C>();
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    mo_px<C> row = mo_zero<C>();
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const mo_px<C> p = mo_padded<C, UNPRE>(a, X - 1 + t, Y - 1 + r);
#pragma unroll
      for (int c = 0; c < C; ++c) row.v[c] += k[t] * p.v[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc.v[c] += k[r] * row.v[c];
  }
  mo_store<C>(a.dst + ((long long)j * a.nw + i) * C, acc);
}

// ---- one level of PyramidGenerator::generate (:393-406) -------------------------------------------------------------------
struct mo_laplace_args {
  const float* high; int hw, hh, hbx, hby;   // image_high and its box
  const float* low; int lw, lh, lbx, lby;    // image_low before unpremultiply(), nullptr at the last level
  const float* mask; int mw, mh, mbx, mby;
  float* diff;
};
template <int C, bool UNPRE_HIGH> __global__ void mo_laplace_kernel(mo_laplace_args a) {
  const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
  if (i >= a.hw || j >= a.hh) return;
  mo_px<C> p = mo_at<C, UNPRE_HIGH>(a.high, a.hw, i, j);
  if (a.low) {   // subtract_expanded (:121-123): the expanded image through ZeroEdgeExtension at bbox - 2 * other.bbox.min()
    const int X = i + a.hbx - 2 * a.lbx, Y = j + a.hby - 2 * a.lby;
    mo_px<C> e = mo_zero<C>();
    if (X >= 0 && Y >= 0 && X < 2 * a.lw && Y < 2 * a.lh) e = mo_expand<C, true>(a.low, a.lw, a.lh, X, Y);
#pragma unroll
    for (int c = 0; c < C; ++c) p.v[c] = p.v[c] - e.v[c];
  }
  const int mx = i + a.hbx - a.mbx, my = j + a.hby - a.mby;   // operator*= (:125-129)
  const float m = mx >= 0 && my >= 0 && mx < a.mw && my < a.mh ? a.mask[(long long)my * a.mw + mx] : 0.0f;
#pragma unroll
  for (int c = 0; c < C; ++c) p.v[c] = p.v[c] * m;
  mo_store<C>(a.diff + ((long long)j * a.hw + i) * C, p);
}

// ---- blend_patch (:468-567) and draft_patch (:573-590) --------------------------------------------------------------------
struct mo_img_ref { const float* a; const float* b; int x0, y0, w, h; };          // a box of one level and what lies in it
struct mo_img_tab { int n, pad; mo_img_ref e[VWGPU_COMPOSITE_MAX_IMAGES]; };      // in insertion order

struct mo_collapse_args {
  int ox, oy, w, h;                          // bbox_pyr[l]
  const float* upper; int uw, uh, offx, offy;   // the composite of level l + 1 (nullptr at the top) and the crop's origin in its expansion
  float* out; long long ostride;             // pixels
};
// sum_pyr[l] and msum_pyr[l] of a pixel (addto, :96-119, in insertion order), sum / msum, plus the expanded composite (:525-535)
template <int C> __global__ void mo_collapse_kernel(mo_collapse_args a, mo_img_tab t) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= a.w || y >= a.h) return;
  mo_px<C> sum = mo_zero<C>();
  float msum = 0.0f;
  for (int k = 0; k < t.n; ++k) {
    const mo_img_ref& e = t.e[k];
    const int i = x + a.ox - e.x0, j = y + a.oy - e.y0;
    if (i < 0 || j < 0 || i >= e.w || j >= e.h) continue;
    const mo_px<C> d = mo_at<C, false>(e.a, e.w, i, j);
#pragma unroll
    for (int c = 0; c < C; ++c) sum.v[c] += d.v[c];
    msum += e.b[(long long)j * e.w + i];
  }
  const mo_px<C> q = mo_safe_div<C>(sum, msum);
  mo_px<C> r = mo_zero<C>();
  if (a.upper) r = mo_expand<C, false>(a.upper, a.uw, a.uh, x + a.offx, y + a.offy);
#pragma unroll
  for (int c = 0; c < C; ++c) r.v[c] += q.v[c];
  mo_store<C>(a.out + ((long long)y * a.ostride + x) * C, r);
}

// composite /= alpha (:537-539), or composite *= max_p alpha_p / alpha (:541-564); in place on the patch at (ox, oy)
template <int C> __global__ void mo_trim_kernel(float* out, long long ostride, int ox, int oy, int w, int h, int fill_holes, mo_img_tab t) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  float* at = out + ((long long)y * ostride + x) * C;
  mo_px<C> p = mo_load<C>(at);
  if (fill_holes) {
    p = mo_safe_div<C>(p, p.v[C - 1]);
  } else {
    float alpha = 0.0f;
    for (int k = 0; k < t.n; ++k) {
      const mo_img_ref& e = t.e[k];
      const int i = x + ox - e.x0, j = y + oy - e.y0;
      if (i < 0 || j < 0 || i >= e.w || j >= e.h) continue;
      const float s = e.a[((long long)j * e.w + i) * C + (C - 1)];
      if (s > alpha) alpha = s;
    }
    const float f = p.v[C - 1] == 0.0f ? 0.0f : alpha / p.v[C - 1];
#pragma unroll
    for (int c = 0; c < C; ++c) p.v[c] = p.v[c] * f;
  }
  mo_store<C>(at, p);
}

// the overlay of addto (:103-115): dest *= 1.0 - alpha / (double)1.0 in double, cast back, then dest += image; without alpha the
// later image overwrites
template <int C> __global__ void mo_draft_kernel(float* out, long long ostride, int ox, int oy, int w, int h, mo_img_tab t) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  mo_px<C> d = mo_zero<C>();
  for (int k = 0; k < t.n; ++k) {
    const mo_img_ref& e = t.e[k];
    const int i = x + ox - e.x0, j = y + oy - e.y0;
    if (i < 0 || j < 0 || i >= e.w || j >= e.h) continue;
    const mo_px<C> p = mo_at<C, false>(e.a, e.w, i, j);
    if (C == 1) {
      d = p;
    } else {
      const double f = 1.0 - (double)p.v[C - 1] / 1.0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        d.v[c] = (float)((double)d.v[c] * f);
        d.v[c] += p.v[c];
      }
    }
  }
  mo_store<C>(out + ((long long)y * ostride + x) * C, d);
}

// ---- host: the box arithmetic ------------------------------------------------------------------------------------------------
struct mo_pos { int cols, rows; mo_box box; };   // a PositionedImage without its pixels: the canvas and the image's box in it
struct mo_reduce_plan { int left, top, right, bottom, pw, ph, sw, sh; mo_pos next; };
// :69-89 word for word; the boxes lie at non-negative coordinates, so / and % act on non-negative numbers
mo_reduce_plan mo_plan_reduce(const mo_pos& p) {
  const int border = 1;
  const mo_box& b = p.box;
  mo_reduce_plan r;
  r.left = std::min(border + (b.x0 + border) % 2, b.x0);
  r.top = std::min(border + (b.y0 + border) % 2, b.y0);
  r.right = std::min(border + (b.w() + r.left + border) % 2, p.cols - b.x0 - b.w());
  r.bottom = std::min(border + (b.h() + r.top + border) % 2, p.rows - b.y0 - b.h());
  r.next.box.x0 = (b.x0 - r.left) / 2;
  r.next.box.y0 = (b.y0 - r.top) / 2;
  r.next.box.x1 = r.next.box.x0 + (b.w() + r.left + r.right + 1) / 2 + 1;
  r.next.box.y1 = r.next.box.y0 + (b.h() + r.top + r.bottom + 1) / 2 + 1;
  r.next.cols = (p.cols + 1) / 2;
  r.next.rows = (p.rows + 1) / 2;
  r.pw = b.w() + r.left + r.right;
  r.ph = b.h() + r.top + r.bottom;
  r.sw = 1 + (r.pw - 1) / 2;   // SubsampleView::cols()
  r.sh = 1 + (r.ph - 1) / 2;
  return r;
}

struct mo_plane { float* px = nullptr; mo_pos pos; };
struct mo_image {
  float* src = nullptr;      // w x h pixels of `channels` floats, dense
  int w = 0, h = 0;
  mo_box box;                // as inserted; translated to the view by prepare
  float* pyr = nullptr;      // one block: mask[0], then per level diff[l], and mask[l] for l > 0
  std::vector<mo_plane> diff, mask;
};

}  // namespace

struct vwgpu_composite {
  int device = 0;
  int channels = 0;
  bool draft = false, fill_holes = false, prepared = false, masks_ready = false, pyr_ready = false, pyr_fill = false;
  mo_box view, data;
  int mindim = 0, levels = 0;
  std::vector<mo_image> img;
  size_t bytes = 0;                 // device bytes held
  float* scratch = nullptr;         // grow-only: the Gaussian chain of one image / the upper composites of one patch
  size_t scratch_cap = 0;
};

namespace {

int mo_check(vwgpu_ctx* ctx, const vwgpu_composite* c, const char* who) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!c) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: null composite", who);
  if (c->device != ctx->device) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: the composite lives on device %d, the context on %d", who, c->device, ctx->device);
  return VWGPU_OK;
}

int mo_alloc(vwgpu_ctx* ctx, vwgpu_composite* c, size_t bytes, float** out) {
  if (c->bytes + bytes > (size_t)VWGPU_COMPOSITE_MAX_BYTES)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "composite: more than %llu device bytes", (unsigned long long)VWGPU_COMPOSITE_MAX_BYTES);
  void* p = nullptr;
  VWGPU_HIP(ctx, hipMalloc(&p, std::max<size_t>(bytes, 256)));
  c->bytes += bytes;
  *out = static_cast<float*>(p);
  return VWGPU_OK;
}
void mo_free(vwgpu_composite* c, float*& p, size_t bytes) {
  if (!p) return;
  (void)hipFree(p);
  p = nullptr;
  c->bytes -= bytes;
}
// Work queued on the stream may still read the old block: wait before it goes.
int mo_scratch(vwgpu_ctx* ctx, vwgpu_composite* c, size_t bytes) {
  if (bytes <= c->scratch_cap) return VWGPU_OK;
  VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
  mo_free(c, c->scratch, c->scratch_cap);
  c->scratch_cap = 0;
  int rc = mo_alloc(ctx, c, bytes, &c->scratch);
  if (rc) return rc;
  c->scratch_cap = bytes;
  return VWGPU_OK;
}
size_t mo_plane_floats(const mo_pos& p, int channels) { return vwgpu_align_up((size_t)p.box.w() * p.box.h() * channels, 64); }

void mo_drop_pyramids(vwgpu_composite* c) {
  for (mo_image& im : c->img) {
    size_t fl = 0;
    for (const mo_plane& d : im.diff) fl += mo_plane_floats(d.pos, c->channels);
    for (const mo_plane& m : im.mask) fl += mo_plane_floats(m.pos, 1);
    mo_free(c, im.pyr, fl * sizeof(float));
    im.diff.clear();
    im.mask.clear();
  }
  c->masks_ready = c->pyr_ready = false;
}

template <int C>
void mo_launch_reduce(hipStream_t s, const mo_plane& in, const mo_reduce_plan& rp, float* dst, bool unpre) {
  mo_reduce_args a;
  a.src = in.px; a.w = in.pos.box.w(); a.h = in.pos.box.h();
  a.left = rp.left; a.top = rp.top; a.pw = rp.pw; a.ph = rp.ph; a.sw = rp.sw; a.sh = rp.sh;
  a.dst = dst; a.nw = rp.next.box.w(); a.nh = rp.next.box.h();
  if (unpre) hipLaunchKernelGGL((mo_reduce_kernel<C, true>), mo_grid(a.nw, a.nh), mo_block, 0, s, a);
  else hipLaunchKernelGGL((mo_reduce_kernel<C, false>), mo_grid(a.nw, a.nh), mo_block, 0, s, a);
}

// The level plan of one image: the boxes of image_high / the mask at every level (they reduce alike)
int mo_plan_levels(vwgpu_ctx* ctx, const vwgpu_composite* c, const mo_image& im, std::vector<mo_pos>* pos, std::vector<mo_reduce_plan>* plans) {
  mo_pos p{c->view.w(), c->view.h(), im.box};
  for (int l = 0; l < c->levels; ++l) {
    pos->push_back(p);
    if (l + 1 == c->levels) break;
    const mo_reduce_plan rp = mo_plan_reduce(p);
    if (rp.pw < 1 || rp.ph < 1) return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "composite: level %d of an image has an empty padded view", l + 1);
    plans->push_back(rp);
    p = rp.next;
  }
  return VWGPU_OK;
}

// generate_masks for every image, into mask[0] of its pyramid block (allocated here with the whole pyramid)
int mo_make_masks(vwgpu_ctx* ctx, vwgpu_composite* c) {
  hipStream_t s = ctx->stream;
  const int n = (int)c->img.size();
  // the pyramid blocks
  for (mo_image& im : c->img) {
    std::vector<mo_pos> pos;
    std::vector<mo_reduce_plan> plans;
    int rc = mo_plan_levels(ctx, c, im, &pos, &plans);
    if (rc) return rc;
    size_t fl = 0;
    for (const mo_pos& p : pos) fl += mo_plane_floats(p, c->channels) + mo_plane_floats(p, 1);
    if ((rc = mo_alloc(ctx, c, fl * sizeof(float), &im.pyr))) return rc;
    float* at = im.pyr;
    im.diff.resize(pos.size());
    im.mask.resize(pos.size());
    for (size_t l = 0; l < pos.size(); ++l) {
      im.mask[l].pos = im.diff[l].pos = pos[l];
      im.mask[l].px = at; at += mo_plane_floats(pos[l], 1);
      im.diff[l].px = at; at += mo_plane_floats(pos[l], c->channels);
    }
  }
  // the grassfire planes of all images (int32), and one alpha plane at a time, in the scratch block
  std::vector<size_t> goff(n);
  size_t words = 0, largest = 0;
  for (int p = 0; p < n; ++p) {
    goff[p] = words;
    const size_t px = vwgpu_align_up((size_t)c->img[p].w * c->img[p].h, 64);
    words += px;
    largest = std::max(largest, px);
  }
  int rc = mo_scratch(ctx, c, (words + largest) * sizeof(float));
  if (rc) return rc;
  int32_t* g = reinterpret_cast<int32_t*>(c->scratch);
  float* alpha = c->scratch + words;
  for (int p = 0; p < n; ++p) {
    const mo_image& im = c->img[p];
    if (c->channels == 2) hipLaunchKernelGGL(mo_alpha_kernel<2>, mo_grid(im.w, im.h), mo_block, 0, s, im.src, im.w, im.h, alpha);
    else hipLaunchKernelGGL(mo_alpha_kernel<4>, mo_grid(im.w, im.h), mo_block, 0, s, im.src, im.w, im.h, alpha);
    if ((rc = vwgpu_grassfire_dev(ctx, VWGPU_GRASSFIRE_F32, alpha, im.w, im.h, im.w, 0, g + goff[p], im.w))) return rc;
  }
  for (int p1 = 0; p1 < n; ++p1) {
    const mo_image& a = c->img[p1];
    mo_mask_tab t;
    t.n = 0; t.first = 1;
    auto flush = [&]() {
      hipLaunchKernelGGL(mo_mask_kernel, mo_grid(a.w, a.h), mo_block, 0, s, g + goff[p1], a.w, a.h, t, c->img[p1].mask[0].px);
      t.n = 0; t.first = 0;
    };
    for (int p2 = 0; p2 < n; ++p2) {
      if (p1 == p2) continue;
      const mo_image& b = c->img[p2];
      const int ox = b.box.x0 - a.box.x0, oy = b.box.y0 - a.box.y0;
      if (ox >= a.w || oy >= a.h || -ox >= b.w || -oy >= b.h) continue;   // :342-345
      t.e[t.n++] = mo_mask_entry{g + goff[p2], ox, oy, b.w, b.h, p2 > p1 ? 1 : 0, 0};
      if (t.n == MO_MASK_TAB) flush();
    }
    if (t.n || t.first) flush();
  }
  VWGPU_HIP(ctx, hipGetLastError());
  c->masks_ready = true;
  return VWGPU_OK;
}

template <int C>
int mo_make_pyramids_c(vwgpu_ctx* ctx, vwgpu_composite* c) {
  hipStream_t s = ctx->stream;
  const bool fill = c->fill_holes;
  // the scratch holds the Gaussian chain G_1 .. G_{levels-1} of the largest image
  std::vector<std::vector<mo_reduce_plan>> plans(c->img.size());
  size_t need = 0;
  for (size_t p = 0; p < c->img.size(); ++p) {
    std::vector<mo_pos> pos;
    int rc = mo_plan_levels(ctx, c, c->img[p], &pos, &plans[p]);
    if (rc) return rc;
    size_t fl = 0;
    for (const mo_reduce_plan& rp : plans[p]) fl += mo_plane_floats(rp.next, C);
    need = std::max(need, fl);
  }
  int rc = mo_scratch(ctx, c, need * sizeof(float));
  if (rc) return rc;
  for (size_t p = 0; p < c->img.size(); ++p) {
    mo_image& im = c->img[p];
    mo_plane high;
    high.px = im.src;
    high.pos = im.diff[0].pos;
    float* at = c->scratch;
    for (int l = 0; l < c->levels; ++l) {
      if (l > 0) mo_launch_reduce<1>(s, im.mask[l - 1], plans[p][l - 1], im.mask[l].px, false);
      mo_plane low;
      if (l < c->levels - 1) {
        const mo_reduce_plan& rp = plans[p][l];
        low.px = at;
        low.pos = rp.next;
        at += mo_plane_floats(rp.next, C);
        mo_launch_reduce<C>(s, high, rp, low.px, l == 0 && fill);   // with fill_holes the source is unpremultiplied first (:382)
      }
      mo_laplace_args a;
      a.high = high.px; a.hw = high.pos.box.w(); a.hh = high.pos.box.h(); a.hbx = high.pos.box.x0; a.hby = high.pos.box.y0;
      a.low = low.px; a.lw = a.lh = a.lbx = a.lby = 0;
      if (low.px) { a.lw = low.pos.box.w(); a.lh = low.pos.box.h(); a.lbx = low.pos.box.x0; a.lby = low.pos.box.y0; }
      const mo_plane& m = im.mask[l];
      a.mask = m.px; a.mw = m.pos.box.w(); a.mh = m.pos.box.h(); a.mbx = m.pos.box.x0; a.mby = m.pos.box.y0;
      a.diff = im.diff[l].px;
      // from level 1 on image_high is the unpremultiplied image_low of the step before (:398-400)
      if (l > 0 || fill) hipLaunchKernelGGL((mo_laplace_kernel<C, true>), mo_grid(a.hw, a.hh), mo_block, 0, s, a);
      else hipLaunchKernelGGL((mo_laplace_kernel<C, false>), mo_grid(a.hw, a.hh), mo_block, 0, s, a);
      high = low;
    }
  }
  VWGPU_HIP(ctx, hipGetLastError());
  c->pyr_ready = true;
  c->pyr_fill = fill;
  return VWGPU_OK;
}

int mo_make_pyramids(vwgpu_ctx* ctx, vwgpu_composite* c) {
  vwgpu_prof_scope ps(ctx, "mosaic_pyramids");
  return c->channels == 2 ? mo_make_pyramids_c<2>(ctx, c) : mo_make_pyramids_c<4>(ctx, c);
}

template <int C>
int mo_blend_patch(vwgpu_ctx* ctx, vwgpu_composite* c, const mo_box& patch, float* d_out, ptrdiff_t ostride) {
  hipStream_t s = ctx->stream;
  const int levels = c->levels;
  std::vector<mo_box> pyr;   // :476-484
  for (int l = 0; l < levels; ++l) {
    if (l == 0) { pyr.push_back(patch); continue; }
    const mo_box& b = pyr[l - 1];
    pyr.push_back(mo_box{b.x0 / 2, b.y0 / 2, b.x0 / 2 + (b.w() + b.x0 % 2) / 2 + 1, b.y0 / 2 + (b.h() + b.y0 % 2) / 2 + 1});
  }
  mo_box padded = patch;   // :488-500
  for (int l = 0; l < levels - 1; ++l) padded = mo_box{padded.x0 / 2, padded.y0 / 2, padded.x1 / 2 + 1, padded.y1 / 2 + 1};
  for (int l = 0; l < levels - 1; ++l) padded = mo_box{2 * padded.x0 - 1, 2 * padded.y0 - 1, 2 * padded.x1, 2 * padded.y1};
  std::vector<int> list;   // a cold cache: insertion order (:504-509)
  for (int p = 0; p < (int)c->img.size(); ++p)
    if (padded.intersects(c->img[p].box)) list.push_back(p);

  std::vector<size_t> off(levels, 0);
  size_t fl = 0;
  for (int l = 1; l < levels; ++l) { off[l] = fl; fl += vwgpu_align_up((size_t)pyr[l].w() * pyr[l].h() * C, 64); }
  int rc = mo_scratch(ctx, c, fl * sizeof(float));
  if (rc) return rc;
  {
    vwgpu_prof_scope ps(ctx, "mosaic_collapse");
    for (int l = levels - 1; l >= 0; --l) {
      mo_img_tab t;
      t.n = 0; t.pad = 0;
      for (int p : list) {
        const mo_plane& d = c->img[p].diff[l];
        t.e[t.n++] = mo_img_ref{d.px, c->img[p].mask[l].px, d.pos.box.x0, d.pos.box.y0, d.pos.box.w(), d.pos.box.h()};
      }
      mo_collapse_args a;
      a.ox = pyr[l].x0; a.oy = pyr[l].y0; a.w = pyr[l].w(); a.h = pyr[l].h();
      a.upper = nullptr; a.uw = a.uh = a.offx = a.offy = 0;
      if (l < levels - 1) {
        a.upper = c->scratch + off[l + 1]; a.uw = pyr[l + 1].w(); a.uh = pyr[l + 1].h();
        a.offx = pyr[l].x0 - 2 * pyr[l + 1].x0; a.offy = pyr[l].y0 - 2 * pyr[l + 1].y0;
      }
      a.out = l == 0 ? d_out : c->scratch + off[l];
      a.ostride = l == 0 ? (long long)ostride : a.w;
      hipLaunchKernelGGL(mo_collapse_kernel<C>, mo_grid(a.w, a.h), mo_block, 0, s, a, t);
    }
  }
  {
    vwgpu_prof_scope ps(ctx, "mosaic_trim");
    mo_img_tab t;
    t.n = 0; t.pad = 0;
    if (!c->fill_holes)
      for (const mo_image& im : c->img)
        if (patch.intersects(im.box)) t.e[t.n++] = mo_img_ref{im.src, nullptr, im.box.x0, im.box.y0, im.w, im.h};
    hipLaunchKernelGGL(mo_trim_kernel<C>, mo_grid(patch.w(), patch.h()), mo_block, 0, s, d_out, (long long)ostride, patch.x0, patch.y0, patch.w(),
                       patch.h(), c->fill_holes ? 1 : 0, t);
  }
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

template <int C>
int mo_draft_patch(vwgpu_ctx* ctx, vwgpu_composite* c, const mo_box& patch, float* d_out, ptrdiff_t ostride) {
  vwgpu_prof_scope ps(ctx, "mosaic_draft");
  mo_img_tab t;
  t.n = 0; t.pad = 0;
  for (const mo_image& im : c->img)
    if (patch.intersects(im.box)) t.e[t.n++] = mo_img_ref{im.src, nullptr, im.box.x0, im.box.y0, im.w, im.h};
  hipLaunchKernelGGL(mo_draft_kernel<C>, mo_grid(patch.w(), patch.h()), mo_block, 0, ctx->stream, d_out, (long long)ostride, patch.x0, patch.y0,
                     patch.w(), patch.h(), t);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int mo_insert_check(vwgpu_ctx* ctx, vwgpu_composite* c, const float* img, int w, int h, ptrdiff_t& stride, int channels, int x, int y) {
  int rc = mo_check(ctx, c, "composite_insert");
  if (rc) return rc;
  if (c->prepared) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_insert: the composite is prepared already");
  if (!img || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_insert: empty image or null pointer");
  if (channels != 1 && channels != 2 && channels != 4) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_insert: %d channels (1, 2 or 4)", channels);
  if (c->channels && channels != c->channels)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_insert: an image of %d channels in a composite of %d", channels, c->channels);
  if (stride == 0) stride = w;
  if (stride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_insert: row stride smaller than row width");
  const long long lim = VWGPU_COMPOSITE_MAX_DIM;
  if (x < -lim || y < -lim || x > lim || y > lim) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_insert: offset (%d, %d) beyond +-%lld", x, y, lim);
  if (w > lim || h > lim || c->img.size() >= (size_t)VWGPU_COMPOSITE_MAX_IMAGES)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "composite_insert: more than %d images or a side above %lld", VWGPU_COMPOSITE_MAX_IMAGES, lim);
  return VWGPU_OK;
}

int mo_insert(vwgpu_ctx* ctx, vwgpu_composite* c, const float* img, int w, int h, ptrdiff_t stride, int channels, int x, int y, hipMemcpyKind kind) {
  int rc = mo_insert_check(ctx, c, img, w, h, stride, channels, x, y);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  mo_image im;
  im.w = w; im.h = h;
  im.box = mo_box{x, y, x + w, y + h};
  const size_t row = (size_t)w * channels * sizeof(float);
  if ((rc = mo_alloc(ctx, c, row * h, &im.src))) return rc;
  hipError_t e = hipMemcpy2DAsync(im.src, row, img, (size_t)stride * channels * sizeof(float), row, h, kind, ctx->stream);
  if (e == hipSuccess && kind == hipMemcpyHostToDevice) e = hipStreamSynchronize(ctx->stream);   // the caller's memory is free on return
  if (e != hipSuccess) {
    mo_free(c, im.src, row * h);
    return vwgpu_fail(ctx, VWGPU_ERR_HIP, "composite_insert: copy failed: %s", hipGetErrorString(e));
  }
  c->channels = channels;
  if (c->img.empty()) {   // :421-430
    c->view = c->data = im.box;
    c->mindim = std::min(w, h);
  } else {
    for (mo_box* b : {&c->view, &c->data}) {
      b->x0 = std::min(b->x0, im.box.x0); b->y0 = std::min(b->y0, im.box.y0);
      b->x1 = std::max(b->x1, im.box.x1); b->y1 = std::max(b->y1, im.box.y1);
    }
    c->mindim = std::min(c->mindim, std::min(w, h));
  }
  c->img.push_back(im);
  return VWGPU_OK;
}

int mo_patch_check(vwgpu_ctx* ctx, vwgpu_composite* c, int x0, int y0, int w, int h, const float* out, ptrdiff_t& ostride) {
  int rc = mo_check(ctx, c, "composite_generate_patch");
  if (rc) return rc;
  if (!c->prepared) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_generate_patch: prepare() has not run");
  if (!out || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_generate_patch: empty patch or null pointer");
  if (x0 < 0 || y0 < 0 || x0 > c->view.w() - w || y0 > c->view.h() - h)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_generate_patch: the patch (%d, %d) %d x %d leaves the %d x %d view", x0, y0, w, h,
                      c->view.w(), c->view.h());
  if (ostride == 0) ostride = w;
  if (ostride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_generate_patch: row stride smaller than row width");
  if (!c->draft && c->channels == 1) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_generate_patch: blending needs an alpha channel");
  if (!c->draft && !c->masks_ready)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_generate_patch: prepare() ran in draft mode and made no masks");
  return VWGPU_OK;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) --------------------------------------------------------------------

extern "C" {

int vwgpu_composite_create(vwgpu_ctx* ctx, vwgpu_composite** out) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!out) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_create: null pointer");
  vwgpu_composite* c = new vwgpu_composite;
  c->device = ctx->device;
  *out = c;
  return VWGPU_OK;
}

void vwgpu_composite_destroy(vwgpu_composite* c) {
  if (!c) return;
  int dev = 0;
  const bool switched = hipGetDevice(&dev) == hipSuccess && dev != c->device && hipSetDevice(c->device) == hipSuccess;
  mo_drop_pyramids(c);
  for (mo_image& im : c->img) (void)hipFree(im.src);
  (void)hipFree(c->scratch);
  if (switched) (void)hipSetDevice(dev);
  delete c;
}

int vwgpu_composite_insert(vwgpu_ctx* ctx, vwgpu_composite* c, const float* img, int w, int h, ptrdiff_t stride, int channels, int x, int y) {
  return mo_insert(ctx, c, img, w, h, stride, channels, x, y, hipMemcpyHostToDevice);
}
int vwgpu_composite_insert_dev(vwgpu_ctx* ctx, vwgpu_composite* c, const float* d_img, int w, int h, ptrdiff_t stride, int channels, int x, int y) {
  return mo_insert(ctx, c, d_img, w, h, stride, channels, x, y, hipMemcpyDeviceToDevice);
}

int vwgpu_composite_set_draft_mode(vwgpu_ctx* ctx, vwgpu_composite* c, int draft_mode) {
  int rc = mo_check(ctx, c, "composite_set_draft_mode");
  if (rc) return rc;
  c->draft = draft_mode != 0;
  return VWGPU_OK;
}
int vwgpu_composite_set_fill_holes(vwgpu_ctx* ctx, vwgpu_composite* c, int fill_holes) {
  int rc = mo_check(ctx, c, "composite_set_fill_holes");
  if (rc) return rc;
  c->fill_holes = fill_holes != 0;
  return VWGPU_OK;
}

int vwgpu_composite_prepare(vwgpu_ctx* ctx, vwgpu_composite* c, const int* total_bbox) {
  int rc = mo_check(ctx, c, "composite_prepare");
  if (rc) return rc;
  if (c->prepared) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_prepare: the composite is prepared already");
  if (c->img.empty()) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_prepare: no image was inserted");
  if (!c->draft && c->channels == 1) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_prepare: blending needs an alpha channel (draft mode takes 1 channel)");
  mo_box view = c->view;
  if (total_bbox) {
    view = mo_box{total_bbox[0], total_bbox[1], total_bbox[2], total_bbox[3]};
    const long long lim = 2LL * VWGPU_COMPOSITE_MAX_DIM;
    if (view.x0 < -lim || view.y0 < -lim || view.x1 > lim || view.y1 > lim)
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_prepare: total_bbox beyond +-%lld", lim);
    if (view.x0 > c->data.x0 || view.y0 > c->data.y0 || view.x1 < c->data.x1 || view.y1 < c->data.y1)
      return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_prepare: total_bbox does not contain every image");
  }
  if (view.w() > 2 * VWGPU_COMPOSITE_MAX_DIM || view.h() > 2 * VWGPU_COMPOSITE_MAX_DIM)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "composite_prepare: a view side above %d", 2 * VWGPU_COMPOSITE_MAX_DIM);
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  // :437-442; the view box itself keeps its place (source_data_bbox())
  const int dx = view.x0, dy = view.y0;
  for (mo_image& im : c->img) im.box = mo_box{im.box.x0 - dx, im.box.y0 - dy, im.box.x1 - dx, im.box.y1 - dy};
  c->data = mo_box{c->data.x0 - dx, c->data.y0 - dy, c->data.x1 - dx, c->data.y1 - dy};
  c->view = view;
  c->levels = (int)floorf(logf((float)c->mindim / 2.0f) / logf(2.0f)) - 1;
  if (c->levels < 1) c->levels = 1;
  c->prepared = true;
  if (c->draft) return VWGPU_OK;
  {
    vwgpu_prof_scope ps(ctx, "mosaic_masks");
    rc = mo_make_masks(ctx, c);
  }
  if (!rc) rc = mo_make_pyramids(ctx, c);
  if (rc) mo_drop_pyramids(c);
  return rc;
}

int vwgpu_composite_cols(const vwgpu_composite* c) { return c ? c->view.w() : 0; }
int vwgpu_composite_rows(const vwgpu_composite* c) { return c ? c->view.h() : 0; }
int vwgpu_composite_levels(const vwgpu_composite* c) { return c && c->prepared ? c->levels : 0; }
int vwgpu_composite_bbox(const vwgpu_composite* c, int which, int* box) {
  if (!c || !box || which < 0 || which > 1 || c->img.empty()) return VWGPU_ERR_ARGUMENT;
  const mo_box& b = which == 0 ? c->data : c->view;
  box[0] = b.x0; box[1] = b.y0; box[2] = b.x1; box[3] = b.y1;
  return VWGPU_OK;
}

int vwgpu_composite_mask(vwgpu_ctx* ctx, vwgpu_composite* c, int index, float* out, ptrdiff_t ostride) {
  int rc = mo_check(ctx, c, "composite_mask");
  if (rc) return rc;
  if (!c->masks_ready) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_mask: no masks (prepare() has not run, or ran in draft mode)");
  if (index < 0 || index >= (int)c->img.size() || !out) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_mask: no image %d, or a null pointer", index);
  const mo_image& im = c->img[index];
  if (ostride == 0) ostride = im.w;
  if (ostride < im.w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "composite_mask: row stride smaller than row width");
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  VWGPU_HIP(ctx, hipMemcpy2DAsync(out, (size_t)ostride * sizeof(float), im.mask[0].px, (size_t)im.w * sizeof(float), (size_t)im.w * sizeof(float), im.h,
                                  hipMemcpyDeviceToHost, ctx->stream));
  VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return VWGPU_OK;
}

int vwgpu_composite_generate_patch_dev(vwgpu_ctx* ctx, vwgpu_composite* c, int x0, int y0, int w, int h, float* d_out, ptrdiff_t ostride) {
  int rc = mo_patch_check(ctx, c, x0, y0, w, h, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  const mo_box patch{x0, y0, x0 + w, y0 + h};
  if (c->draft) {
    switch (c->channels) {
      case 1: return mo_draft_patch<1>(ctx, c, patch, d_out, ostride);
      case 2: return mo_draft_patch<2>(ctx, c, patch, d_out, ostride);
      default: return mo_draft_patch<4>(ctx, c, patch, d_out, ostride);
    }
  }
  if (!c->pyr_ready || c->pyr_fill != c->fill_holes) {   // set_fill_holes after prepare(): the pyramids depend on it (:382)
    if ((rc = mo_make_pyramids(ctx, c))) return rc;
  }
  return c->channels == 2 ? mo_blend_patch<2>(ctx, c, patch, d_out, ostride) : mo_blend_patch<4>(ctx, c, patch, d_out, ostride);
}

int vwgpu_composite_generate_patch(vwgpu_ctx* ctx, vwgpu_composite* c, int x0, int y0, int w, int h, float* out, ptrdiff_t ostride) {
  int rc = mo_patch_check(ctx, c, x0, y0, w, h, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int po = st.add(out, w * c->channels, h, sizeof(float), ostride * c->channels, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = vwgpu_composite_generate_patch_dev(ctx, c, x0, y0, w, h, st.dev<float>(po), w);
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
