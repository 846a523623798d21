// transform.hip — vw::transform / TransformView (src/vw/Image/Transform.h:335-387, :401-437) for the closed-form 2-D maps of
// src/vw/Math/Transform.h:231-443: per output pixel p the chain's reverse(p) in double, then the interpolation
// (src/vw/Image/Interpolation.h:75-225) of the edge-extended source (src/vw/Image/EdgeExtension.tcc:47-272), for float
// images with an optional validity mask (PixelMask<float>).  The pure-host entries make the map descriptors and run the
// same map steps on points.  The arithmetic is image_sample.h; tests/refimpl/transform_ref.cc restates all of it and
// DESIGN §4.20 lists what is reproduced.
//
// One lane per output pixel, blocks of TF_BX x TF_BY, a grid-stride loop over the bands of TF_BY rows, no LDS, no atomics.
// The chain (up to four steps) and the parameters arrive by value and are read through scalar loads; the map and the edge
// kind are wave-uniform switches.  A kernel is instantiated per (interpolation, masked): the table tf_kernels.  A lane
// whose taps all lie inside the source loads them plainly (a bicubic row as one 16-byte load); the others go through the
// edge function.  A wavefront's stores are row-contiguous.
#include <cmath>
#include <cstring>

#include "image_sample.h"
#include "vwgpu_internal.h"

namespace {

constexpr int TF_BX = 64, TF_BY = 4;
constexpr int TF_THREADS = TF_BX * TF_BY;

struct tf_args {
  is_src s;
  int w, h, x0, y0;
  int nodata, buffer;   // transform_nodata on; the interpolation's pixel_buffer
  float nodata_value;
  int nodata_valid;
  float* out;
  long long ostride;
  uint8_t* omask;
  long long omstride;
};

template <int INTERP, bool MASKED>
__global__ __launch_bounds__(TF_THREADS) void tf_image_kernel(tf_args a, is_chain chain) {
  const int x = blockIdx.x * TF_BX + threadIdx.x;
  if (x >= a.w) return;
  const long long step = (long long)gridDim.y * TF_BY;
  for (long long y = (long long)blockIdx.y * TF_BY + threadIdx.y; y < a.h; y += step) {
    // TransformView::operator() (Image/Transform.h:362-365)
    const is_v2 q = is_chain_apply(chain, is_v2{(double)((long long)a.x0 + x), (double)((long long)a.y0 + y)});
    float res;
    bool valid;
    if (a.nodata && is_nodata(q, a.buffer, a.s.w, a.s.h)) {
      res = a.nodata_value;
      valid = a.nodata_valid != 0;
    } else {
      res = is_sample<INTERP, MASKED>(a.s, q.x, q.y, valid);
    }
    a.out[y * a.ostride + x] = res;
    if (MASKED) a.omask[y * a.omstride + x] = valid ? 255 : 0;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// the kernels that exist, one row per interpolation: unmasked, masked
using tf_kernel_t = void (*)(tf_args, is_chain);
struct tf_row { int interp, buffer; tf_kernel_t plain, masked; };
#define TF_ROW(INTERP, BUFFER) {INTERP, BUFFER, tf_image_kernel<INTERP, false>, tf_image_kernel<INTERP, true>}
const tf_row tf_kernels[] = {
  TF_ROW(VWGPU_TRANSFORM_INTERP_NEAREST, 1),    // pixel_buffer (Interpolation.h:211, :114, :190)
  TF_ROW(VWGPU_TRANSFORM_INTERP_BILINEAR, 1),
  TF_ROW(VWGPU_TRANSFORM_INTERP_BICUBIC, 2),
};
#undef TF_ROW
const tf_row* tf_row_of(int interp) {
  for (const tf_row& row : tf_kernels)
    if (row.interp == interp) return &row;
  return nullptr;
}

bool tf_finite(const double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

bool tf_step_ok(const vwgpu_transform& t) {
  return t.kind >= VWGPU_TRANSFORM_IDENTITY && t.kind <= VWGPU_TRANSFORM_HOMOGRAPHY && (t.reserved == 0 || t.reserved == 1);
}

// one direction of a descriptor as the arithmetic image_sample.h runs; vwgpu_transform_invert's bit changes the direction
is_step tf_resolve(const vwgpu_transform& t, int direction) {
  const bool reverse = (direction == VWGPU_TRANSFORM_REVERSE) != (t.reserved != 0);
  is_step s{};
  std::memcpy(s.w, reverse ? t.rev : t.fwd, sizeof(s.w));
  switch (t.kind) {
    case VWGPU_TRANSFORM_TRANSLATE: s.op = reverse ? IS_OP_SUB : IS_OP_ADD; break;
    case VWGPU_TRANSFORM_RESAMPLE: s.op = reverse ? IS_OP_DIV : IS_OP_MUL; break;
    case VWGPU_TRANSFORM_AFFINE: s.op = reverse ? IS_OP_AFFINE_PRE : IS_OP_AFFINE_POST; break;
    case VWGPU_TRANSFORM_HOMOGRAPHY: s.op = IS_OP_HOMOGRAPHY; break;
    default: s.op = IS_OP_IDENTITY;
  }
  return s;
}

// compose(tx1, tx2) (Math/Transform.h:437-443): reverse runs the steps in array order, forward from the last to the first
is_chain tf_chain(const vwgpu_transform* steps, int n, int direction) {
  is_chain c{};
  c.n = n;
  for (int k = 0; k < n; ++k) c.s[k] = tf_resolve(steps[direction == VWGPU_TRANSFORM_REVERSE ? k : n - 1 - k], direction);
  return c;
}

// the eight words of an affine map from its matrix and offset; the inverse is the plain adjugate over the determinant
bool tf_affine(double a, double b, double c, double d, double x, double y, vwgpu_transform* out) {
  const double det = a * d - b * c;
  if (det == 0 || !std::isfinite(det)) return false;
  vwgpu_transform t{};
  t.kind = VWGPU_TRANSFORM_AFFINE;
  t.fwd[0] = a; t.fwd[1] = b; t.fwd[2] = c; t.fwd[3] = d; t.fwd[4] = x; t.fwd[5] = y;
  t.rev[0] = d / det; t.rev[1] = -b / det; t.rev[2] = -c / det; t.rev[3] = a / det; t.rev[4] = x; t.rev[5] = y;
  *out = t;
  return true;
}

struct tf_image_call {
  const float* src; int sw, sh; ptrdiff_t sstride;
  const uint8_t* smask; ptrdiff_t mstride;
  const vwgpu_transform* steps; int n_steps;
  const vwgpu_transform_params* params;
  int w, h, x0, y0;
  float* out; ptrdiff_t ostride;
  uint8_t* omask; ptrdiff_t omstride;
};

int tf_image_check(vwgpu_ctx* ctx, tf_image_call& c) {
  const char* name = "transform_image";
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!c.src || !c.out || !c.steps || !c.params || c.sw <= 0 || c.sh <= 0 || c.w <= 0 || c.h <= 0)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: empty image or null pointer", name);
  if (c.n_steps < 1 || c.n_steps > 4) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: a chain has 1 to 4 steps, not %d", name, c.n_steps);
  for (int k = 0; k < c.n_steps; ++k)
    if (!tf_step_ok(c.steps[k])) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: step %d is no vwgpu_transform (kind %d)", name, k, c.steps[k].kind);
  const vwgpu_transform_params& P = *c.params;
  if (!tf_row_of(P.interp)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: interpolation %d out of range", name, P.interp);
  if (P.edge < VWGPU_TRANSFORM_EDGE_ZERO || P.edge > VWGPU_TRANSFORM_EDGE_LINEAR)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: edge extension %d out of range", name, P.edge);
  if ((c.smask != nullptr) != (c.omask != nullptr))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: a source mask and an output mask go together", name);
  if (c.sstride == 0) c.sstride = c.sw;
  if (c.mstride == 0) c.mstride = c.sw;
  if (c.ostride == 0) c.ostride = c.w;
  if (c.omstride == 0) c.omstride = c.w;
  if (c.sstride < c.sw || (c.smask && c.mstride < c.sw) || c.ostride < c.w || (c.omask && c.omstride < c.w))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
  if ((const void*)c.out == (const void*)c.src || (const void*)c.out == (const void*)c.smask ||
      (c.omask && ((const void*)c.omask == (const void*)c.src || c.omask == c.smask || (const void*)c.omask == (const void*)c.out)))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: an output must not be an input or the other output", name);
  if (P.edge == VWGPU_TRANSFORM_EDGE_VALUE && P.edge_valid && std::isnan(P.edge_value))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: a valid edge pixel must not be NaN", name);
  if (P.nodata && P.nodata_valid && std::isnan(P.nodata_value))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: a valid nodata pixel must not be NaN", name);
  if (P.edge == VWGPU_TRANSFORM_EDGE_REFLECT && (c.sw < 2 || c.sh < 2 || c.sw > (1 << 30) || c.sh > (1 << 30)))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: ReflectEdgeExtension needs a source of 2 x 2 to 2^30 x 2^30 (its period is 2 n - 2)", name);
  if (P.edge == VWGPU_TRANSFORM_EDGE_LINEAR && (c.sw < 2 || c.sh < 2))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: LinearEdgeExtension needs a source of at least 2 x 2", name);
  if (P.edge == VWGPU_TRANSFORM_EDGE_LINEAR && c.smask)
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: LinearEdgeExtension of a masked image is not implemented", name);
  return VWGPU_OK;
}

// all pointers of `c` are device pointers here
int tf_image_run(vwgpu_ctx* ctx, const tf_image_call& c) {
  const vwgpu_transform_params& P = *c.params;
  const tf_row* row = tf_row_of(P.interp);
  const bool value = P.edge == VWGPU_TRANSFORM_EDGE_VALUE;
  tf_args a{};
  a.s = is_src{c.src, (long long)c.sstride, c.sw, c.sh, c.smask, (long long)c.mstride, P.edge, value ? P.edge_value : 0.0f,
               value && P.edge_valid != 0};
  a.w = c.w; a.h = c.h; a.x0 = c.x0; a.y0 = c.y0;
  a.nodata = P.nodata != 0; a.buffer = row->buffer;
  a.nodata_value = P.nodata_value; a.nodata_valid = P.nodata_valid != 0;
  a.out = c.out; a.ostride = (long long)c.ostride;
  a.omask = c.omask; a.omstride = (long long)c.omstride;
  const is_chain chain = tf_chain(c.steps, c.n_steps, VWGPU_TRANSFORM_REVERSE);
  const long long bands = ((long long)c.h + TF_BY - 1) / TF_BY;
  const dim3 grid((unsigned)((c.w + TF_BX - 1) / TF_BX), (unsigned)(bands < 65535 ? bands : 65535));
  vwgpu_prof_scope ps(ctx, "transform_image");
  hipLaunchKernelGGL(c.smask ? row->masked : row->plain, grid, dim3(TF_BX, TF_BY), 0, ctx->stream, a, chain);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------------

extern "C" {

int vwgpu_transform_make(int kind, const double* params, int n, vwgpu_transform* out) {
  if (!out || (!params && n != 0) || n < 0 || n > 9 || !tf_finite(params, n)) return VWGPU_ERR_ARGUMENT;
  vwgpu_transform t{};
  t.kind = kind;
  switch (kind) {
    case VWGPU_TRANSFORM_IDENTITY:
      if (n != 0) return VWGPU_ERR_ARGUMENT;
      break;
    case VWGPU_TRANSFORM_TRANSLATE:
    case VWGPU_TRANSFORM_RESAMPLE:
      if (n != 2 || (kind == VWGPU_TRANSFORM_RESAMPLE && (params[0] == 0 || params[1] == 0))) return VWGPU_ERR_ARGUMENT;
      t.fwd[0] = t.rev[0] = params[0];
      t.fwd[1] = t.rev[1] = params[1];
      break;
    case VWGPU_TRANSFORM_AFFINE:
      if (n != 6 || !tf_affine(params[0], params[1], params[2], params[3], params[4], params[5], &t)) return VWGPU_ERR_ARGUMENT;
      break;
    case VWGPU_TRANSFORM_HOMOGRAPHY: {
      if (n != 9) return VWGPU_ERR_ARGUMENT;
      const double a = params[0], b = params[1], c = params[2], d = params[3], e = params[4], f = params[5], g = params[6], h = params[7],
                   i = params[8];
      const double adj[9] = {e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f,
                             d * h - e * g, b * g - a * h, a * e - b * d};
      const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
      if (det == 0 || !std::isfinite(det)) return VWGPU_ERR_ARGUMENT;
      for (int k = 0; k < 9; ++k) {
        t.fwd[k] = params[k];
        t.rev[k] = adj[k] / det;
      }
      break;
    }
    default: return VWGPU_ERR_ARGUMENT;
  }
  *out = t;
  return VWGPU_OK;
}

int vwgpu_transform_rotate(double theta, double cx, double cy, vwgpu_transform* out) {
  if (!out || !std::isfinite(theta) || !std::isfinite(cx) || !std::isfinite(cy)) return VWGPU_ERR_ARGUMENT;
  // RotateTransform (Math/Transform.h:351-362)
  const double c = std::cos(theta), s = std::sin(theta);
  const double ra = c, rb = -s, rc = s, rd = c;
  const double x = cx - (ra * cx + rb * cy), y = cy - (rc * cx + rd * cy);
  return tf_affine(ra, rb, rc, rd, x, y, out) ? VWGPU_OK : VWGPU_ERR_ARGUMENT;
}

int vwgpu_transform_invert(const vwgpu_transform* in, vwgpu_transform* out) {
  if (!in || !out || !tf_step_ok(*in)) return VWGPU_ERR_ARGUMENT;
  vwgpu_transform t = *in;
  t.reserved ^= 1;
  *out = t;
  return VWGPU_OK;
}

int vwgpu_transform_points(const vwgpu_transform* steps, int n_steps, int direction, const double* points, long long count, double* out) {
  if (!steps || n_steps < 1 || n_steps > 4 || count < 0 || (count > 0 && (!points || !out))) return VWGPU_ERR_ARGUMENT;
  if (direction != VWGPU_TRANSFORM_FORWARD && direction != VWGPU_TRANSFORM_REVERSE) return VWGPU_ERR_ARGUMENT;
  for (int k = 0; k < n_steps; ++k)
    if (!tf_step_ok(steps[k])) return VWGPU_ERR_ARGUMENT;
  const is_chain chain = tf_chain(steps, n_steps, direction);
  for (long long i = 0; i < count; ++i) {
    const is_v2 q = is_chain_apply(chain, is_v2{points[2 * i], points[2 * i + 1]});
    out[2 * i] = q.x;
    out[2 * i + 1] = q.y;
  }
  return VWGPU_OK;
}

int vwgpu_transform_image_dev(vwgpu_ctx* ctx, const float* d_src, int sw, int sh, ptrdiff_t sstride, const uint8_t* d_src_mask,
                              ptrdiff_t mstride, const vwgpu_transform* steps, int n_steps, const vwgpu_transform_params* params, int w,
                              int h, int x0, int y0, float* d_out, ptrdiff_t ostride, uint8_t* d_out_mask, ptrdiff_t omstride) {
  tf_image_call c{d_src, sw, sh, sstride, d_src_mask, mstride, steps, n_steps, params, w, h, x0, y0, d_out, ostride, d_out_mask, omstride};
  int rc = tf_image_check(ctx, c);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return tf_image_run(ctx, c);
}

int vwgpu_transform_image(vwgpu_ctx* ctx, const float* src, int sw, int sh, ptrdiff_t sstride, const uint8_t* src_mask, ptrdiff_t mstride,
                          const vwgpu_transform* steps, int n_steps, const vwgpu_transform_params* params, int w, int h, int x0, int y0,
                          float* out, ptrdiff_t ostride, uint8_t* out_mask, ptrdiff_t omstride) {
  tf_image_call c{src, sw, sh, sstride, src_mask, mstride, steps, n_steps, params, w, h, x0, y0, out, ostride, out_mask, omstride};
  int rc = tf_image_check(ctx, c);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int ps = st.add(src, sw, sh, 4, c.sstride, VWGPU_STAGE_IN), pm = st.add(src_mask, sw, sh, 1, c.mstride, VWGPU_STAGE_IN),
            po = st.add(out, w, h, 4, c.ostride, VWGPU_STAGE_OUT), pk = st.add(out_mask, w, h, 1, c.omstride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  tf_image_call d = c;
  d.src = st.dev<float>(ps); d.sstride = sw;
  d.smask = st.dev<uint8_t>(pm); d.mstride = sw;
  d.out = st.dev<float>(po); d.ostride = w;
  d.omask = st.dev<uint8_t>(pk); d.omstride = w;
  if ((rc = tf_image_run(ctx, d))) return rc;
  return st.finish();
}

}  // extern "C"
