// ip_describe.hip — the descriptors ipfind falls back to without OpenCV: SGradDescriptorGenerator
// (src/vw/InterestPoint/Descriptor.h:120-132, :214-255, :416-471) and SGrad2DescriptorGenerator (IntegralDescriptor.h:76-179),
// on one crop of the image as InterestPointDescriptionTask makes it (Descriptor.h:259-301).
//
// The crop may leave the image; it is rasterised with zero extension first, as the reference does, because both generators
// then extend the CROP (SGrad with zeros, SGrad2's integral with its edge words), not the image.
//   SGrad   one wave per point: the 42 x 42 support through the affine map and the bilinear tap into LDS, its 43 x 43 integral
//           image in the reference's order by the same routine as the detector's (ip_integral.h), 45 cells x 4 gradients, the
//           norm summed serially in the reference's order
//   SGrad2  the crop's integral image by one wave, then one wave per point: 144 sample positions x 2 Haar responses into LDS,
//           128 histogram words each summed over its 18 responses in the reference's order, the two norms serially
#include <cmath>

#include "image_sample.h"
#include "ip_haar.h"
#include "ip_integral.h"
#include "vwgpu_internal.h"

namespace {

constexpr int IPS_SUPPORT = 42, IPS_K = 180, IPS2_K = 128;

struct ips_args {
  const float* img; long long stride; int w, h;      // the image
  int cx, cy, cw, ch;                                // the crop
  float* crop;                                       // cw x ch, dense
  float* integ;                                      // (cw + 1) x (ch + 1), dense (SGrad2)
  int n;
  const float *x, *y, *scale, *orientation;
  float* desc; long long dstride;
};

// crop(edge_extend(view, ZeroEdgeExtension()), bounds) (Descriptor.h:290-291)
__global__ void __launch_bounds__(256) ips_crop_kernel(ips_args a) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= a.cw || y >= a.ch) return;
  const int gx = x + a.cx, gy = y + a.cy;
  a.crop[(long long)y * a.cw + x] = gx >= 0 && gy >= 0 && gx < a.w && gy < a.h ? a.img[(long long)gy * a.stride + gx] : 0.0f;
}

__global__ void __launch_bounds__(64) ips_integral_kernel(ips_args a) {
  ipi_wave_integral<true>(a.crop, a.cw, a.cw, a.ch, a.integ, a.cw + 1);
}

// sqrt(float) to the nearest float: the double square root is correctly rounded on the device, and rounding it once more
// to float cannot land on the wrong side (53 >= 2 * 24 + 2); sqrtf itself lowers to v_sqrt_f32 (1 ulp)
__device__ inline float ips_sqrt_rn(float v) { return (float)__dsqrt_rn((double)v); }

__global__ void __launch_bounds__(64) ips_sgrad_kernel(ips_args a) {
  const int p = blockIdx.x, lane = threadIdx.x;
  __shared__ float support[IPS_SUPPORT * IPS_SUPPORT];
  __shared__ float integral[(IPS_SUPPORT + 1) * (IPS_SUPPORT + 1)];
  __shared__ float desc[IPS_K];
  // the points are re-based to the crop as floats (Descriptor.h:284-287)
  const float px = a.x[p] - (float)a.cx, py = a.y[p] - (float)a.cy;
  // get_support (Descriptor.h:239-255) and AffineTransform (Math/Transform.h:317-339, its inverse Matrix.h:2209-2216)
  const float half_size = ((float)(IPS_SUPPORT - 1)) / 2.0f;
  const float scaling = __fdiv_rn(1.0f, a.scale[p]);
  const float nori = -a.orientation[p];
  const double c = cos((double)nori), s = sin((double)nori);
  const double ma = scaling * c, mb = -scaling * s, mc = scaling * s, md = scaling * c;
  const double mx = scaling * (s * py - c * px) + half_size, my = -scaling * (s * px + c * py) + half_size;
  const double det = ma * md - mb * mc;
  const double ai = md / det, bi = -mb / det, ci = -mc / det, di = ma / det;
  is_src src{};
  src.px = a.crop; src.stride = a.cw; src.w = a.cw; src.h = a.ch; src.edge = VWGPU_TRANSFORM_EDGE_ZERO;
  for (int k = lane; k < IPS_SUPPORT * IPS_SUPPORT; k += 64) {
    const int i = k % IPS_SUPPORT, j = k / IPS_SUPPORT;
    const double qx = (double)i - mx, qy = (double)j - my;
    bool valid;
    support[k] = is_sample<VWGPU_TRANSFORM_INTERP_BILINEAR, false>(src, ai * qx + bi * qy, ci * qx + di * qy, valid);
  }
  __syncthreads();
  ipi_wave_integral<false>(support, IPS_SUPPORT, IPS_SUPPORT, IPS_SUPPORT, integral, IPS_SUPPORT + 1);
  __syncthreads();
  const int box_strt[5] = {17, 15, 9, 6, 0}, box_size[5] = {2, 4, 8, 10, 14}, box_half[5] = {1, 2, 4, 5, 7};   // Descriptor.cc:27-29
  if (lane < 45) {
    const int sc = lane / 9, i = (lane % 9) / 3, j = lane % 3;
    const int bh = box_half[sc], x0 = box_strt[sc] + i * box_size[sc], y0 = box_strt[sc] + j * box_size[sc];
    const float inv_bh2 = __fdiv_rn(1.0f, (float)(bh * bh));
    const int W = IPS_SUPPORT + 1;
    // IntegralBlock (IntegralImage.cc:47-53): I(tl) + I(br) - I(tl.x, br.y) - I(br.x, tl.y)
    auto block = [&](int tx, int ty, int bx, int by) {
      float r = integral[ty * W + tx];
      r += integral[by * W + bx];
      r -= integral[by * W + tx];
      r -= integral[ty * W + bx];
      return r;
    };
    const float q0 = block(x0, y0, x0 + bh, y0 + bh), q1 = block(x0 + bh, y0, x0 + 2 * bh, y0 + bh);
    const float q2 = block(x0, y0 + bh, x0 + bh, y0 + 2 * bh), q3 = block(x0 + bh, y0 + bh, x0 + 2 * bh, y0 + 2 * bh);
    desc[lane * 4 + 0] = (q0 - q2) * inv_bh2;
    desc[lane * 4 + 1] = (q1 - q3) * inv_bh2;
    desc[lane * 4 + 2] = (q0 - q1) * inv_bh2;
    desc[lane * 4 + 3] = (q2 - q3) * inv_bh2;
  }
  __syncthreads();
  float sqr_length = 0.0f;      // every lane runs the same serial sum
  for (int k = 0; k < IPS_K; ++k) sqr_length += desc[k] * desc[k];
  float inv = __fdiv_rn(1.0f, ips_sqrt_rn(sqr_length));
  const float ainv = fabsf(inv);
  if (!(ainv >= 1.17549435e-38f && ainv <= 3.40282347e38f)) inv = 0.0f;      // !std::isnormal
  for (int k = lane; k < IPS_K; k += 64) a.desc[p * a.dstride + k] = desc[k] * inv;
}

struct ips2_tables { double box[16][3]; double hist[8][2]; };

__global__ void __launch_bounds__(64) ips_sgrad2_kernel(ips_args a, ips2_tables t) {
  const int p = blockIdx.x, lane = threadIdx.x;
  __shared__ double rx[16 * 18], ry[16 * 18];
  __shared__ float desc[IPS2_K];
  const float px = a.x[p] - (float)a.cx, py = a.y[p] - (float)a.cy;
  const float scale = a.scale[p];
  const float co = (float)cos((double)a.orientation[p]), si = (float)sin((double)a.orientation[p]);
  const double r00 = co, r01 = -si, r10 = si, r11 = co;      // Matrix2x2 rotate(co, -si, si, co)
  is_src src{};
  src.px = a.integ; src.stride = a.cw + 1; src.w = a.cw + 1; src.h = a.ch + 1; src.edge = VWGPU_TRANSFORM_EDGE_CONSTANT;
  for (int k = lane; k < 16 * 9; k += 64) {
    const int ce = k / 9, of = k % 9;
    const double ox = of / 3 - 1, oy = of % 3 - 1;      // the 3 x 3 offsets, first coordinate slowest
    const double z = t.box[ce][2];
    const double vx = z * ox + t.box[ce][0], vy = z * oy + t.box[ce][1];
    // scale * rotate * v: the matrix is scaled first, then applied
    const double lx = (scale * r00) * vx + (scale * r01) * vy, ly = (scale * r10) * vx + (scale * r11) * vy;
    const float size = (float)((2 * scale) * z);
    float h, v;
    iph_haar(src, lx + px, ly + py, size, &h, &v);
    rx[ce * 18 + 2 * of] = r00 * h + r01 * 0.0;
    ry[ce * 18 + 2 * of] = r10 * h + r11 * 0.0;
    rx[ce * 18 + 2 * of + 1] = r00 * 0.0 + r01 * v;
    ry[ce * 18 + 2 * of + 1] = r10 * 0.0 + r11 * v;
  }
  __syncthreads();
  for (int k = lane; k < IPS2_K; k += 64) {
    const int ce = k / 8, bin = k % 8;
    float d = 0.0f;
    for (int i = 0; i < 18; ++i) {
      const double dot = t.hist[bin][0] * rx[ce * 18 + i] + t.hist[bin][1] * ry[ce * 18 + i];
      if (dot > 0) d = (float)((double)d + dot);
    }
    desc[k] = d;
  }
  __syncthreads();
  // norm_2 (Math/Vector.h:1593-1604): float squares summed in double, the sum rounded to float, the root in double
  for (int round = 0; round < 2; ++round) {
    double sum = 0.0;
    for (int k = 0; k < IPS2_K; ++k) sum += (double)(desc[k] * desc[k]);
    const float distance = (float)__dsqrt_rn((double)(float)sum);
    __syncthreads();
    for (int k = lane; k < IPS2_K; k += 64) {
      float v = __fdiv_rn(desc[k], distance);
      if (round == 0 && (double)v > 0.2) v = (float)0.2;
      desc[k] = v;
    }
    __syncthreads();
  }
  for (int k = lane; k < IPS2_K; k += 64) a.desc[p * a.dstride + k] = desc[k];
}

ips2_tables ips2_make() {
  const double box[16][3] = {{-2, -2, 1}, {2, -2, 1}, {2, 2, 1}, {-2, 2, 1}, {-3.75, -3.75, 1.25}, {0, -3.75, 1.25}, {3.75, -3.75, 1.25},
                             {3.75, 0, 1.25}, {3.75, 3.75, 1.25}, {0, 3.75, 1.25}, {-3.75, 3.75, 1.25}, {-3.75, 0, 1.25}, {-6.4, 0, 1.6},
                             {0, -6.4, 1.6}, {6.4, 0, 1.6}, {0, 6.4, 1.6}};
  const double r = 0.707106781186547;
  const double hist[8][2] = {{0, 1}, {r, r}, {1, 0}, {r, -r}, {0, -1}, {-r, -r}, {-1, 0}, {-r, r}};
  ips2_tables t;
  for (int i = 0; i < 16; ++i) for (int k = 0; k < 3; ++k) t.box[i][k] = box[i][k];
  for (int i = 0; i < 8; ++i) for (int k = 0; k < 2; ++k) t.hist[i][k] = hist[i][k];
  return t;
}

struct ips_call {
  const float* img; int w, h; ptrdiff_t stride;
  const int* crop; int n;
  const float *x, *y, *scale, *orientation;
  int kind; float* desc; ptrdiff_t dstride;
};

int ips_k(int kind) { return kind == VWGPU_IP_DESCRIPTOR_SGRAD ? IPS_K : IPS2_K; }

int ips_check(vwgpu_ctx* ctx, ips_call& c) {
  const char* name = "ip_describe";
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!c.img || !c.crop || c.n < 0 || (c.n > 0 && (!c.x || !c.y || !c.scale || !c.orientation || !c.desc)))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: null pointer or n < 0", name);
  if (c.kind != VWGPU_IP_DESCRIPTOR_SGRAD && c.kind != VWGPU_IP_DESCRIPTOR_SGRAD2)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: descriptor kind %d out of range", name, c.kind);
  if (c.w < 1 || c.h < 1) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: the image is empty", name);
  if (c.stride == 0) c.stride = c.w;
  if (c.dstride == 0) c.dstride = ips_k(c.kind);
  if (c.stride < c.w || c.dstride < ips_k(c.kind)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than the row", name);
  if (c.crop[2] < 1 || c.crop[3] < 1) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: the crop is empty", name);
  const long long lim = 1 << 20;
  if (c.crop[0] < -lim || c.crop[1] < -lim || c.crop[0] > lim || c.crop[1] > lim || c.crop[2] > lim || c.crop[3] > lim ||
      (long long)c.crop[2] * c.crop[3] > ((long long)1 << 28))
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: a crop of more than 2^28 pixels is not implemented", name);
  return VWGPU_OK;
}

int ips_run(vwgpu_ctx* ctx, const ips_call& c) {
  if (c.n == 0) return VWGPU_OK;
  ips_args a{};
  a.img = c.img; a.stride = c.stride; a.w = c.w; a.h = c.h;
  a.cx = c.crop[0]; a.cy = c.crop[1]; a.cw = c.crop[2]; a.ch = c.crop[3];
  const size_t crop_words = vwgpu_align_up((size_t)a.cw * a.ch, 64), integ_words = (size_t)(a.cw + 1) * (a.ch + 1);
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, 4 * (crop_words + integ_words));
  if (rc) return rc;
  a.crop = static_cast<float*>(ctx->scratch.base);
  a.integ = a.crop + crop_words;
  a.n = c.n; a.x = c.x; a.y = c.y; a.scale = c.scale; a.orientation = c.orientation; a.desc = c.desc; a.dstride = c.dstride;
  {
    vwgpu_prof_scope sc(ctx, "ip_crop");
    hipLaunchKernelGGL(ips_crop_kernel, dim3((a.cw + 63) / 64, (a.ch + 3) / 4), dim3(64, 4), 0, ctx->stream, a);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (c.kind == VWGPU_IP_DESCRIPTOR_SGRAD) {
    vwgpu_prof_scope sc(ctx, "ip_sgrad");
    hipLaunchKernelGGL(ips_sgrad_kernel, dim3(c.n), dim3(64), 0, ctx->stream, a);
    VWGPU_HIP(ctx, hipGetLastError());
    return VWGPU_OK;
  }
  static const ips2_tables tables = ips2_make();
  {
    vwgpu_prof_scope sc(ctx, "ip_integral");
    hipLaunchKernelGGL(ips_integral_kernel, dim3(1), dim3(64), 0, ctx->stream, a);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  vwgpu_prof_scope sc(ctx, "ip_sgrad2");
  hipLaunchKernelGGL(ips_sgrad2_kernel, dim3(c.n), dim3(64), 0, ctx->stream, a, tables);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

}  // namespace

extern "C" {

int vwgpu_ip_describe_dev(vwgpu_ctx* ctx, const float* d_img, int w, int h, ptrdiff_t stride, const int* crop, int n, const float* d_x,
                          const float* d_y, const float* d_scale, const float* d_orientation, int kind, float* d_desc, ptrdiff_t dstride) {
  ips_call c{d_img, w, h, stride, crop, n, d_x, d_y, d_scale, d_orientation, kind, d_desc, dstride};
  int rc = ips_check(ctx, c);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return ips_run(ctx, c);
}

int vwgpu_ip_describe(vwgpu_ctx* ctx, const float* img, int w, int h, ptrdiff_t stride, const int* crop, int n, const float* x, const float* y,
                      const float* scale, const float* orientation, int kind, float* desc, ptrdiff_t dstride) {
  ips_call c{img, w, h, stride, crop, n, x, y, scale, orientation, kind, desc, dstride};
  int rc = ips_check(ctx, c);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  if (n == 0) return VWGPU_OK;
  const int k = ips_k(kind);
  vwgpu_stage st(ctx);
  const int qi = st.add(img, w, h, 4, c.stride, VWGPU_STAGE_IN), qx = st.add(x, n, 1, 4, n, VWGPU_STAGE_IN), qy = st.add(y, n, 1, 4, n, VWGPU_STAGE_IN),
            qs = st.add(scale, n, 1, 4, n, VWGPU_STAGE_IN), qo = st.add(orientation, n, 1, 4, n, VWGPU_STAGE_IN),
            qd = st.add(desc, k, n, 4, c.dstride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  ips_call d = c;
  d.img = st.dev<float>(qi); d.stride = w; d.x = st.dev<float>(qx); d.y = st.dev<float>(qy); d.scale = st.dev<float>(qs);
  d.orientation = st.dev<float>(qo); d.desc = st.dev<float>(qd); d.dstride = k;
  if ((rc = ips_run(ctx, d))) return rc;
  return st.finish();
}

}  // extern "C"
