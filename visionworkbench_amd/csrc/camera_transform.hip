// camera_transform.hip — the resampling of epipolar rectification: camera_transform(image, src, dst, size, edge,
// BilinearInterpolation()) (src/vw/Camera/CameraTransform.h:43-183): per output pixel CameraTransform::reverse
// (dst.pixel_to_vector, src.point_to_pixel) and the bilinear tap of src/vw/Image/Interpolation.h:76-110 over a
// ValueEdgeExtension, for float images with an optional validity mask (PixelMask<float>, src/vw/Image/PixelMask.h:321-345,
// :424-433), and CameraTransform::forward / reverse for arrays of points.  tests/refimpl/epipolar_ref.cc restates all of
// it and DESIGN §4.19 lists what is reproduced.  The host arithmetic beside it (epipolar(), the camera matrix,
// linearize_camera, the lens words) is in camera_host.hip.
//
// One lane per output pixel, blocks of CT_BX x CT_BY, every band of CT_BY rows a workgroup of its own, no LDS.  Both
// cameras and the source's camera matrix arrive by value and are read through scalar loads.  A lane gathers up to four
// taps of the source and writes one float (and one mask byte); a wavefront's stores are row-contiguous.  The rays and
// the lenses are those of camera_rays.h.  A kernel is instantiated per (from code, to code) and, for images, masked or
// not: only a `from` with a lens, or a `to` with a lens whose round-trip check is on, carries the Newton loop.  The table
// ct_pairs lists the pairs that exist; a pair without a row is refused.
//
// Everything up to the source position is double in the reference's expression order (-ffp-contract=off); the tap is
// float, every product and sum rounded on its own.
#include <cmath>
#include <cstring>

#include "camera_rays.h"
#include "vwgpu_internal.h"

namespace {

#ifndef CT_BX
#define CT_BX 64
#define CT_BY 4
#endif
constexpr int CT_THREADS = CT_BX * CT_BY;
constexpr int CT_COUNTERS = 1024;

// how a kernel projects into a camera (point_to_pixel): a pinhole without the round-trip check (the lens kind is read at
// run time: distorted_coordinates is closed form), a pinhole without lens with the check, a pinhole whose lens kind is
// read at run time with the check (the Newton loop), CAHV (has no check), CAHVOR (closed form), CAHVORE (a Newton loop
// and two ways to throw), and a pinhole with any of the seven lenses without and with the check (TR_CAM_PINHOLE_LENS: the
// Levenberg-Marquardt loop of the Brown-Conrady and Photometrix lenses, whose failure is a throw with the check off too)
enum {
  CT_TO_PINHOLE_NOCHECK = 0, CT_TO_PINHOLE_NULL_CHECK = 1, CT_TO_PINHOLE_CHECK = 2, CT_TO_CAHV = 3, CT_TO_CAHVOR = 4, CT_TO_CAHVORE = 5,
  CT_TO_PINHOLE_LENS_NOCHECK = 6, CT_TO_PINHOLE_LENS_CHECK = 7
};
__host__ __device__ constexpr bool ct_to_lens(int to) { return to == CT_TO_PINHOLE_LENS_NOCHECK || to == CT_TO_PINHOLE_LENS_CHECK; }
// whether a kernel counts failures: the pinhole's check, a projection through any lens, or a CAHVORE on either side
__host__ __device__ constexpr bool ct_counts(int from, int to) {
  return to == CT_TO_PINHOLE_NULL_CHECK || to == CT_TO_PINHOLE_CHECK || to == CT_TO_CAHVORE || from == TR_CAM_CAHVORE || ct_to_lens(to);
}

struct ct_mat { double m[12]; };   // m_camera_matrix, row-major 3 x 4

// point_to_pixel of the camera `c`; TR_NOT_CONVERGED where PinholeModel::point_to_pixel throws PointToPixelErr (PinholeModel.cc:378-394)
// (PinholeModel.cc:378-394), TR_LENS_NOT_CONVERGED where the lens's distorted_coordinates does
template <int TO>
__device__ inline int ct_point_to_pixel(const vwgpu_camera& c, const ct_mat& M, bool flip, const tr_v3& point, tr_v2& pix) {
  if (TO == CT_TO_CAHV) {
    // CAHVModel::point_to_pixel (CAHVModel.cc:167-171)
    const tr_v3 d = tr_sub(point, tr_load3(c.center));
    const double dDot = tr_dot(d, tr_load3(c.A));
    pix = tr_v2{tr_dot(d, tr_load3(c.H)) / dDot, tr_dot(d, tr_load3(c.V)) / dDot};
    return TR_OK;
  }
  // point_to_pixel_no_check (PinholeModel.cc:351-368)
  const double* m = M.m;
  const double den = m[8] * point.x + m[9] * point.y + m[10] * point.z + m[11];
  tr_v2 pixel{(m[0] * point.x + m[1] * point.y + m[2] * point.z + m[3]) / den,
              (m[4] * point.x + m[5] * point.y + m[6] * point.z + m[7]) / den};
  if (ct_to_lens(TO)) {
    tr_v2 distorted;
    if (!tr_lens_distort(c, pixel, distorted)) return TR_LENS_NOT_CONVERGED;
    pixel = distorted;
  } else if (TO != CT_TO_PINHOLE_NULL_CHECK && c.distortion_kind == VWGPU_DISTORTION_TSAI) {
    pixel = tr_tsai_distort(c, pixel);
  }
  pix = tr_v2{pixel.x / c.pixel_pitch, pixel.y / c.pixel_pitch};
  if (TO == CT_TO_PINHOLE_NOCHECK || TO == CT_TO_PINHOLE_LENS_NOCHECK) return TR_OK;
  // the round trip (:378-394)
  const double ERROR_THRESHOLD = 0.01;
  const tr_v3 pixel_vector = TO == CT_TO_PINHOLE_NULL_CHECK   ? tr_ray<TR_CAM_PINHOLE_NULL>(c, pix, false)
                             : TO == CT_TO_PINHOLE_LENS_CHECK ? tr_ray<TR_CAM_PINHOLE_LENS>(c, pix, false)
                                                              : tr_ray<TR_CAM_PINHOLE>(c, pix, false);
  const tr_v3 phys_vector = tr_normalize(tr_sub(point, tr_load3(c.center)));
  double diff = tr_norm(tr_sub(pixel_vector, phys_vector));
  if (diff >= ERROR_THRESHOLD)
    diff = tr_norm(tr_v3{pixel_vector.x + phys_vector.x, pixel_vector.y + phys_vector.y, pixel_vector.z + phys_vector.z});
  return !(diff >= ERROR_THRESHOLD || diff != diff) ? TR_OK : TR_NOT_CONVERGED;
}

// CameraTransform::reverse / forward (CameraTransform.h:52-74): a pixel of `from` to the pixel of `to` that sees the same
// ray.  TR_OK, or why the reference throws: TR_NOT_CONVERGED also stands for the pinhole's failed round trip.
template <int FROM, int TO>
__device__ inline int ct_transform(const vwgpu_camera& from, bool flip_from, const vwgpu_camera& to, const ct_mat& Mto, const tr_v2& p,
                                   tr_v2& q) {
  tr_v3 vec;
  const int ray = tr_ray_status<FROM>(from, p, flip_from, vec);
  if (ray != TR_OK) return ray;   // PixelToRayErr
  const tr_v3 point{vec.x + from.center[0], vec.y + from.center[1], vec.z + from.center[2]};
  if (TO == CT_TO_CAHVORE) return tr_cahvore_project(to, point, q);
  if (TO == CT_TO_CAHVOR) {
    q = tr_cahvor_project(to, point);
    return TR_OK;
  }
  return ct_point_to_pixel<TO>(to, Mto, false, point, q);
}
// the failures of a workgroup into bank 0 of the counters, those by theta out of bounds (CAHVORE) or by the lens solver
// (a pinhole with any lens) into bank 1 as well
template <int TO>
__device__ inline void ct_count(unsigned long long* counters, unsigned slot, bool failed, bool theta) {
  const int n = __syncthreads_count(failed);
  if (n != 0 && threadIdx.x == 0 && threadIdx.y == 0) atomicAdd(counters + slot, (unsigned long long)n);
  if (TO == CT_TO_CAHVORE || ct_to_lens(TO)) {
    const int nt = __syncthreads_count(theta);
    if (nt != 0 && threadIdx.x == 0 && threadIdx.y == 0) atomicAdd(counters + CT_COUNTERS + slot, (unsigned long long)nt);
  }
}

// ---- the image ---------------------------------------------------------------------------------------------------------
struct ct_args {
  const float* src;
  long long sstride;
  int sw, sh;
  const uint8_t* smask;
  long long mstride;
  int w, h;
  int x0, y0;
  int flip_dst;        // a CAHV or CAHVOR dst: dot(cross(V, H), A) < 0
  float edge_value;
  int edge_valid;
  float* out;
  long long ostride;
  uint8_t* omask;
  long long omstride;
  unsigned long long* failed;   // two banks of CT_COUNTERS words, or nullptr
};

// a pixel of the edge-extended source: ValueEdgeExtension(PixelMask<float>(edge_value) [invalidated])
template <bool MASKED>
__device__ inline float ct_tap(const ct_args& a, int x, int y, bool& valid) {
  if (x >= 0 && y >= 0 && x < a.sw && y < a.sh) {
    if (MASKED && a.smask && a.smask[(long long)y * a.mstride + x] == 0) valid = false;
    return a.src[(long long)y * a.sstride + x];
  }
  if (MASKED && !a.edge_valid) valid = false;
  return a.edge_value;
}

template <int DST, int SRC, bool MASKED>
__global__ __launch_bounds__(CT_THREADS) void ct_image_kernel(ct_args a, vwgpu_camera dst, vwgpu_camera src, ct_mat Msrc) {
  int x, y;
  long long band;
  bool failed = false, theta = false;
  if (tr_band_position<CT_BX, CT_BY>(a.w, a.h, x, y, band)) {
    const tr_v2 p{(double)((long long)a.x0 + x), (double)((long long)a.y0 + y)};
    tr_v2 q;
    float res = a.edge_value;
    bool valid = a.edge_valid != 0;
    const int status = ct_transform<DST, SRC>(dst, a.flip_dst != 0, src, Msrc, p, q);
    if (status == TR_OK) {
      // BilinearInterpolationImpl (Image/Interpolation.h:83-105).  Beyond 2^30 (or NaN) _floor's conversion to int32 is
      // undefined: the result is 0 by definition, and the masked pixel is {0, invalid}.
      const double lim = 1073741824.0;
      res = 0.0f;
      valid = false;
      if (q.x >= -lim && q.x <= lim && q.y >= -lim && q.y <= lim) {
        const int xi = (int)floor(q.x), yi = (int)floor(q.y);
        valid = true;
        if ((double)xi == q.x && (double)yi == q.y) {
          res = ct_tap<MASKED>(a, xi, yi, valid);
        } else {
          const float normx = (float)q.x - (float)xi, normy = (float)q.y - (float)yi;
          const float norm1mx = 1.0f - normx, norm1my = 1.0f - normy;
          res = ct_tap<MASKED>(a, xi, yi, valid) * norm1mx;
          res += ct_tap<MASKED>(a, xi + 1, yi, valid) * normx;
          res *= norm1my;
          float row = ct_tap<MASKED>(a, xi, yi + 1, valid) * norm1mx;
          row += ct_tap<MASKED>(a, xi + 1, yi + 1, valid) * normx;
          res += row * normy;
        }
      }
    } else {
      failed = true;   // PointToPixelErr, PixelToRayErr: the edge pixel, counted
      theta = status == TR_THETA_OUT_OF_BOUNDS || status == TR_LENS_NOT_CONVERGED;
    }
    a.out[(long long)y * a.ostride + x] = res;
    if (MASKED && a.omask) a.omask[(long long)y * a.omstride + x] = valid ? 255 : 0;
  }
  if (ct_counts(DST, SRC)) ct_count<SRC>(a.failed, (unsigned)((band * gridDim.x + blockIdx.x) % CT_COUNTERS), failed, theta);
}

// ---- points ------------------------------------------------------------------------------------------------------------
struct ct_points_args {
  const double* in;
  double* out;
  long long n;
  int flip_from;
  unsigned long long* failed;
};
template <int FROM, int TO>
__global__ __launch_bounds__(CT_THREADS) void ct_points_kernel(ct_points_args a, vwgpu_camera from, vwgpu_camera to, ct_mat Mto) {
  const long long i = (long long)blockIdx.x * CT_THREADS + threadIdx.y * CT_BX + threadIdx.x;
  bool failed = false, theta = false;
  if (i < a.n) {
    const tr_v2 p{a.in[2 * i], a.in[2 * i + 1]};
    tr_v2 q;
    const int status = ct_transform<FROM, TO>(from, a.flip_from != 0, to, Mto, p, q);
    if (status != TR_OK) {
      failed = true;   // PointToPixelErr, PixelToRayErr: a NaN pair, counted
      theta = status == TR_THETA_OUT_OF_BOUNDS || status == TR_LENS_NOT_CONVERGED;
      q = tr_v2{__longlong_as_double(0x7ff8000000000000LL), __longlong_as_double(0x7ff8000000000000LL)};
    }
    a.out[2 * i] = q.x;
    a.out[2 * i + 1] = q.y;
  }
  if (ct_counts(FROM, TO)) ct_count<TO>(a.failed, blockIdx.x % CT_COUNTERS, failed, theta);
}

// the sum of the CT_COUNTERS words of bank blockIdx.x into its word 0 (integers: any order)
__global__ __launch_bounds__(CT_THREADS) void ct_count_fold_kernel(unsigned long long* counters) {
  __shared__ unsigned long long lds[CT_THREADS];
  const int tid = threadIdx.x;
  unsigned long long* bank = counters + (size_t)blockIdx.x * CT_COUNTERS;
  unsigned long long s = 0;
  for (int k = tid; k < CT_COUNTERS; k += CT_THREADS) s += bank[k];
  lds[tid] = s;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < CT_THREADS; ++k) s += lds[k];
    bank[0] = s;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

const dim3 ct_block(CT_BX, CT_BY);
dim3 ct_grid(int w, int h) { return tr_band_grid<CT_BX, CT_BY>(w, h); }

int ct_camera_check(vwgpu_ctx* ctx, const char* name, const char* which, const vwgpu_camera* c, const double* matrix) {
  const int rc = tr_camera_check(ctx, name, which, c);
  if (rc) return rc;
  if (c->kind == VWGPU_CAMERA_PINHOLE && !matrix)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: the %s camera is a pinhole and has no camera matrix", name, which);
  return VWGPU_OK;
}

int ct_same_center(vwgpu_ctx* ctx, const vwgpu_camera* src, const vwgpu_camera* dst) {
  if (src->center[0] == dst->center[0] && src->center[1] == dst->center[1] && src->center[2] == dst->center[2]) return VWGPU_OK;
  return vwgpu_fail(ctx, VWGPU_ERR_LOGIC,
                    "CameraTransformFunctor: Camera transformation require that the camera center is always the same for both cameras.");
}

// the code a kernel carries for the camera it projects into (for the camera whose rays it forms: tr_camera_code).  `lens`:
// one camera of the pair is a pinhole with a lens other than null and Tsai, and every pinhole of the pair takes the
// any-lens code.
int ct_to_code(const vwgpu_camera& c, int check, bool lens) {
  if (tr_new_kind(c)) return c.kind == VWGPU_CAMERA_CAHVOR ? CT_TO_CAHVOR : CT_TO_CAHVORE;
  if (c.kind == VWGPU_CAMERA_CAHV) return CT_TO_CAHV;
  if (lens) return check ? CT_TO_PINHOLE_LENS_CHECK : CT_TO_PINHOLE_LENS_NOCHECK;
  if (!check) return CT_TO_PINHOLE_NOCHECK;
  return c.distortion_kind == VWGPU_DISTORTION_NULL ? CT_TO_PINHOLE_NULL_CHECK : CT_TO_PINHOLE_CHECK;
}

// The (from, to) pairs that have kernels, one row each: the two codes and the three kernels instantiated for them.  Null
// and Tsai pinholes and CAHV in every combination; CAHVOR and CAHVORE with CAHV alone, in either role; a pinhole with the
// any-lens code with another one or with CAHV.  A pair without a row has no kernel (ct_pair_check).
using ct_image_kernel_t = void (*)(ct_args, vwgpu_camera, vwgpu_camera, ct_mat);
using ct_points_kernel_t = void (*)(ct_points_args, vwgpu_camera, vwgpu_camera, ct_mat);
struct ct_pair {
  int from, to;
  ct_image_kernel_t image, image_masked;
  ct_points_kernel_t points;
};
#define CT_ROW(FROM, TO) {FROM, TO, ct_image_kernel<FROM, TO, false>, ct_image_kernel<FROM, TO, true>, ct_points_kernel<FROM, TO>}
const ct_pair ct_pairs[] = {
  CT_ROW(TR_CAM_PINHOLE_NULL, CT_TO_PINHOLE_NOCHECK), CT_ROW(TR_CAM_PINHOLE_NULL, CT_TO_PINHOLE_NULL_CHECK),
  CT_ROW(TR_CAM_PINHOLE_NULL, CT_TO_PINHOLE_CHECK),   CT_ROW(TR_CAM_PINHOLE_NULL, CT_TO_CAHV),
  CT_ROW(TR_CAM_PINHOLE, CT_TO_PINHOLE_NOCHECK),      CT_ROW(TR_CAM_PINHOLE, CT_TO_PINHOLE_NULL_CHECK),
  CT_ROW(TR_CAM_PINHOLE, CT_TO_PINHOLE_CHECK),        CT_ROW(TR_CAM_PINHOLE, CT_TO_CAHV),
  CT_ROW(TR_CAM_CAHV, CT_TO_PINHOLE_NOCHECK),         CT_ROW(TR_CAM_CAHV, CT_TO_PINHOLE_NULL_CHECK),
  CT_ROW(TR_CAM_CAHV, CT_TO_PINHOLE_CHECK),           CT_ROW(TR_CAM_CAHV, CT_TO_CAHV),
  CT_ROW(TR_CAM_CAHVOR, CT_TO_CAHV),                  CT_ROW(TR_CAM_CAHVORE, CT_TO_CAHV),
  CT_ROW(TR_CAM_CAHV, CT_TO_CAHVOR),                  CT_ROW(TR_CAM_CAHV, CT_TO_CAHVORE),
  CT_ROW(TR_CAM_CAHV, CT_TO_PINHOLE_LENS_NOCHECK),    CT_ROW(TR_CAM_CAHV, CT_TO_PINHOLE_LENS_CHECK),
  CT_ROW(TR_CAM_PINHOLE_LENS, CT_TO_PINHOLE_LENS_NOCHECK), CT_ROW(TR_CAM_PINHOLE_LENS, CT_TO_PINHOLE_LENS_CHECK),
  CT_ROW(TR_CAM_PINHOLE_LENS, CT_TO_CAHV),
};
#undef CT_ROW

// the row for rays of `from` projected into `to`, or nullptr
const ct_pair* ct_pair_of(const vwgpu_camera& from, const vwgpu_camera& to, int check) {
  const bool lens = tr_lens_pinhole(from) || tr_lens_pinhole(to);
  const int kf = tr_camera_code(from, lens), kt = ct_to_code(to, check, lens);
  for (const ct_pair& row : ct_pairs)
    if (row.from == kf && row.to == kt) return &row;
  return nullptr;
}

// a call needs a row whether the check is on or off: `from` and `to` are src and dst in the direction the call runs
int ct_pair_check(vwgpu_ctx* ctx, const char* name, const vwgpu_camera* src, const vwgpu_camera* dst, const vwgpu_camera* from,
                  const vwgpu_camera* to) {
  if (!ct_pair_of(*from, *to, 0) || !ct_pair_of(*from, *to, 1))
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: no kernel for the pair %s -> %s: CAHVOR and CAHVORE go with CAHV only", name,
                      tr_kind_name(*src), tr_kind_name(*dst));
  return VWGPU_OK;
}

ct_mat ct_matrix(const double* m) {
  ct_mat M{};
  if (m) std::memcpy(M.m, m, sizeof(M.m));
  return M;
}

// the counters of a call, zeroed; nullptr in *d_counter when the kernel does not count
int ct_counters(vwgpu_ctx* ctx, bool counts, unsigned long long** d_counter) {
  *d_counter = nullptr;
  const size_t bytes = 2 * CT_COUNTERS * sizeof(unsigned long long);   // bank 0: every failure; bank 1: theta out of bounds
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, bytes);
  if (rc) return rc;
  *d_counter = static_cast<unsigned long long*>(ctx->scratch.base);
  // without the check nothing is counted and word 0 stays 0
  VWGPU_HIP(ctx, hipMemsetAsync(*d_counter, 0, counts ? bytes : sizeof(unsigned long long), ctx->stream));
  return VWGPU_OK;
}

// what a host-pointer call learns: the failures, and how many of them were CAHVORE's theta out of bounds
// (for a pinhole with any lens: how many were the lens solver's)
struct ct_failures { long long failed, theta; bool cahvore, lens; };

// after the kernel: fold the counters; d_failed (device, optional) receives the count, *h_failed (host, optional) too (synchronises)
int ct_count_out(vwgpu_ctx* ctx, int from, int to, unsigned long long* d_counter, long long* d_failed, ct_failures* h_failed) {
  const bool counts = ct_counts(from, to), theta = to == CT_TO_CAHVORE || ct_to_lens(to);
  if (counts) hipLaunchKernelGGL(ct_count_fold_kernel, dim3(theta ? 2 : 1), dim3(CT_THREADS), 0, ctx->stream, d_counter);
  VWGPU_HIP(ctx, hipGetLastError());
  if (d_failed) VWGPU_HIP(ctx, hipMemcpyAsync(d_failed, d_counter, 8, hipMemcpyDeviceToDevice, ctx->stream));
  if (h_failed) {
    unsigned long long cnt = 0, cnt_theta = 0;
    VWGPU_HIP(ctx, hipMemcpyAsync(&cnt, d_counter, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (theta) VWGPU_HIP(ctx, hipMemcpyAsync(&cnt_theta, d_counter + CT_COUNTERS, 8, hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *h_failed = ct_failures{(long long)cnt, (long long)cnt_theta, to == CT_TO_CAHVORE || from == TR_CAM_CAHVORE, ct_to_lens(to)};
  }
  return VWGPU_OK;
}

// the reference's message for what it would have thrown.  It throws at the first failing pixel in raster order; here the
// message names non-convergence when any pixel did not converge, and theta otherwise.
int ct_inaccurate(vwgpu_ctx* ctx, const ct_failures& f) {
  if (f.lens && f.theta != 0) return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "LensDistortion: Did not converge. (%lld pixels)", f.failed);
  if (!f.cahvore) return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "PinholeModel: Projection into pinhole camera is inaccurate. (%lld pixels)", f.failed);
  if (f.theta == f.failed) return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "CAHVOREModel: Theta out of bounds. (%lld pixels)", f.failed);
  return vwgpu_fail(ctx, VWGPU_ERR_LOGIC, "CAHVOREModel: Did not converge. (%lld pixels)", f.failed);
}

struct ct_image_call {
  const float* src; int sw, sh; ptrdiff_t sstride;
  const uint8_t* smask; ptrdiff_t mstride;
  const vwgpu_camera* src_cam; const double* src_matrix;
  const vwgpu_camera* dst_cam; const double* dst_matrix;
  int w, h, x0, y0;
  float edge_value; int edge_valid, check;
  float* out; ptrdiff_t ostride;
  uint8_t* omask; ptrdiff_t omstride;
};

int ct_image_check(vwgpu_ctx* ctx, ct_image_call& c) {
  const char* name = "camera_transform";
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!c.src || !c.out || c.sw <= 0 || c.sh <= 0 || c.w <= 0 || c.h <= 0)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: empty image or null pointer", name);
  int rc = ct_camera_check(ctx, name, "source", c.src_cam, c.src_matrix);
  if (rc) return rc;
  if ((rc = ct_camera_check(ctx, name, "destination", c.dst_cam, c.dst_matrix))) return rc;
  if (c.sstride == 0) c.sstride = c.sw;
  if (c.mstride == 0) c.mstride = c.sw;
  if (c.ostride == 0) c.ostride = c.w;
  if (c.omstride == 0) c.omstride = c.w;
  if (c.sstride < c.sw || (c.smask && c.mstride < c.sw) || c.ostride < c.w || (c.omask && c.omstride < c.w))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
  if ((const void*)c.out == (const void*)c.src || (const void*)c.out == (const void*)c.smask ||
      (c.omask && ((const void*)c.omask == (const void*)c.src || c.omask == c.smask || (const void*)c.omask == (const void*)c.out)))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: an output must not be an input or the other output", name);
  if (c.edge_valid && std::isnan(c.edge_value)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: a valid edge pixel must not be NaN", name);
  if ((rc = ct_pair_check(ctx, name, c.src_cam, c.dst_cam, c.dst_cam, c.src_cam))) return rc;
  return ct_same_center(ctx, c.src_cam, c.dst_cam);
}

// all pointers of `c` are device pointers here
int ct_image_run(vwgpu_ctx* ctx, const ct_image_call& c, long long* d_failed, ct_failures* h_failed) {
  const ct_pair* pair = ct_pair_of(*c.dst_cam, *c.src_cam, c.check);
  const int from = pair->from, to = pair->to;
  unsigned long long* d_counter = nullptr;
  const bool want = d_failed || h_failed;
  if (ct_counts(from, to) || want) {
    int rc = ct_counters(ctx, ct_counts(from, to), &d_counter);
    if (rc) return rc;
  }
  ct_args a{c.src, (long long)c.sstride, c.sw, c.sh, c.smask, (long long)c.mstride, c.w, c.h, c.x0, c.y0, tr_cahv_flip(*c.dst_cam),
            c.edge_value, c.edge_valid != 0, c.out, (long long)c.ostride, c.omask, (long long)c.omstride, d_counter};
  const ct_mat M = ct_matrix(c.src_matrix);
  const bool masked = c.smask || c.omask;
  {
    vwgpu_prof_scope ps(ctx, "camera_transform");
    hipLaunchKernelGGL(masked ? pair->image_masked : pair->image, ct_grid(c.w, c.h), ct_block, 0, ctx->stream, a, *c.dst_cam, *c.src_cam, M);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (!want) return VWGPU_OK;
  return ct_count_out(ctx, from, to, d_counter, d_failed, h_failed);
}

int ct_points_check(vwgpu_ctx* ctx, const vwgpu_camera* src, const double* src_matrix, const vwgpu_camera* dst, const double* dst_matrix,
                    int direction, const double* points, long long n, const double* out) {
  const char* name = "camera_transform_points";
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (!points || !out || n <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: no points or null pointer", name);
  if (direction != VWGPU_CAMERA_TRANSFORM_FORWARD && direction != VWGPU_CAMERA_TRANSFORM_REVERSE)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: direction %d is neither forward nor reverse", name, direction);
  int rc = ct_camera_check(ctx, name, "source", src, src_matrix);
  if (rc) return rc;
  if ((rc = ct_camera_check(ctx, name, "destination", dst, dst_matrix))) return rc;
  const bool fwd = direction == VWGPU_CAMERA_TRANSFORM_FORWARD;
  if ((rc = ct_pair_check(ctx, name, src, dst, fwd ? src : dst, fwd ? dst : src))) return rc;
  return ct_same_center(ctx, src, dst);
}

int ct_points_run(vwgpu_ctx* ctx, const vwgpu_camera* src, const double* src_matrix, const vwgpu_camera* dst, const double* dst_matrix,
                  int direction, int check, const double* d_points, long long n, double* d_out, long long* d_failed, ct_failures* h_failed) {
  const bool fwd = direction == VWGPU_CAMERA_TRANSFORM_FORWARD;
  const vwgpu_camera& cfrom = fwd ? *src : *dst;
  const vwgpu_camera& cto = fwd ? *dst : *src;
  const ct_pair* pair = ct_pair_of(cfrom, cto, check);
  const int from = pair->from, to = pair->to;
  unsigned long long* d_counter = nullptr;
  const bool want = d_failed || h_failed;
  if (ct_counts(from, to) || want) {
    int rc = ct_counters(ctx, ct_counts(from, to), &d_counter);
    if (rc) return rc;
  }
  ct_points_args a{d_points, d_out, n, tr_cahv_flip(cfrom), d_counter};
  const ct_mat M = ct_matrix(fwd ? dst_matrix : src_matrix);
  const dim3 grid((unsigned)((n + CT_THREADS - 1) / CT_THREADS));
  {
    vwgpu_prof_scope ps(ctx, "camera_transform_points");
    hipLaunchKernelGGL(pair->points, grid, ct_block, 0, ctx->stream, a, cfrom, cto, M);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (!want) return VWGPU_OK;
  return ct_count_out(ctx, from, to, d_counter, d_failed, h_failed);
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------------

extern "C" {

int vwgpu_camera_transform_dev(vwgpu_ctx* ctx, const float* d_src, int sw, int sh, ptrdiff_t sstride, const uint8_t* d_src_mask,
                               ptrdiff_t mstride, const vwgpu_camera* src_camera, const double* src_matrix,
                               const vwgpu_camera* dst_camera, const double* dst_matrix, int w, int h, int x0, int y0, float edge_value,
                               int edge_valid, int check, float* d_out, ptrdiff_t ostride, uint8_t* d_out_mask, ptrdiff_t omstride,
                               long long* d_failed) {
  ct_image_call c{d_src, sw, sh, sstride, d_src_mask, mstride, src_camera, src_matrix, dst_camera, dst_matrix, w, h, x0, y0,
                  edge_value, edge_valid, check, d_out, ostride, d_out_mask, omstride};
  int rc = ct_image_check(ctx, c);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return ct_image_run(ctx, c, d_failed, nullptr);
}

int vwgpu_camera_transform(vwgpu_ctx* ctx, const float* src, int sw, int sh, ptrdiff_t sstride, const uint8_t* src_mask, ptrdiff_t mstride,
                           const vwgpu_camera* src_camera, const double* src_matrix, const vwgpu_camera* dst_camera,
                           const double* dst_matrix, int w, int h, int x0, int y0, float edge_value, int edge_valid, int check, float* out,
                           ptrdiff_t ostride, uint8_t* out_mask, ptrdiff_t omstride, long long* failed) {
  ct_image_call c{src, sw, sh, sstride, src_mask, mstride, src_camera, src_matrix, dst_camera, dst_matrix, w, h, x0, y0,
                  edge_value, edge_valid, check, out, ostride, out_mask, omstride};
  int rc = ct_image_check(ctx, c);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int ps = st.add(src, sw, sh, 4, c.sstride, VWGPU_STAGE_IN), pm = st.add(src_mask, sw, sh, 1, c.mstride, VWGPU_STAGE_IN),
            po = st.add(out, w, h, 4, c.ostride, VWGPU_STAGE_OUT), pk = st.add(out_mask, w, h, 1, c.omstride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  ct_image_call d = c;
  d.src = st.dev<float>(ps); d.sstride = sw;
  d.smask = st.dev<uint8_t>(pm); d.mstride = sw;
  d.out = st.dev<float>(po); d.ostride = w;
  d.omask = st.dev<uint8_t>(pk); d.omstride = w;
  ct_failures count{};
  if ((rc = ct_image_run(ctx, d, nullptr, &count))) return rc;
  if ((rc = st.finish())) return rc;
  if (failed) *failed = count.failed;
  return count.failed != 0 ? ct_inaccurate(ctx, count) : VWGPU_OK;
}

int vwgpu_camera_transform_points_dev(vwgpu_ctx* ctx, const vwgpu_camera* src_camera, const double* src_matrix,
                                      const vwgpu_camera* dst_camera, const double* dst_matrix, int direction, int check,
                                      const double* d_points, long long n, double* d_out, long long* d_failed) {
  int rc = ct_points_check(ctx, src_camera, src_matrix, dst_camera, dst_matrix, direction, d_points, n, d_out);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return ct_points_run(ctx, src_camera, src_matrix, dst_camera, dst_matrix, direction, check, d_points, n, d_out, d_failed, nullptr);
}

int vwgpu_camera_transform_points(vwgpu_ctx* ctx, const vwgpu_camera* src_camera, const double* src_matrix,
                                  const vwgpu_camera* dst_camera, const double* dst_matrix, int direction, int check, const double* points,
                                  long long n, double* out, long long* failed) {
  int rc = ct_points_check(ctx, src_camera, src_matrix, dst_camera, dst_matrix, direction, points, n, out);
  if (rc) return rc;
  if (n > 0x3fffffff) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "camera_transform_points: too many points for one call");
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pi = st.add(points, (int)n, 1, 16, n, VWGPU_STAGE_IN), po = st.add(out, (int)n, 1, 16, n, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  ct_failures count{};
  if ((rc = ct_points_run(ctx, src_camera, src_matrix, dst_camera, dst_matrix, direction, check, st.dev<double>(pi), n, st.dev<double>(po),
                          nullptr, &count)))
    return rc;
  if ((rc = st.finish())) return rc;
  if (failed) *failed = count.failed;
  return count.failed != 0 ? ct_inaccurate(ctx, count) : VWGPU_OK;
}

}  // extern "C"
