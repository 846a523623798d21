// camera_transform.hip — epipolar rectification: the host arithmetic of epipolar() for two pinholes
// (src/vw/Camera/PinholeModel.cc:679-732, with the quaternion round trip of camera_pose().rotation_matrix(),
// src/vw/Math/Quaternion.h:211-340) and two CAHV models (src/vw/Camera/CAHVModel.cc:297-337), the 3 x 4 camera matrix of
// rebuild_camera_matrix (PinholeModel.cc:593-603), and the resampling camera_transform(image, src, dst, size, edge,
// BilinearInterpolation()) (src/vw/Camera/CameraTransform.h:43-183): per output pixel CameraTransform::reverse
// (dst.pixel_to_vector, src.point_to_pixel) and the bilinear tap of src/vw/Image/Interpolation.h:76-110 over a
// ValueEdgeExtension, for float images with an optional validity mask (PixelMask<float>, src/vw/Image/PixelMask.h:321-345,
// :424-433).  tests/refimpl/epipolar_ref.cc restates all of it and DESIGN §4.19 lists what is reproduced.
//
// One lane per output pixel, blocks of CT_BX x CT_BY, every band of CT_BY rows a workgroup of its own, no LDS.  Both
// cameras and the source's camera matrix arrive by value and are read through scalar loads.  A lane gathers up to four
// taps of the source and writes one float (and one mask byte); a wavefront's stores are row-contiguous.  The rays are
// those of triangulate.hip (camera_rays.h).  A kernel is instantiated per (dst code, src code, masked): only a dst with
// a lens, or a src with a lens whose round-trip check is on, carries the Newton loop.  CAHVOR and CAHVORE
// (camera_rays.h) are paired with CAHV alone, in either role: eight more image kernels and four more point kernels.
// linearize_camera (CAHVORModel.cc:460-547, CAHVOREModel.cc:303-381) is host arithmetic over the same model functions.
// A pair in which a pinhole carries a FOV, fisheye, Brown-Conrady, adjustable Tsai or Photometrix lens takes the any-lens
// codes for its pinholes (TR_CAM_PINHOLE_LENS, CT_TO_PINHOLE_LENS_*): ten more image kernels and five more point kernels,
// with distorted_coordinates of every lens (LensDistortion.cc:175-195, :462-488, :612-632, :832-849), which
// vwgpu_lens_coordinates runs on the host.
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
template <int TO>
__host__ __device__ constexpr bool ct_to_lens() { return TO == CT_TO_PINHOLE_LENS_NOCHECK || TO == CT_TO_PINHOLE_LENS_CHECK; }

struct ct_mat { double m[12]; };   // m_camera_matrix, row-major 3 x 4

// TsaiLensDistortion::distorted_coordinates (LensDistortion.cc:345-369)
__host__ __device__ inline tr_v2 ct_tsai_distort(const vwgpu_camera& c, const tr_v2& p) {
  if (c.fu < 1e-300 || c.fv < 1e-300) return tr_v2{HUGE_VAL, HUGE_VAL};
  const tr_v2 p0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const tr_v2 d = tr_tsai_norm(p0, c.distortion);
  double dx = d.x, dy = d.y;
  dx = dx * c.fu + c.cu;
  dy = dy * c.fv + c.cv;
  return tr_v2{dx, dy};
}

// FovLensDistortion::distorted_coordinates (LensDistortion.cc:462-488); L = {k1, 1 / k1, 2 tan(k1 / 2)}
__host__ __device__ inline tr_v2 ct_fov_distort(const vwgpu_camera& c, const tr_v2& p) {
  const double* L = tr_lens_words(c);
  if (c.fu < 1e-300 || c.fv < 1e-300) return tr_v2{HUGE_VAL, HUGE_VAL};
  const tr_v2 p0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const double ru = tr_norm(p0);
  const double rd = atan(ru * L[2]) * L[1];
  double conv = 1.0;
  if (ru > 1e-8) conv = rd / ru;
  return tr_v2{conv * p0.x * c.fu + c.cu, conv * p0.y * c.fv + c.cv};
}

// FisheyeLensDistortion::distorted_coordinates (:612-632) and AdjustableTsaiLensDistortion::distorted_coordinates (:832-849)
template <class MODEL>
__host__ __device__ inline tr_v2 ct_norm_distort(const vwgpu_camera& c, const tr_v2& p) {
  if (c.fu < 1e-300 || c.fv < 1e-300) return tr_v2{HUGE_VAL, HUGE_VAL};
  const tr_v2 p0{(p.x - c.cu) / c.fu, (p.y - c.cv) / c.fv};
  const tr_v2 d = MODEL{tr_lens_words(c)}.norm(p0);
  return tr_v2{d.x * c.fu + c.cu, d.y * c.fv + c.cv};
}

// DistortOptimizeFunctor (LensDistortion.cc:29-41) for the two lenses that have no distorted_coordinates of their own
__host__ __device__ inline tr_v2 ct_solver_model(const vwgpu_camera& c, const tr_v2& x) {
  return c.distortion_kind == VWGPU_DISTORTION_PHOTOMETRIX ? tr_photometrix_undistort(c, x) : tr_brown_conrady_undistort(c, x);
}

// LensDistortion::distorted_coordinates (LensDistortion.cc:175-195): levenberg_marquardtFixed(model, v, v, status, 1e-16,
// 1e-16, 100) (Math/LevenbergMarquardt.h:389-561) for two unknowns, with the forward-difference Jacobian of
// LeastSquaresModelBaseFixed::jacobian (:344-377) and inverse() of Math/Matrix.h:2209-2216, then the 1e-10 test.  At most
// 100 outer passes of at most 6 inner ones.  false where the reference throws "LensDistortion: Did not converge.", and
// where det(hessian_lm) > 0.0 does not hold (NaN, overflow), for which the reference leaves for LAPACK.
__host__ __device__ inline bool ct_solver_distort(const vwgpu_camera& c, const tr_v2& v, tr_v2& solution) {
  const double abs_tolerance = 1e-16, rel_tolerance = 1e-16;
  const int max_iterations = 100;
  bool done = false;
  const double Rinv = 10;
  double lambda = 0.1;
  tr_v2 x_try{0.0, 0.0}, x = v;
  tr_v2 h = ct_solver_model(c, x);
  tr_v2 error{v.x - h.x, v.y - h.y};
  double norm_start = tr_norm(error);
  if (norm_start < abs_tolerance) done = true;
  for (int outer_iter = 1; outer_iter <= max_iterations && !done; ++outer_iter) {
    bool shortCircuit = false;
    h = ct_solver_model(c, x);
    error = tr_v2{v.x - h.x, v.y - h.y};
    norm_start = tr_norm(error);
    // the Jacobian, J[row][column]
    const tr_v2 h0 = ct_solver_model(c, x);
    const double eps0 = 1e-7 + fabs(x.x * 1e-7), eps1 = 1e-7 + fabs(x.y * 1e-7);
    const tr_v2 h_0 = ct_solver_model(c, tr_v2{x.x + eps0, x.y}), h_1 = ct_solver_model(c, tr_v2{x.x, x.y + eps1});
    const double J00 = (h_0.x - h0.x) / eps0, J10 = (h_0.y - h0.y) / eps0;
    const double J01 = (h_1.x - h0.x) / eps1, J11 = (h_1.y - h0.y) / eps1;
    const double del_J0 = -1.0 * Rinv * (0.0 + J00 * error.x + J10 * error.y);
    const double del_J1 = -1.0 * Rinv * (0.0 + J01 * error.x + J11 * error.y);
    const double H00 = Rinv * (0.0 + J00 * J00 + J10 * J10), H01 = Rinv * (0.0 + J00 * J01 + J10 * J11);
    const double H10 = Rinv * (0.0 + J01 * J00 + J11 * J10), H11 = Rinv * (0.0 + J01 * J01 + J11 * J11);
    int iterations = 0;
    double norm_try = norm_start + 1.0;
    while (norm_try > norm_start && iterations < 6) {
      double d0 = H00, d3 = H11;
      const double d1 = H01, d2 = H10;
      d0 += d0 * lambda + lambda;
      d3 += d3 * lambda + lambda;
      const double det = d0 * d3 - d1 * d2;
      if (!(det > 0.0)) return false;
      const double i0 = d3 / det, i1 = -d1 / det, i2 = -d2 / det, i3 = d0 / det;
      const tr_v2 delta_x{0.0 + i0 * del_J0 + i1 * del_J1, 0.0 + i2 * del_J0 + i3 * del_J1};
      x_try = tr_v2{x.x - delta_x.x, x.y - delta_x.y};
      const tr_v2 h_try = ct_solver_model(c, x_try);
      const tr_v2 error_try{v.x - h_try.x, v.y - h_try.y};
      norm_try = tr_norm(error_try);
      if (norm_try > norm_start) lambda *= 10;
      ++iterations;
      if (iterations > 5) {
        shortCircuit = true;
        norm_try = norm_start;
      }
    }
    if (!shortCircuit && ((norm_start - norm_try) / norm_start) < rel_tolerance) done = true;
    if (norm_try < abs_tolerance) done = true;
    if (!shortCircuit) x = x_try;
    norm_start = norm_try;
    lambda /= 10;
  }
  solution = x;
  const tr_v2 undist = ct_solver_model(c, solution);
  const double nv = tr_norm(v);
  const double err = tr_norm(tr_v2{undist.x - v.x, undist.y - v.y}) / (nv > 0.1 ? nv : 0.1);
  return !(err > 1e-10);
}

// distorted_coordinates of a pinhole's lens, whichever it is; false where the reference throws
__host__ __device__ inline bool ct_lens_distort(const vwgpu_camera& c, const tr_v2& p, tr_v2& out) {
  switch (c.distortion_kind) {
    case VWGPU_DISTORTION_TSAI: out = ct_tsai_distort(c, p); return true;
    case VWGPU_DISTORTION_FOV: out = ct_fov_distort(c, p); return true;
    case VWGPU_DISTORTION_FISHEYE: out = ct_norm_distort<tr_fisheye_model>(c, p); return true;
    case VWGPU_DISTORTION_ADJUSTABLE_TSAI: out = ct_norm_distort<tr_adjustable_tsai_model>(c, p); return true;
    case VWGPU_DISTORTION_BROWN_CONRADY:
    case VWGPU_DISTORTION_PHOTOMETRIX: return ct_solver_distort(c, p, out);
    default: out = p; return true;
  }
}

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
  if (ct_to_lens<TO>()) {
    tr_v2 distorted;
    if (!ct_lens_distort(c, pixel, distorted)) return TR_LENS_NOT_CONVERGED;
    pixel = distorted;
  } else if (TO != CT_TO_PINHOLE_NULL_CHECK && c.distortion_kind == VWGPU_DISTORTION_TSAI) {
    pixel = ct_tsai_distort(c, pixel);
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
// whether a kernel counts failures: the pinhole's check, a projection through any lens, or a CAHVORE on either side
template <int FROM, int TO>
__device__ constexpr bool ct_kernel_counts() {
  return TO == CT_TO_PINHOLE_NULL_CHECK || TO == CT_TO_PINHOLE_CHECK || TO == CT_TO_CAHVORE || FROM == TR_CAM_CAHVORE || ct_to_lens<TO>();
}
// the failures of a workgroup into bank 0 of the counters, those by theta out of bounds (CAHVORE) or by the lens solver
// (a pinhole with any lens) into bank 1 as well
template <int TO>
__device__ inline void ct_count(unsigned long long* counters, unsigned slot, bool failed, bool theta) {
  const int n = __syncthreads_count(failed);
  if (n != 0 && threadIdx.x == 0 && threadIdx.y == 0) atomicAdd(counters + slot, (unsigned long long)n);
  if (TO == CT_TO_CAHVORE || ct_to_lens<TO>()) {
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

// Every band of CT_BY rows has a workgroup of its own, numbered through grid y and then z (as triangulate.hip does).
__device__ inline bool ct_position(int w, int h, int& x, int& y, long long& band) {
  x = blockIdx.x * CT_BX + threadIdx.x;
  band = (long long)blockIdx.z * gridDim.y + blockIdx.y;
  const long long row = band * CT_BY + threadIdx.y;
  y = (int)row;
  return x < w && row < h;
}

template <int DST, int SRC, bool MASKED>
__global__ __launch_bounds__(CT_THREADS) void ct_image_kernel(ct_args a, vwgpu_camera dst, vwgpu_camera src, ct_mat Msrc) {
  int x, y;
  long long band;
  bool failed = false, theta = false;
  if (ct_position(a.w, a.h, x, y, band)) {
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
  if (ct_kernel_counts<DST, SRC>()) ct_count<SRC>(a.failed, (unsigned)((band * gridDim.x + blockIdx.x) % CT_COUNTERS), failed, theta);
}

// ---- points ------------------------------------------------------------------------------------------------------------
struct ct_points_args {
  const double* in;
  double* out;
  long long n;
  int flip_from;
  unsigned long long* failed;
};
template <int FROM, int TO, bool UNUSED>
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
  if (ct_kernel_counts<FROM, TO>()) ct_count<TO>(a.failed, blockIdx.x % CT_COUNTERS, failed, theta);
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
dim3 ct_grid(int w, int h) {
  const long long bands = ((long long)h + CT_BY - 1) / CT_BY, gy = bands < 65535 ? bands : 65535;
  return dim3((unsigned)((w + CT_BX - 1) / CT_BX), (unsigned)gy, (unsigned)((bands + gy - 1) / gy));
}

int ct_cahv_flip(const vwgpu_camera& c) {   // CAHVORModel.cc:306 is the same test
  return (c.kind == VWGPU_CAMERA_CAHV || c.kind == VWGPU_CAMERA_CAHVOR) && tr_dot(tr_cross(tr_load3(c.V), tr_load3(c.H)), tr_load3(c.A)) < 0.0;   // CAHVModel.cc:182
}

int ct_camera_check(vwgpu_ctx* ctx, const char* name, const char* which, const vwgpu_camera* c, const double* matrix) {
  if (!c) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: null %s camera", name, which);
  if (c->kind != VWGPU_CAMERA_PINHOLE && c->kind != VWGPU_CAMERA_CAHV && !tr_new_kind(*c))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: unknown camera kind %d", name, c->kind);
  if (c->kind == VWGPU_CAMERA_PINHOLE && !tr_lens_valid(*c))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: unknown lens distortion kind %d", name, c->distortion_kind);
  if (c->kind == VWGPU_CAMERA_PINHOLE && !matrix)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: the %s camera is a pinhole and has no camera matrix", name, which);
  return VWGPU_OK;
}

// CAHVOR and CAHVORE are paired with CAHV alone (in either role); every other pair with one of them has no kernel
int ct_pair_check(vwgpu_ctx* ctx, const char* name, const vwgpu_camera* src, const vwgpu_camera* dst) {
  if ((tr_new_kind(*src) && dst->kind != VWGPU_CAMERA_CAHV) || (tr_new_kind(*dst) && src->kind != VWGPU_CAMERA_CAHV))
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: no kernel for the pair %s -> %s: CAHVOR and CAHVORE go with CAHV only", name,
                      tr_kind_name(*src), tr_kind_name(*dst));
  return VWGPU_OK;
}

int ct_same_center(vwgpu_ctx* ctx, const vwgpu_camera* src, const vwgpu_camera* dst) {
  if (src->center[0] == dst->center[0] && src->center[1] == dst->center[1] && src->center[2] == dst->center[2]) return VWGPU_OK;
  return vwgpu_fail(ctx, VWGPU_ERR_LOGIC,
                    "CameraTransformFunctor: Camera transformation require that the camera center is always the same for both cameras.");
}

// the code a kernel carries for the camera whose rays it forms / for the camera it projects into.  `lens`: one camera of
// the pair is a pinhole with a lens other than null and Tsai, and every pinhole of the pair takes the any-lens code.
int ct_from_code(const vwgpu_camera& c, bool lens) {
  if (tr_new_kind(c)) return c.kind == VWGPU_CAMERA_CAHVOR ? TR_CAM_CAHVOR : TR_CAM_CAHVORE;
  if (lens && c.kind == VWGPU_CAMERA_PINHOLE) return TR_CAM_PINHOLE_LENS;
  return c.kind == VWGPU_CAMERA_CAHV ? TR_CAM_CAHV : c.distortion_kind == VWGPU_DISTORTION_NULL ? TR_CAM_PINHOLE_NULL : TR_CAM_PINHOLE;
}
int ct_to_code(const vwgpu_camera& c, int check, bool lens) {
  if (tr_new_kind(c)) return c.kind == VWGPU_CAMERA_CAHVOR ? CT_TO_CAHVOR : CT_TO_CAHVORE;
  if (c.kind == VWGPU_CAMERA_CAHV) return CT_TO_CAHV;
  if (lens) return check ? CT_TO_PINHOLE_LENS_CHECK : CT_TO_PINHOLE_LENS_NOCHECK;
  if (!check) return CT_TO_PINHOLE_NOCHECK;
  return c.distortion_kind == VWGPU_DISTORTION_NULL ? CT_TO_PINHOLE_NULL_CHECK : CT_TO_PINHOLE_CHECK;
}
bool ct_lens_to(int to) { return to == CT_TO_PINHOLE_LENS_NOCHECK || to == CT_TO_PINHOLE_LENS_CHECK; }
bool ct_counts(int from, int to) {
  return to == CT_TO_PINHOLE_NULL_CHECK || to == CT_TO_PINHOLE_CHECK || to == CT_TO_CAHVORE || from == TR_CAM_CAHVORE || ct_lens_to(to);
}

ct_mat ct_matrix(const double* m) {
  ct_mat M{};
  if (m) std::memcpy(M.m, m, sizeof(M.m));
  return M;
}

#define CT_LAUNCH_TO(KERNEL, FROM, TO, FLAG, GRID, ...)                                                                             \
  do {                                                                                                                              \
    switch (TO) {                                                                                                                   \
      case CT_TO_PINHOLE_NOCHECK: hipLaunchKernelGGL((KERNEL<FROM, CT_TO_PINHOLE_NOCHECK, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__); break;       \
      case CT_TO_PINHOLE_NULL_CHECK: hipLaunchKernelGGL((KERNEL<FROM, CT_TO_PINHOLE_NULL_CHECK, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__); break; \
      case CT_TO_PINHOLE_CHECK: hipLaunchKernelGGL((KERNEL<FROM, CT_TO_PINHOLE_CHECK, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__); break;           \
      default: hipLaunchKernelGGL((KERNEL<FROM, CT_TO_CAHV, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__); break;           \
    }                                                                                                                               \
  } while (0)
#define CT_LAUNCH_FROM(KERNEL, FROM, TO, FLAG, GRID, ...)                                                        \
  do {                                                                                                           \
    switch (FROM) {                                                                                              \
      case TR_CAM_PINHOLE_NULL: CT_LAUNCH_TO(KERNEL, TR_CAM_PINHOLE_NULL, TO, FLAG, GRID, __VA_ARGS__); break;   \
      case TR_CAM_PINHOLE: CT_LAUNCH_TO(KERNEL, TR_CAM_PINHOLE, TO, FLAG, GRID, __VA_ARGS__); break;             \
      default: CT_LAUNCH_TO(KERNEL, TR_CAM_CAHV, TO, FLAG, GRID, __VA_ARGS__); break;                            \
    }                                                                                                            \
  } while (0)

// the four pairs with a CAHVOR or CAHVORE camera: the other one is CAHV (ct_pair_check)
#define CT_LAUNCH_NEW(KERNEL, FROM, TO, FLAG, GRID, ...)                                                                                    \
  do {                                                                                                                                      \
    if (FROM == TR_CAM_CAHVOR) hipLaunchKernelGGL((KERNEL<TR_CAM_CAHVOR, CT_TO_CAHV, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__);  \
    else if (FROM == TR_CAM_CAHVORE) hipLaunchKernelGGL((KERNEL<TR_CAM_CAHVORE, CT_TO_CAHV, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__); \
    else if (TO == CT_TO_CAHVOR) hipLaunchKernelGGL((KERNEL<TR_CAM_CAHV, CT_TO_CAHVOR, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<TR_CAM_CAHV, CT_TO_CAHVORE, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__);                      \
  } while (0)
// the five pairs in which a pinhole carries the any-lens code: the other camera is such a pinhole or CAHV
#define CT_LAUNCH_LENS(KERNEL, FROM, TO, FLAG, GRID, ...)                                                                                   \
  do {                                                                                                                                      \
    if (FROM == TR_CAM_CAHV) {                                                                                                              \
      if (TO == CT_TO_PINHOLE_LENS_CHECK) hipLaunchKernelGGL((KERNEL<TR_CAM_CAHV, CT_TO_PINHOLE_LENS_CHECK, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__); \
      else hipLaunchKernelGGL((KERNEL<TR_CAM_CAHV, CT_TO_PINHOLE_LENS_NOCHECK, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__);       \
    } else if (TO == CT_TO_PINHOLE_LENS_CHECK) {                                                                                            \
      hipLaunchKernelGGL((KERNEL<TR_CAM_PINHOLE_LENS, CT_TO_PINHOLE_LENS_CHECK, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__);      \
    } else if (TO == CT_TO_PINHOLE_LENS_NOCHECK) {                                                                                          \
      hipLaunchKernelGGL((KERNEL<TR_CAM_PINHOLE_LENS, CT_TO_PINHOLE_LENS_NOCHECK, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__);    \
    } else {                                                                                                                                \
      hipLaunchKernelGGL((KERNEL<TR_CAM_PINHOLE_LENS, CT_TO_CAHV, FLAG>), (GRID), ct_block, 0, ctx->stream, __VA_ARGS__);                    \
    }                                                                                                                                       \
  } while (0)
bool ct_lens_pair(int from, int to) { return from == TR_CAM_PINHOLE_LENS || ct_lens_to(to); }
bool ct_new_pair(int from, int to) { return from == TR_CAM_CAHVOR || from == TR_CAM_CAHVORE || to == CT_TO_CAHVOR || to == CT_TO_CAHVORE; }

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
  const bool counts = ct_counts(from, to), theta = to == CT_TO_CAHVORE || ct_lens_to(to);
  if (counts) hipLaunchKernelGGL(ct_count_fold_kernel, dim3(theta ? 2 : 1), dim3(CT_THREADS), 0, ctx->stream, d_counter);
  VWGPU_HIP(ctx, hipGetLastError());
  if (d_failed) VWGPU_HIP(ctx, hipMemcpyAsync(d_failed, d_counter, 8, hipMemcpyDeviceToDevice, ctx->stream));
  if (h_failed) {
    unsigned long long cnt = 0, cnt_theta = 0;
    VWGPU_HIP(ctx, hipMemcpyAsync(&cnt, d_counter, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (theta) VWGPU_HIP(ctx, hipMemcpyAsync(&cnt_theta, d_counter + CT_COUNTERS, 8, hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *h_failed = ct_failures{(long long)cnt, (long long)cnt_theta, to == CT_TO_CAHVORE || from == TR_CAM_CAHVORE, ct_lens_to(to)};
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
  if ((rc = ct_pair_check(ctx, name, c.src_cam, c.dst_cam))) return rc;
  return ct_same_center(ctx, c.src_cam, c.dst_cam);
}

// all pointers of `c` are device pointers here
int ct_image_run(vwgpu_ctx* ctx, const ct_image_call& c, long long* d_failed, ct_failures* h_failed) {
  const bool lens = tr_lens_pinhole(*c.dst_cam) || tr_lens_pinhole(*c.src_cam);
  const int from = ct_from_code(*c.dst_cam, lens), to = ct_to_code(*c.src_cam, c.check, lens);
  unsigned long long* d_counter = nullptr;
  const bool want = d_failed || h_failed;
  if (ct_counts(from, to) || want) {
    int rc = ct_counters(ctx, ct_counts(from, to), &d_counter);
    if (rc) return rc;
  }
  ct_args a{c.src, (long long)c.sstride, c.sw, c.sh, c.smask, (long long)c.mstride, c.w, c.h, c.x0, c.y0, ct_cahv_flip(*c.dst_cam),
            c.edge_value, c.edge_valid != 0, c.out, (long long)c.ostride, c.omask, (long long)c.omstride, d_counter};
  const ct_mat M = ct_matrix(c.src_matrix);
  const bool masked = c.smask || c.omask;
  {
    vwgpu_prof_scope ps(ctx, "camera_transform");
    if (ct_lens_pair(from, to)) {
      if (masked) CT_LAUNCH_LENS(ct_image_kernel, from, to, true, ct_grid(c.w, c.h), a, *c.dst_cam, *c.src_cam, M);
      else CT_LAUNCH_LENS(ct_image_kernel, from, to, false, ct_grid(c.w, c.h), a, *c.dst_cam, *c.src_cam, M);
    } else if (ct_new_pair(from, to)) {
      if (masked) CT_LAUNCH_NEW(ct_image_kernel, from, to, true, ct_grid(c.w, c.h), a, *c.dst_cam, *c.src_cam, M);
      else CT_LAUNCH_NEW(ct_image_kernel, from, to, false, ct_grid(c.w, c.h), a, *c.dst_cam, *c.src_cam, M);
    } else if (masked) {
      CT_LAUNCH_FROM(ct_image_kernel, from, to, true, ct_grid(c.w, c.h), a, *c.dst_cam, *c.src_cam, M);
    } else {
      CT_LAUNCH_FROM(ct_image_kernel, from, to, false, ct_grid(c.w, c.h), a, *c.dst_cam, *c.src_cam, M);
    }
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
  if ((rc = ct_pair_check(ctx, name, src, dst))) return rc;
  return ct_same_center(ctx, src, dst);
}

int ct_points_run(vwgpu_ctx* ctx, const vwgpu_camera* src, const double* src_matrix, const vwgpu_camera* dst, const double* dst_matrix,
                  int direction, int check, const double* d_points, long long n, double* d_out, long long* d_failed, ct_failures* h_failed) {
  const bool fwd = direction == VWGPU_CAMERA_TRANSFORM_FORWARD;
  const vwgpu_camera& cfrom = fwd ? *src : *dst;
  const vwgpu_camera& cto = fwd ? *dst : *src;
  const bool lens = tr_lens_pinhole(cfrom) || tr_lens_pinhole(cto);
  const int from = ct_from_code(cfrom, lens), to = ct_to_code(cto, check, lens);
  unsigned long long* d_counter = nullptr;
  const bool want = d_failed || h_failed;
  if (ct_counts(from, to) || want) {
    int rc = ct_counters(ctx, ct_counts(from, to), &d_counter);
    if (rc) return rc;
  }
  ct_points_args a{d_points, d_out, n, ct_cahv_flip(cfrom), d_counter};
  const ct_mat M = ct_matrix(fwd ? dst_matrix : src_matrix);
  const dim3 grid((unsigned)((n + CT_THREADS - 1) / CT_THREADS));
  {
    vwgpu_prof_scope ps(ctx, "camera_transform_points");
    if (ct_lens_pair(from, to)) CT_LAUNCH_LENS(ct_points_kernel, from, to, false, grid, a, cfrom, cto, M);
    else if (ct_new_pair(from, to)) CT_LAUNCH_NEW(ct_points_kernel, from, to, false, grid, a, cfrom, cto, M);
    else CT_LAUNCH_FROM(ct_points_kernel, from, to, false, grid, a, cfrom, cto, M);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (!want) return VWGPU_OK;
  return ct_count_out(ctx, from, to, d_counter, d_failed, h_failed);
}

// ---- host arithmetic -----------------------------------------------------------------------------------------------------

// MatrixMatrixProduct (src/vw/Math/Matrix.h:2081-2086): a dot_prod per element, the accumulator starting from zero
void ct_mat_mul3(const double* a, const double* b, double* out) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += a[i * 3 + k] * b[k * 3 + j];
      out[i * 3 + j] = s;
    }
}

// Quaternion(rotation).rotation_matrix() (Math/Quaternion.h:211-252, :314-329): what camera_pose().rotation_matrix() returns
void ct_pose_round_trip(const double* rot, double* out) {
  const double d0 = rot[0], d1 = rot[4], d2 = rot[8];
  const double ww = 1.0 + d0 + d1 + d2;
  const double xx = 1.0 + d0 - d1 - d2;
  const double yy = 1.0 - d0 + d1 - d2;
  const double zz = 1.0 - d0 - d1 + d2;
  double max = ww;
  if (xx > max) max = xx;
  if (yy > max) max = yy;
  if (zz > max) max = zz;
  double c[4];
  if (ww == max) {
    const double w4 = sqrt(ww * 4.0);
    c[0] = w4 / 4;
    c[1] = (rot[7] - rot[5]) / w4;
    c[2] = (rot[2] - rot[6]) / w4;
    c[3] = (rot[3] - rot[1]) / w4;
  } else if (xx == max) {
    const double x4 = sqrt(xx * 4.0);
    c[0] = (rot[7] - rot[5]) / x4;
    c[1] = x4 / 4;
    c[2] = (rot[1] + rot[3]) / x4;
    c[3] = (rot[2] + rot[6]) / x4;
  } else if (yy == max) {
    const double y4 = sqrt(yy * 4.0);
    c[0] = (rot[2] - rot[6]) / y4;
    c[1] = (rot[1] + rot[3]) / y4;
    c[2] = y4 / 4;
    c[3] = (rot[5] + rot[7]) / y4;
  } else {
    const double z4 = sqrt(zz * 4.0);
    c[0] = (rot[3] - rot[1]) / z4;
    c[1] = (rot[2] + rot[6]) / z4;
    c[2] = (rot[5] + rot[7]) / z4;
    c[3] = z4 / 4;
  }
  const double w = c[0], x = c[1], y = c[2], z = c[3];
  const double w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
  const double wx = w * x, wy = w * y, wz = w * z;
  const double xy = x * y, yz = y * z, zx = z * x;
  out[0] = w2 + x2 - y2 - z2;
  out[4] = w2 - x2 + y2 - z2;
  out[8] = w2 - x2 - y2 + z2;
  out[1] = 2 * (xy - wz);
  out[2] = 2 * (zx + wy);
  out[5] = 2 * (yz - wx);
  out[3] = 2 * (xy + wz);
  out[6] = 2 * (zx - wy);
  out[7] = 2 * (yz + wx);
}

tr_v3 ct_scale(const tr_v3& a, double s) { return tr_v3{a.x * s, a.y * s, a.z * s}; }
tr_v3 ct_div(const tr_v3& a, double s) { return tr_v3{a.x / s, a.y / s, a.z / s}; }
tr_v3 ct_add(const tr_v3& a, const tr_v3& b) { return tr_v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
void ct_store3(const tr_v3& a, double* p) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }

// pixel_to_vector of a CAHVOR or CAHVORE descriptor on the host: the text the kernels run
int ct_host_ray(const vwgpu_camera& c, double x, double y, tr_v3& vec) {
  if (c.kind == VWGPU_CAMERA_CAHVORE) return tr_cahvore_ray(c, tr_v2{x, y}, vec);
  vec = tr_cahvor_ray(c, tr_v2{x, y}, ct_cahv_flip(c) != 0);
  return TR_OK;
}

// the six landmarks on the left and right edge (hpts) and on the top and bottom edge (vpts) of linearize_camera.  The
// midpoints are the reference's: CAHVOR halves in double but for vpts[4] (CAHVORModel.cc:472-484), CAHVORE divides the
// integers everywhere (CAHVOREModel.cc:314-326).
void ct_landmarks(bool cahvore, int w, int h, tr_v2* hpts, tr_v2* vpts) {
  const double xe = w - 1, ye = h - 1;
  const double ymid = cahvore ? (double)((h - 1) / 2) : (h - 1) / 2.0;
  const double xmid1 = cahvore ? (double)((w - 1) / 2) : (w - 1) / 2.0;
  const double xmid4 = (double)((w - 1) / 2);
  hpts[0] = tr_v2{0, 0}; hpts[1] = tr_v2{0, ymid}; hpts[2] = tr_v2{0, ye};
  hpts[3] = tr_v2{xe, 0}; hpts[4] = tr_v2{xe, ymid}; hpts[5] = tr_v2{xe, ye};
  vpts[0] = tr_v2{0, 0}; vpts[1] = tr_v2{xmid1, 0}; vpts[2] = tr_v2{xe, 0};
  vpts[3] = tr_v2{0, ye}; vpts[4] = tr_v2{xmid4, ye}; vpts[5] = tr_v2{xe, ye};
}

// u3 - dot(d, u3) * d, normalised
tr_v3 ct_reject(const tr_v3& u3, const tr_v3& d) {
  const double s = tr_dot(d, u3);
  return tr_normalize(tr_v3{u3.x - s * d.x, u3.y - s * d.y, u3.z - s * d.z});
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------------

extern "C" {

int vwgpu_pinhole_camera_matrix(const double* center, const double* rotation, double fu, double fv, double cu, double cv,
                                const double* u_dir, const double* v_dir, const double* w_dir, double pixel_pitch, int distortion_kind,
                                const double* distortion, double* out) {
  (void)pixel_pitch; (void)distortion;
  if (!center || !rotation || !u_dir || !v_dir || !w_dir || !out) return VWGPU_ERR_ARGUMENT;
  if (distortion_kind != VWGPU_DISTORTION_NULL && distortion_kind != VWGPU_DISTORTION_TSAI) return VWGPU_ERR_ARGUMENT;
  // the asserts of rebuild_camera_matrix (PinholeModel.cc:586-591)
  const tr_v3 u = tr_load3(u_dir), v = tr_load3(v_dir), w = tr_load3(w_dir);
  if (!(tr_dot(u, v) == 0) || !(tr_dot(u, w) == 0) || !(tr_dot(v, w) == 0)) return VWGPU_ERR_ARGUMENT;
  if (!(fabs(tr_norm(u) - 1) < 0.001) || !(fabs(tr_norm(v) - 1) < 0.001) || !(fabs(tr_norm(w) - 1) < 0.001)) return VWGPU_ERR_ARGUMENT;
  const double uvw[9] = {u.x, u.y, u.z, v.x, v.y, v.z, w.x, w.y, w.z};
  const double rt[9] = {rotation[0], rotation[3], rotation[6], rotation[1], rotation[4], rotation[7], rotation[2], rotation[5], rotation[8]};
  double neg_rt[9], r33[9], t33[9], ext[12];
  for (int k = 0; k < 9; ++k) neg_rt[k] = -rt[k];
  ct_mat_mul3(uvw, rt, r33);       // :600
  ct_mat_mul3(uvw, neg_rt, t33);   // :601, (uvwRotation * (-rotation_inverse)) * m_camera_center
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) ext[i * 4 + j] = r33[i * 3 + j];
    ext[i * 4 + 3] = tr_dot(tr_load3(t33 + 3 * i), tr_load3(center));
  }
  const double k[9] = {fu, 0, cu, 0, fv, cv, 0, 0, 1};
  for (int i = 0; i < 3; ++i)      // :603
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      for (int q = 0; q < 3; ++q) s += k[i * 3 + q] * ext[q * 4 + j];
      out[i * 4 + j] = s;
    }
  return VWGPU_OK;
}

int vwgpu_camera_set_lens(vwgpu_camera* cam, int distortion_kind, const double* params, int n) {
  if (!cam || cam->kind != VWGPU_CAMERA_PINHOLE || !tr_lens_known(distortion_kind) || n < 0 || (n > 0 && !params)) return VWGPU_ERR_ARGUMENT;
  bool n_ok = false;
  switch (distortion_kind) {
    case VWGPU_DISTORTION_NULL: n_ok = n == 0; break;
    case VWGPU_DISTORTION_TSAI: n_ok = n == 4 || n == 5; break;
    case VWGPU_DISTORTION_FOV: n_ok = n == 1; break;
    case VWGPU_DISTORTION_FISHEYE: n_ok = n == 4; break;
    case VWGPU_DISTORTION_BROWN_CONRADY: n_ok = n == 8; break;
    case VWGPU_DISTORTION_ADJUSTABLE_TSAI: n_ok = n >= 4 && n <= 13; break;
    default: n_ok = n == 9; break;   // Photometrix
  }
  if (!n_ok) return VWGPU_ERR_ARGUMENT;
  double L[14] = {0};
  for (int k = 0; k < n; ++k) {
    if (!std::isfinite(params[k])) return VWGPU_ERR_ARGUMENT;
    L[k] = params[k];
  }
  if (distortion_kind == VWGPU_DISTORTION_FOV) {
    // FovLensDistortion::set_distortion_parameters (LensDistortion.cc:441-455)
    if (L[0] <= 0) return VWGPU_ERR_ARGUMENT;
    L[1] = 1 / L[0];
    L[2] = 2 * tan(L[0] / 2);
  } else if (distortion_kind == VWGPU_DISTORTION_BROWN_CONRADY) {
    L[8] = sin(L[7]);
    L[9] = cos(L[7]);
  } else if (distortion_kind == VWGPU_DISTORTION_ADJUSTABLE_TSAI) {
    L[13] = (double)n;
  }
  cam->distortion_kind = distortion_kind;
  std::memcpy(cam->distortion, L, 5 * sizeof(double));
  std::memcpy(cam->A, L + 5, 3 * sizeof(double));
  std::memcpy(cam->H, L + 8, 3 * sizeof(double));
  std::memcpy(cam->V, L + 11, 3 * sizeof(double));
  return VWGPU_OK;
}

int vwgpu_lens_coordinates(const vwgpu_camera* cam, int direction, const double* points, long long n, double* out, long long* failed) {
  if (failed) *failed = 0;
  if (!cam || cam->kind != VWGPU_CAMERA_PINHOLE || !tr_lens_valid(*cam) || (direction != 0 && direction != 1) || n < 0 ||
      (n > 0 && (!points || !out)))
    return VWGPU_ERR_ARGUMENT;
  const vwgpu_camera c = *cam;
  long long count = 0;
  for (long long i = 0; i < n; ++i) {
    const tr_v2 p{points[2 * i], points[2 * i + 1]};
    tr_v2 q;
    if (direction == 1) {
      q = tr_lens_undistort(c, p);
    } else if (!ct_lens_distort(c, p, q)) {
      q = tr_v2{std::nan(""), std::nan("")};
      ++count;
    }
    out[2 * i] = q.x;
    out[2 * i + 1] = q.y;
  }
  if (failed) *failed = count;
  return count != 0 ? VWGPU_ERR_LOGIC : VWGPU_OK;
}

int vwgpu_epipolar_pinhole(const double* center0, const double* rotation0, const double* focal0, const double* offset0, double pitch0,
                           const double* center1, const double* rotation1, const double* focal1, const double* offset1, double pitch1,
                           double* rotation, double* focal, double* offset, double* pitch) {
  if (!center0 || !rotation0 || !focal0 || !offset0 || !center1 || !rotation1 || !focal1 || !offset1 || !rotation || !focal || !offset ||
      !pitch)
    return VWGPU_ERR_ARGUMENT;
  const tr_v3 c0 = tr_load3(center0), c1 = tr_load3(center1);
  if (c0.x == c1.x && c0.y == c1.y && c0.z == c1.z) return VWGPU_ERR_ARGUMENT;   // no baseline
  double rot0[9], rot1[9];
  ct_pose_round_trip(rotation0, rot0);
  ct_pose_round_trip(rotation1, rot1);
  const tr_v3 look0{-1 * rot0[2], -1 * rot0[5], -1 * rot0[8]}, look1{-1 * rot1[2], -1 * rot1[5], -1 * rot1[8]};
  const tr_v3 u = ct_div(tr_sub(c1, c0), tr_norm(tr_sub(c1, c0)));
  const tr_v3 mean_look = ct_div(ct_add(look0, look1), 2.0);
  const tr_v3 temp = tr_cross(u, tr_cross(mean_look, u));
  const tr_v3 w = ct_div(temp, tr_norm(temp));
  const tr_v3 v = tr_cross(w, u);
  const double new_rot[9] = {u.x, -v.x, -w.x, u.y, -v.y, -w.y, u.z, -v.z, -w.z};
  std::memcpy(rotation, new_rot, sizeof(new_rot));
  focal[0] = (focal0[0] + focal1[0]) / 2.0;
  focal[1] = (focal0[1] + focal1[1]) / 2.0;
  offset[0] = (offset0[0] + offset1[0]) / 2.0;
  offset[1] = (offset0[1] + offset1[1]) / 2.0;
  *pitch = (pitch0 + pitch1) / 2.0;
  return VWGPU_OK;
}

int vwgpu_epipolar_cahv(const vwgpu_camera* src0, const vwgpu_camera* src1, vwgpu_camera* dst0, vwgpu_camera* dst1) {
  if (!src0 || !src1 || !dst0 || !dst1) return VWGPU_ERR_ARGUMENT;
  if (src0->kind != VWGPU_CAMERA_CAHV || src1->kind != VWGPU_CAMERA_CAHV) return VWGPU_ERR_ARGUMENT;
  const tr_v3 C0 = tr_load3(src0->center), C1 = tr_load3(src1->center);
  if (C0.x == C1.x && C0.y == C1.y && C0.z == C1.z) return VWGPU_ERR_ARGUMENT;
  const tr_v3 A0 = tr_load3(src0->A), H0 = tr_load3(src0->H), V0 = tr_load3(src0->V);
  const tr_v3 A1 = tr_load3(src1->A), H1 = tr_load3(src1->H), V1 = tr_load3(src1->V);
  const double hc = tr_dot(H0, A0) / 2.0 + tr_dot(H1, A1) / 2.0;
  const double vc = tr_dot(V0, A0) / 2.0 + tr_dot(V1, A1) / 2.0;
  const double hs = tr_norm(tr_cross(A0, H0)) / 2.0 + tr_norm(tr_cross(A1, H1)) / 2.0;
  const double vs = tr_norm(tr_cross(A0, V0)) / 2.0 + tr_norm(tr_cross(A1, V1)) / 2.0;
  tr_v3 app = ct_add(A0, A1);
  const tr_v3 f = tr_cross(tr_cross(app, tr_sub(C1, C0)), app);
  tr_v3 hp;
  if (tr_dot(f, H0) > 0) hp = ct_div(ct_scale(f, hs), tr_norm(f));
  else hp = ct_div(ct_scale(tr_v3{-f.x, -f.y, -f.z}, hs), tr_norm(f));
  app = ct_scale(app, 0.5);
  const tr_v3 g = ct_div(ct_scale(hp, tr_dot(app, hp)), hs * hs);
  const tr_v3 a = tr_normalize(tr_sub(app, g));
  const tr_v3 vp = ct_div(ct_scale(tr_cross(a, hp), vs), hs);
  vwgpu_camera out{};
  out.kind = VWGPU_CAMERA_CAHV;
  ct_store3(a, out.A);
  ct_store3(ct_add(hp, ct_scale(a, hc)), out.H);
  ct_store3(ct_add(vp, ct_scale(a, vc)), out.V);
  ct_store3(C1, out.center);
  const vwgpu_camera second = out;
  ct_store3(C0, out.center);
  *dst0 = out;
  *dst1 = second;
  return VWGPU_OK;
}

int vwgpu_cahvor_camera(const double* C, const double* A, const double* H, const double* V, const double* O, const double* R,
                        vwgpu_camera* out) {
  if (!C || !A || !H || !V || !O || !R || !out) return VWGPU_ERR_ARGUMENT;
  std::memset(out, 0, sizeof(*out));
  out->kind = VWGPU_CAMERA_CAHVOR;
  std::memcpy(out->center, C, sizeof(out->center));
  std::memcpy(out->A, A, sizeof(out->A));
  std::memcpy(out->H, H, sizeof(out->H));
  std::memcpy(out->V, V, sizeof(out->V));
  std::memcpy(out->inv_camera_transform, O, 3 * sizeof(double));
  std::memcpy(out->inv_camera_transform + 3, R, 3 * sizeof(double));
  return VWGPU_OK;
}

int vwgpu_cahvore_camera(const double* C, const double* A, const double* H, const double* V, const double* O, const double* R,
                         const double* E, int type, double P, vwgpu_camera* out) {
  if (!E) return VWGPU_ERR_ARGUMENT;
  // CAHVOREModel(C, A, H, V, O, R, E, T, P) (CAHVOREModel.cc:111-124)
  switch (type) {
    case 1: P = 1.0; break;
    case 2: P = 0.0; break;
    case 3:
      if (P < 0 || P > 1 || P != P) return VWGPU_ERR_ARGUMENT;
      break;
    default: return VWGPU_ERR_ARGUMENT;
  }
  int rc = vwgpu_cahvor_camera(C, A, H, V, O, R, out);
  if (rc) return rc;
  out->kind = VWGPU_CAMERA_CAHVORE;
  std::memcpy(out->inv_camera_transform + 6, E, 3 * sizeof(double));
  out->distortion[0] = P;
  return VWGPU_OK;
}

int vwgpu_linearize_camera(const vwgpu_camera* src, int in_w, int in_h, int out_w, int out_h, vwgpu_camera* dst) {
  if (!src || !dst || !tr_new_kind(*src) || in_w <= 0 || in_h <= 0 || out_w <= 0 || out_h <= 0) return VWGPU_ERR_ARGUMENT;
  const vwgpu_camera cam = *src;   // dst may be src
  const bool cahvore = cam.kind == VWGPU_CAMERA_CAHVORE;
  tr_v2 hpts[6], vpts[6];
  ct_landmarks(cahvore, in_w, in_h, hpts, vpts);
  tr_v3 hray[6], vray[6];
  for (int k = 0; k < 6; ++k)
    if (ct_host_ray(cam, hpts[k].x, hpts[k].y, hray[k]) != TR_OK || ct_host_ray(cam, vpts[k].x, vpts[k].y, vray[k]) != TR_OK) return VWGPU_ERR_LOGIC;
  tr_v3 A{0.0, 0.0, 0.0};
  if (cahvore) {
    // the ray of the real-valued centre (CAHVOREModel.cc:329-330)
    if (ct_host_ray(cam, (in_w - 1) / 2.0, (in_h - 1) / 2.0, A) != TR_OK) return VWGPU_ERR_LOGIC;
  } else {
    // the normalised sum over vpts, then hpts (CAHVORModel.cc:486-492)
    for (int k = 0; k < 6; ++k) A = ct_add(A, vray[k]);
    for (int k = 0; k < 6; ++k) A = ct_add(A, hray[k]);
    A = tr_normalize(A);
  }
  // the original right and down vectors, made orthogonal to the new axis
  const tr_v3 srcA = tr_load3(cam.A), srcH = tr_load3(cam.H);
  tr_v3 dn = tr_cross(srcA, srcH);
  tr_v3 rt = tr_normalize(tr_cross(dn, srcA));
  dn = tr_normalize(dn);
  rt = tr_cross(dn, A);
  dn = tr_normalize(tr_cross(A, rt));
  rt = tr_normalize(rt);
  double hmin = 1, hmax = -1, vmin = 1, vmax = -1;
  for (int k = 0; k < 6; ++k) {
    const tr_v3 n = ct_reject(hray[k], dn);
    const double v = cahvore ? tr_dot(A, n) : tr_norm(tr_cross(A, n));
    if (hmin > v) hmin = v;
    if (hmax < v) hmax = v;
  }
  for (int k = 0; k < 6; ++k) {
    const tr_v3 n = ct_reject(vray[k], rt);
    const double v = cahvore ? tr_dot(A, n) : tr_norm(tr_cross(A, n));
    if (vmin > v) vmin = v;
    if (vmax < v) vmax = v;
  }
  double scale[2], centre[2] = {(out_w - 1) / 2.0, (out_h - 1) / 2.0};
  if (cahvore) {
    // minfov: the larger cosines, limited to a field of view of 135 degrees (CAHVOREModel.cc:359-371)
    const double limfov = 3.14159265358979323846 * 3 / 4;
    double cosines[2] = {hmax, vmax};
    if (acos(cosines[0]) > limfov) cosines[0] = cos(limfov);
    if (acos(cosines[1]) > limfov) cosines[1] = cos(limfov);
    scale[0] = (out_w / 2.0 * cosines[0]) / sqrt(1 - cosines[0] * cosines[0]);
    scale[1] = (out_h / 2.0 * cosines[1]) / sqrt(1 - cosines[1] * cosines[1]);
  } else {
    // minfov: the smaller sines (CAHVORModel.cc:527-534)
    const double c2[2] = {centre[0] * centre[0], centre[1] * centre[1]};
    scale[0] = sqrt(c2[0] / (hmin * hmin) - c2[0]);
    scale[1] = sqrt(c2[1] / (vmin * vmin) - c2[1]);
  }
  vwgpu_camera out{};
  out.kind = VWGPU_CAMERA_CAHV;
  std::memcpy(out.center, cam.center, sizeof(out.center));
  ct_store3(A, out.A);
  ct_store3(ct_add(ct_scale(rt, scale[0]), ct_scale(A, centre[0])), out.H);
  ct_store3(ct_add(ct_scale(dn, scale[1]), ct_scale(A, centre[1])), out.V);
  *dst = out;
  return VWGPU_OK;
}

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
