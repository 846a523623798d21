// triangulate.hip — from a disparity map and two cameras to a point image: src/vw/Stereo/StereoModel.{h,cc} for two
// cameras (triangulate_pair :35-48, are_nearly_parallel :68-91, operator()(pixVec, errorVec) :97-147, convergence_angle
// :174-177, the image overload with its statistics :254-309), StereoView::operator() (src/vw/Stereo/StereoView.h:91-99)
// with DispHelper (:37-53) and UniverseRadiusFunc (:139-222).  The rays come from the part of vw::camera this needs:
// PinholeModel::pixel_to_vector (src/vw/Camera/PinholeModel.cc:422-434) with the null and the Tsai lens distortion
// (src/vw/Camera/LensDistortion.cc:260-400 over src/vw/Math/NewtonRaphson.cc:58-119) and CAHVModel::pixel_to_vector
// (src/vw/Camera/CAHVModel.cc:173-189).  tests/refimpl/triangulate_ref.cc restates them and DESIGN §4.18 lists what is
// reproduced.
//
// One lane per pixel, blocks of 64 x 4, every band of four rows a workgroup of its own, no neighbourhood and no LDS (the
// statistics variant keeps one partial per wavefront there).  The cameras arrive by value: they are uniform and are read
// through scalar loads.  A lane reads the 12 bytes of its pixel and writes 24 contiguous bytes of xyz, so a wavefront's
// stores cover 1536 contiguous bytes.  The kernels are instantiated per pair of camera codes (camera_rays.h), so that
// the common case, two pinholes without lens distortion, carries no Newton loop; the table tr_pairs lists the pairs
// that exist, and a pair without a row is refused.  A CAHVORE ray that does not converge gives the zero point.
// vwgpu_pinhole_camera, pure host arithmetic, is in camera_host.hip.
//
// Everything is double in the reference's expression order; the Makefile's -ffp-contract=off keeps products and sums
// apart, and fp64 division and square root are correctly rounded on the device.  Sums written `0.0 + ...` are the
// reference's accumulators (dot_prod, norm_2_sqr: src/vw/Math/Vector.h:1593-1598, :1719-1726), which start from zero.
#include <cmath>
#include <cstring>

#include "camera_rays.h"
#include "vwgpu_internal.h"

namespace {

constexpr int TR_BX = 64, TR_BY = 4, TR_THREADS = TR_BX * TR_BY;
constexpr int TR_LAYOUT_MASK = 0x300;
constexpr long long TR_FOLD_CHUNK = 2048;   // partials one workgroup of the first fold level takes

__device__ inline bool tr_pixel_skipped(const tr_v2& pix) {
  return pix.x != pix.x || pix.y != pix.y || (pix.x == -1e8 && pix.y == -1e8);   // StereoModel.cc:117-119
}

// ---- the pixel pair --------------------------------------------------------------------------------------------------
struct tr_args {
  const uint32_t* disp;
  long long dstride;
  int w, h;
  int x0, y0;
  int int_type, layout, model;
  int flip1, flip2;   // CAHV and CAHVOR cameras: dot(cross(V, H), A) < 0
  double tol;
  double* xyz;
  long long xstride;
  double* error;
  long long estride;
  double* errvec;
  long long vstride;
  vwgpu_triangulate_stats* partial;
};

// the disparity pixel (x, y) in the layouts of DispHelper (StereoView.h:37-53): words {a, b} and whether it is valid
__device__ inline bool tr_load_disp(const tr_args& a, int x, int y, uint32_t& da, uint32_t& db) {
  const long long i = (long long)y * a.dstride + x;
  uint32_t v;
  // word by word (the compiler merges them into one access): a pixel struct chosen in a switch goes through private memory
  switch (a.layout) {
    case VWGPU_DISPARITY_LAYOUT_DXDYV: {
      const uint32_t* q = a.disp + i * 3;
      da = q[0]; db = q[1]; v = q[2];
      break;
    }
    case VWGPU_DISPARITY_LAYOUT_DXDY: {
      const uint32_t* q = a.disp + i * 2;
      da = q[0]; db = q[1];
      return true;
    }
    case VWGPU_DISPARITY_LAYOUT_DV: {
      const uint32_t* q = a.disp + i * 2;
      da = q[0]; db = 0; v = q[1];   // 0 is +0.0f and 0: DispHelper's second component
      break;
    }
    default:
      da = a.disp[i]; db = 0;
      return true;
  }
  return a.int_type ? v != 0 : __uint_as_float(v) != 0.f;
}

__device__ inline void tr_pixel_pair(const tr_args& a, int x, int y, uint32_t da, uint32_t db, tr_v2& pix1, tr_v2& pix2) {
  const long long ix = (long long)a.x0 + x, iy = (long long)a.y0 + y;
  pix1 = tr_v2{(double)ix, (double)iy};
  if (a.model) {
    // StereoModel.cc:278-280: int32 + float in float (int32 + int32 in int32), then widened
    if (a.int_type) {
      pix2.x = (double)(int32_t)((uint32_t)ix + da);
      pix2.y = (double)(int32_t)((uint32_t)iy + db);
    } else {
      const float fx = (float)(int32_t)ix + __uint_as_float(da), fy = (float)(int32_t)iy + __uint_as_float(db);
      pix2.x = (double)fx;
      pix2.y = (double)fy;
    }
  } else {
    // StereoView.h:94-95: Vector2(i, j) + Vector2((double)dx, (double)dy)
    pix2.x = pix1.x + (a.int_type ? (double)(int32_t)da : (double)__uint_as_float(da));
    pix2.y = pix1.y + (a.int_type ? (double)(int32_t)db : (double)__uint_as_float(db));
  }
}

// StereoModel::operator()(pixVec, errorVec) for two cameras (StereoModel.cc:97-147)
template <int CAM1, int CAM2>
__device__ inline tr_v3 tr_triangulate(const tr_args& a, const vwgpu_camera& cam1, const vwgpu_camera& cam2, const tr_v2& pix1,
                                       const tr_v2& pix2, tr_v3& errorVec) {
  const double tol = a.tol;
  errorVec = tr_v3{0.0, 0.0, 0.0};
  const tr_v3 zero{0.0, 0.0, 0.0};
  if (tr_pixel_skipped(pix1) || tr_pixel_skipped(pix2)) return zero;   // fewer than two rays
  // a ray with a Newton loop first: fewer scalar registers stay live across the loop (the values do not depend on the order)
  tr_v3 dir0, dir1;
  if (CAM1 == TR_CAM_CAHVOR || CAM1 == TR_CAM_CAHVORE) {
    // catch (PixelToRayErr) (:144-146): the zero point and the zero error vector
    const int s0 = tr_ray_status<CAM1>(cam1, pix1, a.flip1 != 0, dir0), s1 = tr_ray_status<CAM2>(cam2, pix2, a.flip2 != 0, dir1);
    if (s0 != TR_OK || s1 != TR_OK) return zero;
  } else if (CAM1 == TR_CAM_CAHV && CAM2 == TR_CAM_PINHOLE) {
    dir1 = tr_ray<CAM2>(cam2, pix2, false);
    dir0 = tr_ray<CAM1>(cam1, pix1, a.flip1 != 0);
  } else {
    dir0 = tr_ray<CAM1>(cam1, pix1, a.flip1 != 0);
    dir1 = tr_ray<CAM2>(cam2, pix2, a.flip2 != 0);
  }
  const tr_v3 ctr0 = tr_load3(cam1.center), ctr1 = tr_load3(cam2.center);
  if (!(1 - tr_dot(dir0, dir1) >= tol)) return zero;   // are_nearly_parallel (:85-90)
  // triangulate_pair (:35-48)
  const tr_v3 v12 = tr_cross(dir0, dir1);
  const tr_v3 v1 = tr_cross(v12, dir0);
  const tr_v3 v2 = tr_cross(v12, dir1);
  const double s1 = tr_dot(v2, tr_sub(ctr1, ctr0)) / tr_dot(v2, dir0);
  const double s2 = tr_dot(v1, tr_sub(ctr0, ctr1)) / tr_dot(v1, dir1);
  const tr_v3 closestPoint1{ctr0.x + s1 * dir0.x, ctr0.y + s1 * dir0.y, ctr0.z + s1 * dir0.z};
  const tr_v3 closestPoint2{ctr1.x + s2 * dir1.x, ctr1.y + s2 * dir1.y, ctr1.z + s2 * dir1.z};
  errorVec = tr_sub(closestPoint1, closestPoint2);
  tr_v3 result{0.5 * (closestPoint1.x + closestPoint2.x), 0.5 * (closestPoint1.y + closestPoint2.y),
               0.5 * (closestPoint1.z + closestPoint2.z)};
  // reflect points that fall behind one of the two cameras (:136-140)
  const bool reflect = tr_dot(tr_sub(result, ctr0), dir0) < 0 || tr_dot(tr_sub(result, ctr1), dir1) < 0;
  if (reflect) result = tr_v3{-result.x + 2 * ctr0.x, -result.y + 2 * ctr0.y, -result.z + 2 * ctr0.z};
  return result;
}

// ---- statistics: lanes of a wavefront by shuffles, wavefronts through LDS, in a fixed order --------------------------
struct tr_acc {
  long long n;
  double mx, sum;
};
__device__ inline void tr_acc_merge(tr_acc& r, const tr_acc& o) {
  r.n += o.n;
  r.mx = o.mx > r.mx ? o.mx : r.mx;
  r.sum += o.sum;
}
__device__ inline void tr_acc_block_reduce(tr_acc& r, tr_acc* lds, int tid, int nthreads) {
  const int ws = warpSize;
  for (int d = ws >> 1; d > 0; d >>= 1) {
    tr_acc o;
    o.n = __shfl_down(r.n, d);
    o.mx = __shfl_down(r.mx, d);
    o.sum = __shfl_down(r.sum, d);
    tr_acc_merge(r, o);
  }
  const int lane = tid % ws, wave = tid / ws, nw = (nthreads + ws - 1) / ws;
  if (lane == 0) lds[wave] = r;
  __syncthreads();
  if (tid == 0)
    for (int k = 1; k < nw; ++k) tr_acc_merge(r, lds[k]);
}

// one pixel of the point image, and its share of the statistics
template <int CAM1, int CAM2, bool STATS>
__device__ inline void tr_pixel(const tr_args& a, const vwgpu_camera& cam1, const vwgpu_camera& cam2, int x, int y, tr_acc& acc) {
  uint32_t da, db;
  tr_v3 p{0.0, 0.0, 0.0}, ev{0.0, 0.0, 0.0};
  double err = 0.0;
  if (tr_load_disp(a, x, y, da, db)) {
    tr_v2 pix1, pix2;
    tr_pixel_pair(a, x, y, da, db, pix1, pix2);
    p = tr_triangulate<CAM1, CAM2>(a, cam1, cam2, pix1, pix2, ev);
    err = tr_norm(ev);
    if (err >= 0) {
      if (STATS) {
        acc.n += 1;
        acc.mx = err > acc.mx ? err : acc.mx;
        acc.sum += err;
      }
    } else if (a.model) {
      p.x = p.y = p.z = 0.0;   // StereoModel.cc:289-293
    }
  }
  double* o = a.xyz + ((long long)y * a.xstride + x) * 3;
  o[0] = p.x; o[1] = p.y; o[2] = p.z;
  if (a.error) a.error[(long long)y * a.estride + x] = err;
  if (a.errvec) {
    double* e = a.errvec + ((long long)y * a.vstride + x) * 3;
    e[0] = ev.x; e[1] = ev.y; e[2] = ev.z;
  }
}

template <int CAM1, int CAM2>
__global__ __launch_bounds__(TR_THREADS) void tr_triangulate_kernel(tr_args a, vwgpu_camera cam1, vwgpu_camera cam2) {
  int x, y;
  long long band;
  tr_acc acc{0, 0.0, 0.0};
  if (tr_band_position<TR_BX, TR_BY>(a.w, a.h, x, y, band)) tr_pixel<CAM1, CAM2, false>(a, cam1, cam2, x, y, acc);
}

// the statistics variant: one partial per workgroup
template <int CAM1, int CAM2>
__global__ __launch_bounds__(TR_THREADS) void tr_triangulate_stats_kernel(tr_args a, vwgpu_camera cam1, vwgpu_camera cam2) {
  __shared__ tr_acc lds[TR_THREADS / 32];
  int x, y;
  long long band;
  tr_acc acc{0, 0.0, 0.0};
  if (tr_band_position<TR_BX, TR_BY>(a.w, a.h, x, y, band)) tr_pixel<CAM1, CAM2, true>(a, cam1, cam2, x, y, acc);
  tr_acc_block_reduce(acc, lds, threadIdx.y * TR_BX + threadIdx.x, TR_THREADS);
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    vwgpu_triangulate_stats* s = a.partial + (band * gridDim.x + blockIdx.x);
    s->point_count = acc.n;
    s->max_error = acc.mx;
    s->sum_error = acc.sum;
  }
}

// workgroup b folds partial[b * chunk, (b + 1) * chunk) into out[b]: lane by lane in index order, then the block reduction
__global__ __launch_bounds__(TR_THREADS) void tr_stats_fold_kernel(const vwgpu_triangulate_stats* partial, long long npartial,
                                                                   long long chunk, vwgpu_triangulate_stats* out) {
  __shared__ tr_acc lds[TR_THREADS / 32];
  tr_acc r{0, 0.0, 0.0};
  const long long lo = (long long)blockIdx.x * chunk, hi = lo + chunk < npartial ? lo + chunk : npartial;
  for (long long k = lo + threadIdx.x; k < hi; k += blockDim.x) {
    const vwgpu_triangulate_stats s = partial[k];
    tr_acc_merge(r, tr_acc{s.point_count, s.max_error, s.sum_error});
  }
  tr_acc_block_reduce(r, lds, threadIdx.x, blockDim.x);
  if (threadIdx.x == 0) {
    vwgpu_triangulate_stats* o = out + blockIdx.x;
    o->point_count = r.n;
    o->max_error = r.mx;
    o->sum_error = r.sum;
  }
}

// StereoModel::convergence_angle (StereoModel.cc:174-177)
template <int CAM1, int CAM2>
__global__ __launch_bounds__(TR_THREADS) void tr_angle_kernel(tr_args a, vwgpu_camera cam1, vwgpu_camera cam2) {
  int x, y;
  long long band;
  if (!tr_band_position<TR_BX, TR_BY>(a.w, a.h, x, y, band)) return;
  uint32_t da, db;
  double ang = 0.0;
  if (tr_load_disp(a, x, y, da, db)) {
    tr_v2 pix1, pix2;
    tr_pixel_pair(a, x, y, da, db, pix1, pix2);
    tr_v3 dir0, dir1;
    const int s0 = tr_ray_status<CAM1>(cam1, pix1, a.flip1 != 0, dir0), s1 = tr_ray_status<CAM2>(cam2, pix2, a.flip2 != 0, dir1);
    // where CAHVOREModel::pixel_to_vector throws the reference has no angle: NaN
    ang = s0 == TR_OK && s1 == TR_OK ? acos(tr_dot(dir0, dir1)) : __longlong_as_double(0x7ff8000000000000LL);
  }
  a.error[(long long)y * a.estride + x] = ang;
}

// UniverseRadiusFunc::operator() (StereoView.h:172-220) for Vector<double, 3 | 4 | 6>.  The rejected pixels of a workgroup are
// counted together and added to one of TR_COUNTERS words chosen by the workgroup's number: a single word would take
// an atomic per workgroup, and on a 4096^2 image those queue up for longer than the image takes to stream.
constexpr int TR_COUNTERS = 1024;
struct tr_universe_args {
  const double* in;
  long long istride;
  int w, h;
  double ox, oy, oz, near_radius, far_radius;
  double* out;
  long long ostride;
  unsigned long long* rejected;   // TR_COUNTERS words
};
template <int CH>
__global__ __launch_bounds__(TR_THREADS) void tr_universe_kernel(tr_universe_args a) {
  int x, y;
  long long band;
  bool rejected = false;
  if (tr_band_position<TR_BX, TR_BY>(a.w, a.h, x, y, band)) {
    const double* p = a.in + ((long long)y * a.istride + x) * CH;
    double v[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) v[k] = p[k];
    bool keep = false;
    if (v[0] != 0.0 || v[1] != 0.0 || v[2] != 0.0) {
      const double dist = tr_norm(tr_v3{v[0] - a.ox, v[1] - a.oy, v[2] - a.oz});
      rejected = (a.near_radius != 0 && dist < a.near_radius) || (a.far_radius != 0 && dist > a.far_radius);
      keep = !rejected;
    }
    double* o = a.out + ((long long)y * a.ostride + x) * CH;
#pragma unroll
    for (int k = 0; k < CH; ++k) o[k] = keep ? v[k] : 0.0;
  }
  const int n = __syncthreads_count(rejected);
  if (n != 0 && threadIdx.x == 0 && threadIdx.y == 0)
    atomicAdd(a.rejected + (unsigned)((band * gridDim.x + blockIdx.x) % TR_COUNTERS), (unsigned long long)n);
}
// the sum of the TR_COUNTERS words into word 0 (integers: any order)
__global__ __launch_bounds__(TR_THREADS) void tr_universe_fold_kernel(unsigned long long* counters) {
  __shared__ unsigned long long lds[TR_THREADS];
  unsigned long long s = 0;
  for (int k = threadIdx.x; k < TR_COUNTERS; k += TR_THREADS) s += counters[k];
  lds[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < TR_THREADS; ++k) s += lds[k];
    counters[0] = s;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

const dim3 tr_block(TR_BX, TR_BY);
dim3 tr_grid(int w, int h) { return tr_band_grid<TR_BX, TR_BY>(w, h); }

int tr_elem_words(int layout) {
  return layout == VWGPU_DISPARITY_LAYOUT_DXDYV ? 3 : layout == VWGPU_DISPARITY_LAYOUT_D ? 1 : 2;
}

// The camera pairs that have kernels, one row each: the codes of the two cameras and the three kernels instantiated for
// them.  Two pinholes without lens distortion, the other null / Tsai pinhole pairs, the three pairs with a CAHV camera,
// two CAHVOR and two CAHVORE cameras, and the three pairs in which a pinhole carries the any-lens code.  A pair without
// a row has no kernel (tr_check).
using tr_kernel = void (*)(tr_args, vwgpu_camera, vwgpu_camera);
struct tr_pair {
  int cam1, cam2;
  tr_kernel triangulate, triangulate_stats, angle;
};
#define TR_ROW(C1, C2) {C1, C2, tr_triangulate_kernel<C1, C2>, tr_triangulate_stats_kernel<C1, C2>, tr_angle_kernel<C1, C2>}
const tr_pair tr_pairs[] = {
  TR_ROW(TR_CAM_PINHOLE_NULL, TR_CAM_PINHOLE_NULL),
  TR_ROW(TR_CAM_PINHOLE, TR_CAM_PINHOLE),
  TR_ROW(TR_CAM_PINHOLE, TR_CAM_CAHV),
  TR_ROW(TR_CAM_CAHV, TR_CAM_PINHOLE),
  TR_ROW(TR_CAM_CAHV, TR_CAM_CAHV),
  TR_ROW(TR_CAM_CAHVOR, TR_CAM_CAHVOR),
  TR_ROW(TR_CAM_CAHVORE, TR_CAM_CAHVORE),
  TR_ROW(TR_CAM_PINHOLE_LENS, TR_CAM_PINHOLE_LENS),
  TR_ROW(TR_CAM_PINHOLE_LENS, TR_CAM_CAHV),
  TR_ROW(TR_CAM_CAHV, TR_CAM_PINHOLE_LENS),
};
#undef TR_ROW

// the row of a camera pair, or nullptr.  The codes are those of tr_camera_code, but a pinhole takes the no-lens code only
// when both cameras are pinholes without lens distortion: the common case carries no Newton loop.
const tr_pair* tr_cams_of(const vwgpu_camera& c1, const vwgpu_camera& c2) {
  const bool lens = tr_lens_pinhole(c1) || tr_lens_pinhole(c2);
  int k1 = tr_camera_code(c1, lens), k2 = tr_camera_code(c2, lens);
  if (k1 != k2) {
    if (k1 == TR_CAM_PINHOLE_NULL) k1 = TR_CAM_PINHOLE;
    if (k2 == TR_CAM_PINHOLE_NULL) k2 = TR_CAM_PINHOLE;
  }
  for (const tr_pair& row : tr_pairs)
    if (row.cam1 == k1 && row.cam2 == k2) return &row;
  return nullptr;
}

// the checks the triangulation and the convergence angle share; strides of 0 become the packed ones
int tr_check(vwgpu_ctx* ctx, const char* name, int type, const void* disp, int w, int h, ptrdiff_t& dstride, const vwgpu_camera* cam1,
             const vwgpu_camera* cam2, int semantics) {
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (type != VWGPU_DISPARITY_I32 && type != VWGPU_DISPARITY_F32)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: disparity type %d is neither int32 nor float", name, type);
  if (!disp || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: empty image or null pointer", name);
  const int sem = semantics & ~TR_LAYOUT_MASK;
  if (semantics < 0 || (sem != VWGPU_TRIANGULATE_VIEW && sem != VWGPU_TRIANGULATE_MODEL))
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: semantics %d is neither view nor model, with a disparity layout", name, semantics);
  int rc = tr_camera_check(ctx, name, nullptr, cam1);
  if (rc) return rc;
  if ((rc = tr_camera_check(ctx, name, nullptr, cam2))) return rc;
  if (!tr_cams_of(*cam1, *cam2))
    return vwgpu_fail(ctx, VWGPU_ERR_NOIMPL, "%s: no kernel for the pair %s + %s: a CAHVOR or CAHVORE camera goes with one of its own kind", name,
                      tr_kind_name(*cam1), tr_kind_name(*cam2));
  if (dstride == 0) dstride = w;
  if (dstride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
  return VWGPU_OK;
}

int tr_out_stride(vwgpu_ctx* ctx, const char* name, const void* p, ptrdiff_t& stride, int w) {
  if (!p) return VWGPU_OK;
  if (stride == 0) stride = w;
  if (stride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
  return VWGPU_OK;
}

int triangulate_check(vwgpu_ctx* ctx, int type, const void* disp, int w, int h, ptrdiff_t& dstride, const vwgpu_camera* cam1,
                      const vwgpu_camera* cam2, double angle_tol, int semantics, const double* xyz, ptrdiff_t& xstride,
                      const double* error, ptrdiff_t& estride, const double* errvec, ptrdiff_t& vstride) {
  const char* name = "stereo_triangulate";
  int rc = tr_check(ctx, name, type, disp, w, h, dstride, cam1, cam2, semantics);
  if (rc) return rc;
  if (!xyz) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: empty image or null pointer", name);
  if (std::isnan(angle_tol)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: angle_tol is NaN", name);
  if (xyz == error || xyz == errvec || (error && error == errvec) || (const void*)xyz == disp || (const void*)error == disp ||
      (const void*)errvec == disp)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: the images must be different", name);
  if ((rc = tr_out_stride(ctx, name, xyz, xstride, w))) return rc;
  if ((rc = tr_out_stride(ctx, name, error, estride, w))) return rc;
  return tr_out_stride(ctx, name, errvec, vstride, w);
}

tr_args tr_make_args(int type, const void* d_disp, int w, int h, ptrdiff_t dstride, int x0, int y0, int semantics, const vwgpu_camera& cam1,
                     const vwgpu_camera& cam2) {
  tr_args a{};
  a.flip1 = tr_cahv_flip(cam1);
  a.flip2 = tr_cahv_flip(cam2);
  a.disp = static_cast<const uint32_t*>(d_disp);
  a.dstride = dstride; a.w = w; a.h = h; a.x0 = x0; a.y0 = y0;
  a.int_type = type == VWGPU_DISPARITY_I32;
  a.layout = semantics & TR_LAYOUT_MASK;
  a.model = (semantics & ~TR_LAYOUT_MASK) == VWGPU_TRIANGULATE_MODEL;
  return a;
}

int triangulate_run(vwgpu_ctx* ctx, int type, const void* d_disp, int w, int h, ptrdiff_t dstride, int x0, int y0,
                    const vwgpu_camera* cam1, const vwgpu_camera* cam2, double angle_tol, int semantics, double* d_xyz, ptrdiff_t xstride,
                    double* d_error, ptrdiff_t estride, double* d_errvec, ptrdiff_t vstride, vwgpu_triangulate_stats* d_stats) {
  tr_args a = tr_make_args(type, d_disp, w, h, dstride, x0, y0, semantics, *cam1, *cam2);
  a.tol = angle_tol > 0 ? angle_tol : 1e-4;   // StereoModel.cc:81-83
  a.xyz = d_xyz; a.xstride = xstride; a.error = d_error; a.estride = estride; a.errvec = d_errvec; a.vstride = vstride;
  const tr_pair* pair = tr_cams_of(*cam1, *cam2);
  vwgpu_prof_scope ps(ctx, "stereo_triangulate");
  if (!d_stats) {
    hipLaunchKernelGGL(pair->triangulate, tr_grid(w, h), tr_block, 0, ctx->stream, a, *cam1, *cam2);
    VWGPU_HIP(ctx, hipGetLastError());
    return VWGPU_OK;
  }
  const dim3 grid = tr_grid(w, h);
  // one partial per workgroup, folded in two levels whose shape depends on the image size alone: the order of the sum is fixed
  const long long npartial = (long long)grid.x * grid.y * grid.z, nfold = (npartial + TR_FOLD_CHUNK - 1) / TR_FOLD_CHUNK;
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, (size_t)(npartial + nfold) * sizeof(vwgpu_triangulate_stats));
  if (rc) return rc;
  a.partial = static_cast<vwgpu_triangulate_stats*>(ctx->scratch.base);
  hipLaunchKernelGGL(pair->triangulate_stats, grid, tr_block, 0, ctx->stream, a, *cam1, *cam2);
  VWGPU_HIP(ctx, hipGetLastError());
  if (nfold > 1) {
    vwgpu_triangulate_stats* second = a.partial + npartial;
    hipLaunchKernelGGL(tr_stats_fold_kernel, dim3((unsigned)nfold), dim3(TR_THREADS), 0, ctx->stream, a.partial, npartial, TR_FOLD_CHUNK, second);
    hipLaunchKernelGGL(tr_stats_fold_kernel, dim3(1), dim3(TR_THREADS), 0, ctx->stream, second, nfold, nfold, d_stats);
  } else {
    hipLaunchKernelGGL(tr_stats_fold_kernel, dim3(1), dim3(TR_THREADS), 0, ctx->stream, a.partial, npartial, npartial, d_stats);
  }
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int angle_check(vwgpu_ctx* ctx, int type, const void* disp, int w, int h, ptrdiff_t& dstride, const vwgpu_camera* cam1,
                const vwgpu_camera* cam2, int semantics, const double* out, ptrdiff_t& ostride) {
  const char* name = "convergence_angle";
  int rc = tr_check(ctx, name, type, disp, w, h, dstride, cam1, cam2, semantics);
  if (rc) return rc;
  if (!out || (const void*)out == disp) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: null output, or the input itself", name);
  return tr_out_stride(ctx, name, out, ostride, w);
}

int angle_run(vwgpu_ctx* ctx, int type, const void* d_disp, int w, int h, ptrdiff_t dstride, int x0, int y0, const vwgpu_camera* cam1,
              const vwgpu_camera* cam2, int semantics, double* d_out, ptrdiff_t ostride) {
  tr_args a = tr_make_args(type, d_disp, w, h, dstride, x0, y0, semantics, *cam1, *cam2);
  a.error = d_out; a.estride = ostride;
  const tr_pair* pair = tr_cams_of(*cam1, *cam2);
  vwgpu_prof_scope ps(ctx, "convergence_angle");
  hipLaunchKernelGGL(pair->angle, tr_grid(w, h), tr_block, 0, ctx->stream, a, *cam1, *cam2);
  VWGPU_HIP(ctx, hipGetLastError());
  return VWGPU_OK;
}

int universe_check(vwgpu_ctx* ctx, const double* points, int channels, int w, int h, ptrdiff_t& stride, const double* origin,
                   double near_radius, double far_radius, const double* out, ptrdiff_t& ostride) {
  const char* name = "universe_radius";
  if (!ctx) return VWGPU_ERR_ARGUMENT;
  ctx->err.clear();
  if (channels != 3 && channels != 4 && channels != 6)
    return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: %d channels, not 3, 4 or 6", name, channels);
  if (!points || !out || !origin || w <= 0 || h <= 0) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: empty image or null pointer", name);
  if (!(near_radius >= 0 && far_radius >= 0)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "UniverseRadius: radii must be >= 0.");
  if (!(near_radius <= far_radius)) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "UniverseRadius: near radius must be <= far radius.");
  if (stride == 0) stride = w;
  if (ostride == 0) ostride = w;
  if (stride < w || ostride < w) return vwgpu_fail(ctx, VWGPU_ERR_ARGUMENT, "%s: row stride smaller than row width", name);
  return VWGPU_OK;
}

int universe_run(vwgpu_ctx* ctx, const double* d_points, int channels, int w, int h, ptrdiff_t stride, const double* origin,
                 double near_radius, double far_radius, double* d_out, ptrdiff_t ostride, long long* counts) {
  const size_t counter_bytes = TR_COUNTERS * sizeof(unsigned long long);
  int rc = vwgpu_arena_reserve(ctx, &ctx->scratch, counter_bytes);
  if (rc) return rc;
  unsigned long long* d_counter = static_cast<unsigned long long*>(ctx->scratch.base);
  VWGPU_HIP(ctx, hipMemsetAsync(d_counter, 0, counter_bytes, ctx->stream));
  tr_universe_args a{d_points, (long long)stride, w, h, origin[0], origin[1], origin[2], near_radius, far_radius, d_out,
                     (long long)ostride, d_counter};
  const dim3 grid = tr_grid(w, h);
  {
    vwgpu_prof_scope ps(ctx, "universe_radius");
    if (channels == 3) hipLaunchKernelGGL(tr_universe_kernel<3>, grid, tr_block, 0, ctx->stream, a);
    else if (channels == 4) hipLaunchKernelGGL(tr_universe_kernel<4>, grid, tr_block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(tr_universe_kernel<6>, grid, tr_block, 0, ctx->stream, a);
    if (counts) hipLaunchKernelGGL(tr_universe_fold_kernel, dim3(1), dim3(TR_THREADS), 0, ctx->stream, d_counter);
    VWGPU_HIP(ctx, hipGetLastError());
  }
  if (counts) {
    unsigned long long cnt = 0;
    VWGPU_HIP(ctx, hipMemcpyAsync(&cnt, d_counter, 8, hipMemcpyDeviceToHost, ctx->stream));
    VWGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    counts[0] = (long long)w * (long long)h;
    counts[1] = (long long)cnt;
  }
  return VWGPU_OK;
}

}  // namespace

// ---- extern "C" entry points (include/vwgpu.h) -------------------------------------------------------------------------

extern "C" {

int vwgpu_stereo_triangulate_dev(vwgpu_ctx* ctx, int type, const void* d_disp, int w, int h, ptrdiff_t dstride, int x0, int y0,
                                 const vwgpu_camera* cam1, const vwgpu_camera* cam2, double angle_tol, int semantics, double* d_xyz,
                                 ptrdiff_t xstride, double* d_error, ptrdiff_t estride, double* d_errvec, ptrdiff_t vstride,
                                 vwgpu_triangulate_stats* d_stats) {
  int rc = triangulate_check(ctx, type, d_disp, w, h, dstride, cam1, cam2, angle_tol, semantics, d_xyz, xstride, d_error, estride,
                             d_errvec, vstride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return triangulate_run(ctx, type, d_disp, w, h, dstride, x0, y0, cam1, cam2, angle_tol, semantics, d_xyz, xstride, d_error, estride,
                         d_errvec, vstride, d_stats);
}

int vwgpu_stereo_triangulate(vwgpu_ctx* ctx, int type, const void* disp, int w, int h, ptrdiff_t dstride, int x0, int y0,
                             const vwgpu_camera* cam1, const vwgpu_camera* cam2, double angle_tol, int semantics, double* xyz,
                             ptrdiff_t xstride, double* error, ptrdiff_t estride, double* errvec, ptrdiff_t vstride,
                             vwgpu_triangulate_stats* stats) {
  int rc = triangulate_check(ctx, type, disp, w, h, dstride, cam1, cam2, angle_tol, semantics, xyz, xstride, error, estride, errvec,
                             vstride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pd = st.add(disp, w, h, 4 * (size_t)tr_elem_words(semantics & TR_LAYOUT_MASK), dstride, VWGPU_STAGE_IN),
            px = st.add(xyz, w, h, 24, xstride, VWGPU_STAGE_OUT), pe = st.add(error, w, h, 8, estride, VWGPU_STAGE_OUT),
            pv = st.add(errvec, w, h, 24, vstride, VWGPU_STAGE_OUT),
            ps = st.add(stats, 1, 1, sizeof(vwgpu_triangulate_stats), 1, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = triangulate_run(ctx, type, st.dev<void>(pd), w, h, w, x0, y0, cam1, cam2, angle_tol, semantics, st.dev<double>(px), w,
                       st.dev<double>(pe), w, st.dev<double>(pv), w, st.dev<vwgpu_triangulate_stats>(ps));
  if (rc) return rc;
  return st.finish();
}

int vwgpu_convergence_angle_dev(vwgpu_ctx* ctx, int type, const void* d_disp, int w, int h, ptrdiff_t dstride, int x0, int y0,
                                const vwgpu_camera* cam1, const vwgpu_camera* cam2, int semantics, double* d_out, ptrdiff_t ostride) {
  int rc = angle_check(ctx, type, d_disp, w, h, dstride, cam1, cam2, semantics, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return angle_run(ctx, type, d_disp, w, h, dstride, x0, y0, cam1, cam2, semantics, d_out, ostride);
}

int vwgpu_convergence_angle(vwgpu_ctx* ctx, int type, const void* disp, int w, int h, ptrdiff_t dstride, int x0, int y0,
                            const vwgpu_camera* cam1, const vwgpu_camera* cam2, int semantics, double* out, ptrdiff_t ostride) {
  int rc = angle_check(ctx, type, disp, w, h, dstride, cam1, cam2, semantics, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const int pd = st.add(disp, w, h, 4 * (size_t)tr_elem_words(semantics & TR_LAYOUT_MASK), dstride, VWGPU_STAGE_IN),
            po = st.add(out, w, h, 8, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = angle_run(ctx, type, st.dev<void>(pd), w, h, w, x0, y0, cam1, cam2, semantics, st.dev<double>(po), w);
  if (rc) return rc;
  return st.finish();
}

int vwgpu_universe_radius_dev(vwgpu_ctx* ctx, const double* d_points, int channels, int w, int h, ptrdiff_t stride,
                              const double* origin, double near_radius, double far_radius, double* d_out, ptrdiff_t ostride,
                              long long* counts) {
  int rc = universe_check(ctx, d_points, channels, w, h, stride, origin, near_radius, far_radius, d_out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  return universe_run(ctx, d_points, channels, w, h, stride, origin, near_radius, far_radius, d_out, ostride, counts);
}

int vwgpu_universe_radius(vwgpu_ctx* ctx, const double* points, int channels, int w, int h, ptrdiff_t stride, const double* origin,
                          double near_radius, double far_radius, double* out, ptrdiff_t ostride, long long* counts) {
  int rc = universe_check(ctx, points, channels, w, h, stride, origin, near_radius, far_radius, out, ostride);
  if (rc) return rc;
  VWGPU_HIP(ctx, hipSetDevice(ctx->device));
  vwgpu_stage st(ctx);
  const size_t elem = 8 * (size_t)channels;
  const int pi = st.add(points, w, h, elem, stride, VWGPU_STAGE_IN), po = st.add(out, w, h, elem, ostride, VWGPU_STAGE_OUT);
  if ((rc = st.commit())) return rc;
  rc = universe_run(ctx, st.dev<double>(pi), channels, w, h, w, origin, near_radius, far_radius, st.dev<double>(po), w, counts);
  if (rc) return rc;
  return st.finish();
}

}  // extern "C"
