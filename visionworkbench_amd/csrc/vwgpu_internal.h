// vwgpu_internal.h — context object and launch helpers shared by the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "vwgpu.h"
#include "zone_task.h"

struct vwgpu_prof_rec {
  const char* name;
  hipEvent_t a, b;
};

// Grow-only device scratch arena: one allocation reused across calls so that steady-state calls do no
// hipMalloc/hipFree (they would serialise the stream).
struct vwgpu_arena {
  void* base = nullptr;
  size_t cap = 0;
};

struct vwgpu_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  bool stream_is_own = true;
  std::string err;
  int forced_path = VWGPU_PATH_NONE;
  int last_path = VWGPU_PATH_NONE;
  bool profiling = false;
  std::vector<vwgpu_prof_rec> prof;
  std::vector<hipEvent_t> event_pool;
  std::vector<void*> graveyard;   // outgrown arena blocks (vwgpu_arena_reserve): released by vwgpu_synchronize / vwgpu_trim / with the context
  size_t graveyard_bytes = 0;
  vwgpu_arena scratch;   // kernel scratch (NCC precision images)
  vwgpu_arena flags;     // two alternating "input not representable" flags of the packed-u8 path
  bool flags_init = false;
  void* flags_base_seen = nullptr;
  int flag_parity = 0;
  int* last_flag = nullptr;
  vwgpu_arena staging;   // device copies of host images for the host-pointer entry points
  vwgpu_arena filt;      // intermediate image of composite filters (prefilter_image)
  vwgpu_arena misc;      // small device words (disparity range of parabola_subpixel)
  vwgpu_arena pyr;       // pyramids, masks and per-level disparities of one pyramid_correlate tile
  vwgpu_arena ztab;      // zone / tile tables of the batched zone kernels (two halves, alternating)
  int ztab_parity = 0;
  vwgpu_arena zrl;       // right-to-left disparity images of all zones of pyramid level 0
  vwgpu_arena zext;      // zone scheduler: leaf boxes of the quad tree and their measured disparity extents
  vwgpu_arena sgm;       // SGM: u8 images, census words, disparity bounds, ragged starts
  vwgpu_arena sgm_main;  // SGM: ragged cost (u8) + accumulated cost (u16) buffers
  vwgpu_arena sgm_bnd;   // SGM fused sweeps: ticket counter + boundary rows handed from block to block (zero-initialised, words tagged with sgm_epoch)
  unsigned sgm_epoch = 0;
  int sgm_sweep = 0;     // VWGPU_OPT_SGM_SWEEP
  int mgm_sweep = 0;     // VWGPU_OPT_MGM_SWEEP
  int sgm_path_mode = 0; // VWGPU_OPT_SGM_PATH_MODE
  vwgpu_arena xvol;      // exact-order path: column-sum volumes, band state, per-zone NCC precision images (bm_exact.hip)
  vwgpu_arena xtab;      // exact-order path: zone / work-item tables of one call
  vwgpu_arena xcarry;    // exact-order path: compare-chain state per pixel between the disparity groups of a zone with > 512 disparities
  // Pinned host memory for the small tables that cross PCIe inside a call (zone / tile tables up, leaf extents down): a copy from or
  // to pageable memory is staged by the runtime and blocks the calling thread.  A ring of two halves: vwgpu_host_ring() hands out the
  // next piece and waits, before it re-enters a half, for the event that marks the last copy queued from that half.
  char* host_ring = nullptr;
  size_t host_cap = 0, host_pos = 0;
  int host_half = 0;
  hipEvent_t ring_event[2] = {nullptr, nullptr};
  bool ring_event_set[2] = {false, false};
  int host_ring_kb = 16384;   // VWGPU_OPT_HOST_RING_KB
  unsigned long long ring_wraps = 0;   // half crossings so far (VWGPU_OPT_HOST_RING_WRAPS, read only: tests)
  struct LeafRects { int w, h; size_t n; void* d_rects; };
  std::vector<LeafRects> leaf_rects;   // zone scheduler: device copies of the leaf boxes of the level sizes seen so far
  bool measure_first = false; // the previous calc_disparity was refused by the packed-u8 kernels: measure the input class first
  bool defer_exact = false;   // VWGPU_OPT_DEFER_EXACTNESS: calc_disparity_dev never waits for the input-class flags
  int sad_groups = 0;         // VWGPU_OPT_SAD_GROUPS
  int sad_layout = 0;         // VWGPU_OPT_SAD_LAYOUT
  int sad_last_launch = 0;    // VWGPU_OPT_SAD_LAST_LAUNCH
  int sad_round_slots = 0;    // VWGPU_OPT_SAD_ROUND_SLOTS
  int exact_scratch_mb = 4096;// VWGPU_OPT_EXACT_SCRATCH_MB
  int ip_scratch_mb = 1024;   // VWGPU_OPT_IP_SCRATCH_MB
  int sgm_last_form = 0;      // VWGPU_OPT_SGM_LAST_FORM
  int exact_split = 0;        // VWGPU_OPT_EXACT_SPLIT: 0 by the longest chain, 1 always the split pass 2, 2 always the fused one
  int trace = 0;              // VWGPU_OPT_TRACE
  int certify = 1;            // VWGPU_OPT_CERTIFY
  int zone_tile16 = 2;        // VWGPU_OPT_ZONE_TILE16: zones that fit 16 x 16 on the one-wavefront tile kernels: 0 = in tile groups, 1 = always, 2 = never
  int cert_f32 = 1;           // VWGPU_OPT_CERT_F32: the certified pass runs its fp32 tier first (bm_zones.hip)
  int zone_sxc = 0;           // VWGPU_OPT_ZONE_SXC: 0 = 16 dx per right patch, else at most this many
  unsigned long long cert_px[3] = {0, 0, 0};   // with VWGPU_OPT_TRACE bit 2: pixels in certified tiles / in flagged tiles / in tiles the fp32 tier passed on to float64, so far
  vwgpu_arena hole;      // hole filling (hole_fill.hip): union-find parents, roots and scan partials of one labelling
  vwgpu_arena hole_tab;  // hole filling: per-blob statistics, the kept-blob numbering, the internal label image and table of fill_holes_grass
  int inpaint_overlap = 1;    // VWGPU_OPT_INPAINT_OVERLAP
  vwgpu_arena istats;    // image statistics (image_stats.hip): results, histogram bins, reduction slabs, sampling tables of one call
  int num_cu = 256;
  void* host_pool = nullptr;  // helper threads for the per-tile host work of tile groups (host_pool.hip), created on first use
};
// fn(i) for i in [0, n) on the context's helper threads and the calling thread; returns when all are done.  fn must not throw.
void vwgpu_pool_run(vwgpu_ctx* ctx, int n, void (*fn)(void*, int), void* arg);
void vwgpu_pool_destroy(vwgpu_ctx* ctx);

int vwgpu_fail(vwgpu_ctx* ctx, int status, const char* fmt, ...);
int vwgpu_arena_reserve(vwgpu_ctx* ctx, vwgpu_arena* a, size_t bytes);
void* vwgpu_host_ring(vwgpu_ctx* ctx, size_t bytes);     // nullptr: the request does not fit (the caller copies from its own memory)

#define VWGPU_HIP(ctx, call)                                                                     \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess)                                                                        \
      return vwgpu_fail((ctx), e_ == hipErrorOutOfMemory ? VWGPU_ERR_NOMEM : VWGPU_ERR_HIP,      \
                        "%s failed: %s", #call, hipGetErrorString(e_));                          \
  } while (0)

// RAII event bracket around one kernel launch when profiling is on.
struct vwgpu_prof_scope {
  vwgpu_ctx* ctx;
  hipEvent_t b = nullptr;
  vwgpu_prof_scope(vwgpu_ctx* c, const char* name);
  ~vwgpu_prof_scope();
};

static inline size_t vwgpu_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Host-pointer entry points (vwgpu_abi.hip): a plan of dense 2-D pieces in ctx->staging.  An entry registers its operands, commits (ONE
// reservation, then the uploads), runs the device path on dev<T>() pointers with dense strides, and finishes (the downloads, one
// synchronise).  Every copy is a hipMemcpy2DAsync on ctx->stream.
enum { VWGPU_STAGE_NONE = 0, VWGPU_STAGE_IN = 1, VWGPU_STAGE_OUT = 2, VWGPU_STAGE_INOUT = 3 };
struct vwgpu_stage {
  static constexpr int MAX_PIECES = 24;
  explicit vwgpu_stage(vwgpu_ctx* c) : ctx(c) {}
  // A piece of w x h elements of `elem` bytes, vwgpu_align_up(w * h * elem, 256) bytes of the arena, in registration order; host_stride in
  // elements.  dir: IN = uploaded by commit, OUT = downloaded by finish, INOUT = both (outputs the kernels write only in part), NONE = device
  // scratch that is never copied.  host == nullptr with another dir than NONE: an absent optional operand, no bytes, dev() == nullptr.
  int add(const void* host, int w, int h, size_t elem, ptrdiff_t host_stride, int dir);
  int commit();
  template <class T> T* dev(int piece) const { return reinterpret_cast<T*>(p[piece].dev); }
  // Queue the download of the first h rows of w elements of a piece whose rows are w elements apart (extents known only after the call).
  int download(int piece, void* host, int w, int h, ptrdiff_t host_stride);
  int finish();
 private:
  struct piece { void* host; char* dev; size_t off, elem; ptrdiff_t stride; int w, h, dir; bool present; };
  vwgpu_ctx* ctx;
  piece p[MAX_PIECES];
  int n = 0;
  size_t total = 0;
};

// ---- kernel-family launchers (each in its own .hip) ------------------------------------------------
// All pointers are device pointers; every launcher enqueues on ctx->stream and returns a vwgpu_status.

// The operands of one whole-raster block-matching call, as vwgpu_calc_disparity_dev received them (os defaulted).
struct vwgpu_bm_args {
  int cost_type;
  const float* left; int lw, lh; ptrdiff_t ls;
  const float* right; int rw, rh; ptrdiff_t rs;
  int kx, ky, sx, sy;
  int32_t* out; ptrdiff_t os;
  int ow() const { return lw - kx + 1; }
  int oh() const { return lh - ky + 1; }
};

int vwgpu_launch_bm_generic(vwgpu_ctx* ctx, const vwgpu_bm_args& a);

// A packed-integer matcher: exact on integer-valued pixels of its class, and it checks the class itself while converting — input
// outside it leaves *d_flag (device int) nonzero once the launch has run, and the caller must then take another path.
//   bm_sad_u8.hip    SAD, [0,255] (v_qsad_pk_u16_u8)
//   bm_corr_u8.hip   SSD / NCC, [0,255], register-blocked v_dot4_u32_u8 (preferred over bm_dot_u8 where instantiated)
//   bm_dot_u8.hip    SSD / NCC, [0,255], v_dot4_u32_u8
//   bm_sad_u16.hip   SAD, [0,65535] (v_sad_u16 on pixel pairs)
//   bm_corr_u16.hip  SSD / NCC, [0,4095] (v_dot2_u32_u16 on pixel pairs)
struct vwgpu_bm_matcher {
  int path;           // what vwgpu_last_path reports
  int max_hi;         // the largest `hi` exponent of vwgpu_float_grain inside the class
  const char* what;   // names the path in the NOIMPL text of a forced call
  bool (*supported)(const vwgpu_bm_args& a);                              // false: this configuration has no such kernel
  int (*launch)(vwgpu_ctx* ctx, const vwgpu_bm_args& a, int** d_flag);
};
// (Not const objects: the device compilation would emit a constant-initialised const object too, and has no such host functions.)
extern vwgpu_bm_matcher vwgpu_bm_sad_u8, vwgpu_bm_corr_u8, vwgpu_bm_dot_u8, vwgpu_bm_sad_u16, vwgpu_bm_corr_u16;

// The start of every packed launcher: the call's two alternating flags (*d_flag = the one this call raises, `clear` the next call's)
// and, for a request of more than 64 KiB, the dynamic-LDS limit of the kernel.
struct vwgpu_flag_pair { int* set = nullptr; int* clear = nullptr; };
int vwgpu_packed_prologue(vwgpu_ctx* ctx, const void* kernel, size_t shmem, int** d_flag, vwgpu_flag_pair* flags);

// Scratch of the integer NCC matchers (bm_corr_u8.hip, bm_corr_u16.hip) in ctx->scratch: the window sums of squares of both images and
// the queue of pixels that ncc_full_kernel evaluates over every disparity in float64 (the count zeroed).  `who` names the caller in errors.
struct vwgpu_ncc_plan {
  uint32_t *a2 = nullptr, *b2 = nullptr;
  int b2w = 0;
  uint32_t *full_list = nullptr, *full_count = nullptr;
  uint32_t cap = 0;
};
int vwgpu_ncc_plan_reserve(vwgpu_ctx* ctx, const vwgpu_bm_args& a, const char* who, vwgpu_ncc_plan* p);
int vwgpu_launch_ncc_full(vwgpu_ctx* ctx, const vwgpu_bm_args& a, const vwgpu_ncc_plan& p, int* flag);

// bm_exact.hip: the reference's own summation order (serial column / row chains of fast_box_sum) for inputs whose
// partial sums are not exactly representable; see the file header.
struct vwgpu_zone_task;
bool vwgpu_bm_exact_supported(int sx, int sy);
bool vwgpu_sums_order_free(int cost_type, int kx, int ky, int lo, int hi, int nonfinite);
int vwgpu_sums_bits(int cost_type, int kx, int ky, int lo, int hi, int nonfinite);      // <= 53: any order in float64; <= 24: in float32 too
int vwgpu_float_grain(vwgpu_ctx* ctx, const float* a, int aw, int ah, ptrdiff_t as, const float* b, int bw, int bh, ptrdiff_t bs,
                      int* lo, int* hi, int* nonfinite);
void vwgpu_launch_float_grain(vwgpu_ctx* ctx, int n, const float* const* img, const int* w, const int* h, const ptrdiff_t* stride, int* const* d_cells);
int vwgpu_launch_bm_exact(vwgpu_ctx* ctx, int cost_type, const float* A, int aw, int ah, ptrdiff_t as,
                          const float* B, int bw, int bh, ptrdiff_t bs, int kx, int ky,
                          const vwgpu_zone_task* zones, int n, int32_t* out, const int* d_gate = nullptr,   // d_gate[i] == 0 (device): zone i is skipped
                          const int* rows = nullptr, int nranges = 0);   // one zone only: produce just the output rows [rows[2i], rows[2i+1]) (sorted, disjoint); the column chains still run from row 0
int vwgpu_launch_box_sum_exact(vwgpu_ctx* ctx, const float* img, int w, int h, ptrdiff_t stride, int kx, int ky, double* d_out);

int vwgpu_launch_lr_check(vwgpu_ctx* ctx, int32_t* l2r, int lw, int lh, ptrdiff_t ls,
                          const int32_t* r2l, int rw, int rh, ptrdiff_t rs, float thr);
int vwgpu_launch_lr_check_diff(vwgpu_ctx* ctx, int32_t* l2r, int lw, int lh, ptrdiff_t ls,
                               const int32_t* r2l, int rw, int rh, ptrdiff_t rs, float thr,
                               float* diff2, ptrdiff_t dstride, int ulx, int uly);

// filters.hip
// One launch serves up to VWGPU_MAX_IMG_JOBS images (blockIdx.z = job): the pyramid of a tile is ~60 filter launches of 10-20 us on small
// images, launch bound — the left and right image of a level, or all twelve level images of a prefilter, go through ONE launch.
constexpr int VWGPU_MAX_IMG_JOBS = 12;
struct vwgpu_img_job {
  const void* src; ptrdiff_t stride; int w, h;        // source image
  void* dst; ptrdiff_t dstride; int ow, oh;           // destination and output size
  int offx, offy;                                     // source position of output (0, 0)
  const float* b; ptrdiff_t bs;                       // second operand (subtract / edge_extend_sub), or nullptr
};
// a job of vwgpu_launch_sepconv_jobs with bs == VWGPU_JOB_MASK_BY_TWO is a uint8 mask halved by subsample_mask_by_two instead of an image
constexpr ptrdiff_t VWGPU_JOB_MASK_BY_TWO = -7;
int vwgpu_launch_sepconv_jobs(vwgpu_ctx* ctx, const vwgpu_img_job* jobs, int n, const float* xk, int nx, int cx, const float* yk, int ny, int cy,
                              int edge, int step);
int vwgpu_launch_conv2d_jobs(vwgpu_ctx* ctx, const vwgpu_img_job* jobs, int n, const float* k, int kw, int kh, int ci, int cj, int edge);
int vwgpu_launch_mask_by_two_jobs(vwgpu_ctx* ctx, const vwgpu_img_job* jobs, int n);
int vwgpu_launch_subtract_jobs(vwgpu_ctx* ctx, const vwgpu_img_job* jobs, int n);
int vwgpu_prefilter_images_dev(vwgpu_ctx* ctx, int n, const float* const* srcs, const int* ws, const int* hs, int mode, float width, float* const* dsts);
int vwgpu_launch_sepconv(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t stride,
                         const float* xk, int nx, int cx, const float* yk, int ny, int cy,
                         int edge, int step, float* dst, ptrdiff_t dstride);
int vwgpu_launch_conv2d(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t stride,
                        const float* k, int kw, int kh, int ci, int cj, int edge, float* dst, ptrdiff_t dstride);
int vwgpu_launch_mask_by_two(vwgpu_ctx* ctx, const uint8_t* src, int w, int h, ptrdiff_t stride,
                             uint8_t* dst, ptrdiff_t dstride);
int vwgpu_launch_subtract(vwgpu_ctx* ctx, const float* a, ptrdiff_t as, const float* b, ptrdiff_t bs, int w, int h,
                          float* dst, ptrdiff_t ds);
int vwgpu_launch_sepconv_region(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t stride,
                                const float* xk, int nx, int cx, const float* yk, int ny, int cy,
                                int edge, int step, float* dst, ptrdiff_t dstride, int ow, int oh, int offx, int offy);
int vwgpu_launch_conv2d_region(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t stride,
                               const float* k, int kw, int kh, int ci, int cj, int edge, float* dst, ptrdiff_t dstride,
                               int ow, int oh, int offx, int offy);
int vwgpu_launch_ext_sub(vwgpu_ctx* ctx, const float* a, ptrdiff_t as, int w, int h, const float* b, ptrdiff_t bs,
                         float* dst, ptrdiff_t ds, int ow, int oh, int offx, int offy);
int vwgpu_prefilter_region(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t stride, int mode, float width,
                           int x0, int y0, int bw, int bh, float* dst, float* scratch);
extern "C" int vwgpu_generate_gaussian_kernel(double sigma, int size, float* taps, int cap);

// subpixel.hip
int vwgpu_launch_parabola_prepass(vwgpu_ctx* ctx, const float* disp3f, int w, int h, ptrdiff_t stride_px, int* d_out4,
                                  const float* L, int lw, int lh, ptrdiff_t ls, const float* R, int rw, int rh, ptrdiff_t rs, int* d_cell);
void vwgpu_launch_f32_ext_to_u8_raster(vwgpu_ctx* ctx, const float* src, ptrdiff_t stride, int w, int h, int x0, int y0, int bw, int bh,
                                       uint8_t* dst, int pitch);
int vwgpu_parabola_u8_pitch(int w);
int vwgpu_launch_parabola(vwgpu_ctx* ctx, const float* disp3f, int w, int h, ptrdiff_t dstride_px,
                          const float* lras, int lrw, const float* rras, int rrw, int range_minx, int range_miny,
                          int kx, int ky, float* out3f, ptrdiff_t ostride_px, int integer_class = 0);

// affine_subpixel.hip — the PyramidSubpixelView tile loop (tile ranges, prefiltered crops, pyramids, disparity_subsample /
// disparity_upsample, the final write of each box).  One level of one tile, as a refiner sees it: the level's left and
// right patches and its disparity map {dx, dy, v}, updated in place on the ROI plus its 1-pixel ring [x0, x1) x [y0, y1).
struct vwgpu_pyr_level_view {
  int w, h;
  const float *L, *R;
  float *dx, *dy;
  uint8_t* v;
};
// A refiner of pixels that do not depend on each other (SUBPIXEL_PHASE): called for every level of every tile instead
// of the raster-order fixpoint of the other algorithms.  Returns a vwgpu_status.
struct vwgpu_pyr_refiner {
  int (*refine)(vwgpu_ctx* ctx, const vwgpu_pyr_level_view& lv, int kx, int ky, int x0, int y0, int x1, int y1, void* user);
  void* user;
};
// Arguments as vwgpu_pyramid_subpixel_dev, checked by the caller.  refiner == nullptr: `algorithm` runs in the fixpoint
// and stats receives its three counters; otherwise `algorithm` is ignored and stats is not touched.
int vwgpu_pyramid_subpixel_tiles(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride,
                                 const float* d_left, ptrdiff_t lstride, const float* d_right, int rw, int rh, ptrdiff_t rstride,
                                 int mode, float width, int kx, int ky, int levels, int algorithm, const vwgpu_pyr_refiner* refiner,
                                 const int* tiles, int ntiles, float* d_out, ptrdiff_t ostride, long long* stats);

// bm_zones.hip — the zone tables (vwgpu_zone_task, vwgpu_zone_group, vwgpu_zone_row_flags) are in zone_task.h
bool vwgpu_bm_zones_supported(int kx, int ky);
// f32_sums: vwgpu_sums_bits <= 24 for BOTH images.  cert_hi != INT_MIN: certify against the reference's summation order (bm_zones.hip),
// d_zflag[n] (zeroed by the caller) receives the zones that need vwgpu_launch_bm_exact; d_stats (optional): {pixels in certified tiles, in flagged tiles}
int vwgpu_launch_bm_zones(vwgpu_ctx* ctx, int cost_type, const float* A, int aw, int ah, const float* B, int bw, int bh,
                          int kx, int ky, const vwgpu_zone_task* zones, int n, int32_t* out, int f32_sums = 0,
                          int cert_hi = (-2147483647 - 1), int* d_zflag = nullptr, unsigned long long* d_stats = nullptr,
                          int* d_any = nullptr,       // d_any (optional, zeroed by the caller): set to 1 when some zone was flagged
                          const int* d_need = nullptr, const unsigned char* d_cells = nullptr,      // (optional) what to match of every zone, from vwgpu_launch_zone_need
                          int edge_m = 0, int edge_k = 0, int edge_lo = 0, int edge_hi = 0,      // certified passes: edge_m > 0 turns the "cannot matter" certificate on (bm_zones.hip, ZEdge)
                          ptrdiff_t as = 0, ptrdiff_t bs = 0,                                      // row strides of A / B in floats (0: the widths)
                          const vwgpu_zone_group* grp = nullptr,                                   // several image pairs in one launch sequence; d_any then has n_img words
                          int* d_tflag = nullptr);                                                 // certified passes without d_need: one int per 32-row band of every zone (vwgpu_zone_row_flags of them, zeroed by the caller; zone i's begin where the bands of zones 0 .. i-1 end), set for bands with an unproven pixel
// The flagged bands of one zone as row ranges {begin, end}, ... for vwgpu_launch_bm_exact; returns the number of flagged rows.
inline int vwgpu_zone_flagged_rows(const int* bands, int zh, std::vector<int>* rows) {
  int flagged = 0;
  rows->clear();
  for (int ty = 0; ty * 32 < zh; ++ty) {
    if (!bands[ty]) continue;
    const int a = ty * 32, b = std::min(zh, a + 32);
    flagged += b - a;
    if (!rows->empty() && rows->back() == a) rows->back() = b; else { rows->push_back(a); rows->push_back(b); }
  }
  return flagged;
}
// The part of every zone's R->L image that its L/R check (vwgpu_launch_zone_lr, same tasks) will read, from the finished L->R result:
// a rectangle per zone (d_need, 8 ints per zone) and a flag per 16 x 16 cell (d_cells; vwgpu_zone_need_cells numbers the cells into the
// tasks' `ay` slot and returns their count).  d_zflag (optional): L->R zones still to be matched again ask for the whole image.
size_t vwgpu_zone_need_cells(vwgpu_zone_task* zones, int n);
int vwgpu_launch_zone_need(vwgpu_ctx* ctx, const vwgpu_zone_task* zones, int n, const int32_t* l2r, const int* d_zflag, int* d_need,
                           unsigned char* d_cells, size_t ncells);
// lr tasks: ax = pixel offset of the zone's R->L image, (bx, by) = its size, (sx, sy) = the zone's origin in the diff image
int vwgpu_launch_zone_lr(vwgpu_ctx* ctx, const vwgpu_zone_task* zones, int n, int32_t* l2r, const int32_t* r2l, float thr,
                         float* diff2, ptrdiff_t dstride);

// pyramid_filters.hip
int vwgpu_launch_disparity_filter(vwgpu_ctx* ctx, const int32_t* src, int w, int h, int hh, int hv, double pthr, double rthr,
                                  bool cleanup, int32_t* tmp_padded, int32_t* dst, bool inner_only = false,      // inner_only: stop after the first pass (tmp_padded)
                                  int tiles = 1, size_t tile_ints = 0);                                        // tile groups: `tiles` images at a stride of tile_ints ints
int vwgpu_launch_blob_filter(vwgpu_ctx* ctx, int32_t* d, int w, int h, int area, int* scratch);
int vwgpu_launch_disparity_mask(vwgpu_ctx* ctx, int32_t* d, int w, int h, const uint8_t* m1, const uint8_t* m2, int m2w, int m2h);
// pyramid.hip
int vwgpu_pyramid_correlate_impl(vwgpu_ctx* ctx, const float* left, int lw, int lh, ptrdiff_t ls,
                                 const float* right, int rw, int rh, ptrdiff_t rs,
                                 const uint8_t* lmask, ptrdiff_t lms, const uint8_t* rmask, ptrdiff_t rms,
                                 const vwgpu_pyramid_params* P, int bx, int by, int bw, int bh,
                                 float* out, ptrdiff_t os, float* lr_diff);

// tile groups (pyramid.hip): several equal-sized tiles of one image pair through the level loop together
bool vwgpu_pyramid_group_eligible(const vwgpu_ctx* ctx, const vwgpu_pyramid_params* P, int n, const int* bw, const int* bh);
int vwgpu_pyramid_group_impl(vwgpu_ctx* ctx, const float* left, int lw, int lh, ptrdiff_t ls, const float* right, int rw, int rh, ptrdiff_t rs,
                             const uint8_t* lmask, ptrdiff_t lms, const uint8_t* rmask, ptrdiff_t rms, const vwgpu_pyramid_params* P,
                             int n, const int* bxs, const int* bys, int bw, int bh, float* const* outs, const ptrdiff_t* oss);

// sgm.hip
int vwgpu_sgm_impl(vwgpu_ctx* ctx, const vwgpu_sgm_params* P, const float* left, int lw, int lh, ptrdiff_t ls,
                   const float* right, int rw, int rh, ptrdiff_t rs, int sx, int sy,
                   const uint8_t* lmask, int lmw, int lmh, const uint8_t* rmask, int rmw, int rmh,
                   const int32_t* prev, int pw, int ph, int32_t* out_disp, float* out_sub, size_t out_cap_pixels, int* ow, int* oh);
