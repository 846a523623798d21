/* vwgpu.h — C ABI of the MI355X-native stereo-correlation engine (libvwgpu.so).
 *
 * This is the drop-in boundary for Vision Workbench's dense block-matching hot path.  The reference has no
 * FFI/plugin interface (the path is ordinary C++ linked into libVwStereo.so), so each entry
 * point below is what the body of the cited reference function would call once its inputs are rasterised.
 * The C++ surface that keeps the reference's own signatures (vw::stereo::calc_disparity, ...) lives in
 * visionworkbench_amd/vwlite/ and is a thin wrapper over these calls; INTEGRATION.md shows the binding a
 * Vision Workbench maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.  Images are row-major, `stride` in ELEMENTS per row.
 *   - `*_dev` entry points take DEVICE pointers and are asynchronous on the context's stream;
 *     the un-suffixed ones take HOST pointers, stage through HBM and return when the result is in host memory.
 *   - every call returns VWGPU_OK (0) or a negative vwgpu_status; nothing throws.  One context per
 *     (host thread x GPU), mirroring the reference's one-thread-per-tile model
 *     (src/vw/Image/ImageIO.h:228-251); a context is not thread-safe, different contexts are independent.
 *   - disparity images use the vw::PixelMask<Vector2i> memory layout: 3 x int32 per pixel {dx, dy, valid},
 *     valid = INT32_MAX or 0 (src/vw/Image/PixelMask.h:48-120, src/vw/Image/PixelTypeInfo.h:95-102);
 *     float disparities use vw::PixelMask<Vector2f>: 3 x float {dx, dy, valid in {0.f, 1.f}}.
 */
#ifndef VWGPU_H
#define VWGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): struct vwgpu_sgm_params carries allow_block_cost (appended in round 3 without a bump: a host compiled against
 *     version 1 passes a struct that is 8 bytes shorter), VWGPU_PATH_REFUSED replaces the silent float64 fallback of
 *     VWGPU_OPT_DEFER_EXACTNESS, vwgpu_trim, vwgpu_halo_headers_agree, the host-ring and certification options; options 7
 *     (VWGPU_OPT_EXACT_LDS) and 10 (VWGPU_OPT_CORR_MFMA) are gone with the two slower kernel variants they selected.
 * 3 (round 5): vwgpu_pyramid_correlate_batch[_dev] (tile groups); vwgpu_last_path() may answer VWGPU_PATH_CERTIFIED (single-level calls on
 *     float rasters proven equal to the reference's summation order); options VWGPU_OPT_CERT_F32, _CERT_F64_PERMILLE, _ZONE_TILE16.  No struct
 *     of version 2 changed, but observable behaviour did (VWGPU_PATH_CERTIFIED where a version-2 host saw VWGPU_PATH_EXACT_ORDER), and hosts
 *     compare versions for EQUALITY: a host built against version 2 refuses this library and is rebuilt against this header.
 *     Round 6 added option values only (VWGPU_OPT_SGM_PATH_MODE, VWGPU_OPT_SAD_GROUPS = 3): same version.
 *     VWGPU_OPT_SAD_LAYOUT, VWGPU_OPT_SAD_LAST_LAUNCH, VWGPU_OPT_SAD_ROUND_SLOTS (options 20, 21, 22) likewise, and
 *     VWGPU_OPT_IP_SCRATCH_MB (23) with the interest-point entries, VWGPU_OPT_SGM_LAST_FORM (24, read only) likewise.
 *     The hole-filling entries (vwgpu_grassfire .. vwgpu_fill_nodata_with_avg) and VWGPU_OPT_INPAINT_OVERLAP (25) are additions: same version.
 *     The vwgpu_composite entries (Mosaic/ImageComposite.h) are additions: same version.
 * A host checks vwgpu_abi_version() == VWGPU_ABI_VERSION once after loading the library (vw::engine does, vw/Engine.h). */
#define VWGPU_ABI_VERSION 3

typedef struct vwgpu_ctx vwgpu_ctx;

/* Status codes; the C++ wrappers map them to the reference's exception types
 * (src/vw/Core/Exception.h:225-253): ARGUMENT -> vw::ArgumentErr, NOIMPL -> vw::NoImplErr,
 * LOGIC/HIP/NOMEM -> vw::LogicErr. */
typedef enum vwgpu_status {
  VWGPU_OK = 0,
  VWGPU_ERR_ARGUMENT = -1,
  VWGPU_ERR_NOIMPL = -2,
  VWGPU_ERR_HIP = -3,
  VWGPU_ERR_NOMEM = -4,
  VWGPU_ERR_LOGIC = -5,
  VWGPU_ERR_CAPACITY = -6   /* an output segment is too small; the call's counts say how large it must be */
} vwgpu_status;

/* vw::stereo::CostFunctionType, src/vw/Stereo/CostFunctions.h:143-149 (same numeric values). */
typedef enum vwgpu_cost_type {
  VWGPU_ABSOLUTE_DIFFERENCE = 0,
  VWGPU_SQUARED_DIFFERENCE = 1,
  VWGPU_CROSS_CORRELATION = 2,
  VWGPU_CENSUS_TRANSFORM = 3,          /* SGM only (src/vw/Stereo/SGM.cc:1874-1893) */
  VWGPU_TERNARY_CENSUS_TRANSFORM = 4   /* SGM only */
} vwgpu_cost_type;

/* Which kernel family served the last calc_disparity call (vwgpu_last_path). */
typedef enum vwgpu_path {
  VWGPU_PATH_NONE = 0,
  VWGPU_PATH_GENERIC_F64 = 1,  /* any float input, float64 accumulators (reference arithmetic)          */
  VWGPU_PATH_SAD_U8 = 2,       /* integer-valued inputs in [0,255]: packed u8 SAD (v_qsad_pk_u16_u8)      */
  VWGPU_PATH_DOT_U8 = 3,       /* integer-valued inputs in [0,255]: SSD / NCC on v_dot4_u32_u8            */
  VWGPU_PATH_EXACT_ORDER = 4,  /* inputs whose box sums round: the reference's serial summation order     */
  VWGPU_PATH_SAD_U16 = 5,      /* integer-valued inputs in [0,65535]: SAD on v_sad_u16 pixel pairs        */
  VWGPU_PATH_DOT_U16 = 6,      /* integer-valued inputs in [0,4095]: SSD / NCC on v_dot2_u32_u16          */
  VWGPU_PATH_REFUSED = 7,      /* vwgpu_last_path only: a packed kernel queued WITHOUT waiting for its verdict
                                  (vwgpu_force_path, VWGPU_OPT_DEFER_EXACTNESS) met input outside its domain; that
                                  call produced NO result — repeat it with automatic dispatch                   */
  VWGPU_PATH_CERTIFIED = 8     /* vwgpu_last_path only: inputs whose box sums round, matched by the tile-parallel
                                  kernels with every pixel PROVEN equal to the reference's serial summation order
                                  (winner ahead of the runner-up by more than twice a bound on the difference of the
                                  two orders); a call with a pixel that cannot be proven is redone in the reference's
                                  order and reports VWGPU_PATH_EXACT_ORDER.  VWGPU_OPT_CERTIFY = 0 turns it off      */
} vwgpu_path;

/* ---- context ------------------------------------------------------------------------------------- */

int vwgpu_abi_version(void);

/* Creates a context on HIP device `device` with its own stream. Fails with VWGPU_ERR_HIP if no GPU. */
int vwgpu_create(vwgpu_ctx** ctx, int device);
void vwgpu_destroy(vwgpu_ctx* ctx);

/* Enqueue on an externally owned hipStream_t (passed as void*).  NULL means the legacy default stream
 * (that is what torch's default stream is), NOT the context's own stream — see vwgpu_reset_stream. */
int vwgpu_set_stream(vwgpu_ctx* ctx, void* hip_stream);
/* Back to the context's own (non-blocking) stream. */
int vwgpu_reset_stream(vwgpu_ctx* ctx);
/* Blocks until everything queued on the context's stream is done (and releases the scratch blocks the context has outgrown). */
int vwgpu_synchronize(vwgpu_ctx* ctx);
/* Memory policy: a context keeps one grow-only scratch arena per purpose (pyramids, SGM volumes, exact-order column sums, ...), sized by
 * the largest call it has served — steady-state calls do no hipMalloc / hipFree, which would stall every stream of the device.  A long-lived
 * tile thread therefore holds the high-water mark of every arena until vwgpu_destroy.  vwgpu_trim gives the memory back in between:
 * it waits for the context's stream, then frees every arena (and the outgrown blocks); the next call allocates what it needs again.
 * Call it when a thread changes workload (e.g. after the one config-4-sized SGM strip of a session) or before another context needs
 * the memory; *freed_bytes (optional) receives the amount released. */
int vwgpu_trim(vwgpu_ctx* ctx, size_t* freed_bytes);

const char* vwgpu_strerror(int status);
/* Detail text of the last failing call on this context ("" if none). */
const char* vwgpu_last_error(const vwgpu_ctx* ctx);

/* Per-context options.
 *   VWGPU_OPT_DEFER_EXACTNESS  calc_disparity_dev picks its kernel family from the DATA: integer-valued pixels in [0,255] take
 *       the packed kernels, other inputs the float64 kernel when every box-sum partial is exactly representable (then any
 *       summation order returns the reference's bits), and the reference's own serial summation order otherwise
 *       (VWGPU_PATH_EXACT_ORDER).  The classes are measured on the device; by default (0) the call waits for them, so that
 *       the result is bit-exact for any input.  1 = pipelined callers that queue many calls on byte imagery without a host
 *       round trip: where a packed-u8 kernel exists for the configuration the call is that ONE launch and never waits.  The
 *       option cannot change a result, it can only withhold one: input outside the kernel's domain raises a device flag,
 *       nothing else is computed, vwgpu_last_path() answers VWGPU_PATH_REFUSED for that call (its output buffer is
 *       undefined) and the caller repeats it with the option off.  bench.py asserts VWGPU_PATH_SAD_U8 after its timed steps.
 *       Configurations without a packed-u8 kernel behave as with 0.
 *   VWGPU_OPT_DEVICE_COUNT (read only): HIP devices visible to the process.
 *   The remaining options never change a result (they choose between kernels / schedules that return identical bits, and are
 *   what tests and tools use to reach every variant); values outside the stated range are rejected with VWGPU_ERR_ARGUMENT:
 *   VWGPU_OPT_SAD_GROUPS       packed-u8 SAD matcher flavour: 0 = chosen by the launcher's cost model (default), 1 = one wave
 *       group per tile, 2 = two wave groups per tile, 3 = four wave groups on 512-column tiles of 16 rows (sizes without that flavour
 *       keep the launcher's choice).  Same results in every flavour.
 *   VWGPU_OPT_SAD_LAYOUT       LDS word-group array of the packed-u8 SAD matcher: 0 (default) = entry-major wherever it fits the LDS budget
 *       (row offsets are immediates; its rows are padded, so the widest searches keep the row-major array), 1 = always row-major.  Same results.
 *   VWGPU_OPT_SAD_LAST_LAUNCH  (read only) what the launcher chose for the context's last packed-u8 SAD launch (0 = none yet): bits 0-7 = tile
 *       rows, bits 8-11 = tile columns / 256, bits 12-15 = wave groups per tile, bit 16 = entry-major word groups, bit 17 = the kernel
 *       with streaming output stores (one-group grids of two rounds or more).  For tests and tools.
 *   VWGPU_OPT_SAD_ROUND_SLOTS  workgroup slots the packed-u8 SAD launcher assumes when it marks the first and the last round of dispatch of a
 *       one-group grid (the first-round hand-off and the end balance engage on grids of at least two rounds): 0 (default) = from the
 *       device's CU count, n (1 .. 1048576) = n slots — the launcher then plans, tile choice included, for a device of n / 2 CUs, so that
 *       small grids reach the round logic of the kernels a large image runs.  Timing only; same results.  For tests and tools.
 *   VWGPU_OPT_EXACT_SCRATCH_MB scratch budget of the exact-order path in MiB (16 .. 65536, default 4096): column-sum volumes
 *       beyond it are swept in row bands / zone groups / disparity groups.
 *   VWGPU_OPT_IP_SCRATCH_MB    scratch budget of vwgpu_ip_detect in MiB (1 .. 65536, default 1024): the tiles of a call are taken in
 *       batches whose integral images, interest planes and candidate lists fit it (at least one tile per batch).  Same results.
 *   VWGPU_OPT_TRACE            bit 0: host-side timeline of a pyramid tile on stderr, bit 1: the zone shapes of a level, bit 2: certification
 *       statistics of every tile (one host round trip per tile; VWGPU_OPT_CERT_PERMILLE reads the running total).
 *   VWGPU_OPT_CERTIFY          pyramid levels whose box sums could round (prefiltered imagery, float imagery, deep levels under SSD / NCC): 1
 *       (default) = the tile-parallel kernels match every zone first and CERTIFY each pixel — best cost ahead of the runner-up by more
 *       than twice a rigorous bound on the difference between any-order float64 sums and fast_box_sum's serial running sums
 *       (src/vw/Stereo/Algorithms.h:43-129) — and only zones that hold an uncertified pixel are redone by the exact-order kernels.
 *       A second certificate covers candidates whose partner lies far outside the other image (tiles at the side of a pair: NaN or exactly
 *       tied costs in the margin that no bound can order): when only such candidates can win, the pixel is erased by the mask pass (L->R)
 *       or fails the consistency check (R->L) whichever of them the reference picks, so the tile is the reference's without knowing which.
 *       0 = every zone of such a level goes to the exact-order kernels (the round-3 schedule).  Same results either way.
 *   VWGPU_OPT_ZONE_SXC         horizontal disparities per staged right patch: 0 (default) = 16, n = at most n (1 .. 4096; the LDS budget caps it).
 *   VWGPU_OPT_CERT_PERMILLE    (read only) per mille of the pixels in certified tiles since VWGPU_OPT_TRACE was last set with bit 2; -1 = none.
 *   VWGPU_OPT_CERT_F32         1 (default): the certified pass is two tiers in one launch — float32 window sums and compare chain first,
 *       proven against the reference's order AND their own float32 roundings; a 32 x 32 tile with a pixel that tier cannot prove runs again
 *       in float64, and only what float64 cannot prove goes to the exact-order kernels.  0: float64 only (the round-4 schedule).  Same results.
 *   VWGPU_OPT_ZONE_TILE16      zone matcher tiles for 16 x 16 leaf zones: 0 (default) = 32 x 32 workgroup tiles for every zone, 1 = one-wavefront
 *       16 x 16 tiles for zones of at most 16 x 16 pixels, 2 = those tiles for every zone (measurements).  Same results.
 *   VWGPU_OPT_CERT_F64_PERMILLE (read only) per mille of the counted pixels that lay in tiles the fp32 tier passed on to float64; -1 = none.
 *   VWGPU_OPT_SGM_SWEEP        SGM path aggregation of full-range one-row searches (<= 256 disparities): 0 = one direction per launch
 *       (default: eight passes over the u16 sums, bandwidth bound), 1 = two concurrent fused raster sweeps of four directions each
 *       (a fifth of the HBM traffic, the same sums; slower on MI355X because a sweep is W + 2 H dependent pixel steps), 2 .. 15 = the
 *       sweeps with that many rows per workgroup (tuning).
 *   VWGPU_OPT_SGM_PATH_MODE    the one-direction-per-launch schedule of full-range one-row searches (tuning / measurements; the same sums in every
 *       mode): bits 0-3 = scan lines per workgroup (0 = default: 4 neighbouring lines; 8 = eight lines with a ring of three chunks; the register
 *       kernel: < 4 = one line), bit 5 = the round-2 kernel that prefetches into registers (path_uniform_reg_kernel) instead of the LDS ring
 *       (path_ring_kernel, vector strides up to 160 bytes), bits 8-10 = log2 of the consecutive workgroups given to one XCD, bit 11 = the ring
 *       kernel forms the census costs itself from the census rasters (up to 129 disparities; no u8 cost volume; measured slower).
 *       Ragged boxes (a previous level's disparities given): bit 4 / bit 7 = four / two scan lines per wavefront whatever the level's boxes
 *       (path_multi_kernel; default: chosen per level from the share of small boxes), bit 6 = always one line per wavefront.
 *   VWGPU_OPT_SGM_LAST_FORM    (read only) the form the context's last calc_disparity_sgm call took (0 = none yet, or that call failed; a pyramid's SGM
 *       levels count, the last one stays).  Every form returns the same result; tests assert this word so that a wrong route fails.
 *       bits 0-3   aggregation: 1 = ring per direction (path_ring_kernel), 2 = register per direction (path_uniform_reg_kernel), 3 = fused
 *                  sweeps, 4 = MGM sweeps, 5 = MGM fronts, register form, 6 = MGM fronts, ragged form, 7 = all-direction uniform 2-D
 *                  (path_uniform_kernel), 8 / 9 = multi-line with four / two scan lines per wavefront (path_multi_kernel), 10 = in-place
 *                  (path_inplace_kernel), 11 = three-phase (path_kernel); 0 with bit 20
 *       bits 4-8   width of a launch: forms 1 / 2 = scan lines per workgroup of the last direction launched, 3 / 4 = rows / lines per
 *                  workgroup, 5 = disparity pairs per lane, 6 = pixels per workgroup, 7 = disparities per lane, 8 / 9 = 4 / 2,
 *                  10 = its R (64 R disparities at most), 11 = 0
 *       bit 9      forms 7 - 11: the eight directions went in one launch (0 = eight launches)
 *       bits 10-12 form 1: log2 of the consecutive workgroups given to one XCD
 *       bits 13-15 costs: 0 = none (census costs formed in the ring), 1 = cost_row, 2 = cost_uniform16, 3 = ragged census (cost_kernel),
 *                  4 = block row, 5 = block generic
 *       bits 16-17 winners: 0 = the general kernel only, 1 = wta_uniform first, 2 = taken in the last direction
 *       bits 18-19 memory conservation level at which the loop stopped (0 .. 3)
 *       bit 20     no level fitted the memory limit: the all-invalid result, nothing else ran
 *   VWGPU_OPT_EXACT_SPLIT      pass 2 of the exact-order matchers: 0 = chosen by the width of a zone (the recurrence alone + a parallel
 *       selection for zones of 1024 pixels and more (whole rasters), the tiled form — row sums transposed through LDS — for narrower
 *       ones), 1 = always the split form, 2 = always the fused form (selection across the disparity lanes inside the chain), 3 = always
 *       the tiled form.  Same results in every form.
 *   VWGPU_OPT_MGM_SWEEP        use_mgm on full-range one-row searches (<= 256 disparities): 0 = the eight passes as four concurrent
 *       sweeps (default), 1 = one launch per front (the round-2 schedule), 2 .. 15 = the sweeps with that many lines per workgroup.
 *   VWGPU_OPT_HOST_RING_KB     size in KiB (16 .. 1048576, default 16384) of the pinned host ring through which zone / work-item tables
 *       reach the device; pieces larger than a quarter of it are copied from pageable memory and waited for.  A small ring makes the
 *       library wait for the device more often, nothing else (tests use it to wrap the ring on small rasters).
 *   VWGPU_OPT_HOST_RING_WRAPS  (read only) how often the ring cursor has changed halves so far.
 *   VWGPU_OPT_INPAINT_OVERLAP  the sweeps of vwgpu_inpaint / vwgpu_fill_holes_grass: 1 (default) = consecutive sweeps over a blob overlap
 *       in time, 0 = a sweep starts when the previous one has ended.  Same words in both forms. */
typedef enum vwgpu_option {
  VWGPU_OPT_DEFER_EXACTNESS = 1, VWGPU_OPT_DEVICE_COUNT = 2, VWGPU_OPT_SAD_GROUPS = 3, VWGPU_OPT_EXACT_SCRATCH_MB = 4,
  VWGPU_OPT_TRACE = 5, VWGPU_OPT_SGM_SWEEP = 6, /* 7: removed in ABI 2 */ VWGPU_OPT_MGM_SWEEP = 8, VWGPU_OPT_EXACT_SPLIT = 9,
  /* 10: removed in ABI 2 */ VWGPU_OPT_HOST_RING_KB = 11, VWGPU_OPT_HOST_RING_WRAPS = 12, VWGPU_OPT_CERTIFY = 13,
  VWGPU_OPT_CERT_PERMILLE = 14, VWGPU_OPT_ZONE_SXC = 15, VWGPU_OPT_CERT_F32 = 16, VWGPU_OPT_CERT_F64_PERMILLE = 17, VWGPU_OPT_ZONE_TILE16 = 18,
  VWGPU_OPT_SGM_PATH_MODE = 19, VWGPU_OPT_SAD_LAYOUT = 20, VWGPU_OPT_SAD_LAST_LAUNCH = 21, VWGPU_OPT_SAD_ROUND_SLOTS = 22,
  VWGPU_OPT_IP_SCRATCH_MB = 23, VWGPU_OPT_SGM_LAST_FORM = 24, VWGPU_OPT_INPAINT_OVERLAP = 25
} vwgpu_option;
int vwgpu_set_option(vwgpu_ctx* ctx, int option, int value);
int vwgpu_get_option(const vwgpu_ctx* ctx, int option, int* value);

/* Forces a kernel family (testing / benchmarking): VWGPU_PATH_NONE = automatic dispatch (default). */
int vwgpu_force_path(vwgpu_ctx* ctx, int path);
int vwgpu_last_path(const vwgpu_ctx* ctx);

/* Per-kernel timing with HIP events on the context's stream (bench.py roofline leg).
 * enable=1 records an event pair around every kernel launch of subsequent calls; vwgpu_profile_read
 * synchronises and returns up to `cap` (name, milliseconds) records since the last reset. */
int vwgpu_profile_enable(vwgpu_ctx* ctx, int enable);
int vwgpu_profile_reset(vwgpu_ctx* ctx);
int vwgpu_profile_read(vwgpu_ctx* ctx, const char** names, float* ms, int cap);

/* ---- block matching: calc_disparity -------------------------------------------------------------- */

/* Replaces vw::stereo::calc_disparity (decl src/vw/Stereo/Correlation.h:50-57, impl
 * src/vw/Stereo/Correlation.cc:330-375) from the point where it has rasterised its two crops (:356-359)
 * and calls best_of_search_convolution (:33-137) with fast_box_sum (src/vw/Stereo/Algorithms.h:43-129)
 * and the cost functors of src/vw/Stereo/CostFunctions.h:153-236.
 *
 *   left   lw x lh  : crop(left_in, left_region)
 *   right  rw x rh  : crop(right_in, left_region grown by search_volume-1 on the max side);
 *                     rw >= lw+sx-1 and rh >= lh+sy-1 (larger is allowed, the excess is ignored)
 *   kx,ky  kernel_size (odd; <= lw, lh),  sx,sy search_volume (>= 1)
 *   out    (lw-kx+1) x (lh-ky+1) pixels x {dx,dy,valid}; ostride in PIXELS (0 = dense).
 *          dx in [0,sx), dy in [0,sy): offsets into the right crop, exactly as the reference returns them.
 *
 * Semantics kept from the reference: raster order dy-outer/dx-inner, strict comparison, first wins;
 * a pixel is invalid iff its best and worst cost are equal (so search_volume (1,1) is all-invalid).
 * Bit-exact against the reference for any float input and any search volume: inputs whose box sums could round take the
 * kernels that follow fast_box_sum's serial summation order (VWGPU_PATH_EXACT_ORDER; more than 512 disparities are swept in
 * groups of 512 with the compare-chain state carried from group to group).  See VWGPU_OPT_DEFER_EXACTNESS for the
 * asynchronous variant (which either returns the same bits or reports that it returned none). */
int vwgpu_calc_disparity_dev(vwgpu_ctx* ctx, int cost_type,
                             const float* d_left, int lw, int lh, ptrdiff_t lstride,
                             const float* d_right, int rw, int rh, ptrdiff_t rstride,
                             int kx, int ky, int sx, int sy,
                             int32_t* d_out, ptrdiff_t ostride);

int vwgpu_calc_disparity(vwgpu_ctx* ctx, int cost_type,
                         const float* left, int lw, int lh, ptrdiff_t lstride,
                         const float* right, int rw, int rh, ptrdiff_t rstride,
                         int kx, int ky, int sx, int sy,
                         int32_t* out, ptrdiff_t ostride);

/* ---- box sums ------------------------------------------------------------------------------------------ */

/* Replaces vw::stereo::fast_box_sum<double>(image, kernel) (src/vw/Stereo/Algorithms.h:41-129): out(x, y) = sum of the
 * kx x ky window whose top-left pixel is (x, y), float64, (w-kx+1) x (h-ky+1) pixels, ostride in ELEMENTS (0 = dense).
 * The sums are formed in the reference's order (running column sums down the rows, running row sums along the columns:
 * :62-75, :81-110), so the result is bit-identical for ANY float input, not just exactly summable ones.
 * kx, ky must be odd (the reference's always-on VW_ASSERT, :45-46) and fit the image. */
int vwgpu_fast_box_sum_dev(vwgpu_ctx* ctx, const float* d_img, int w, int h, ptrdiff_t stride, int kx, int ky,
                           double* d_out, ptrdiff_t ostride);
int vwgpu_fast_box_sum(vwgpu_ctx* ctx, const float* img, int w, int h, ptrdiff_t stride, int kx, int ky,
                       double* out, ptrdiff_t ostride);

/* ---- left/right consistency check --------------------------------------------------------------- */

/* Replaces vw::stereo::cross_corr_consistency_check (src/vw/Stereo/Correlate.cc:1441-1502; decl
 * src/vw/Stereo/Correlate.h:52-58): invalidates l2r(c,r) when the r2l pixel at (c+dx, r+dy) is out of
 * bounds or invalid, or when max(|dx+dx'|, |dy+dy'|) > threshold.  In place on l2r. Strides in pixels. */
int vwgpu_cross_corr_consistency_check_dev(vwgpu_ctx* ctx,
                                           int32_t* d_l2r, int lw, int lh, ptrdiff_t lstride,
                                           const int32_t* d_r2l, int rw, int rh, ptrdiff_t rstride,
                                           float threshold);
int vwgpu_cross_corr_consistency_check(vwgpu_ctx* ctx,
                                       int32_t* l2r, int lw, int lh, ptrdiff_t lstride,
                                       const int32_t* r2l, int rw, int rh, ptrdiff_t rstride,
                                       float threshold);

/* The same with the reference's optional lr_disp_diff output (Correlate.cc:1441-1502): diff is a PixelMask<float> image
 * {value, valid} of dcols x drows (stride in pixels, 0 = dcols); every KEPT pixel (c, r) writes {max(|dx+dx'|, |dy+dy'|), 1}
 * at (c + ulx, r + uly), which must lie inside the image. */
int vwgpu_cross_corr_consistency_check_diff_dev(vwgpu_ctx* ctx, int32_t* d_l2r, int lw, int lh, ptrdiff_t lstride,
                                                const int32_t* d_r2l, int rw, int rh, ptrdiff_t rstride, float cross_corr_threshold,
                                                float* d_diff, int dcols, int drows, ptrdiff_t dstride, int ulx, int uly);
int vwgpu_cross_corr_consistency_check_diff(vwgpu_ctx* ctx, int32_t* l2r, int lw, int lh, ptrdiff_t lstride,
                                            const int32_t* r2l, int rw, int rh, ptrdiff_t rstride, float cross_corr_threshold,
                                            float* diff, int dcols, int drows, ptrdiff_t dstride, int ulx, int uly);

/* ---- image filters on the path: Gaussian pyramid and prefilters ------------------------------------- */

/* vw::ConstantEdgeExtension / vw::ZeroEdgeExtension (src/vw/Image/EdgeExtension.h). */
typedef enum vwgpu_edge { VWGPU_EDGE_CONSTANT = 0, VWGPU_EDGE_ZERO = 1 } vwgpu_edge;
/* vw::stereo::PrefilterModeType, src/vw/Stereo/PrefilterEnum.h:24-28 (same numeric values). */
typedef enum vwgpu_prefilter { VWGPU_PREFILTER_NONE = 0, VWGPU_PREFILTER_MEANSUB = 1, VWGPU_PREFILTER_LOG = 2 } vwgpu_prefilter;

/* Replaces vw::generate_gaussian_kernel<float> (src/vw/Image/Filter.tcc:37-78; default size
 * vw::compute_kernel_size, src/vw/Image/Filter.cc:32-37).  Host-side math (erf in double), no context needed.
 * size == 0 selects the default size.  Returns the number of taps written (0 for sigma == 0) or a negative
 * vwgpu_status if cap is too small. */
int vwgpu_generate_gaussian_kernel(double sigma, int size, float* taps, int cap);

/* Replaces rasterising vw::separable_convolution_filter(src, x_kernel, y_kernel, cx, cy, edge)
 * (src/vw/Image/Filter.h:156-191 -> SeparableConvolutionView::rasterize, src/vw/Image/Convolution.h:275-328) over the
 * whole image, optionally followed by vw::subsample(., subsample) (src/vw/Image/Manipulation.h:214-311) — the
 * pyramid-level operation of build_image_pyramids (src/vw/Stereo/CorrelationView.cc:210-214).
 *   nx / ny may be 0 (axis not filtered); cx, cy = kernel origins ((n-1)/2 is the reference's default).
 *   dst is (1+(w-1)/subsample) x (1+(h-1)/subsample).  x_kernel / y_kernel are HOST pointers in both variants.
 * Accumulation order and float arithmetic are the reference's; results are bit-identical for any float input.
 * Accepted kernels: at most 160 taps per axis, and the two tiles of a workgroup must fit 64 KB of LDS:
 *     ((15 s + 1 + max(ny - 1, 0)) * ((63 s + 1 + max(nx - 1, 0)) + 64)) * 4 <= 65536      (s = subsample)
 *   so 67 x 67 taps at s = 1 (also 160 x 0 and 0 x 113), 39 x 39 at s = 2, 15 x 15 at s = 3.  Larger: VWGPU_ERR_NOIMPL.
 * In place: NOT allowed.  Every output reads source pixels that other workgroups would overwrite; the _dev entry returns
 *   VWGPU_ERR_ARGUMENT before any device work when the byte ranges of d_src and d_dst (strides included) overlap.
 *   The host entry stages both images and may be given dst == src. */
int vwgpu_separable_convolution_dev(vwgpu_ctx* ctx, const float* d_src, int w, int h, ptrdiff_t stride,
                                    const float* x_kernel, int nx, int cx, const float* y_kernel, int ny, int cy,
                                    int edge, int subsample, float* d_dst, ptrdiff_t dstride);
int vwgpu_separable_convolution(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t stride,
                                const float* x_kernel, int nx, int cx, const float* y_kernel, int ny, int cy,
                                int edge, int subsample, float* dst, ptrdiff_t dstride);

/* Replaces rasterising vw::convolution_filter(src, kernel, ci, cj, edge) for small 2-D kernels (<= 49 taps)
 * (ConvolutionView, src/vw/Image/Convolution.h:105-170); kernel is row-major kw x kh, HOST pointer.
 * vw::laplacian_filter (src/vw/Image/Filter.h:320-335) is this call with {0,1,0,1,-4,1,0,1,0}, origin (1,1).
 * More than 49 taps: VWGPU_ERR_NOIMPL.  In place: NOT allowed, as for vwgpu_separable_convolution(_dev): overlapping
 * d_src / d_dst are VWGPU_ERR_ARGUMENT before any device work; the host entry stages and may be given dst == src. */
int vwgpu_convolution_2d_dev(vwgpu_ctx* ctx, const float* d_src, int w, int h, ptrdiff_t stride,
                             const float* kernel, int kw, int kh, int ci, int cj, int edge,
                             float* d_dst, ptrdiff_t dstride);
int vwgpu_convolution_2d(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t stride,
                         const float* kernel, int kw, int kh, int ci, int cj, int edge,
                         float* dst, ptrdiff_t dstride);

/* Replaces vw::stereo::subsample_mask_by_two (src/vw/Stereo/CorrelationView.cc:38-63): a 2x2 block with at least
 * two non-zero pixels gives 255, else 0; dst is (1+(w-1)/2) x (1+(h-1)/2).
 * In place: NOT allowed (an output's 2 x 2 block lies where other outputs are written): overlapping d_src / d_dst are
 * VWGPU_ERR_ARGUMENT before any device work; the host entry stages and may be given dst == src. */
int vwgpu_subsample_mask_by_two_dev(vwgpu_ctx* ctx, const uint8_t* d_src, int w, int h, ptrdiff_t stride,
                                    uint8_t* d_dst, ptrdiff_t dstride);
int vwgpu_subsample_mask_by_two(vwgpu_ctx* ctx, const uint8_t* src, int w, int h, ptrdiff_t stride,
                                uint8_t* dst, ptrdiff_t dstride);

/* Replaces vw::stereo::prefilter_image (src/vw/Stereo/PreFilter.h:76-95): NONE = copy, MEANSUB = image -
 * gaussian_filter(image, width), LOG = laplacian_filter(gaussian_filter(image, width)); constant edge extension.
 * The Gaussian has max(3, 7 * width rounded down to odd) taps on each axis and goes through vwgpu_separable_convolution's
 * limit at s = 1: 67 taps, width < 9.86 (69 taps).  Wider: VWGPU_ERR_NOIMPL.
 * In place (d_dst == d_src, same stride): allowed for NONE, MEANSUB at any width and LOG with a non-empty kernel: the
 *   Gaussian goes to a scratch image first, and what follows reads only that, or only the pixel it writes.  LOG with
 *   width 0 is the bare Laplacian of the source: overlapping d_src / d_dst are VWGPU_ERR_ARGUMENT before any device work.
 *   Operands that overlap without being the same image are undefined in the allowed forms too.  The host entry stages. */
int vwgpu_prefilter_image_dev(vwgpu_ctx* ctx, const float* d_src, int w, int h, ptrdiff_t stride,
                              int mode, float width, float* d_dst, ptrdiff_t dstride);
int vwgpu_prefilter_image(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t stride,
                          int mode, float width, float* dst, ptrdiff_t dstride);

/* ---- parabola sub-pixel refinement ------------------------------------------------------------------- */

/* Replaces rasterising vw::stereo::parabola_subpixel(disparity, left, right, prefilter_mode, prefilter_width,
 * kernel_size) (src/vw/Stereo/ParabolaSubpixelView.h:112-117; ParabolaSubpixelView::prerasterize + evaluate,
 * src/vw/Stereo/ParabolaSubpixelView.cc:31-330) over the whole image.
 *   disp  w x h x {dx, dy, valid in {0.f,1.f}} float (PixelMask<Vector2f>; truncated to int like the reference),
 *         same size as the left image (the reference VW_ASSERTs this); strides of disp / out in PIXELS.
 *   left  w x h float, right rw x rh float; both are prefiltered internally (mode / width as in prefilter_image),
 *         with the reference's constant edge extension wherever a window leaves an image.
 *   out   w x h x {dx, dy, valid}: integer disparity + parabola offset (if |offset| < 5 and the nine costs differ),
 *         invalid pixels -> {0,0,0}.
 * Bit-exact on integer-valued imagery with PREFILTER_NONE; otherwise to float rounding. */
int vwgpu_parabola_subpixel_dev(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride,
                                const float* d_left, ptrdiff_t lstride,
                                const float* d_right, int rw, int rh, ptrdiff_t rstride,
                                int prefilter_mode, float prefilter_width, int kx, int ky,
                                float* d_out, ptrdiff_t ostride);
int vwgpu_parabola_subpixel(vwgpu_ctx* ctx, const float* disp, int w, int h, ptrdiff_t dstride,
                            const float* left, ptrdiff_t lstride,
                            const float* right, int rw, int rh, ptrdiff_t rstride,
                            int prefilter_mode, float prefilter_width, int kx, int ky,
                            float* out, ptrdiff_t ostride);

/* ---- pyramid (affine-adaptive) sub-pixel refinement ---------------------------------------------------- */

/* PyramidSubpixelView_Algorithm, src/vw/Stereo/SubpixelView.h:28-33.  vwgpu_pyramid_subpixel[_dev] does not run PHASE:
 * phase refinement is reached through vwgpu_phase_subpixel[_dev] below, which takes its accuracy argument. */
typedef enum vwgpu_subpixel_algorithm {
  VWGPU_SUBPIXEL_LUCAS_KANADE = 0, VWGPU_SUBPIXEL_FAST_AFFINE = 1, VWGPU_SUBPIXEL_BAYES_EM = 2, VWGPU_SUBPIXEL_PHASE = 3
} vwgpu_subpixel_algorithm;

/* Replaces rasterising vw::stereo::lk_subpixel / affine_subpixel / bayes_em_subpixel(disparity, left, right,
 * prefilter_mode, prefilter_width, kernel_size, max_pyramid_levels) (src/vw/Stereo/SubpixelView.h:111-133) tile by tile:
 * one PyramidSubpixelView::prerasterize(bbox) per box (src/vw/Stereo/SubpixelView.cc:33-224; subpixel_optimized_LK_2d,
 * subpixel_optimized_affine_2d and subpixel_optimized_affine_2d_EM, src/vw/Stereo/Correlate.cc:1203-1391, 848-1200,
 * 500-845).
 * The result of a pixel depends on its tile, as in the reference.
 *   disp   w x h x {dx, dy, valid (!= 0)} float, the left image's size; a tile's disparity range is taken over its valid
 *          pixels (zeros without any), as in the reference (DisparityMap.h:48-66, Image/Statistics.h:283-290): what an
 *          invalid pixel stores is never read.  Strides of disp / out in PIXELS.
 *   left   w x h float, right rw x rh float (any size); prefiltered internally (mode / width as prefilter_image) with the
 *          constant edge extension of the source wherever a crop leaves an image (as vwgpu_parabola_subpixel).
 *          A non-finite disparity in a valid pixel of a tile: VWGPU_ERR_ARGUMENT; every tile is checked before the
 *          first one is written.
 *   kx, ky odd (even sizes: VWGPU_ERR_ARGUMENT); max_pyramid_levels < 0 counts as 0.
 *   algorithm  VWGPU_SUBPIXEL_LUCAS_KANADE, VWGPU_SUBPIXEL_FAST_AFFINE or VWGPU_SUBPIXEL_BAYES_EM; VWGPU_SUBPIXEL_PHASE
 *          returns VWGPU_ERR_NOIMPL (use vwgpu_phase_subpixel[_dev]).
 *   tiles  HOST array of ntiles boxes {x, y, w, h} inside the left image; pixels outside every box are not written.
 *   out    refined {dx, dy, 1}, invalid {0, 0, 0}.  Must not alias disp.
 *   stats  optional HOST array of 3: {fixpoint rounds summed over tiles and levels, the most rounds of one tile level,
 *          window-loop iterations run (re-evaluations included; BAYES_EM counts every EM pass over a window)}; NULL
 *          skips the iteration counter.
 * Bit-identical to the reference's sequential in-place order (DESIGN.md sections 4.11, 4.12; the 2 x 2 and 6 x 6 solves
 * follow the LAPACK reference SPOTRF2 / SPOTRS; BAYES_EM's float k * exp(e) is the double form of the host libm).
 * The device entry synchronises the context's stream (data-dependent patch sizes and fixpoint rounds).  VWGPU_ERR_NOMEM
 * when one tile's patch (tile + disparity range + 2 kernels per axis) cannot be held. */
int vwgpu_pyramid_subpixel_dev(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride,
                               const float* d_left, ptrdiff_t lstride,
                               const float* d_right, int rw, int rh, ptrdiff_t rstride,
                               int prefilter_mode, float prefilter_width, int kx, int ky, int max_pyramid_levels,
                               int algorithm, const int* tiles, int ntiles, float* d_out, ptrdiff_t ostride, long long* stats);
int vwgpu_pyramid_subpixel(vwgpu_ctx* ctx, const float* disp, int w, int h, ptrdiff_t dstride,
                           const float* left, ptrdiff_t lstride,
                           const float* right, int rw, int rh, ptrdiff_t rstride,
                           int prefilter_mode, float prefilter_width, int kx, int ky, int max_pyramid_levels,
                           int algorithm, const int* tiles, int ntiles, float* out, ptrdiff_t ostride, long long* stats);

/* Replaces rasterising vw::stereo::phase_subpixel(disparity, left, right, prefilter_mode, prefilter_width, kernel_size,
 * max_pyramid_levels = 0, phase_subpixel_accuracy = 20) (src/vw/Stereo/SubpixelView.h:136-144): PyramidSubpixelView with
 * SUBPIXEL_PHASE, one prerasterize(bbox) per box, whose refiner is subpixel_phase_2d (src/vw/Stereo/PhaseSubpixelView.cc:
 * 231-326): two phase correlations per valid pixel (accuracy / 2, then accuracy on the bicubic-shifted right crop); a
 * pixel whose total offset d has norm_2(d) > 3 or is NaN is invalidated, any other gets disparity -= d.
 * Arguments, tiles, error codes and the out layout as vwgpu_pyramid_subpixel[_dev], without `algorithm`, plus
 *   phase_subpixel_accuracy  the pad factor of the second call (the first gets accuracy / 2); a call whose factor is <= 2
 *          stops after the first pass, as in the reference (so 2, 1, 0 and negative values are accepted).
 * Limits: kx, ky <= 41 and phase_subpixel_accuracy <= 64; larger values return VWGPU_ERR_NOIMPL.
 *   stats  optional HOST array of 3: {pixels refined, pixels invalidated by the 3-pixel / NaN rule, tiles}.
 * The reference's OpenCV DFTs have no reproducible order; the transforms follow the order defined in DESIGN.md section 4.13
 * (direct sums, one fmaf chain per output) and are bit-identical to tests/refimpl/phase_ref.cc.  As the reference's get_dft,
 * every patch is first converted to 8 bits with percentile_scale_convert (2 % / 98 %, 256 bins).
 * The device entry synchronises the context's stream. */
int vwgpu_phase_subpixel_dev(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride,
                             const float* d_left, ptrdiff_t lstride,
                             const float* d_right, int rw, int rh, ptrdiff_t rstride,
                             int prefilter_mode, float prefilter_width, int kx, int ky, int max_pyramid_levels,
                             int phase_subpixel_accuracy, const int* tiles, int ntiles, float* d_out, ptrdiff_t ostride,
                             long long* stats);
int vwgpu_phase_subpixel(vwgpu_ctx* ctx, const float* disp, int w, int h, ptrdiff_t dstride,
                         const float* left, ptrdiff_t lstride,
                         const float* right, int rw, int rh, ptrdiff_t rstride,
                         int prefilter_mode, float prefilter_width, int kx, int ky, int max_pyramid_levels,
                         int phase_subpixel_accuracy, const int* tiles, int ntiles, float* out, ptrdiff_t ostride,
                         long long* stats);

/* ---- disparity quality evaluation ------------------------------------------------------------------------- */

/* CorrEval's metric strings, src/vw/Stereo/CorrEval.h:88-90: "ncc", "stddev", "parabola_curvature", "cramer_rao". */
typedef enum vwgpu_corr_eval_metric {
  VWGPU_CORR_EVAL_NCC = 0, VWGPU_CORR_EVAL_STDDEV = 1, VWGPU_CORR_EVAL_PARABOLA_CURVATURE = 2, VWGPU_CORR_EVAL_CRAMER_RAO = 3
} vwgpu_corr_eval_metric;

/* Replaces rasterising vw::stereo::corr_eval(left, right, disp, kernel_size, metric, sample_rate, round_to_int,
 * prefilter_mode, prefilter_kernel_width) (src/vw/Stereo/CorrEval.h:117-128): one CorrEval::prerasterize(bbox) per box
 * (src/vw/Stereo/CorrEval.cc:139-317).  For each sampled valid pixel p of a box: the NCC of the left kx x ky patch around
 * p against the bilinearly resampled right patch around p + d(p) (NCC), the mean of the two patches' standard
 * deviations (STDDEV), or sigma = sqrt(1 / k_x + 1 / k_y) from the NCC curvature k_x = 2 C - ncc(d + (1, 0)) -
 * ncc(d - (1, 0)), k_y alike (PARABOLA_CURVATURE), times sqrt(max(1 - C, 0)) (CRAMER_RAO).
 *   disp   w x h x {dx, dy, valid (!= 0)} float (PixelMask<Vector2f>), the left image's size.
 *   left   w x h float; left_valid optional w x h uint8 (!= 0 valid; NULL: all valid) with the left image's stride.
 *   right  rw x rh float (any size); right_valid optional, with the right image's stride.  Strides in ELEMENTS (pixels
 *          for disp / out); 0 = packed.
 *   kx, ky positive and odd (VWGPU_ERR_ARGUMENT otherwise); at most 63 x 63 (a workgroup's staged left block then fits
 *          64 KB of LDS at sample rates up to 3); larger kernels return VWGPU_ERR_NOIMPL.
 *   metric a vwgpu_corr_eval_metric (others: VWGPU_ERR_ARGUMENT).  sample_rate >= 1 (the reference divides by zero).
 *   prefilter_mode  accepted and unused, as in the reference; prefilter_kernel_width only sets the right crop's padding
 *          (int)ceil(width) + 5, which must lie in [0, INT_MAX] (a negative padding makes the reference throw when a
 *          patch leaves its left crop): VWGPU_ERR_ARGUMENT otherwise.
 *   tiles  HOST array of ntiles boxes {x, y, w, h} inside the left image; pixels outside every box are not written.
 *          The boxes must not overlap: a pixel inside two boxes receives the result of one of them, unspecified which
 *          (the reference's sequential prerasterize calls would leave the last one's).
 *   out    w x h x {value, valid in {0.f, 1.f}} (PixelMask<float>); every pixel of a box is written, invalid = {0, 0}.
 *   stats  optional HOST array of 4: {sampled valid pixels evaluated, valid results, boxes, boxes whose right box is
 *          degenerate (see below)}.
 * What the reference computes, and the port reproduces bit for bit (tests/refimpl/corr_eval_ref.cc):
 *   - a result depends on its box: a pixel is evaluated only if its column and row inside the box are multiples of
 *     sample_rate, and the right image is read through the box's crop right_box: floor and ceil of bbox.min + (col, row)
 *     + d over the box's sampled valid pixels, expanded by the half kernel, 1, 2, the padding and, for the two curvature
 *     metrics, 1 more.  Interpolation takes coordinates relative to right_box.min, formed in double as
 *     (double(x) + double(dx)) - right_box.min; its integer shortcut compares the double coordinates, its weights are
 *     float(i) - float(floor(i)), and the blend follows BilinearInterpolationImpl's float operation order;
 *   - BBox::expand does nothing on an empty box (min >= max on an axis): when every sampled valid pixel of a box lands on
 *     one integer coordinate in an axis (one sampled row with dy = 0, say), the crop is empty and every right sample is
 *     nodata, so NCC is -1 and the box's results are invalid.  With round_to_int the reference then reads an empty image
 *     out of bounds (undefined); here such reads are nodata too.  A box without sampled valid pixels is all invalid;
 *   - NCC = num / sqrt(den1 den2) in double, c outer, r inner, over the STORED value of every sample: the reference's
 *     validity test is misparenthesised and always passes, so masked left pixels, bilinear blends of invalid right
 *     neighbourhoods and nodata (0) all count; -1 unless den1 > 0 and den2 > 0; a result is valid when >= 0.  No mean
 *     is subtracted.  STDDEV skips invalid samples (two passes in double, sqrt(sum / n));
 *   - the neighbour disparities of the curvature metrics are d + shift in float, so fl32(dx + 1) need not be dx + 1;
 *     sigma is valid when C and the four neighbour NCCs are >= 0 and k_x, k_y > 0;
 *   - round_to_int rounds d half away from zero (roundf) before the box is built and reads the crop without
 *     interpolation;
 *   - the result is the double value cast to float.
 * A non-finite sampled valid disparity (after rounding), a right coordinate outside int32 or a right box that does not
 * fit int32: VWGPU_ERR_ARGUMENT (undefined in the reference); values at invalid or unsampled pixels are never read.
 * Two launches on the context's stream (per-box right boxes, then the evaluation).  Both entries synchronise the
 * context's stream once, after the evaluation, to report the box pass's argument checks; stats add no synchronisation
 * of their own. */
int vwgpu_corr_eval_dev(vwgpu_ctx* ctx, const float* d_disp, int w, int h, ptrdiff_t dstride,
                        const float* d_left, const uint8_t* d_left_valid, ptrdiff_t lstride,
                        const float* d_right, const uint8_t* d_right_valid, int rw, int rh, ptrdiff_t rstride,
                        int kx, int ky, int metric, int sample_rate, int round_to_int,
                        int prefilter_mode, float prefilter_kernel_width, const int* tiles, int ntiles,
                        float* d_out, ptrdiff_t ostride, long long* stats);
int vwgpu_corr_eval(vwgpu_ctx* ctx, const float* disp, int w, int h, ptrdiff_t dstride,
                    const float* left, const uint8_t* left_valid, ptrdiff_t lstride,
                    const float* right, const uint8_t* right_valid, int rw, int rh, ptrdiff_t rstride,
                    int kx, int ky, int metric, int sample_rate, int round_to_int,
                    int prefilter_mode, float prefilter_kernel_width, const int* tiles, int ntiles,
                    float* out, ptrdiff_t ostride, long long* stats);

/* ---- disparity post-filters of Stereo/Algorithms.h ------------------------------------------------------- */

/* The reference's three disparity filters begin with `disparity_out = disparity_in`, a shallow ImageView copy
 * (src/vw/Image/ImageView.h:72, 95-103, 136-148: no user-written copy assignment, the buffer is shared), and then read
 * disparity_in while they write disparity_out in raster order: they run IN PLACE.  A window sees filtered values in the
 * rows above and to the left in its own row, unfiltered values elsewhere.
 *   VWGPU_FILTER_REFERENCE  that recursion, bit for bit; `out` may be the same image as `in` (same pointer and stride).
 *   VWGPU_FILTER_SNAPSHOT   every window reads the unmodified input (what the functions' comments describe); `out`
 *                           must be a different image. */
typedef enum vwgpu_filter_semantics { VWGPU_FILTER_REFERENCE = 0, VWGPU_FILTER_SNAPSHOT = 1 } vwgpu_filter_semantics;

/* Common to the entries below (tests/refimpl/disparity_filters_ref.cc):
 *   in / out  w x h x {dx, dy, valid (!= 0)}, float (PixelMask<Vector2f>) or int32 (PixelMask<Vector2i>); strides in
 *          PIXELS, 0 = packed.  A pixel the filter replaces becomes {dx, dy, 1}; every other pixel of `out` is a copy.
 *   boxes  HOST array of nboxes boxes {x, y, w, h} inside the image that do not overlap (VWGPU_ERR_ARGUMENT otherwise).
 *          Every box is filtered as an image of its own: its own untouched border, edge extension and raster order, as
 *          a caller filtering tile by tile gets.  Pixels outside every box are copied.  One box {0, 0, w, h} is the
 *          reference's call on the whole image.
 *   stats  optional HOST array of 1: pixels whose dx, dy or validity changed (asking for it synchronises the stream).
 * The device entries run on the context's stream and synchronise it once, for the box table. */

/* Replaces vw::stereo::disparity_median_filter (src/vw/Stereo/Algorithms.cc:26-67; math::destructive_median,
 * src/vw/Math/Functors.h:393-398): per channel the median of the valid disparities of the kernel window as doubles, the
 * mean of the two middle ones ((a + b) / 2.0) for an even count, narrowed to float.  half = (kernel_size - 1) / 2 (an
 * even size uses the next smaller odd window); a border of `half` pixels and invalid centres are untouched;
 * kernel_size < 3 copies; negative: VWGPU_ERR_ARGUMENT; above 31: VWGPU_ERR_NOIMPL.  A window with a NaN among its valid
 * disparities (std::sort is undefined there) leaves its pixel unchanged; the sign of a zero median is unspecified. */
int vwgpu_disparity_median_filter_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, int kernel_size,
                                      int semantics, const int* boxes, int nboxes, float* d_out, ptrdiff_t ostride,
                                      long long* stats);
int vwgpu_disparity_median_filter(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, int kernel_size,
                                  int semantics, const int* boxes, int nboxes, float* out, ptrdiff_t ostride,
                                  long long* stats);

/* Replaces vw::stereo::disparity_neighbor_filter (src/vw/Stereo/Algorithms.cc:69-110): among the 8 neighbours in the
 * reference's order, each valid one counts the neighbours equal to it in dx, dy and validity; the first strictly larger
 * count wins and, at 5 or more, replaces the centre whatever the centre's own validity.  A 1-pixel border is untouched. */
int vwgpu_disparity_neighbor_filter_dev(vwgpu_ctx* ctx, const int32_t* d_in, int w, int h, ptrdiff_t istride, int semantics,
                                        const int* boxes, int nboxes, int32_t* d_out, ptrdiff_t ostride, long long* stats);
int vwgpu_disparity_neighbor_filter(vwgpu_ctx* ctx, const int32_t* in, int w, int h, ptrdiff_t istride, int semantics,
                                    const int* boxes, int nboxes, int32_t* out, ptrdiff_t ostride, long long* stats);

/* Replaces vw::stereo::texture_measure on a plain float image (src/vw/Stereo/Algorithms.h:144-209): per pixel, over the
 * (2 half + 1)^2 window (half = (kernel_size - 1) / 2) of the edge-extended image, score = float(gradient_weight *
 * sum(|dx| + |dy|) / (2 n) + stddev_weight * sqrt(sum((v - mean)^2) / n)), with dx, dy = derivative_filter (kernel
 * {0.5, 0, -0.5}, constant edge extension, the derivative images edge-extended again), |dx| + |dy| a float add, all
 * sums in double in the reference's order (r outer, c inner).  out: w x h float, written inside the boxes only (a box
 * is an image of its own, see above); strides in elements.  kernel_size < 1: VWGPU_ERR_ARGUMENT; above 31:
 * VWGPU_ERR_NOIMPL.  max_score: optional HOST float, the largest score written (0 when none is positive; the
 * reference's caller scales texture_max from it; asking for it synchronises the stream). */
int vwgpu_texture_measure_dev(vwgpu_ctx* ctx, const float* d_image, int w, int h, ptrdiff_t stride, int kernel_size,
                              double gradient_weight, double stddev_weight, const int* boxes, int nboxes, float* d_out,
                              ptrdiff_t ostride, float* max_score);
int vwgpu_texture_measure(vwgpu_ctx* ctx, const float* image, int w, int h, ptrdiff_t stride, int kernel_size,
                          double gradient_weight, double stddev_weight, const int* boxes, int nboxes, float* out,
                          ptrdiff_t ostride, float* max_score);

/* Replaces vw::stereo::texture_preserving_disparity_filter<float> (src/vw/Stereo/Algorithms.h:215-281): a valid pixel
 * with texture t >= 0 gets the window size floor(max(texture_max - t, 0) * (max_kernel_size / texture_max)) (float
 * arithmetic), made odd; sizes below 3 or above max_kernel_size leave the pixel; otherwise the pixel becomes the mean,
 * summed in double and narrowed to float, of the valid pixels of that window of the edge-extended (clamped) disparity.
 * texture: w x h float (tstride in elements, 0 = packed).  max_kernel_size < 3 or texture_max <= 0 copies; negative
 * max_kernel_size or NaN texture_max: VWGPU_ERR_ARGUMENT; max_kernel_size above 31: VWGPU_ERR_NOIMPL.  A pixel whose
 * texture or window-size product is not finite (undefined in the reference) is left unchanged. */
int vwgpu_texture_preserving_disparity_filter_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride,
                                                  const float* d_texture, ptrdiff_t tstride, float texture_max,
                                                  int max_kernel_size, int semantics, const int* boxes, int nboxes,
                                                  float* d_out, ptrdiff_t ostride, long long* stats);
int vwgpu_texture_preserving_disparity_filter(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride,
                                              const float* texture, ptrdiff_t tstride, float texture_max,
                                              int max_kernel_size, int semantics, const int* boxes, int nboxes,
                                              float* out, ptrdiff_t ostride, long long* stats);

/* ---- local outlier filters of Stereo/DisparityMap.h and std_dev_image ---------------------------------- */

/* The window filters of DisparityMap.h besides rm_outliers_using_thresh (vwgpu_disparity_filter below). */
typedef enum vwgpu_outlier_method { VWGPU_OUTLIER_MEAN = 0, VWGPU_OUTLIER_STDDEV = 1, VWGPU_OUTLIER_PLANE = 2 } vwgpu_outlier_method;
/* RmOutliersUsingMeanFunc skips a pixel whose magnitude exceeds the cutoff with a `continue` that also skips
 * col_acc.next_col() (src/vw/Stereo/DisparityMap.h:525): the accessor stops advancing and the rest of that window row is
 * never read.
 *   VWGPU_OUTLIER_REFERENCE  that behaviour: a window row ends at its first valid pixel above the cutoff.
 *   VWGPU_OUTLIER_SKIP       only the offending pixel is skipped (what the comment at :492-496 describes).
 * The other two methods ignore the value (it must still be one of the two). */
typedef enum vwgpu_outlier_semantics { VWGPU_OUTLIER_REFERENCE = 0, VWGPU_OUTLIER_SKIP = 1 } vwgpu_outlier_semantics;
/* PixelMask<Vector2i> as int32 {dx, dy, valid != 0}; PixelMask<Vector2f> as float {dx, dy, valid != 0}. */
typedef enum vwgpu_disparity_type { VWGPU_DISPARITY_I32 = 0, VWGPU_DISPARITY_F32 = 1 } vwgpu_disparity_type;

/* Replaces rasterising, over a whole image of either disparity pixel type (DESIGN.md section 4.16;
 * tests/refimpl/outlier_filters_ref.cc),
 *   VWGPU_OUTLIER_MEAN    vw::stereo::rm_outliers_using_mean(d, half_h, half_v, p0 = max_mean_diff)
 *                         (src/vw/Stereo/DisparityMap.h:444-578; p1 is ignored),
 *   VWGPU_OUTLIER_STDDEV  vw::stereo::rm_outliers_using_stddev(d, half_h, half_v, p0 = pixel_threshold,
 *                         p1 = rejection_threshold) (DisparityMap.h:600-748),
 *   VWGPU_OUTLIER_PLANE   vw::stereo::rm_outliers_using_plane(d, half_h, half_v, p0 = pixel_threshold,
 *                         p1 = rejection_threshold) (DisparityMap.h:769-927, DisparityMap.cc:37-118),
 * and with cleanup != 0 disparity_cleanup_using_mean (:580-598), disparity_cleanup_using_stddev (:750-767),
 * disparity_clean_using_plane (:929-947): the filter followed by RmOutliersUsingThreshFunc(1, 1, 3.0, 0.2) (:357-385)
 * on the inner VIEW, which is also read one pixel outside the image, where the inner functor runs on clamped reads.
 * Every window is (2 half_h + 1) x (2 half_v + 1) pixels of edge_extend(d, ConstantEdgeExtension()), rows outer and
 * columns inner, read from the unmodified input; arithmetic is double in the reference's order without contraction.
 * An invalid centre is copied (stored values included); a rejected pixel becomes {0, 0, 0}.
 *   mean    cutoff = 2.0 * sorted(|dx| + |dy| of the valid pixels)[(int)(0.75 n)] (a float add for float pixels, an int
 *           add for int pixels); the mean of the valid pixels with magnitude <= cutoff (see vwgpu_outlier_semantics);
 *           rejected when (x-mx)*(x-mx) + (y-my)*(y-my) > p0*p0, or with no pixel matched (max_mean_diff^2 + 1.0 >
 *           max_mean_diff^2, as :536 has it).  A window with a NaN among its valid disparities (std::sort is undefined
 *           there) leaves its pixel unchanged.
 *   stddev  mean, then sigma = sqrt(sum((v - mean)^2) / n) per channel, raised to p1 when below it; rejected when
 *           |x - mx| > p0 * sigma_x or |y - my| > p0 * sigma_y.  The reference sizes its value buffer (2 half_v + 1)^2
 *           (:656): half_h > half_v is outside what it defines; the evident result is computed.
 *   plane   per channel z = a xk + b yk + c fitted to the valid pixels at window offsets (xk, yk) by the normal
 *           equations of fitPlaneToPoints; sigma = sqrt(sum(dist^2) / n) with dist = |a xk + b yk - z + c| /
 *           sqrt(a^2 + b^2 + 1), raised to p1 when below it; rejected when the distance of (0, 0, z_centre) exceeds
 *           p0 * sigma in either channel.  The reference solves with LAPACK gesv and keeps the pixel when that reports
 *           an exactly zero pivot (:866-875).  LAPACK's bits are not pinned; the specification is the restatement's
 *           elimination: unblocked LU with partial pivoting (column-wise search, the first largest |a| wins),
 *           multipliers by the reciprocal of the pivot, rank-1 update, two triangular solves; an exactly zero pivot
 *           keeps the pixel.
 * in / out  w x h pixels of `type`, strides in PIXELS, 0 = packed; they must be different images.
 * half_h, half_v  1 .. 15; <= 0: VWGPU_ERR_ARGUMENT ("half kernel sizes must be non-zero."); above 15: VWGPU_ERR_NOIMPL.
 * A NaN threshold: VWGPU_ERR_ARGUMENT.
 * stats  optional HOST long long[2]: pixels rejected by the filter and by the clean-up pass, both counted inside the
 *        image (asking for it synchronises the stream). */
int vwgpu_rm_outliers_dev(vwgpu_ctx* ctx, int method, int type, const void* d_in, int w, int h, ptrdiff_t istride, int half_h,
                          int half_v, double p0, double p1, int cleanup, int semantics, void* d_out, ptrdiff_t ostride,
                          long long* stats);
int vwgpu_rm_outliers(vwgpu_ctx* ctx, int method, int type, const void* in, int w, int h, ptrdiff_t istride, int half_h,
                      int half_v, double p0, double p1, int cleanup, int semantics, void* out, ptrdiff_t ostride,
                      long long* stats);

/* Replaces rasterising vw::stereo::std_dev_image(image, kernel_width, kernel_height[, edge]) on a plain float image
 * (src/vw/Stereo/DisparityMap.h:949-1014, DisparityMap.cc:24-34): float accumulators in the reference's order over the
 * offsets -k/2 .. k/2 in each direction (an even size reads k + 1 samples), mean = sum / (kw kh), result = sum of
 * squared differences / (kw kh - 1): the variance, despite the name; at 1 x 1 that is 0.0f / 0, NaN.  edge:
 * VWGPU_EDGE_ZERO (the reference's default overload) or VWGPU_EDGE_CONSTANT.  Strides in elements, 0 = packed.  A size
 * <= 0: VWGPU_ERR_ARGUMENT ("kernel sizes must be non-zero."); above 31: VWGPU_ERR_NOIMPL. */
int vwgpu_std_dev_image_dev(vwgpu_ctx* ctx, const float* d_image, int w, int h, ptrdiff_t stride, int kernel_width,
                            int kernel_height, int edge, float* d_out, ptrdiff_t ostride);
int vwgpu_std_dev_image(vwgpu_ctx* ctx, const float* image, int w, int h, ptrdiff_t stride, int kernel_width, int kernel_height,
                        int edge, float* out, ptrdiff_t ostride);

/* ---- the rest of Stereo/DisparityMap.h: range, masks, transforms, resampling ---------------------------- */

/* Common to the entries of this block (tests/refimpl/disparity_map_ref.cc): `type` is a
 * vwgpu_disparity_type, pixels are {dx, dy, valid != 0} of int32 or float; strides are in PIXELS, 0 = packed; the _dev
 * form takes device pointers and works on the context's stream, the other form host pointers.  Arithmetic is the
 * reference's types in its order, without contraction.  Operators that use a pixel's location take x0, y0: the image
 * coordinates of pixel (0, 0) of the buffer handed in, so a tile or a row strip of a larger map gives the same pixels as
 * the whole map.  Null pointers, sizes <= 0, an unknown type / semantics / mode, a NaN in min / max / matrix, a stride
 * below the width and in == out where it is not allowed give VWGPU_ERR_ARGUMENT before any device work; nothing here
 * returns VWGPU_ERR_NOIMPL. */

/* Replaces vw::stereo::get_disparity_range (src/vw/Stereo/DisparityMap.h:48-66) with its accumulator
 * PixelAccumulator<EWMinMaxAccumulator> (src/vw/Image/Statistics.h:193-224, :283-290): range = {min.x, min.y, max.x,
 * max.y} over the VALID pixels (PixelAccumulator skips the others, Statistics.h:287, whatever the TODO at
 * DisparityMap.h:56 supposes), {0, 0, 0, 0} when there is none.  For int32 pixels the extrema are taken in int32 and
 * converted to float at the end.  The accumulator's `if (arg < min) .. else if (arg > max)` never admits a NaN after the
 * first sample: a NaN component makes both extrema of that component NaN when it sits in the first valid pixel in raster
 * order, and is ignored anywhere else.  The sign of a zero extremum depends on the reference's visiting order and is not
 * pinned (compare with ==).
 * _dev: d_range (device float[4]) and host_range (host float[4]) are both optional, one of them must be given; only
 * host_range synchronises the stream. */
int vwgpu_get_disparity_range_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, float* d_range,
                                  float* host_range);
int vwgpu_get_disparity_range(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, float* range);

/* DisparityRangeMaskFunc compares the lower bound of y with m_min[0] (src/vw/Stereo/DisparityMap.h:279).
 *   VWGPU_RANGE_MASK_REFERENCE  that comparison as written.
 *   VWGPU_RANGE_MASK_FIXED      the lower bound of y is min[1]. */
typedef enum vwgpu_range_mask_semantics { VWGPU_RANGE_MASK_REFERENCE = 0, VWGPU_RANGE_MASK_FIXED = 1 } vwgpu_range_mask_semantics;

/* Replaces rasterising vw::stereo::disparity_range_mask(d, min, max) (src/vw/Stereo/DisparityMap.h:255-300): a valid
 * pixel at location loc = (x0 + x, y0 + y) becomes {0, 0, 0} when loc + d leaves [min, max - 1) in x or y; loc + d is a
 * double sum of the double location and the channel, the bounds are values of the pixel's channel type and max - 1 is
 * computed in that type (min, max arrive as double[2] and are converted to it first: for int32 pixels they are truncated
 * and must fit int32, max above INT32_MIN).  Invalid pixels are copied, stored values included.  in == out is allowed.
 * stats  optional HOST long long[1]: the number of pixels masked (asking for it synchronises the stream). */
int vwgpu_disparity_range_mask_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, int x0, int y0,
                                   const double* min, const double* max, int semantics, void* d_out, ptrdiff_t ostride,
                                   long long* stats);
int vwgpu_disparity_range_mask(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, int x0, int y0,
                               const double* min, const double* max, int semantics, void* out, ptrdiff_t ostride, long long* stats);

/*   VWGPU_TRANSFORM_FUNCTOR          transform_disparities(d, transform) (src/vw/Stereo/DisparityMap.h:1016-1057)
 *   VWGPU_TRANSFORM_SUBREGION        transform_disparities(false, subregion, T, d) (:1190-1224)
 *   VWGPU_TRANSFORM_SUBREGION_ROUND  transform_disparities(true, subregion, T, d) */
typedef enum vwgpu_transform_mode {
  VWGPU_TRANSFORM_FUNCTOR = 0, VWGPU_TRANSFORM_SUBREGION = 1, VWGPU_TRANSFORM_SUBREGION_ROUND = 2
} vwgpu_transform_mode;

/* Replaces both overloads of vw::stereo::transform_disparities.  matrix is a row-major double[9] applied to a point
 * exactly as HomographyTransform::forward does (src/vw/Math/Transform.h:383-387): w = m20 px + m21 py + m22 first, then
 * ((m00 px + m01 py + m02) / w, (m10 px + m11 py + m12) / w).  A translation or an affine transform is a matrix with last
 * row (0, 0, 1).  With loc = (x0 + x, y0 + y) as doubles:
 *   FUNCTOR    q = M(loc + d); the pixel becomes (q.x - loc.x, q.y - loc.y) converted to the channel type (for int32
 *              the C++ conversion, toward zero); the mask word is copied, and an invalid pixel gets the transformed
 *              stored values too (:1037-1042).  The functor calls transform.reverse(): the ABI is pinned on the APPLIED
 *              matrix, which for HomographyTransform(H) is inverse(H).  The C++ and Python layers compute that inverse
 *              with a plain 3 x 3 adjugate; the bits of the reference's inverse() are not pinned.
 *   SUBREGION  (x0, y0) = subregion.min(), M = T: diff = M(loc + d) - loc, rounded with C round() in the _ROUND mode,
 *              converted as above; an invalid pixel gives {0, 0, 0}.
 * When the conversion of a result to int32 would leave int32 the pixel is unspecified.  in == out is allowed. */
int vwgpu_transform_disparities_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, int x0, int y0,
                                    const double* matrix, int mode, void* d_out, ptrdiff_t ostride);
int vwgpu_transform_disparities(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, int x0, int y0,
                                const double* matrix, int mode, void* out, ptrdiff_t ostride);

/* Replaces rasterising vw::stereo::disparity_subsample(d) (src/vw/Stereo/DisparityMap.h:1251-1322): out is
 * (1 + (w - 1) / 2) x (1 + (h - 1) / 2); pixel (i, j) sums the valid ones of nine taps of edge_extend(d,
 * ConstantEdgeExtension()) around (2i, 2j) in the order (0,0) (+1,0) (0,+1) (-1,0) (0,-1) (+1,+1) (-1,-1) (-1,+1)
 * (+1,-1) with weights 10, 5, 5, 5, 5, 2, 2, 2, 2.  The accumulator is AccumulatorType<channel>
 * (src/vw/Core/FundamentalTypes.h:118, :121): int64 for int32 pixels, double for float pixels.  The first three taps
 * are cast to it before the product, the other six are multiplied in the pixel's own type (:1273-1299; an int32 product
 * that overflows wraps).  The result is buffer / (count * 2) in the accumulator type (an integer division toward zero
 * for int32 pixels), converted to the channel type, with the mask word validate() writes (INT32_MAX or 1.0f); with no
 * valid tap {0, 0, 0}.  in and out must differ. */
int vwgpu_disparity_subsample_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, void* d_out,
                                  ptrdiff_t ostride);
int vwgpu_disparity_subsample(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, void* out, ptrdiff_t ostride);

/* Replaces rasterising vw::stereo::disparity_upsample(d) (src/vw/Stereo/DisparityMap.h:1324-1358): out is 2w x 2h and
 * pixel (i, j) is d(i >> 1, j >> 1) * 2 in the pixel's type (stored values of invalid pixels too), the mask word copied.
 * in and out must differ. */
int vwgpu_disparity_upsample_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, void* d_out,
                                 ptrdiff_t ostride);
int vwgpu_disparity_upsample(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, void* out, ptrdiff_t ostride);

/* Replaces rasterising transform(right, DisparityTransform(disparity)) (src/vw/Stereo/DisparityMap.h:1164-1187): the
 * right image seen from the left one.  right and out are float images of rw x rh, disparity a float {dx, dy, valid} map
 * of dw x dh (strides in elements / pixels, 0 = packed).  Output pixel (x, y): the offset is disparity(x, y) inside
 * dw x dh and invalid outside (nearest interpolation at an integer position over ZeroEdgeExtension); an invalid offset
 * gives p = (-1, y), a valid one p = (x + (double)dx, y + (double)dy); the result is BilinearInterpolationImpl
 * (src/vw/Image/Interpolation.h:76-110) at p on the zero-extended right image, in float: right(px, py) itself when both
 * coordinates are integers, otherwise normx = float(p.x) - float(floor p.x) (normy alike) and
 * ((r00 (1 - normx) + r10 normx) (1 - normy)) + (r01 (1 - normx) + r11 normx) normy, every product and sum rounded on
 * its own.  The reference converts floor(p) to int32, which is undefined for a NaN or a huge p; THIS project defines the
 * result as 0 when a coordinate of p is NaN or beyond +-2^30.  The output must differ from both inputs. */
int vwgpu_disparity_warp_dev(vwgpu_ctx* ctx, const float* d_right, int rw, int rh, ptrdiff_t rstride, const float* d_disparity, int dw,
                             int dh, ptrdiff_t dstride, float* d_out, ptrdiff_t ostride);
int vwgpu_disparity_warp(vwgpu_ctx* ctx, const float* right, int rw, int rh, ptrdiff_t rstride, const float* disparity, int dw, int dh,
                         ptrdiff_t dstride, float* out, ptrdiff_t ostride);

/* Replaces rasterising vw::stereo::missing_pixel_image(d) (src/vw/Stereo/DisparityMap.h:68-87): out is w x h pixels of
 * three uint8 (PixelRGB<uint8>; ostride in pixels), (200, 200, 200) for a valid pixel and (255, 0, 0) for an invalid one. */
int vwgpu_missing_pixel_image_dev(vwgpu_ctx* ctx, int type, const void* d_in, int w, int h, ptrdiff_t istride, unsigned char* d_out,
                                  ptrdiff_t ostride);
int vwgpu_missing_pixel_image(vwgpu_ctx* ctx, int type, const void* in, int w, int h, ptrdiff_t istride, unsigned char* out,
                              ptrdiff_t ostride);

/* Replaces rasterising vw::stereo::intersect_mask_and_data(data, mask) (src/vw/Stereo/DisparityMap.h:1226-1249) on two
 * maps of the same type and size: the data pixel if it is valid, else the mask pixel if that is valid, else the data
 * pixel.  out may be either input. */
int vwgpu_intersect_mask_and_data_dev(vwgpu_ctx* ctx, int type, const void* d_data, ptrdiff_t dstride, const void* d_mask,
                                      ptrdiff_t mstride, int w, int h, void* d_out, ptrdiff_t ostride);
int vwgpu_intersect_mask_and_data(vwgpu_ctx* ctx, int type, const void* data, ptrdiff_t dstride, const void* mask, ptrdiff_t mstride,
                                  int w, int h, void* out, ptrdiff_t ostride);

/* ---- Image/Grassfire.h, BlobIndex.h, ErodeView.h, InpaintView.h: filling the holes of a masked image ---------- */
/* (tests/refimpl/hole_fill_ref.cc.)  Strides are in pixels, 0 = packed.  Masked pixels:
 *   VWGPU_PIXEL_MASK_U8        one uint8, non-zero = valid
 *   VWGPU_PIXEL_MASKED_F32     PixelMask<float> as float {value, valid != 0}
 *   VWGPU_PIXEL_DISPARITY_I32  PixelMask<Vector2i> as int32 {dx, dy, valid != 0}
 *   VWGPU_PIXEL_DISPARITY_F32  PixelMask<Vector2f> as float {dx, dy, valid != 0}
 * An image holds at most 2^31 - 1 pixels. */
typedef enum vwgpu_pixel_kind {
  VWGPU_PIXEL_MASK_U8 = 0, VWGPU_PIXEL_MASKED_F32 = 1, VWGPU_PIXEL_DISPARITY_I32 = 2, VWGPU_PIXEL_DISPARITY_F32 = 3
} vwgpu_pixel_kind;
typedef enum vwgpu_grassfire_type { VWGPU_GRASSFIRE_U8 = 0, VWGPU_GRASSFIRE_I32 = 1, VWGPU_GRASSFIRE_F32 = 2 } vwgpu_grassfire_type;
/* InpaintTask leaves a blob alone when its bounding box grown by one has min < 0 or max >= cols / rows with an EXCLUSIVE max
 * (src/vw/Image/InpaintView.h:76-80): a blob touching column 0 or row 0 is skipped, and so is one whose last column is >= cols - 2 or
 * whose last row is >= rows - 2, although a hole with one valid column to its right has its whole ring inside the image.
 *   VWGPU_HOLE_EDGE_REFERENCE  that rule as written (what the reference gives when it rasterises the whole image as one tile).
 *   VWGPU_HOLE_EDGE_FIXED      exactly the blobs that touch the image border are skipped; any tiling of the reference then gives
 *                              these pixels wherever its tile's crop does not cut the rule short. */
typedef enum vwgpu_hole_edge_semantics { VWGPU_HOLE_EDGE_REFERENCE = 0, VWGPU_HOLE_EDGE_FIXED = 1 } vwgpu_hole_edge_semantics;
/* The largest hole_fill_len / max_len: a blob's bounding box grown by one lives in the LDS of one workgroup. */
#define VWGPU_HOLE_FILL_MAX_LEN 64

/* Replaces vw::grassfire(src, dst, ignore_borders) (src/vw/Image/Grassfire.h:79-228) with an int32 output: the Manhattan distance
 * to the nearest pixel with src == 0 (a NaN is non-zero, -0.0f is zero).  ignore_borders == 0: everything outside the image counts
 * as zero; otherwise it does not and the result is capped at cols + rows.  cols <= 1 or rows <= 1 gives zeros (:86).
 * src_type: a vwgpu_grassfire_type.  out must not overlap src. */
int vwgpu_grassfire_dev(vwgpu_ctx* ctx, int src_type, const void* d_src, int w, int h, ptrdiff_t sstride, int ignore_borders,
                        int32_t* d_out, ptrdiff_t ostride);
int vwgpu_grassfire(vwgpu_ctx* ctx, int src_type, const void* src, int w, int h, ptrdiff_t sstride, int ignore_borders, int32_t* out,
                    ptrdiff_t ostride);

/* Replaces BlobIndexThreaded(src, max_area, tile_size) with the whole image as ONE tile, followed by wipe_big_blobs(wipe_size)
 * when wipe_size > 0 (src/vw/Image/BlobIndex.h:113-306, :385-477): the 8-connected components of the valid pixels (invert != 0: of
 * the invalid ones, invert_mask), in the reference's order (the k-th blob is the one whose first pixel in raster order comes
 * k-th); max_area > 0 drops blobs of more than max_area pixels (:445-453), wipe_size > 0 those whose bounding box is wider or
 * taller than wipe_size (:457-477).  *count (host, required) receives the number of blobs kept.
 *   labels (optional, int32 w x h): the 1-based number of the kept blob a pixel belongs to, else 0.  NOT what blob_index() of the
 *       reference returns: that image keeps the provisional labels of the raster pass (:267-304).
 *   table (optional, table_cap rows of 5 int32): {min.x, min.y, max.x, max.y, size} per kept blob, the box half-open.  With more
 *       blobs than table_cap the call returns VWGPU_ERR_CAPACITY, *count says how many rows it takes, the table is not written.
 * The _dev form takes labels and table on the device and waits for the device (count).  Multi-tile consolidate() and its
 * tile-dependent blob order are not reproduced. */
int vwgpu_blob_index_dev(vwgpu_ctx* ctx, int kind, const void* d_img, int w, int h, ptrdiff_t istride, int invert, int max_area,
                         int wipe_size, int32_t* d_labels, ptrdiff_t lstride, int32_t* d_table, int table_cap, int* count);
int vwgpu_blob_index(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, int invert, int max_area, int wipe_size,
                     int32_t* labels, ptrdiff_t lstride, int32_t* table, int table_cap, int* count);

/* Replaces vw::get_blob_sizes(image, expand, limit) (src/vw/Image/BlobIndex.h:507-615) with the image as one tile: every valid
 * pixel receives min(size of its blob, limit), every invalid pixel 0 (uint32 w x h). */
int vwgpu_blob_sizes_dev(vwgpu_ctx* ctx, int kind, const void* d_img, int w, int h, ptrdiff_t istride, uint32_t limit, uint32_t* d_out,
                         ptrdiff_t ostride);
int vwgpu_blob_sizes(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, uint32_t limit, uint32_t* out,
                     ptrdiff_t ostride);

/* Replaces applyErodeView(src, BlobIndexThreaded(src, max_area, ..)) (src/vw/Image/ErodeView.h:199-221) on any pixel kind: every
 * pixel of a blob of VALID pixels with at most max_area pixels becomes the default pixel (every word 0, invalid), everything else
 * is copied; max_area < 1 copies.  For int32 disparities this is vwgpu_disparity_blob_filter.  out may be the input. */
int vwgpu_erode_blobs_dev(vwgpu_ctx* ctx, int kind, const void* d_img, int w, int h, ptrdiff_t istride, int max_area, void* d_out,
                          ptrdiff_t ostride);
int vwgpu_erode_blobs(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, int max_area, void* out, ptrdiff_t ostride);

/* Replaces rasterising vw::inpaint(src, bindex, use_grassfire, default_inpaint_val) (src/vw/Image/InpaintView.h:44-237) in one
 * call over the whole image, for VWGPU_PIXEL_MASKED_F32 and VWGPU_PIXEL_DISPARITY_F32.  The blob selection {labels, table, count}
 * is what vwgpu_blob_index returned, kept on the device for the _dev form.  Every blob is filled independently from the unpatched
 * input; a blob skipped by the edge rule (vwgpu_hole_edge_semantics) or wider or taller than max_len (<= VWGPU_HOLE_FILL_MAX_LEN;
 * as wipe_big_blobs(max_len) would have removed it) is left as it is.
 *   use_grassfire != 0: 10 * max_distance^2 in-place sweeps over the blob's pixels in the order (grassfire distance, column, row);
 *       a pixel becomes the weighted sum of its eight neighbours (.176765 diagonal, .073235 side; UL U UR L R DL D DR), each term
 *       added in double and rounded to the float accumulator (:120-138), and valid.  The stored values of the invalid pixels are
 *       the initial guess.  Word for word the serial result.
 *   use_grassfire == 0: the blob's pixels become default_pixel (host; 2 or 3 floats, validity last; NULL = zeros) as given.
 * out may be the input: a blob reads only itself and its ring of valid pixels. */
int vwgpu_inpaint_dev(vwgpu_ctx* ctx, int kind, const void* d_img, int w, int h, ptrdiff_t istride, const int32_t* d_labels, ptrdiff_t lstride,
                      const int32_t* d_table, int count, int use_grassfire, const float* default_pixel, int semantics, int max_len,
                      void* d_out, ptrdiff_t ostride);
int vwgpu_inpaint(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, const int32_t* labels, ptrdiff_t lstride,
                  const int32_t* table, int count, int use_grassfire, const float* default_pixel, int semantics, int max_len, void* out,
                  ptrdiff_t ostride);

/* Replaces rasterising vw::fill_holes_grass(img, hole_fill_len) (src/vw/Image/InpaintView.h:239-311) in one call over the whole
 * image: the blobs of the INVALID pixels, wipe_big_blobs(hole_fill_len) (which implies the area limit hole_fill_len^2), inpaint
 * with grassfire.  0 <= hole_fill_len <= VWGPU_HOLE_FILL_MAX_LEN, else VWGPU_ERR_ARGUMENT before any device work.  The result
 * does not depend on a tiling except through the edge rule, which the reference applies to its tile's crop.  Float kinds only.
 * out may be the input.  Waits for the device (the number of blobs). */
int vwgpu_fill_holes_grass_dev(vwgpu_ctx* ctx, int kind, const void* d_img, int w, int h, ptrdiff_t istride, int hole_fill_len, int semantics,
                               void* d_out, ptrdiff_t ostride);
int vwgpu_fill_holes_grass(vwgpu_ctx* ctx, int kind, const void* img, int w, int h, ptrdiff_t istride, int hole_fill_len, int semantics,
                           void* out, ptrdiff_t ostride);

/* Replaces rasterising vw::fill_nodata_with_avg(img, kernel_size) (src/vw/Image/InpaintView.h:317-387) on PixelMask<float>
 * {value, valid}: an invalid pixel becomes the float sum of the valid pixels of its kernel_size x kernel_size window clipped to
 * the image (column outer, row inner) divided by their count, and valid; it is unchanged without any.  kernel_size is odd and
 * > 0.  out must not be the input. */
int vwgpu_fill_nodata_with_avg_dev(vwgpu_ctx* ctx, const float* d_img, int w, int h, ptrdiff_t istride, int kernel_size, float* d_out,
                                   ptrdiff_t ostride);
int vwgpu_fill_nodata_with_avg(vwgpu_ctx* ctx, const float* img, int w, int h, ptrdiff_t istride, int kernel_size, float* out,
                               ptrdiff_t ostride);

/* ---- Mosaic/ImageComposite.h: multi-band blending of positioned images ---------- */
/* (tests/refimpl/mosaic_ref.cc.)  vw::mosaic::ImageComposite<PixelT> for float pixels with premultiplied
 * alpha, interleaved, alpha last: channels = 2 is PixelGrayA<float>, 4 is PixelRGBA<float>; draft mode also takes channels = 1
 * (no alpha: a later image overwrites).  Finite values only.  Every image lives on the device: insert copies it, so the caller's
 * buffer is free when the call returns (_dev: once the work queued on the context's stream has run).  Strides are in pixels,
 * 0 = packed.  Boxes are {min.x, min.y, max.x, max.y}, max exclusive.  A composite belongs to the device of the context that
 * created it, takes a context of that device in every call, and is destroyed before that device's last context.
 *
 * Not here: the reference's cache and its mask.N.png files (the masks stay on the device as exactly 0.0f and 1.0f),
 * set_reuse_masks, sparse_check, integer pixels.  blend_patch adds the images in insertion order, which is the reference's order
 * with a cold cache.
 *
 * Limits: at most VWGPU_COMPOSITE_MAX_IMAGES images, image sides up to VWGPU_COMPOSITE_MAX_DIM, view sides up to twice that,
 * VWGPU_COMPOSITE_MAX_BYTES device bytes per composite (sources, pyramids and scratch): VWGPU_ERR_NOIMPL above.
 * VWGPU_ERR_ARGUMENT before any device work: null pointers, an empty image, a stride below the width, channels other than 1, 2, 4
 * or other than the first image's, insert after prepare, prepare twice or without an image, a total box that does not contain
 * every image (the reference's / 2 and % 2 would act on negative numbers), generate_patch before prepare or with a patch that
 * leaves the view, blending 1-channel images, blending after a prepare() in draft mode (it made no masks). */
#define VWGPU_COMPOSITE_MAX_IMAGES 64
#define VWGPU_COMPOSITE_MAX_DIM 65536
#define VWGPU_COMPOSITE_MAX_BYTES (1ull << 34)
typedef struct vwgpu_composite vwgpu_composite;
/* ImageComposite() (:246-247) and its destructor. */
int vwgpu_composite_create(vwgpu_ctx* ctx, vwgpu_composite** out);
void vwgpu_composite_destroy(vwgpu_composite* c);
/* insert(image, x, y) (:411-431): the view and data boxes grow, mindim shrinks. */
int vwgpu_composite_insert_dev(vwgpu_ctx* ctx, vwgpu_composite* c, const float* d_img, int w, int h, ptrdiff_t stride, int channels, int x, int y);
int vwgpu_composite_insert(vwgpu_ctx* ctx, vwgpu_composite* c, const float* img, int w, int h, ptrdiff_t stride, int channels, int x, int y);
/* set_draft_mode / set_fill_holes (:261-263).  fill_holes may change after prepare: the next patch builds the pyramids again. */
int vwgpu_composite_set_draft_mode(vwgpu_ctx* ctx, vwgpu_composite* c, int draft_mode);
int vwgpu_composite_set_fill_holes(vwgpu_ctx* ctx, vwgpu_composite* c, int fill_holes);
/* prepare() / prepare(total_bbox) (:434-455): total_bbox is a HOST box or NULL.  The boxes move to the view's origin,
 * levels = max(1, (int)floorf(logf(mindim / 2.0f) / logf(2.0f)) - 1); outside draft mode generate_masks (:331-369) runs, on the
 * float grassfire of every alpha plane, and so does PyramidGenerator::generate (:373-408) for every image, which the reference
 * defers to the first patch. */
int vwgpu_composite_prepare(vwgpu_ctx* ctx, vwgpu_composite* c, const int* total_bbox);
/* cols(), rows() (:267-268), the level count (0 before prepare), and bbox() (which = 0: the data box, moved by prepare) /
 * source_data_bbox() (which = 1: the view box, which keeps its place) (:271-272). */
int vwgpu_composite_cols(const vwgpu_composite* c);
int vwgpu_composite_rows(const vwgpu_composite* c);
int vwgpu_composite_levels(const vwgpu_composite* c);
int vwgpu_composite_bbox(const vwgpu_composite* c, int which, int* box);
/* The level-0 mask of image `index` (what the reference writes to mask.N.png, :362-365) into HOST floats of the image's size:
 * 1 where the image's grassfire distance is positive and beats every other image's, the later image winning a tie. */
int vwgpu_composite_mask(vwgpu_ctx* ctx, vwgpu_composite* c, int index, float* out, ptrdiff_t ostride);
/* generate_patch(BBox2i(x0, y0, w, h)) (:255-258): blend_patch (:468-567) or, in draft mode, draft_patch (:573-590), into
 * w x h pixels.  operator()(x, y) (:274-279) is the 1 x 1 patch. */
int vwgpu_composite_generate_patch_dev(vwgpu_ctx* ctx, vwgpu_composite* c, int x0, int y0, int w, int h, float* d_out, ptrdiff_t ostride);
int vwgpu_composite_generate_patch(vwgpu_ctx* ctx, vwgpu_composite* c, int x0, int y0, int w, int h, float* out, ptrdiff_t ostride);

/* ---- Image/Statistics.h, ImageThresh.h, Algorithms.h, AutoNormalize.h: image statistics and intensity scaling ---------- */

/* Common to the entries of this block (tests/refimpl/image_stats_ref.cc, csrc/image_stats.hip):
 * images are single-channel float, `mask` is an optional uint8 validity image of the same size (non-zero = valid, NULL =
 * every pixel valid: the PixelMask of the reference); strides are in PIXELS, 0 = packed; the _dev form takes device
 * pointers and works on the context's stream, the other form host pointers.  sample_cols, sample_rows: 0, 0 = every
 * pixel, else the pass visits only the sampling grid of the second otsu_threshold overload (src/vw/Image/ImageThresh.h:
 * 156-166): rows round(i * (rows - 1) / (sample_rows - 1)), columns likewise, computed on the host in double; a pixel that
 * two grid points name counts twice, as it does there.  Null pointers, sizes <= 0, a stride below the width, one sampling
 * count zero and the other not, a sampling count < 2 (the reference divides by n - 1) and the argument ranges named at the
 * entries give VWGPU_ERR_ARGUMENT before any device work.  Integer and multi-channel pixels and alpha weighting are not
 * covered. */

typedef struct vwgpu_image_range { double min, max; long long count, nan_count; } vwgpu_image_range;
/*   VWGPU_MIN_MAX_FIND   find_image_min_max (src/vw/Image/Statistics.h:113-127): min = DBL_MAX, max = -DBL_MAX, then
 *                        `if (val < min) min = val; if (val > max) max = val;` in double over the valid pixels: a NaN never
 *                        enters, and with no valid (non-NaN) pixel the two stay DBL_MAX and -DBL_MAX.
 *   VWGPU_MIN_MAX_ACCUM  min_max_channel_values (:98-108) with MinMaxAccumulator<float> (src/vw/Math/Functors.h:355-372):
 *                        the first valid pixel in raster order sets both, later ones enter through `arg < min`,
 *                        `max < arg`: a NaN is admitted only as that first pixel (both extrema are then NaN for good), the
 *                        rule of vwgpu_get_disparity_range.  No valid pixel: the accumulator throws "no valid samples";
 *                        here min = max = 0, count = 0, and the call returns VWGPU_ERR_ARGUMENT where it hands the result
 *                        to the host.
 * count: the valid pixels visited, nan_count: those of them that are NaN.  The sign of a zero extremum is not pinned. */
typedef enum vwgpu_min_max_mode { VWGPU_MIN_MAX_FIND = 0, VWGPU_MIN_MAX_ACCUM = 1 } vwgpu_min_max_mode;
/* _dev: d_result (device) and host_result are both optional, one of them must be given; only host_result synchronises. */
int vwgpu_image_min_max_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                            int sample_cols, int sample_rows, int mode, vwgpu_image_range* d_result, vwgpu_image_range* host_result);
int vwgpu_image_min_max(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                        int sample_cols, int sample_rows, int mode, vwgpu_image_range* result);

/* moments = {count, sum of x, sum of (double)x * x} in double over the valid pixels: what Accumulator, MeanAccumulator and
 * StdDevAccumulator (src/vw/Math/Functors.h:469-518) hold after sum_of_channel_values, mean_channel_value and
 * stddev_channel_value (src/vw/Image/Statistics.h:129-172); vwgpu_moments_mean / vwgpu_moments_stddev apply their value()
 * formulas.  The reference adds in raster order; here every lane adds its pixels in a fixed order, a workgroup folds its lanes
 * in a fixed order into one row of a slab and a second kernel folds the slab, with no float atomics: two calls on the same
 * pixels return the same bits, whichever form is called and wherever the image lies in memory, and on imagery whose partial
 * sums are exact (integer-valued pixels below 2^53 in sum) they are the reference's bits.  Otherwise sum and sum of squares
 * are within 2 (N - 1) u / (1 - (N - 1) u) * sum |term|, u = 2^-53, of the raster-order sums.
 * _dev: d_result (device double[3]) and host_result (host double[3]) as above. */
int vwgpu_image_moments_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                            int sample_cols, int sample_rows, double* d_result, double* host_result);
int vwgpu_image_moments(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                        int sample_cols, int sample_rows, double* result);
/* MeanAccumulator::value (Functors.h:483-486) and StdDevAccumulator::value (:509-512); count 0 ("no valid samples") or a
 * null pointer: VWGPU_ERR_ARGUMENT.  Host functions, no context. */
int vwgpu_moments_mean(const double* moments, double* mean);
int vwgpu_moments_stddev(const double* moments, double* stddev);

#define VWGPU_HISTOGRAM_MAX_BINS 4096
/* Replaces vw::histogram (src/vw/Image/ImageThresh.h:53-73) over math::Histogram::initialize / add_value with saturate =
 * true (src/vw/Math/Statistics.cc:34-76): max == min becomes min + 1; a valid pixel v goes to bin
 * (int)round(max_bin * ((v - min) / range)) in IEEE double, round half away from zero, max_bin = num_bins - 1, range =
 * max - min; negative bins saturate to 0 and bins >= num_bins to max_bin.
 * counts: uint64[num_bins + 2]: the bins, then counts[num_bins] = the total (get_total_num_values) and
 * counts[num_bins + 1] = nan_count.  The one deliberate deviation: a pixel whose bin argument is NaN (a NaN pixel, or any
 * pixel when min / max are not finite) makes the reference convert NaN to int, which is undefined; here it is counted in
 * nan_count and in no bin, nor in the total.  An argument beyond the int range (also undefined there) saturates by its sign.
 * accumulate != 0 adds into the counts that are already there, so that the tiles or row strips of a larger image give
 * exactly the counts of the whole image; 0 zeroes them first.  bin_width: optional HOST double, range / num_bins
 * (get_bin_width).  num_bins outside [1, VWGPU_HISTOGRAM_MAX_BINS], NaN min / max: VWGPU_ERR_ARGUMENT.
 * The _dev form does not synchronise. */
int vwgpu_image_histogram_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                              int sample_cols, int sample_rows, int num_bins, double min, double max, int accumulate,
                              uint64_t* d_counts, double* bin_width);
int vwgpu_image_histogram(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                          int sample_cols, int sample_rows, int num_bins, double min, double max, int accumulate,
                          uint64_t* counts, double* bin_width);

/* Host functions on counts (the first num_bins words of the above), no context.
 * vwgpu_histogram_percentile: Histogram::get_percentile (src/vw/Math/Statistics.cc:85-104): the first bin at which the
 * running sum of counts[i] / (double)total reaches `percentile`.  percentile outside [0, 1] (or NaN): VWGPU_ERR_ARGUMENT;
 * no bin reaches it ("Illegal histogram encountered", e.g. total == 0): VWGPU_ERR_LOGIC.
 * vwgpu_otsu_from_histogram: what otsu_threshold does after its histogram is built.  overload 1 (ImageThresh.h:97-144): the
 * between-class variance per bin, the indices of its maximum averaged when it is reached more than once, threshold = min +
 * mean_index / (num_bins - 1) * (max - min); overload 2 (:204-238): the mu1 *= q1 recurrence, the FLT_EPSILON skip, the first
 * strict maximum, threshold = (max - min) * (pos / (num_bins - 1)) + min.  min, max are the values the histogram was built
 * with after `if (max == min) max++`.  total == 0 gives 0.0 in both.  Another overload number, num_bins < 1: ARGUMENT. */
int vwgpu_histogram_percentile(const uint64_t* counts, int num_bins, uint64_t total, double percentile, int* bin);
int vwgpu_otsu_from_histogram(const uint64_t* counts, int num_bins, uint64_t total, double min, double max, int overload,
                              double* threshold);
/* otsu_threshold(view) (overload 1: num_bins must be 256 and the sampling counts 0) and otsu_threshold(view,
 * num_sample_rows, num_sample_cols, num_bins) (overload 2; sampling counts 0, 0 = cols, rows, which is every pixel once):
 * vwgpu_image_min_max (FIND), `if (max == min) max++`, vwgpu_image_histogram, vwgpu_otsu_from_histogram.  A NaN pixel is
 * left out (in the reference it would be converted to int).  threshold is a HOST double; both forms synchronise. */
int vwgpu_otsu_threshold_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                             int sample_cols, int sample_rows, int num_bins, int overload, double* threshold);
int vwgpu_otsu_threshold(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                         int sample_cols, int sample_rows, int num_bins, int overload, double* threshold);

/* The k-th smallest valid pixel, exactly, without sorting: a radix select over the order-preserving 32-bit key of a float,
 * three digits (12, 12 and 8 bits) counted by the histogram kernel, the digit choice made on the device.
 *   VWGPU_ORDER_RANK        arg = k, 0-based, clamped to the last valid pixel: sorted[k]
 *   VWGPU_ORDER_MEDIAN      destructive_median (src/vw/Math/Functors.h:393-398), what median_channel_value returns: with len
 *                           valid pixels sorted[len / 2] for odd len, else (sorted[len / 2 - 1] + sorted[len / 2]) / 2.0 —
 *                           the sum of two floats, as written there, divided in double
 *   VWGPU_ORDER_PERCENTILE  destructive_percentile (:424-444), arg = percentile in [0, 100]: sorted[ceil(arg / 100 * len) - 1],
 *                           the index clamped to [0, len - 1]
 * -0.0 and +0.0 compare equal in std::sort: the sign of a zero result is not pinned.  A NaN among the valid pixels
 * (std::sort has no defined result) or no valid pixel ("no valid samples"): the device result is NaN and the call returns
 * VWGPU_ERR_ARGUMENT where it hands the result to the host.  w * h above INT_MAX (the reference's int len), a NaN or
 * negative arg, a percentile above 100: VWGPU_ERR_ARGUMENT.
 * _dev: d_result (device double[1]) and host_result (host double[1]), one of them must be given; only host_result
 * synchronises. */
typedef enum vwgpu_order_kind { VWGPU_ORDER_RANK = 0, VWGPU_ORDER_MEDIAN = 1, VWGPU_ORDER_PERCENTILE = 2 } vwgpu_order_kind;
int vwgpu_image_order_statistic_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask,
                                    ptrdiff_t mstride, int kind, double arg, double* d_result, double* host_result);
int vwgpu_image_order_statistic(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                                int kind, double arg, double* result);

/* The per-pixel pass of src/vw/Image/Algorithms.h, params a HOST double array:
 *   VWGPU_RESCALE_CLAMP            clamp(image, low, high) (:30-61), params {low, high}: v > high ? high : v < low ? low : v
 *   VWGPU_RESCALE_NORMALIZE        normalize(image, old_low, old_high, new_low, new_high) (:105-126, :171-188), params in that
 *                                  order: (float)((v - old_low) * ratio + new_low), v - old_low in float, ratio the double
 *                                  (new_high - new_low) / (double)(old_high - old_low) with both differences in float, 0 when
 *                                  old_high == old_low
 *   VWGPU_RESCALE_CLAMP_NORMALIZE  normalize(clamp(image, low, high), old_low, ...) in one pass, params {low, high, old_low,
 *                                  old_high, new_low, new_high}
 *   VWGPU_RESCALE_THRESHOLD        threshold(image, thresh, low, high) (:192-208), params {thresh, low, high}: v > thresh ?
 *                                  high : low
 * Every parameter is cast to float first (the functors hold channel_type), nothing is contracted.  out_type (what `out`
 * holds): VWGPU_PIXEL_F32 the float result; VWGPU_PIXEL_U8 pixel_cast<uint8> of it, the C truncation; VWGPU_PIXEL_U8_AS_F32
 * that uint8 value as a float (integer-valued imagery for vwgpu_calc_disparity).  Where the C conversion is undefined this
 * one is defined: a NaN becomes 0, values below 0 become 0 and values of 256 and above 255.  in == out is allowed for the two
 * float outputs.  There is no mask operand: UnaryCompoundFunctor applies the functor to the value of an invalid PixelMask
 * pixel too and only carries the validity over (src/vw/Image/PixelMask.h:514-523), so the caller's mask stays as it is.
 * A NaN parameter, an unknown mode or out_type: VWGPU_ERR_ARGUMENT. */
typedef enum vwgpu_rescale_mode {
  VWGPU_RESCALE_CLAMP = 0, VWGPU_RESCALE_NORMALIZE = 1, VWGPU_RESCALE_CLAMP_NORMALIZE = 2, VWGPU_RESCALE_THRESHOLD = 3
} vwgpu_rescale_mode;
typedef enum vwgpu_rescale_pixel { VWGPU_PIXEL_F32 = 0, VWGPU_PIXEL_U8 = 1, VWGPU_PIXEL_U8_AS_F32 = 2 } vwgpu_rescale_pixel;
int vwgpu_image_rescale_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, int mode, const double* params,
                            int out_type, void* d_out, ptrdiff_t ostride);
int vwgpu_image_rescale(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, int mode, const double* params,
                        int out_type, void* out, ptrdiff_t ostride);

/* percentile_scale_convert (src/vw/Image/ImageThresh.h:243-270): find_image_min_max, histogram(num_bins), low_bin / high_bin
 * = get_percentile(low / high percentile), low_value = (low_bin + 1) * bin_width + min and high_value likewise, then
 * pixel_cast<uint8>(normalize(clamp(image, low_value, high_value), low_value, high_value, 0.0, 255.0)).
 * u8_convert (:274-286): min, max, `if (max == min) max = min + 1`, the same stretch between them.
 * auto_normalize: normalize(image, low, high) of src/vw/Image/AutoNormalize.h:33-49: min_max_channel_values, then
 * normalize(image, old_min, old_max, low, high) into floats (normalize(image) is low = 0, high = 1).
 * The mask serves the statistics only; every pixel of the image is converted.  The _dev forms make NO host
 * synchronisation: a one-workgroup kernel computes the percentile bins and the stretch on the device, in the double
 * arithmetic of vwgpu_histogram_percentile, and hands them to the convert pass through device memory.  host_params:
 * optional HOST double[4] {min, max, low_value, high_value} ({old_min, old_max, low, high} for auto_normalize); asking
 * for it synchronises.  With no valid pixel, or no bin reaching a percentile, the reference throws: here every output
 * pixel is new_low (0), and the call returns VWGPU_ERR_ARGUMENT where host_params is asked for or the form is the host one.
 * Percentiles outside [0, 1], num_bins outside [1, VWGPU_HISTOGRAM_MAX_BINS], a NaN low / high: VWGPU_ERR_ARGUMENT. */
int vwgpu_percentile_scale_convert_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask,
                                       ptrdiff_t mstride, double low_percentile, double high_percentile, int num_bins, int out_type,
                                       void* d_out, ptrdiff_t ostride, double* host_params);
int vwgpu_percentile_scale_convert(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask,
                                   ptrdiff_t mstride, double low_percentile, double high_percentile, int num_bins, int out_type,
                                   void* out, ptrdiff_t ostride, double* host_params);
int vwgpu_u8_convert_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                         int out_type, void* d_out, ptrdiff_t ostride, double* host_params);
int vwgpu_u8_convert(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                     int out_type, void* out, ptrdiff_t ostride, double* host_params);
int vwgpu_auto_normalize_dev(vwgpu_ctx* ctx, const float* d_in, int w, int h, ptrdiff_t istride, const uint8_t* d_mask, ptrdiff_t mstride,
                             double low, double high, float* d_out, ptrdiff_t ostride, double* host_params);
int vwgpu_auto_normalize(vwgpu_ctx* ctx, const float* in, int w, int h, ptrdiff_t istride, const uint8_t* mask, ptrdiff_t mstride,
                         double low, double high, float* out, ptrdiff_t ostride, double* host_params);

/* ---- Stereo/StereoModel.{h,cc} and Stereo/StereoView.h: triangulation and the universe radius ---------- */

/* The part of vw::camera that triangulation needs (tests/refimpl/triangulate_ref.cc): a flat
 * descriptor, passed to the kernels by value.
 *   VWGPU_CAMERA_PINHOLE  PinholeModel::pixel_to_vector / camera_center (src/vw/Camera/PinholeModel.cc:422-434):
 *                         normalize(inv_camera_transform * (undistort(pix * pixel_pitch), 1)) from `center`.
 *                         inv_camera_transform is the reference's m_inv_camera_transform, row-major.
 *     VWGPU_DISTORTION_NULL  the identity.
 *     VWGPU_DISTORTION_TSAI  TsaiLensDistortion::undistorted_coordinates (src/vw/Camera/LensDistortion.cc:371-400) with
 *                            distortion = {k1, k2, p1, p2, k3}: TsaiDistortionNorm (:260-276), the analytic Jacobian
 *                            (:286-324) and NewtonRaphson::solve (src/vw/Math/NewtonRaphson.cc:58-119) with its start
 *                            point, its 19 passes, its best-so-far fallbacks and its 1e-9 stop on the step; fu or fv
 *                            below 1e-300 gives HUGE_VAL.
 *   VWGPU_CAMERA_CAHV     CAHVModel::pixel_to_vector / camera_center (src/vw/Camera/CAHVModel.cc:173-189):
 *                         normalize(cross(V - y A, H - x A)), times -1.0 when dot(cross(V, H), A) < 0, from C = `center`.
 *   VWGPU_CAMERA_CAHVOR   CAHVORModel::pixel_to_vector and point_to_pixel without partials (src/vw/Camera/CAHVORModel.cc:297-348,
 *                         :431-448): radial distortion about the axis O with the coefficients R.  The Newton loop on
 *                         k5 u^5 + k3 u^3 + k1 u = 1 keeps its exits (20 passes, deriv <= 0, |du| < 1e-6 after the step); none
 *                         of them is a failure.  Only + - * / sqrt fabs: the reference's bits.
 *   VWGPU_CAMERA_CAHVORE  CAHVOREModel::pixel_to_vector and point_to_pixel (src/vw/Camera/CAHVOREModel.cc:167-301): fisheye
 *                         with the linearity P (1 perspective, 0 fisheye) and the moving entrance pupil E.  Where the
 *                         reference throws ("Did not converge." after 101 Newton steps, "Theta out of bounds.") the pixel
 *                         counts as failed, as below.  sin, cos, tan, atan, atan2 and asin are the device library's.
 * The kinds 3 and 4 follow 1: the value 2 was refused with VWGPU_ERR_ARGUMENT before they existed, callers and tests rely on
 * that, and it stays unassigned and refused.
 * The descriptor keeps its 256 bytes.  For a CAHVOR or CAHVORE camera center, A, H, V mean what they mean for CAHV, and
 * O, R, E and P live in storage only a pinhole uses:
 *   inv_camera_transform[0..2] = O, [3..5] = R, [6..8] = E (CAHVORE);  distortion[0] = P (CAHVORE).
 * Callers do not write these by hand: vwgpu_cahvor_camera and vwgpu_cahvore_camera fill a descriptor.
 * Which pairs have a kernel — the rule: pinholes (with any lens) and CAHV cameras go with one another in every entry point;
 * a CAHVOR or CAHVORE camera goes with a CAHV camera alone in vwgpu_camera_transform*, in either role, and with a camera
 * of its own kind alone in triangulation and the convergence angle.  Every other pair is VWGPU_ERR_NOIMPL with a message
 * that names the pair, before any device work.  (The engine keeps one table of instantiated pairs per entry-point family,
 * and a pair without a row is refused.) */
typedef enum vwgpu_camera_kind {
  VWGPU_CAMERA_PINHOLE = 0, VWGPU_CAMERA_CAHV = 1, VWGPU_CAMERA_CAHVOR = 3, VWGPU_CAMERA_CAHVORE = 4
} vwgpu_camera_kind;
/* The lenses of a pinhole beyond null and Tsai (src/vw/Camera/LensDistortion.cc).  The 14 doubles
 * from distortion[0] to V[2] are contiguous, a pinhole uses none of A, H, V, and they hold the lens words L[0..13], which
 * only vwgpu_camera_set_lens fills:
 *   VWGPU_DISTORTION_FOV              FovLensDistortion (:462-515), both directions closed form.  L0 = k1, L1 = 1 / k1,
 *                                     L2 = 2 tan(k1 / 2), the reference's two precomputed members.
 *   VWGPU_DISTORTION_FISHEYE          FisheyeLensDistortion (:573-658).  L0..3 = k1..k4.  undistorted_coordinates is
 *                                     NewtonRaphson::solve with the numerical Jacobian (src/vw/Math/NewtonRaphson.cc:27-47,
 *                                     step 1e-6, tol 1e-9), with every exit of the solver.
 *   VWGPU_DISTORTION_BROWN_CONRADY    BrownConradyDistortion (:731-744).  L0..7 = xp, yp, k1, k2, k3, p1, p2, phi, L8 =
 *                                     sin(phi), L9 = cos(phi).  distorted_coordinates is the base class's (:175-195):
 *                                     levenberg_marquardtFixed (src/vw/Math/LevenbergMarquardt.h:389-561) for the 2 x 2
 *                                     case with tolerances 1e-16 and 100 passes, then the 1e-10 test whose failure is the
 *                                     reference's throw "LensDistortion: Did not converge.".
 *   VWGPU_DISTORTION_ADJUSTABLE_TSAI  AdjustableTsaiLensDistortion (:799-880).  L0..n-1 = the n coefficients (n - 3
 *                                     radial, two tangential, alpha), L13 = n, 4 <= n <= 13.  The same Newton solver.
 *   VWGPU_DISTORTION_PHOTOMETRIX      PhotometrixLensDistortion (:961-999).  L0..8 = xp, yp, k1, k2, k3, p1, p2, b1, b2
 *                                     (b1, b2 unused, as in the reference).  The same Levenberg-Marquardt solver.
 * fu or fv below 1e-300 gives HUGE_VAL for FOV, fisheye and adjustable Tsai.  FOV and fisheye call the device library's
 * atan and tan; the other three use + - * / sqrt fabs alone.  Every entry that takes a camera accepts these kinds on a
 * pinhole, in any combination on the two cameras.  A pixel whose projection fails the 1e-10 test counts as failed like a
 * pixel that fails the pinhole's round-trip check, whether that check is on or off.
 * The value 5 is unassigned and refused with VWGPU_ERR_ARGUMENT: callers and tests rely on it as a kind out of range.
 * RPCLensDistortion has no kind: its coefficients do not fit the descriptor. */
typedef enum vwgpu_distortion_kind {
  VWGPU_DISTORTION_NULL = 0, VWGPU_DISTORTION_TSAI = 1, VWGPU_DISTORTION_FOV = 2, VWGPU_DISTORTION_FISHEYE = 3,
  VWGPU_DISTORTION_BROWN_CONRADY = 4, VWGPU_DISTORTION_ADJUSTABLE_TSAI = 6, VWGPU_DISTORTION_PHOTOMETRIX = 7
} vwgpu_distortion_kind;
typedef struct vwgpu_camera {
  int kind;                          /* vwgpu_camera_kind */
  int distortion_kind;               /* vwgpu_distortion_kind (pinhole) */
  double center[3];                  /* camera centre (pinhole), C (CAHV, CAHVOR, CAHVORE) */
  double inv_camera_transform[9];    /* pinhole; O, R, E of CAHVOR / CAHVORE */
  double pixel_pitch, fu, fv, cu, cv;
  double distortion[5];              /* pinhole; [0] = P of CAHVORE */
  double A[3], H[3], V[3];           /* CAHV, CAHVOR, CAHVORE */
} vwgpu_camera;

/* Fills a pinhole descriptor the way PinholeModel::rebuild_camera_matrix does (src/vw/Camera/PinholeModel.cc:553-605):
 * inv_camera_transform = inverse(uvwRotation * transpose(rotation)) * inverse(K), with the rows of uvwRotation u_dir,
 * v_dir, w_dir and K = [fu 0 cu; 0 fv cv; 0 0 1]; both inverses are plain 3 x 3 adjugates, the bits of the reference's
 * inverse() are not pinned.  center, u_dir, v_dir, w_dir: double[3]; rotation: row-major double[9]; distortion:
 * double[5] {k1, k2, p1, p2, k3} or NULL with VWGPU_DISTORTION_NULL.  u, v, w that are not orthonormal under the
 * reference's own asserts (:586-591: the three dot products == 0, every norm within 0.001 of 1), a null pointer or an
 * unknown distortion kind: VWGPU_ERR_ARGUMENT.  Pure host arithmetic, no context. */
int vwgpu_pinhole_camera(const double* center, const double* rotation, double fu, double fv, double cu, double cv,
                         const double* u_dir, const double* v_dir, const double* w_dir, double pixel_pitch, int distortion_kind,
                         const double* distortion, vwgpu_camera* out);

/* Sets the lens of a pinhole descriptor that vwgpu_pinhole_camera built: the distortion kind and the lens words.  params
 * holds n doubles in the order of the reference's distortion_parameters(): none for NULL, {k1, k2, p1, p2, k3} for TSAI
 * (n = 5, or 4 with k3 = 0), {k1} for FOV, {k1..k4} for FISHEYE, {xp, yp, k1, k2, k3, p1, p2, phi} for BROWN_CONRADY, 4 to
 * 13 coefficients for ADJUSTABLE_TSAI, {xp, yp, k1, k2, k3, p1, p2, b1, b2} for PHOTOMETRIX.  The words the kind does not use
 * become 0.  A camera that is no pinhole, a null pointer, kind 5 or an unknown kind, a wrong n, FOV with k1 <= 0 (the
 * reference's IOErr) or a parameter that is not finite: VWGPU_ERR_ARGUMENT, the descriptor unchanged.  Pure host
 * arithmetic, no context. */
int vwgpu_camera_set_lens(vwgpu_camera* cam, int distortion_kind, const double* params, int n);

/* distorted_coordinates (direction 0) or undistorted_coordinates (direction 1) of the lens of a pinhole descriptor for n
 * points {x, y} in focal-plane units (pixel * pixel_pitch), on the host, through the functions the kernels run.  A point
 * whose Brown-Conrady or Photometrix solve fails the reference's 1e-10 test becomes a NaN pair and is counted in *failed
 * (optional); the call then returns VWGPU_ERR_LOGIC.  out may be points.  A camera that is no pinhole, an unknown lens kind
 * or direction, a null pointer or n < 0: VWGPU_ERR_ARGUMENT.  Pure host arithmetic, no context. */
int vwgpu_lens_coordinates(const vwgpu_camera* cam, int direction, const double* points, long long n, double* out, long long* failed);

/* CAHVORModel(C, A, H, V, O, R) and CAHVOREModel(C, A, H, V, O, R, E, T, P) (src/vw/Camera/CAHVOREModel.cc:111-124) into a
 * descriptor; every vector is double[3].  type (T) 1 sets P = 1, 2 sets P = 0, 3 takes P in [0, 1]; any other type or P:
 * VWGPU_ERR_ARGUMENT, as a null pointer.  Pure host arithmetic, no context. */
int vwgpu_cahvor_camera(const double* C, const double* A, const double* H, const double* V, const double* O, const double* R,
                        vwgpu_camera* out);
int vwgpu_cahvore_camera(const double* C, const double* A, const double* H, const double* V, const double* O, const double* R,
                         const double* E, int type, double P, vwgpu_camera* out);

/* linearize_camera(CAHVORModel | CAHVOREModel, input size, output size) (src/vw/Camera/CAHVORModel.cc:460-547,
 * src/vw/Camera/CAHVOREModel.cc:303-381): the CAHV camera with the same centre that sees the common field of view of the
 * six landmarks on each pair of edges of an in_w x in_h frame, for an out_w x out_h image.  Reproduced as it is, with the
 * reference's integer and real midpoints (an even and an odd width differ by more than the half pixel).  It runs the
 * model functions of the kernels on the host.  src of another kind, a size <= 0, a null pointer: VWGPU_ERR_ARGUMENT; a
 * CAHVORE landmark ray that does not converge: VWGPU_ERR_LOGIC.  dst may be src.  Pure host arithmetic, no context. */
int vwgpu_linearize_camera(const vwgpu_camera* src, int in_w, int in_h, int out_w, int out_h, vwgpu_camera* dst);

/* How the right pixel of a pair is formed (the two entry points of the reference differ, and the difference is kept):
 *   VWGPU_TRIANGULATE_VIEW   StereoView::operator() (src/vw/Stereo/StereoView.h:91-99): Vector2(i, j) + Vector2((double)dx,
 *                            (double)dy), a double add.
 *   VWGPU_TRIANGULATE_MODEL  StereoModel::operator()(disparity_map, error) (src/vw/Stereo/StereoModel.cc:276-281): x + dx
 *                            with x an int32 and dx a float, added in float and then widened (int32 pixels: added in
 *                            int32).  In this overload a point whose error is not >= 0 (a NaN) becomes zero (:283-293).
 * OR one vwgpu_disparity_layout into `semantics` for the other pixel forms DispHelper accepts (StereoView.h:37-53); the
 * channel type stays `type` and the disparity stride stays in pixels of that layout:
 *   VWGPU_DISPARITY_LAYOUT_DXDYV  {dx, dy, valid}, PixelMask<Vector2> (default)
 *   VWGPU_DISPARITY_LAYOUT_DXDY   {dx, dy}, every pixel valid
 *   VWGPU_DISPARITY_LAYOUT_DV     {dx, valid}, dy = 0 (a masked scalar)
 *   VWGPU_DISPARITY_LAYOUT_D      {dx}, dy = 0, every pixel valid */
typedef enum vwgpu_triangulate_semantics { VWGPU_TRIANGULATE_VIEW = 0, VWGPU_TRIANGULATE_MODEL = 1 } vwgpu_triangulate_semantics;
typedef enum vwgpu_disparity_layout {
  VWGPU_DISPARITY_LAYOUT_DXDYV = 0, VWGPU_DISPARITY_LAYOUT_DXDY = 0x100, VWGPU_DISPARITY_LAYOUT_DV = 0x200,
  VWGPU_DISPARITY_LAYOUT_D = 0x300
} vwgpu_disparity_layout;

/* The quantities StereoModel::operator()(disparity_map, error) reports (StereoModel.cc:258-307) over the valid pixels whose
 * error is >= 0 (every pixel but a NaN error; nearly parallel rays count with error 0).  max_error is exact; sum_error is
 * summed lane by lane, wavefront by wavefront and workgroup by workgroup in a fixed order without floating-point atomics:
 * two calls return the same bits, the reference's raster-order sum may differ in the last places. */
typedef struct vwgpu_triangulate_stats {
  long long point_count;
  double max_error, sum_error;
} vwgpu_triangulate_stats;

/* Replaces rasterising vw::stereo::stereo_triangulate(d, cam1, cam2) (StereoView, src/vw/Stereo/StereoView.h:56-130) and
 * StereoModel::operator()(disparity_map, error) (src/vw/Stereo/StereoModel.cc:254-309) for two cameras.  disp is w x h
 * pixels of `type` (a vwgpu_disparity_type) in the layout named in `semantics`; x0, y0 are the image coordinates of pixel
 * (0, 0) of the buffer, so a tile or row strip equals that region of the whole-map call.  Per valid pixel, with pix1 =
 * (x0 + x, y0 + y) and pix2 by `semantics`, StereoModel::operator()(pixVec, errorVec) (:97-147): a pixel that is NaN or
 * equals CameraModel::invalid_pixel() = (-1e8, -1e8) gives no ray, and with fewer than two rays the point and the error
 * vector are zero; rays with !(1 - dot(d0, d1) >= tol) (tol = 1e-4, or angle_tol when angle_tol > 0) give a zero point;
 * otherwise triangulate_pair (:35-48) in its expression order, reflected (-p + 2 ctr0) when the point lies behind either
 * camera.  error = norm_2(errvec).  An invalid disparity pixel gives a zero point, error and error vector.
 *   xyz     w x h x 3 double (stride in pixels); error (optional) w x h double; errvec (optional) w x h x 3 double.
 *   stats   optional vwgpu_triangulate_stats: a DEVICE pointer for _dev (no synchronisation), a host pointer otherwise.
 * A CAHVORE ray that does not converge gives the zero point and error vector (the catch of PixelToRayErr, :144-146).
 * Null disp / xyz / cameras, w or h <= 0, a stride below the width, type, camera kind, distortion kind, semantics or layout
 * out of range, NaN angle_tol: VWGPU_ERR_ARGUMENT before any device work; a CAHVOR or CAHVORE camera beside a camera of
 * another kind: VWGPU_ERR_NOIMPL.  Outputs must not alias each other. */
int vwgpu_stereo_triangulate_dev(vwgpu_ctx* ctx, int type, const void* d_disp, int w, int h, ptrdiff_t dstride, int x0, int y0,
                                 const vwgpu_camera* cam1, const vwgpu_camera* cam2, double angle_tol, int semantics, double* d_xyz,
                                 ptrdiff_t xstride, double* d_error, ptrdiff_t estride, double* d_errvec, ptrdiff_t vstride,
                                 vwgpu_triangulate_stats* d_stats);
int vwgpu_stereo_triangulate(vwgpu_ctx* ctx, int type, const void* disp, int w, int h, ptrdiff_t dstride, int x0, int y0,
                             const vwgpu_camera* cam1, const vwgpu_camera* cam2, double angle_tol, int semantics, double* xyz,
                             ptrdiff_t xstride, double* error, ptrdiff_t estride, double* errvec, ptrdiff_t vstride,
                             vwgpu_triangulate_stats* stats);

/* Replaces StereoModel::convergence_angle (src/vw/Stereo/StereoModel.cc:174-177) over a disparity map: out is w x h double,
 * acos(dot(cam1.pixel_to_vector(pix1), cam2.pixel_to_vector(pix2))) with the pixel pair formed as above (no pixel is
 * skipped: a NaN pixel gives a NaN angle); invalid disparity pixels give 0.  The dot product is the reference's bits, acos
 * is the device library's.  A CAHVORE ray that does not converge (the reference throws) gives a NaN angle. */
int vwgpu_convergence_angle_dev(vwgpu_ctx* ctx, int type, const void* d_disp, int w, int h, ptrdiff_t dstride, int x0, int y0,
                                const vwgpu_camera* cam1, const vwgpu_camera* cam2, int semantics, double* d_out, ptrdiff_t ostride);
int vwgpu_convergence_angle(vwgpu_ctx* ctx, int type, const void* disp, int w, int h, ptrdiff_t dstride, int x0, int y0,
                            const vwgpu_camera* cam1, const vwgpu_camera* cam2, int semantics, double* out, ptrdiff_t ostride);

/* Replaces per_pixel_filter(points, UniverseRadiusFunc(origin, near, far)) (src/vw/Stereo/StereoView.h:139-222) on a point
 * image of `channels` = 3, 4 or 6 doubles per pixel (xyz; xyz + error; xyz + error vector; strides in pixels): a pixel
 * whose first three channels are all zero becomes all zero; otherwise, with dist = norm_2(xyz - origin), the whole pixel
 * becomes zero when (near_radius != 0 && dist < near_radius) || (far_radius != 0 && dist > far_radius), else it is
 * copied.  counts (optional HOST long long[2], asking for it synchronises the stream) = {total_points (every pixel),
 * rejected_points}.  Negative or NaN radii, near_radius > far_radius (the constructor's asserts), other channel counts:
 * VWGPU_ERR_ARGUMENT.  out == points is allowed. */
int vwgpu_universe_radius_dev(vwgpu_ctx* ctx, const double* d_points, int channels, int w, int h, ptrdiff_t stride,
                              const double* origin, double near_radius, double far_radius, double* d_out, ptrdiff_t ostride,
                              long long* counts);
int vwgpu_universe_radius(vwgpu_ctx* ctx, const double* points, int channels, int w, int h, ptrdiff_t stride, const double* origin,
                          double near_radius, double far_radius, double* out, ptrdiff_t ostride, long long* counts);

/* ---- epipolar rectification (tests/refimpl/epipolar_ref.cc) ---------------------- */

/* The 3 x 4 row-major m_camera_matrix of PinholeModel::rebuild_camera_matrix (src/vw/Camera/PinholeModel.cc:593-603):
 * K * [uvw * R^T | (uvw * (-R^T)) * C], every product a dot_prod whose accumulator starts from zero.  Same arguments and
 * the same checks as vwgpu_pinhole_camera (pixel_pitch and distortion are not used); out receives 12 doubles.  The forward
 * projection needs exactly these bits, and inv_camera_transform of the descriptor cannot give them back, so the matrix
 * travels beside the descriptor.  Pure host arithmetic, no context. */
int vwgpu_pinhole_camera_matrix(const double* center, const double* rotation, double fu, double fv, double cu, double cv,
                                const double* u_dir, const double* v_dir, const double* w_dir, double pixel_pitch, int distortion_kind,
                                const double* distortion, double* out);

/* epipolar(PinholeModel, PinholeModel, ...) (src/vw/Camera/PinholeModel.cc:679-732): from the centres, the camera-to-world
 * rotations (3 x 3 row-major), focal lengths (fu, fv), point offsets (cu, cv) and pixel pitches of two pinholes, the common
 * rotation, focal length, point offset and pitch of the two rectified cameras.  The rotations go through
 * camera_pose().rotation_matrix(), a round trip through a quaternion (src/vw/Math/Quaternion.h:211-340), as in the
 * reference.  The caller builds the output cameras with the null lens, the default u, v, w and the input centres.
 * Null pointers or equal centres (no baseline): VWGPU_ERR_ARGUMENT.  Pure host arithmetic, no context. */
int vwgpu_epipolar_pinhole(const double* center0, const double* rotation0, const double* focal0, const double* offset0, double pitch0,
                           const double* center1, const double* rotation1, const double* focal1, const double* offset1, double pitch1,
                           double* rotation, double* focal, double* offset, double* pitch);

/* epipolar(CAHVModel, CAHVModel, ...) (src/vw/Camera/CAHVModel.cc:297-337).  Anything but two CAHV descriptors, null
 * pointers or equal centres: VWGPU_ERR_ARGUMENT.  Pure host arithmetic, no context. */
int vwgpu_epipolar_cahv(const vwgpu_camera* src0, const vwgpu_camera* src1, vwgpu_camera* dst0, vwgpu_camera* dst1);

/* Replaces rasterising camera_transform(image, src_camera, dst_camera, size, edge, BilinearInterpolation())
 * (src/vw/Camera/CameraTransform.h:43-183) for a float image with an optional validity mask (PixelMask<float>).
 *   src          sw x sh floats; src_mask optional uint8 of the same size (0 = invalid); strides in elements, 0 = packed
 *   src_matrix, dst_matrix   vwgpu_pinhole_camera_matrix of a pinhole camera; NULL for a CAHV, CAHVOR or CAHVORE camera
 *   w, h         output size; x0, y0 the image coordinates of output pixel (0, 0): a tile equals that region of the whole call
 *   edge_value, edge_valid   the ValueEdgeExtension pixel; 0, 0 is ZeroEdgeExtension
 *   check        PinholeModel::set_do_point_to_pixel_check of the source camera (the reference's default is on)
 *   out          w x h floats; out_mask optional uint8 (255 valid, 0 invalid)
 *   failed       optional count of pixels whose projection failed the check: a DEVICE long long for _dev (no
 *                synchronisation), a host long long otherwise
 * Output pixel p = (x0 + x, y0 + y): CameraTransform::reverse, q = src.point_to_pixel(dst.pixel_to_vector(p) + centre) in
 * double in the reference's expression order (the rays of vwgpu_stereo_triangulate; CAHVModel.cc:167-171 or
 * PinholeModel.cc:351-368 with TsaiLensDistortion::distorted_coordinates), then BilinearInterpolationImpl
 * (src/vw/Image/Interpolation.h:76-110) exactly as vwgpu_disparity_warp computes it: the pixel itself at an integer
 * position, otherwise four taps weighted in float, every product and sum rounded on its own; taps outside the source are
 * the edge pixel.  A coordinate that is NaN or beyond +-2^30 gives 0, and in the masked form {0, invalid}.  The masked
 * value is formed from the values whatever their validity, and is valid only if every tap used is valid
 * (src/vw/Image/PixelMask.h:321-345, :424-433).  Where the reference throws PointToPixelErr (the round trip of
 * PinholeModel.cc:378-394, ERROR_THRESHOLD 0.01) the pixel is written as the edge pixel and counted; the host-pointer
 * entry then returns VWGPU_ERR_LOGIC with the reference's message and the count in vwgpu_last_error (the images are
 * complete), the _dev entry only writes the count.  The throws of a CAHVORE camera are treated the same way, a dst ray
 * that does not converge (PixelToRayErr) and a src projection that does not converge or whose theta is out of bounds: the
 * message is "CAHVOREModel: Did not converge." if any pixel did not converge, else "CAHVOREModel: Theta out of bounds.".
 * A CAHVOR or CAHVORE camera goes with a CAHV camera only, in either role: any other pair is VWGPU_ERR_NOIMPL.
 * Cameras whose centres differ: VWGPU_ERR_LOGIC (the reference's assert) before any device work.  Null src / out /
 * cameras, sizes <= 0, a stride below the width, a camera or lens kind out of range, a pinhole without its matrix, out or
 * out_mask aliasing an input or each other, a NaN edge_value with edge_valid: VWGPU_ERR_ARGUMENT before any device work. */
int vwgpu_camera_transform_dev(vwgpu_ctx* ctx, const float* d_src, int sw, int sh, ptrdiff_t sstride, const uint8_t* d_src_mask,
                               ptrdiff_t mstride, const vwgpu_camera* src_camera, const double* src_matrix,
                               const vwgpu_camera* dst_camera, const double* dst_matrix, int w, int h, int x0, int y0, float edge_value,
                               int edge_valid, int check, float* d_out, ptrdiff_t ostride, uint8_t* d_out_mask, ptrdiff_t omstride,
                               long long* d_failed);
int vwgpu_camera_transform(vwgpu_ctx* ctx, const float* src, int sw, int sh, ptrdiff_t sstride, const uint8_t* src_mask, ptrdiff_t mstride,
                           const vwgpu_camera* src_camera, const double* src_matrix, const vwgpu_camera* dst_camera,
                           const double* dst_matrix, int w, int h, int x0, int y0, float edge_value, int edge_valid, int check, float* out,
                           ptrdiff_t ostride, uint8_t* out_mask, ptrdiff_t omstride, long long* failed);

/* CameraTransform::forward / reverse (CameraTransform.h:52-74) of n points (x, y double pairs): forward is
 * dst.point_to_pixel(src.pixel_to_vector(p) + centre), reverse the other way round.  `check` is that of the camera
 * projected into.  A point whose projection fails the check becomes a NaN pair and is counted (failed as above; the
 * host-pointer entry returns VWGPU_ERR_LOGIC).  This is what compute_transformed_bbox_fast needs for
 * resize_epipolar_cameras_to_fit: the Tsai Newton solver exists on the device only.  n <= 0, null pointers, a direction
 * out of range and the camera errors above: VWGPU_ERR_ARGUMENT; unequal centres: VWGPU_ERR_LOGIC.  out == points is allowed. */
typedef enum vwgpu_camera_transform_direction { VWGPU_CAMERA_TRANSFORM_FORWARD = 0, VWGPU_CAMERA_TRANSFORM_REVERSE = 1 } vwgpu_camera_transform_direction;
int vwgpu_camera_transform_points_dev(vwgpu_ctx* ctx, const vwgpu_camera* src_camera, const double* src_matrix,
                                      const vwgpu_camera* dst_camera, const double* dst_matrix, int direction, int check,
                                      const double* d_points, long long n, double* d_out, long long* d_failed);
int vwgpu_camera_transform_points(vwgpu_ctx* ctx, const vwgpu_camera* src_camera, const double* src_matrix,
                                  const vwgpu_camera* dst_camera, const double* dst_matrix, int direction, int check, const double* points,
                                  long long n, double* out, long long* failed);

/* ---- vw::transform: closed-form 2-D maps, interpolations, edge extensions ------------------------------ */

/* The map functors of src/vw/Math/Transform.h:231-443 as plain descriptors, in fp64 and in the reference's expression
 * order, with only + - * /:
 *   IDENTITY    p                                                                     (IdentityTransform, :231-237)
 *   TRANSLATE   forward p + (fwd[0], fwd[1]); reverse p - (rev[0], rev[1])            (TranslateTransform, :281-287)
 *   RESAMPLE    forward p * (fwd[0], fwd[1]); reverse p / (rev[0], rev[1]): a division, no reciprocal
 *                                                                                     (ResampleTransform, :256-262)
 *   AFFINE      forward (fwd[0] x + fwd[1] y + fwd[4], fwd[2] x + fwd[3] y + fwd[5]); reverse px = x - rev[4],
 *               py = y - rev[5], (rev[0] px + rev[1] py, rev[2] px + rev[3] py): fwd holds the matrix, rev its inverse,
 *               both the offset (AffineTransform, :329-339; LinearTransform is the offset 0, RotateTransform the words
 *               of vwgpu_transform_rotate)
 *   HOMOGRAPHY  w = m[6] x + m[7] y + m[8] first, then ((m[0] x + m[1] y + m[2]) / w, (m[3] x + m[4] y + m[5]) / w)
 *               with m = fwd (H, row-major) for forward and m = rev (its inverse) for reverse
 *                                                                                     (HomographyTransform, :377-387)
 * A caller may fill the struct by hand (a homography known by its inverse alone: rev, and fwd unused by images).
 * reserved is 0; vwgpu_transform_invert leaves 1 there, which makes forward and reverse change places
 * (InverseTransform, :394-411).  Words a kind does not name are ignored. */
typedef enum vwgpu_transform_kind {
  VWGPU_TRANSFORM_IDENTITY = 0, VWGPU_TRANSFORM_TRANSLATE = 1, VWGPU_TRANSFORM_RESAMPLE = 2, VWGPU_TRANSFORM_AFFINE = 3,
  VWGPU_TRANSFORM_HOMOGRAPHY = 4
} vwgpu_transform_kind;
/* NearestPixelInterpolation, BilinearInterpolation, BicubicInterpolation (src/vw/Image/Interpolation.h:75-225) */
typedef enum vwgpu_transform_interp {
  VWGPU_TRANSFORM_INTERP_NEAREST = 0, VWGPU_TRANSFORM_INTERP_BILINEAR = 1, VWGPU_TRANSFORM_INTERP_BICUBIC = 2
} vwgpu_transform_interp;
/* Zero, Value, Constant, Periodic, Cylindrical, Reflect and LinearEdgeExtension (src/vw/Image/EdgeExtension.tcc:47-272).
 * An enum of its own: vwgpu_edge keeps its two values. */
typedef enum vwgpu_transform_edge {
  VWGPU_TRANSFORM_EDGE_ZERO = 0, VWGPU_TRANSFORM_EDGE_VALUE = 1, VWGPU_TRANSFORM_EDGE_CONSTANT = 2, VWGPU_TRANSFORM_EDGE_PERIODIC = 3,
  VWGPU_TRANSFORM_EDGE_CYLINDRICAL = 4, VWGPU_TRANSFORM_EDGE_REFLECT = 5, VWGPU_TRANSFORM_EDGE_LINEAR = 6
} vwgpu_transform_edge;
typedef enum vwgpu_transform_direction { VWGPU_TRANSFORM_FORWARD = 0, VWGPU_TRANSFORM_REVERSE = 1 } vwgpu_transform_direction;
typedef struct vwgpu_transform {
  int kind;       /* vwgpu_transform_kind */
  int reserved;   /* 0; 1 after vwgpu_transform_invert */
  double fwd[9];
  double rev[9];
} vwgpu_transform;
/* How vwgpu_transform_image samples: the interpolation and the edge extension of interpolate(v, interp, edge)
 * (src/vw/Image/Interpolation.h:228-310), and the switch of transform_nodata (src/vw/Image/Transform.h:401-437, :606-618). */
typedef struct vwgpu_transform_params {
  int interp;           /* vwgpu_transform_interp */
  int edge;             /* vwgpu_transform_edge */
  float edge_value;     /* the pixel of ValueEdgeExtension (other kinds ignore it) ... */
  int edge_valid;       /* ... and its validity in a masked call */
  int nodata;           /* nonzero: TransformViewNoData */
  float nodata_value;   /* the nodata pixel ... */
  int nodata_valid;     /* ... and its validity in a masked call */
} vwgpu_transform_params;

/* The descriptor of one map (src/vw/Math/Transform.h:231-389).  params, n:  IDENTITY none, 0;  TRANSLATE {tx, ty};
 * RESAMPLE {fx, fy};  AFFINE {a, b, c, d, x, y} (the matrix row-major, then the offset);  HOMOGRAPHY row-major H[9].
 * The inverse matrix is the plain adjugate over the determinant (the bits of the reference's inverse() are not pinned).
 * A determinant that is 0 or not finite, a parameter that is not finite, a resample factor of 0, a wrong n, an unknown
 * kind or a null pointer: VWGPU_ERR_ARGUMENT, out unchanged.  Pure host arithmetic, no context. */
int vwgpu_transform_make(int kind, const double* params, int n, vwgpu_transform* out);
/* RotateTransform(theta, (cx, cy)) (src/vw/Math/Transform.h:351-362): the affine map with the matrix (c, -s, s, c) of
 * cos and sin on the host and the offset translate - rotate * translate.  Pure host arithmetic, no context. */
int vwgpu_transform_rotate(double theta, double cx, double cy, vwgpu_transform* out);
/* InverseTransform (src/vw/Math/Transform.h:394-411): forward and reverse change places.  out may be in. */
int vwgpu_transform_invert(const vwgpu_transform* in, vwgpu_transform* out);
/* forward or reverse of a chain of 1 to 4 maps on count points (x, y double pairs) with the functions the kernel runs.
 * The chain is compose(steps[0], compose(steps[1], ...)) (src/vw/Math/Transform.h:429-443): reverse applies the steps'
 * reverse in array order, forward their forward from the last to the first.  out == points is allowed.  A null pointer,
 * n_steps outside 1..4, a kind or direction out of range, count < 0: VWGPU_ERR_ARGUMENT.  Pure host arithmetic, no context. */
int vwgpu_transform_points(const vwgpu_transform* steps, int n_steps, int direction, const double* points, long long count, double* out);

/* Replaces rasterising transform(image, tx, w, h, edge, interp) and transform_nodata(...) (src/vw/Image/Transform.h:335-387,
 * :401-437, :485-618) for a float image with an optional validity mask (PixelMask<float>), and with them resample, resize,
 * translate and rotate (:624-843).
 *   src          sw x sh floats; src_mask optional uint8 of the same size (0 = invalid); strides in elements, 0 = packed
 *   steps        HOST array of n_steps (1..4) maps, the chain of vwgpu_transform_points
 *   params       HOST vwgpu_transform_params
 *   w, h         output size; x0, y0 the image coordinates of output pixel (0, 0): a tile equals that region of the whole call
 *   out          w x h floats; out_mask uint8 (255 valid, 0 invalid), present exactly when src_mask is
 * Output pixel p = (x0 + x, y0 + y): TransformView::operator() (:362-365), q = reverse(p) in double, then the
 * interpolation of the edge-extended source at q (src/vw/Image/Interpolation.h:75-225):
 *   NEAREST   the pixel at (_round(q.x), _round(q.y)), _round(v) = int32(v - 0.5) for v < 0 and int32(v + 0.5) otherwise
 *             (src/vw/Math/Functions.h:48-51)
 *   BILINEAR  exactly as vwgpu_disparity_warp computes it: the pixel itself at an integer position, otherwise four taps
 *             weighted in float, every product and sum rounded on its own (:83-105)
 *   BICUBIC   the pixel itself at an integer position; otherwise the weights s0..s3, t0..t3 in double from
 *             normx = q.x - floor q.x, four row sums of four double * float products from left to right over the taps
 *             (x-1, y-1) .. (x+2, y+2), t0 row0 + t1 row1 + t2 row2 + t3 row3 in that order, * 0.25, one conversion to
 *             float (:143-184)
 * Taps outside the source come from the edge extension (src/vw/Image/EdgeExtension.tcc:47-272), each kind with the
 * reference's integer index arithmetic, LINEAR with its float extrapolation in the reference's expression order.
 * With a mask the value is formed from the tap values whatever their validity and is valid only if every tap used is
 * (src/vw/Image/PixelMask.h:321-345, :424-433): 1 tap at an integer position and for NEAREST, else 4 or 16; a ZERO tap
 * outside is {0, invalid}, a VALUE tap {edge_value, edge_valid}.
 * params->nodata (TransformViewNoData, :430-437): with b = 1 for NEAREST and BILINEAR and 2 for BICUBIC the output is
 * {nodata_value, nodata_valid} where q.x < b - 1 || q.x >= sw - b || q.y < b - 1 || q.y >= sh - b, compared in double; a
 * NaN passes none of them and is interpolated.
 * A coordinate of q that is NaN or beyond +-2^30 has an undefined int32 conversion in the reference: 0 here, and
 * {0, invalid} with a mask, for every edge kind.
 * VWGPU_ERR_ARGUMENT before any device work: null src / out / steps / params, sizes <= 0, a stride below the width,
 * n_steps outside 1..4, a kind, interp or edge out of range, one mask without the other, out or out_mask aliasing an
 * input or each other, a NaN edge_value (with VALUE) or nodata_value (with nodata) that is marked valid, REFLECT on a
 * source with a side of 1 (a % 0 in the reference) or above 2^30, LINEAR on a side below 2 (it reads outside the
 * image).  LINEAR with a mask is VWGPU_ERR_NOIMPL; every other edge works masked.  No atomics, no counters, and the _dev
 * entry does not synchronise. */
int vwgpu_transform_image_dev(vwgpu_ctx* ctx, const float* d_src, int sw, int sh, ptrdiff_t sstride, const uint8_t* d_src_mask,
                              ptrdiff_t mstride, const vwgpu_transform* steps, int n_steps, const vwgpu_transform_params* params, int w,
                              int h, int x0, int y0, float* d_out, ptrdiff_t ostride, uint8_t* d_out_mask, ptrdiff_t omstride);
int vwgpu_transform_image(vwgpu_ctx* ctx, const float* src, int sw, int sh, ptrdiff_t sstride, const uint8_t* src_mask, ptrdiff_t mstride,
                          const vwgpu_transform* steps, int n_steps, const vwgpu_transform_params* params, int w, int h, int x0, int y0,
                          float* out, ptrdiff_t ostride, uint8_t* out_mask, ptrdiff_t omstride);

/* ---- vw::ip matching and the RANSAC alignment of vw::math ------------------------------------------------ */

typedef enum vwgpu_ip_metric { VWGPU_IP_METRIC_L2 = 0, VWGPU_IP_METRIC_HAMMING = 1 } vwgpu_ip_metric;
typedef enum vwgpu_ip_mode { VWGPU_IP_MODE_SIMPLE = 0, VWGPU_IP_MODE_KNN = 1 } vwgpu_ip_mode;
typedef enum vwgpu_ip_constraint {
  VWGPU_IP_CONSTRAINT_NONE = 0, VWGPU_IP_CONSTRAINT_SCALE_ORIENTATION = 1, VWGPU_IP_CONSTRAINT_POSITION = 2
} vwgpu_ip_constraint;
typedef struct vwgpu_ip_match_params {
  int metric;          /* vwgpu_ip_metric */
  int mode;            /* vwgpu_ip_mode */
  double threshold;    /* m_threshold */
  int constraint;      /* vwgpu_ip_constraint; read in KNN mode only (InterestPointMatcherSimple never calls its constraint) */
  int bidirectional;   /* KNN: the constraint is checked both ways (src/vw/InterestPoint/Matcher.h:262-276) */
  double bounds[4];    /* scale_ratio_min, scale_ratio_max, ori_diff_min, ori_diff_max | min_x, max_x, min_y, max_y */
} vwgpu_ip_match_params;

/* The number of list-2 candidates one workgroup searches for n2 candidates in all; the partial results of the chunks are
 * merged by a second kernel.  Tests place their scenes at its multiples. */
int vwgpu_ip_match_chunk(int n2);

/* Replaces InterestPointMatcherSimple (VWGPU_IP_MODE_SIMPLE, src/vw/InterestPoint/Matcher.h:435-508) and the index-list
 * call of InterestPointMatcher (VWGPU_IP_MODE_KNN, :282-386), the latter with an exact two-nearest search where the
 * reference asks FLANN.
 *   desc1, desc2   n1 x k and n2 x k descriptors: float for L2, uint8 for HAMMING; stride1 / stride2 elements between rows
 *                  (0 = k), so a matrix may be a column slice of a wider one.  k is 1 .. 512.
 *   pol1, pol2     uint8 polarity per point, both or neither; neither means all equal.  SIMPLE skips a candidate whose
 *                  byte differs from the query's; KNN does not read them.
 *   attr1, attr2   float[n][4] = x, y, scale, orientation; needed in KNN mode with a constraint other than NONE
 *   params         HOST vwgpu_ip_match_params
 *   index          int32[n1]: the matched row of list 2, or -1
 *   dist           optional float[n1][2]: the smallest and the second smallest distance, +inf where there is none
 *   stats          optional HOST long long[2] = {matched, queries}; asking for it makes the _dev entry synchronise
 * Distances.  L2 (L2NormMetric, Matcher.cc:34-44): one float accumulator, dist += (a[k] - b[k]) * (a[k] - b[k]) for
 * k = 0 .. K-1 in that order, each operation rounded to float, no contraction.  HAMMING (HammingMetric, :47-102): the bit
 * count of the XOR of the bytes, as a float (exact).
 * SIMPLE: first_pick is the smallest and second_pick the second smallest distance of the multiset over the candidates
 * of equal polarity (a duplicate of the minimum is the second), the index the lowest j that attains the minimum; a
 * missing pick is 1e100; no match when first_pick > threshold * second_pick, in double.  KNN: no polarity test; fewer
 * than two candidates means no match; otherwise the constraint (ScaleOrientationConstraint, PositionConstraint,
 * Matcher.cc:119-147: float quotient and differences compared in double, the orientation difference wrapped by 2 pi
 * once) is checked with the nearest candidate as baseline_ip and the query as test_ip, with `bidirectional` also the
 * other way round, and the match is accepted when (double)dist0 < threshold * (double)dist1.  Ties go to the lowest
 * index.  A distance that is NaN or +inf is never picked, in either mode.
 * Deviation: where the KNN constraint fails the reference pushes nothing, so that its index list comes out short and
 * later entries shift; here the entry of that point is -1.
 * VWGPU_ERR_ARGUMENT before any device work: a null desc1 / desc2 / params / index, n1 / n2 / k < 1, a stride below k,
 * an unknown metric, mode or constraint, a NaN threshold, one polarity list without the other, a constraint in KNN
 * mode without attr1 and attr2, index or dist equal to an input or to each other.  k > 512: VWGPU_ERR_NOIMPL. */
int vwgpu_ip_match_dev(vwgpu_ctx* ctx, const void* d_desc1, int n1, ptrdiff_t stride1, const void* d_desc2, int n2, ptrdiff_t stride2,
                       int k, const uint8_t* d_pol1, const uint8_t* d_pol2, const float* d_attr1, const float* d_attr2,
                       const vwgpu_ip_match_params* params, int32_t* d_index, float* d_dist, long long* stats);
int vwgpu_ip_match(vwgpu_ctx* ctx, const void* desc1, int n1, ptrdiff_t stride1, const void* desc2, int n2, ptrdiff_t stride2, int k,
                   const uint8_t* pol1, const uint8_t* pol2, const float* attr1, const float* attr2,
                   const vwgpu_ip_match_params* params, int32_t* index, float* dist, long long* stats);

/* The entries below run on the host and take no context.  Each clears, and on failure sets, a detail text kept per
 * calling thread: vwgpu_host_last_error() returns it ("" after a success). */
const char* vwgpu_host_last_error(void);

/* remove_duplicates (src/vw/InterestPoint/Matcher.cc:152-195) of n matched pairs: xy1, xy2 float[n][2].  Walking from
 * the last pair to the first, a pair is kept only if neither its list-1 (x, y) nor its list-2 (x, y) was kept before (a
 * skipped pair blocks nothing).  keep: uint8[n], 1 = kept; the kept pairs in input order are the result.  n >= 0. */
int vwgpu_ip_remove_duplicates(const float* xy1, const float* xy2, long long n, uint8_t* keep, long long* n_kept);

typedef enum vwgpu_fit_kind { VWGPU_FIT_SIMILARITY = 0, VWGPU_FIT_AFFINE = 1, VWGPU_FIT_HOMOGRAPHY = 2 } vwgpu_fit_kind;

/* SimilarityFittingFunctor, AffineFittingFunctor, HomographyFittingFunctor (src/vw/Math/Geometry.h:50-351): the row-major
 * 3 x 3 matrix H that takes p1 to p2, both double[n][2]; n >= 3, 3, 4.
 *   SIMILARITY  literally :305-347: the scale is the ratio of the mean distances to the centroids, the rotation
 *               transpose(VT) * transpose(U) of the SVD of the 2 x 2 cross-covariance sum (p1 - m1)(p2 - m2)^T, with no
 *               determinant fix (a reflection comes out as one), the translation m2 - scale * R * m1
 *   AFFINE      the least-squares problem of :222-270 (normal equations on centred points)
 *   HOMOGRAPHY  n == 4: the normalised DLT divided by H(2,2) (:136-147).  n > 4: the minimum of
 *               sum |p2 - proj(H p1)|^2 over the first eight entries with H(2,2) = 1, by damped Gauss-Newton from `seed`
 *               (double[9]), or from the DLT of the first four pairs when seed is null (:149-190)
 * The reference calls LAPACK and its own Levenberg-Marquardt; results agree to rounding and conditioning, not bit for bit.
 * VWGPU_ERR_ARGUMENT: null pointers, too few pairs, an unknown kind, coordinates that are not finite; VWGPU_ERR_LOGIC: a
 * degenerate configuration (all points equal, four points with three in a line). */
int vwgpu_fit_transform(int kind, const double* p1, const double* p2, long long n, const double* seed, double* H);

/* RandomSampleConsensus<FitT, HomogeneousL2NormErrorMetric<2>> (src/vw/Math/RANSAC.h:77-100, :212-330).
 *   samples       int32[iterations][m], m = 3 for SIMILARITY and AFFINE, 4 for HOMOGRAPHY: the rows to fit in every
 *                 iteration.  The reference draws them with an unseeded rand() (:139-155); here the caller does.
 *   inlier_flags  optional uint8[n]: inlier_indices of the returned H;  num_inliers optional: their count
 * Per iteration: fit the sampled rows, take the inliers by error < inlier_threshold, skip with fewer than min_inliers,
 * refit on the inliers with the first fit as seed, take the mean inlier error; the lowest mean wins, the earliest
 * iteration on a tie (the reference's OpenMP order is unspecified).  An iteration whose fit is degenerate is skipped.
 * reduce_if_no_fit: up to ten attempts with min_inliers = int(min_inliers / 1.5), stopping below 2 (:212-243).
 * Deviation: the same table serves every attempt, where the reference draws afresh.
 * VWGPU_ERR_ARGUMENT: null pointers, n < m, iterations < 1, min_inliers < m, a NaN threshold, a row of `samples` with a
 * repeated or out-of-range index.  VWGPU_ERR_LOGIC with the text "RANSAC was unable to find a fit that matched the
 * supplied data." when no attempt finds a model. */
int vwgpu_ransac(int kind, const double* p1, const double* p2, long long n, const int32_t* samples, int iterations,
                 double inlier_threshold, int min_inliers, int reduce_if_no_fit, double* H, uint8_t* inlier_flags,
                 long long* num_inliers);

/* ---- vw::ip detection: IntegralImage, the OBALoG detectors and their orientation --------------------------- */

/* Replaces IntegralImage(source) (src/vw/InterestPoint/IntegralImage.h:43-91): out is (w + 1) x (h + 1) floats with row 0
 * and column 0 zero and out(x + 1, y + 1) = ((src(x, y) + out(x, y + 1)) + out(x + 1, y)) - out(x, y), every operation
 * rounded to float in that order: the reference's words, not those of a prefix sum.  Strides in elements (0 = dense).
 * VWGPU_ERR_ARGUMENT: null pointers, an empty image, a stride below the width, out == src. */
int vwgpu_integral_image_dev(vwgpu_ctx* ctx, const float* d_src, int w, int h, ptrdiff_t sstride, float* d_out, ptrdiff_t ostride);
int vwgpu_integral_image(vwgpu_ctx* ctx, const float* src, int w, int h, ptrdiff_t sstride, float* out, ptrdiff_t ostride);

typedef enum vwgpu_ip_detector { VWGPU_IP_DETECTOR_IAGD = 0, VWGPU_IP_DETECTOR_OBALOG = 1 } vwgpu_ip_detector;
typedef struct vwgpu_ip_detect_params {
  int detector;        /* vwgpu_ip_detector: IntegralAutoGainDetector | IntegralInterestPointDetector */
  int scales;          /* m_scales, 1 .. 8; fewer than 3 give no points */
  double threshold;    /* OBALoGInterestOperator's m_threshold; IAGD constructs its operator with 0 */
  int max_points;      /* m_max_points; <= 0: no limit */
  int reserved;        /* 0 */
} vwgpu_ip_detect_params;
/* The fields of vw::ip::InterestPoint that a detector sets, as arrays (polarity, octave and scale_lvl stay 0). */
typedef struct vwgpu_ip_points {
  float *x, *y;
  int32_t *ix, *iy;
  float *orientation, *scale, *interest;
} vwgpu_ip_points;

/* Replaces IntegralAutoGainDetector::process_image and IntegralInterestPointDetector::process_image
 * (src/vw/InterestPoint/IntegralDetector.cc:150-245, :264-370) on every tile of detect_interest_points
 * (DetectorBase.h:225-236, :267-296): a tile is an independent crop with its own integral image, and its points are
 * shifted by its origin.
 *   tiles            HOST int[n_tiles][4] = x, y, w, h inside the image
 *   params           HOST vwgpu_ip_detect_params
 *   desired_num_ip   optional HOST int[n_tiles]; an entry > 0 overrides max_points for its tile
 *   out              HOST struct of seven arrays of n_tiles x capacity elements (device arrays for _dev): tile i's points
 *                    are the first stats[3 i + 2] elements of its segment, which begins at i * capacity
 *   stats            HOST int[n_tiles][3] = {extrema, points that passed the threshold and Harris, points written}
 * Order: scale ascending, then rows, then columns; where the reference sorts (OBALoG whenever the limit is positive, IAGD
 * when the limit is positive and below the count) by interest descending with ties in that order, then cut at the limit.
 * OBALoG records a point one pixel right and down of its extremum and tests and orients it there, as the reference does.
 * A tile with more points than `capacity`: VWGPU_ERR_CAPACITY; no tile's points are then to be used, and every stats row
 * is valid, so a second call can be sized.  Both entries synchronise the stream (the counts decide the later launches).
 * VWGPU_ERR_ARGUMENT before any device work: null pointers, sizes < 1, a tile that leaves the image, an unknown detector,
 * a NaN threshold.  scales > 8: VWGPU_ERR_NOIMPL (the reference's rows 8 and 9 are placeholders that read outside). */
int vwgpu_ip_detect_dev(vwgpu_ctx* ctx, const float* d_img, int w, int h, ptrdiff_t stride, const int* tiles, int n_tiles,
                        const vwgpu_ip_detect_params* params, const int* desired_num_ip, int capacity, const vwgpu_ip_points* d_out,
                        int* stats);
int vwgpu_ip_detect(vwgpu_ctx* ctx, const float* img, int w, int h, ptrdiff_t stride, const int* tiles, int n_tiles,
                    const vwgpu_ip_detect_params* params, const int* desired_num_ip, int capacity, const vwgpu_ip_points* out, int* stats);

/* Replaces AssignOrientation (IntegralDetector.cc:37-104) for n points {ix, iy, scale} of an integral image of iw x ih
 * floats: 113 Haar responses on the bilinear view of the integral with constant extension, sorted into 13 slices by an
 * atan2f that is the same on the host and the device, the orientation that of the strongest slice. */
int vwgpu_ip_orientation_dev(vwgpu_ctx* ctx, const float* d_integral, int iw, int ih, ptrdiff_t istride, int n, const int32_t* d_ix,
                             const int32_t* d_iy, const float* d_scale, float* d_orientation);
int vwgpu_ip_orientation(vwgpu_ctx* ctx, const float* integral, int iw, int ih, ptrdiff_t istride, int n, const int32_t* ix, const int32_t* iy,
                         const float* scale, float* orientation);

typedef enum vwgpu_ip_descriptor { VWGPU_IP_DESCRIPTOR_SGRAD = 0, VWGPU_IP_DESCRIPTOR_SGRAD2 = 1 } vwgpu_ip_descriptor;

/* Replaces SGradDescriptorGenerator (src/vw/InterestPoint/Descriptor.h:120-132, :214-255, :416-471; 180 floats) and
 * SGrad2DescriptorGenerator (IntegralDescriptor.h:76-179; 128 floats) run on one crop of the image, which is what
 * InterestPointDescriptionTask does per tile (Descriptor.h:259-301).
 *   crop          HOST int[4] = x, y, w, h; it may leave the image and is rasterised with zero extension.  The crop is part
 *                 of the result: SGrad extends the crop with zeros, SGrad2 integrates the crop.
 *   x, y, scale, orientation   n points in IMAGE coordinates; they are re-based to the crop as floats
 *   desc          n rows of 180 or 128 floats, dstride elements apart (0 = dense), so that it feeds vwgpu_ip_match_dev
 * SGRAD: the 42 x 42 support through the affine map of 1 / scale and cos, sin(-orientation) in double and the bilinear tap
 * with zero extension, its own integral image in IntegralImage's order, 5 scales x 3 x 3 cells x 4 quadrant differences, the
 * float sum of squares in order, the reciprocal of its correctly rounded root (0 when that is no normal number).
 * SGRAD2: the integral image of the crop, bilinear with constant extension, 16 boxes x 9 positions x 2 Haar responses
 * rotated in double, each histogram word a double sum rounded to float at every step, two norm_2 normalisations with the
 * clamp at 0.2 between them.  cos and sin are the device library's: with an orientation other than 0 the words agree with a
 * host run to rounding, not bit for bit.
 * VWGPU_ERR_ARGUMENT before any device work: null pointers, n < 0, an empty image or crop, an unknown kind, a stride
 * below the row.  A crop of more than 2^28 pixels: VWGPU_ERR_NOIMPL. */
int vwgpu_ip_describe_dev(vwgpu_ctx* ctx, const float* d_img, int w, int h, ptrdiff_t stride, const int* crop, int n, const float* d_x,
                          const float* d_y, const float* d_scale, const float* d_orientation, int kind, float* d_desc, ptrdiff_t dstride);
int vwgpu_ip_describe(vwgpu_ctx* ctx, const float* img, int w, int h, ptrdiff_t stride, const int* crop, int n, const float* x, const float* y,
                      const float* scale, const float* orientation, int kind, float* desc, ptrdiff_t dstride);

/* The cull of the two detectors on the host, with the comparison the device uses: n candidates in natural order with
 * their interests, the limit (desired_num_ip if positive, else max_points).  order: int32[n], the indices kept, in output
 * order; n_out their count.  No context. */
int vwgpu_ip_cull_order(int detector, int limit, int n, const float* interest, int32_t* order, int* n_out);

/* ---- disparity clean-up filters and the zone scheduler ------------------------------------------------- */

/* Replaces rasterising vw::stereo::rm_outliers_using_thresh (cleanup == 0) or
 * vw::stereo::disparity_cleanup_using_thresh (cleanup != 0: a second pass with the hard-coded (1,1,3.0,0.20))
 * over a whole PixelMask<Vector2i> image (src/vw/Stereo/DisparityMap.h:318-441).  src and dst must not alias;
 * strides are dense (w pixels). */
int vwgpu_disparity_filter_dev(vwgpu_ctx* ctx, const int32_t* d_src, int w, int h, int half_h_kernel, int half_v_kernel,
                               double pixel_threshold, double rejection_threshold, int cleanup, int32_t* d_dst);
int vwgpu_disparity_filter(vwgpu_ctx* ctx, const int32_t* src, int w, int h, int half_h_kernel, int half_v_kernel,
                           double pixel_threshold, double rejection_threshold, int cleanup, int32_t* dst);
/* Replaces rasterising vw::stereo::disparity_mask(disparity, left_mask, right_mask)
 * (src/vw/Stereo/DisparityMap.h:97-253), in place; the left mask has the disparity's size. */
int vwgpu_disparity_mask_dev(vwgpu_ctx* ctx, int32_t* d_disp, int w, int h, const uint8_t* d_left_mask,
                             const uint8_t* d_right_mask, int rmw, int rmh);
int vwgpu_disparity_mask(vwgpu_ctx* ctx, int32_t* disp, int w, int h, const uint8_t* left_mask,
                         const uint8_t* right_mask, int rmw, int rmh);
/* Replaces PyramidCorrelationView::disparity_blob_filter at one level (src/vw/Stereo/CorrelationView.cc:242-271:
 * BlobIndexThreaded over the whole image as one tile + ErodeView): every 8-connected component of VALID pixels with at
 * most max_blob_area pixels is erased (pixels become {0,0,0}); max_blob_area < 1 is a no-op.  In place. */
int vwgpu_disparity_blob_filter_dev(vwgpu_ctx* ctx, int32_t* d_disp, int w, int h, int max_blob_area);
int vwgpu_disparity_blob_filter(vwgpu_ctx* ctx, int32_t* disp, int w, int h, int max_blob_area);
/* Replaces vw::stereo::subdivide_regions(disparity, bounding_box(disparity), list, kernel_size)
 * (src/vw/Stereo/Correlation.cc:139-328).  Host logic on a HOST disparity image; each zone is 8 ints
 * {region.min.x, region.min.y, region.max.x, region.max.y, range.min.x, range.min.y, range.max.x, range.max.y}.
 * Returns the number of zones found (only `cap` are written) or a negative vwgpu_status. */
int vwgpu_subdivide_regions(const int32_t* disp, int w, int h, int kx, int ky, int32_t* zones, int cap);

/* ---- pyramid block matching -------------------------------------------------------------------------- */

/* Arguments of vw::stereo::pyramid_correlate (src/vw/Stereo/CorrelationView.h:195-230) that steer one tile. */
typedef struct vwgpu_pyramid_params {
  int prefilter_mode;            /* vwgpu_prefilter */
  float prefilter_width;
  int search_min_x, search_min_y, search_max_x, search_max_y;   /* BBox2i search_region, half open */
  int kernel_x, kernel_y;
  int cost_type;                 /* vwgpu_cost_type */
  int corr_timeout;              /* seconds; 0 = none.  Uses the reference's estimate seconds_per_op * search volume */
  double seconds_per_op;
  float consistency_threshold;   /* < 0: no L/R check */
  int min_consistency_level;     /* accepted for signature parity; block matching checks at level 0 only */
  int filter_half_kernel;        /* 0: no clean-up filtering */
  int max_pyramid_levels;
  int algorithm;                 /* 0 = VW_CORRELATION_BM, 1 = _SGM, 2 = _MGM (use_mgm at every level), 3 = _FINAL_MGM (at level 0 only; CorrelationView.cc:365-366) */
  int blob_filter_area;          /* 0 = off; level i erases blobs of <= area / 2^i valid pixels */
  /* SGM only (CorrelationView.h:211-214): */
  int sgm_subpixel_mode;         /* vwgpu_sgm_subpixel; the reference's default is LC_BLEND */
  int sgm_search_buffer_x, sgm_search_buffer_y;   /* default (2,2) */
  size_t memory_limit_mb;        /* default 6000 */
  int sgm_num_threads;           /* enters the memory-cap formula only; 0 = 1 */
  /* Optional L-R / R-L discrepancy output of the level-0 consistency check (m_lr_disp_diff, m_region_ul,
   * CorrelationView.h:84; cross_corr_consistency_check, Correlate.cc:1441-1502): PixelMask<float> = {value, valid} per pixel,
   * lr_disp_diff_cols x _rows, covering image pixels starting at (region_ul_x, region_ul_y); stride in pixels (0 = cols).
   * Device pointer for the _dev entry point, host pointer for the host one; NULL = off.  Only kept pixels are written. */
  float* lr_disp_diff;
  int lr_disp_diff_cols, lr_disp_diff_rows;
  ptrdiff_t lr_disp_diff_stride;
  int region_ul_x, region_ul_y;
} vwgpu_pyramid_params;

/* Replaces PyramidCorrelationView::prerasterize(bbox) for VW_CORRELATION_BM (src/vw/Stereo/CorrelationView.cc:273-886):
 * one output tile [bx,bx+bw) x [by,by+bh) of pyramid_correlate(left, right, left_mask, right_mask, ...).
 * Masks may be NULL (everything valid); out is bw x bh x {dx, dy, valid} float (PixelMask<Vector2f>), ostride in pixels. */
int vwgpu_pyramid_correlate_dev(vwgpu_ctx* ctx, const float* d_left, int lw, int lh, ptrdiff_t lstride,
                                const float* d_right, int rw, int rh, ptrdiff_t rstride,
                                const uint8_t* d_left_mask, ptrdiff_t lmstride,
                                const uint8_t* d_right_mask, ptrdiff_t rmstride,
                                const vwgpu_pyramid_params* params, int bx, int by, int bw, int bh,
                                float* d_out, ptrdiff_t ostride);
int vwgpu_pyramid_correlate(vwgpu_ctx* ctx, const float* left, int lw, int lh, ptrdiff_t lstride,
                            const float* right, int rw, int rh, ptrdiff_t rstride,
                            const uint8_t* left_mask, ptrdiff_t lmstride,
                            const uint8_t* right_mask, ptrdiff_t rmstride,
                            const vwgpu_pyramid_params* params, int bx, int by, int bw, int bh,
                            float* out, ptrdiff_t ostride);

/* Several output tiles of the SAME image pair and parameters in one call (round 5) — what the reference's block rasteriser hands to its tile
 * threads one by one (src/vw/Image/ImageIO.h:228-251, BlockProcessor.h:52-176; tools/correlate.cc:266 cuts 1024^2 tiles).  Tile t is
 * [bx[t], bx[t] + bw[t]) x [by[t], by[t] + bh[t]) and goes to outs[t] (bw[t] x bh[t] x 3 floats, row stride ostride[t] pixels; ostride NULL
 * or 0 = dense).  Runs of consecutive tiles of EQUAL size (at most 16) go through the pyramid level loop TOGETHER: every launch serves the
 * whole group and one host round trip per level brings back the zone scheduler's tables of all its tiles (a lone tile is ~50 dependent
 * launches of which the coarse levels are pure latency).  Each tile's result is identical to vwgpu_pyramid_correlate[_dev] on that tile.
 * Grouping applies to VW_CORRELATION_BM without lr_disp_diff, blob filter and corr_timeout; everything else runs tile by tile inside the
 * call.  One context = one group at a time; callers that want more in flight use one context per host thread, as for single tiles. */
int vwgpu_pyramid_correlate_batch_dev(vwgpu_ctx* ctx, const float* d_left, int lw, int lh, ptrdiff_t lstride,
                                      const float* d_right, int rw, int rh, ptrdiff_t rstride,
                                      const uint8_t* d_left_mask, ptrdiff_t lmstride,
                                      const uint8_t* d_right_mask, ptrdiff_t rmstride,
                                      const vwgpu_pyramid_params* params, int n_tiles, const int* bx, const int* by, const int* bw, const int* bh,
                                      float* const* d_outs, const ptrdiff_t* ostride);
int vwgpu_pyramid_correlate_batch(vwgpu_ctx* ctx, const float* left, int lw, int lh, ptrdiff_t lstride,
                                  const float* right, int rw, int rh, ptrdiff_t rstride,
                                  const uint8_t* left_mask, ptrdiff_t lmstride,
                                  const uint8_t* right_mask, ptrdiff_t rmstride,
                                  const vwgpu_pyramid_params* params, int n_tiles, const int* bx, const int* by, const int* bw, const int* bh,
                                  float* const* outs, const ptrdiff_t* ostride);

/* ---- semi-global matching ---------------------------------------------------------------------------- */

typedef enum vwgpu_sgm_subpixel {      /* SemiGlobalMatcher::SgmSubpixelMode, src/vw/Stereo/SGM.h:93-99 */
  VWGPU_SUBPIXEL_NONE = 0, VWGPU_SUBPIXEL_PARABOLA = 1, VWGPU_SUBPIXEL_LINEAR = 2, VWGPU_SUBPIXEL_POLY4 = 3,
  VWGPU_SUBPIXEL_COSINE = 4, VWGPU_SUBPIXEL_LC_BLEND = 5
} vwgpu_sgm_subpixel;

/* The arguments of vw::stereo::calc_disparity_sgm / SemiGlobalMatcher::set_parameters that are not images
 * (src/vw/Stereo/SGM.h:108-147, 360-375). */
typedef struct vwgpu_sgm_params {
  int cost_type;                 /* VWGPU_CENSUS_TRANSFORM or VWGPU_TERNARY_CENSUS_TRANSFORM (others: NOIMPL, like the reference; see allow_block_cost) */
  int use_mgm;                   /* != 0: accum_mgm_multithread (SGM.cc:2619-2700) instead of the eight independent path sweeps */
  int kernel_size;               /* 3, 5, 7 or 9 */
  int subpixel_mode;             /* vwgpu_sgm_subpixel */
  int search_buffer_x, search_buffer_y;
  size_t memory_limit_mb;        /* cap on the cost + accumulation buffers, as in calc_main_buf_size (SGM.cc:677-731) */
  int p1, p2;                    /* 0 = the reference's defaults for the cost type / kernel size */
  int ternary_census_threshold;  /* the reference's default is 5 */
  int num_threads;               /* only enters the memory-cap formula (line buffers per thread); >= 1 */
  int allow_block_cost;          /* 0 (default): costs other than census return VWGPU_ERR_NOIMPL, as compute_disparity_costs throws
                                  * (SGM.cc:1887-1892).  1: VWGPU_ABSOLUTE_DIFFERENCE / VWGPU_SQUARED_DIFFERENCE run the code behind that
                                  * throw — fill_costs_block's mean-abs-difference block cost (:1651-1738, p1 = 3, p2 = 250 by default),
                                  * odd kernel sizes 1 .. 15.  A reference code path that is unreachable upstream: explicit opt-in only. */
} vwgpu_sgm_params;

/* Replaces vw::stereo::calc_disparity_sgm (src/vw/Stereo/SGM.cc:167-229) on already cropped regions:
 *   left  lw x lh float, right rw x rh float with rw >= lw + sx, rh >= lh + sy (the reference crops the right image to
 *   left_region grown by search_volume, :190-191); search_volume (sx, sy) is INCLUSIVE here: (sx+1) x (sy+1) disparities.
 *   left_mask (optional)  : exactly the output size; right_mask (optional): at least output size + (sx, sy);
 *   prev_disparity (optional): half-resolution PixelMask<Vector2i> of the previous pyramid level.
 *   out_disp : ow x oh x {dx, dy, valid} int32 with ow = lw - kernel + 1 (when the right image is large enough);
 *   out_subpixel (optional): the matcher's create_disparity_view_subpixel (SGM.cc:1497-1614) of that result.
 * cap_pixels = capacity of the output buffers in pixels; *ow / *oh receive the output size. */
int vwgpu_calc_disparity_sgm_dev(vwgpu_ctx* ctx, const vwgpu_sgm_params* params,
                                 const float* d_left, int lw, int lh, ptrdiff_t lstride,
                                 const float* d_right, int rw, int rh, ptrdiff_t rstride, int sx, int sy,
                                 const uint8_t* d_left_mask, int lmw, int lmh, const uint8_t* d_right_mask, int rmw, int rmh,
                                 const int32_t* d_prev_disparity, int pw, int ph,
                                 int32_t* d_out_disp, float* d_out_subpixel, size_t cap_pixels, int* ow, int* oh);
int vwgpu_calc_disparity_sgm(vwgpu_ctx* ctx, const vwgpu_sgm_params* params,
                             const float* left, int lw, int lh, ptrdiff_t lstride,
                             const float* right, int rw, int rh, ptrdiff_t rstride, int sx, int sy,
                             const uint8_t* left_mask, int lmw, int lmh, const uint8_t* right_mask, int rmw, int rmh,
                             const int32_t* prev_disparity, int pw, int ph,
                             int32_t* out_disp, float* out_subpixel, size_t cap_pixels, int* ow, int* oh);

/* Host-side view of the launch schedule of the MGM passes (use_mgm; accum_mgm_multithread, src/vw/Stereo/SGM.cc:2619-2700): the
 * raster loops of the eight SmoothPathAccumTask passes (src/vw/Stereo/SGMAssist.h:911-1236) are walked as FRONTS, sets of pixels whose
 * two predecessors lie in the previous front (csrc/mgm_schedule.h).  Direction 0 L, 1 TL, 2 R, 3 BR, 4 T, 5 BL, 6 B, 7 TR.
 * vwgpu_mgm_front_count: number of fronts of a direction on a cols x rows output (< 0: bad arguments).
 * vwgpu_mgm_front_pixel: pixel `index` of front `front`: returns 1 and fills c_r = {c, r}, preds = {c + ax, r + ay, c + bx, r + by}
 *   (path predecessor, second predecessor) and *uses_preds (the task's border test: 0 = the pixel keeps its local costs);
 *   0 when the front has no such pixel, < 0 on bad arguments.  No context, no device work: this is what the launcher enumerates. */
int vwgpu_mgm_front_count(int cols, int rows, int direction);
int vwgpu_mgm_front_pixel(int cols, int rows, int direction, int front, int index, int* c_r, int* preds, int* uses_preds);

/* ---- multi-GPU: halo rows of a row-sharded source (csrc/halo.hip) ---------------------------------------------------------
 * The reference has no distributed mode; its tiles are independent (CorrelationView.cc:89-97, CorrelationView.h:123-133), so one
 * process per GPU can own a strip of tile rows.  When the SOURCE image is sharded the same way, rank g holds rows
 * [g*rows/world, (g+1)*rows/world) and its tiles additionally read `halo_above` / `halo_below` rows of the neighbours
 * (half_kernel * 2^levels + search + collar).  These calls fetch them with RCCL point-to-point transfers (librccl.so is opened
 * at run time; VWGPU_ERR_NOIMPL when it is absent).  The unique id is produced on one rank and handed to the others by the host
 * application (file, MPI, torch store ...), exactly as ncclGetUniqueId / ncclCommInitRank expect. */
typedef struct vwgpu_comm vwgpu_comm;
#define VWGPU_COMM_ID_BYTES 128
int vwgpu_comm_unique_id(void* id128);
int vwgpu_comm_create(vwgpu_ctx* ctx, const void* id128, int rank, int world, vwgpu_comm** comm);
int vwgpu_comm_destroy(vwgpu_comm* comm);
/* rows owned by `rank` and the rows its window spans (clipped to the image); pure host arithmetic, no context */
int vwgpu_halo_plan(int rank, int world, int rows_total, int halo_above, int halo_below, int* owned_a, int* owned_b, int* need_a,
                    int* need_b);
/* The verdict of the request check below from a table of gathered headers {rows_total, halo_above, halo_below, bytes per row} x world:
 * 1 = every rank asked for the same image and halos, 0 = not (rank_a / rank_b: the first differing pair).  Pure host arithmetic. */
int vwgpu_halo_headers_agree(const long long* headers, int world, int* rank_a, int* rank_b);
/* d_owned: the rank's rows (owned_b - owned_a) x cols, contiguous; d_window: (need_b - need_a) x cols, receives own rows + halos;
 * every rank of the communicator must make the call.  The requests of all ranks are compared first — one 32-byte all-gather over
 * the communicator and one host round trip — and either EVERY rank enters the data exchange or every rank returns
 * VWGPU_ERR_ARGUMENT; the exchange itself (one send / recv per neighbour that owns needed rows) is queued on the context's stream
 * and the call returns without waiting for it.  *first_row = need_a. */
int vwgpu_fetch_strip_window_dev(vwgpu_ctx* ctx, vwgpu_comm* comm, const void* d_owned, int cols, int elem_bytes, int rows_total,
                                 int halo_above, int halo_below, void* d_window, int* first_row);

#ifdef __cplusplus
}
#endif
#endif /* VWGPU_H */
