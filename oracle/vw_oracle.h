/* vw_oracle.h — C interface of the CPU parity oracle.
 *
 * TEST INFRASTRUCTURE ONLY.  This is a dependency-free restatement of the
 * Vision Workbench reference algorithms on the dense block-matching hot path.
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * it; the product (visionworkbench_amd, libvwgpu.so) never does.
 *
 * The reference itself cannot be compiled here (every VW header needs Boost,
 * first failure src/vw/Core/FundamentalTypes.h:32), so each function below
 * cites the reference file:line it restates and is pinned by the reference's
 * own known-answer tests re-typed in tests/test_oracle_golden.py.
 *
 * Image layout everywhere: row-major, contiguous, `cols` fastest
 * (vw::ImageView, src/vw/Image/ImageView.h:209-239).
 * Disparity layout: 3 x int32 per pixel {dx, dy, valid}, valid = INT32_MAX or 0
 * (vw::PixelMask<Vector2i>, src/vw/Image/PixelMask.h:48-120).
 */
#ifndef VW_ORACLE_H
#define VW_ORACLE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* CostFunctionType, src/vw/Stereo/CostFunctions.h:143-149 */
enum { VWO_ABSOLUTE_DIFFERENCE = 0, VWO_SQUARED_DIFFERENCE = 1, VWO_CROSS_CORRELATION = 2 };

/* fast_box_sum<double>, src/vw/Stereo/Algorithms.h:43-129.
 * in: w x h (float or double), out: (w-kx+1) x (h-ky+1) double. returns 0, or -1 on even kernel. */
int vwo_fast_box_sum_f32(const float* in, int w, int h, int kx, int ky, double* out);
int vwo_fast_box_sum_f64(const double* in, int w, int h, int kx, int ky, double* out);

/* Per-pixel cost images (the lazy BinaryPerPixelView of CostFunctions.h:153-236 rasterised to double).
 * NCC returns the raw float product (no normalisation), as NCCCost::operator() does. */
int vwo_cost_image(int cost_type, const float* a, const float* b, int w, int h, double* out);

/* best_of_search_convolution, src/vw/Stereo/Correlation.cc:33-137, on already-cropped rasters
 * (what calc_disparity, Correlation.cc:330-375, hands it):
 *   left  lw x lh, right rw x rh with rw >= lw+sx-1, rh >= lh+sy-1 (row strides in elements).
 *   out   (lw-kx+1) x (lh-ky+1) x {dx,dy,valid}. */
int vwo_calc_disparity(int cost_type,
                       const float* left, int lw, int lh, int64_t lstride,
                       const float* right, int rw, int rh, int64_t rstride,
                       int kx, int ky, int sx, int sy, int32_t* out);

/* The reference's real execution model for a big image: output split into tile x tile blocks,
 * `threads` workers pull tiles from a queue, each tile calls single-threaded calc_disparity on its
 * padded crop (src/vw/Image/ImageIO.h:228-251, src/vw/tools/correlate.cc:266).
 * max_tiles > 0 bounds the number of tiles processed (bench sample); returns #output pixels done
 * through *pixels_done. */
int vwo_calc_disparity_tiled(int cost_type,
                             const float* left, int lw, int lh,
                             const float* right, int rw, int rh,
                             int kx, int ky, int sx, int sy, int32_t* out,
                             int tile, int threads, int max_tiles, int64_t* pixels_done);

/* cross_corr_consistency_check, src/vw/Stereo/Correlate.cc:1441-1502 (in place on l2r). */
int vwo_cross_corr_consistency_check(int32_t* l2r, int lw, int lh,
                                     const int32_t* r2l, int rw, int rh, float thr);

/* ---- image filters on the path (pyramid + prefilters) ---------------------------------------------------- */

enum { VWO_EDGE_CONSTANT = 0, VWO_EDGE_ZERO = 1 };
enum { VWO_PREFILTER_NONE = 0, VWO_PREFILTER_MEANSUB = 1, VWO_PREFILTER_LOG = 2 };

/* generate_gaussian_kernel<float>, src/vw/Image/Filter.tcc:37-78 + compute_kernel_size, Filter.cc:32-37.
 * size == 0 -> default size.  Returns the number of taps (0 for sigma == 0), writes them to out (cap >= result). */
int vwo_generate_gaussian_kernel_f32(double sigma, int size, float* out, int cap);
int vwo_generate_gaussian_kernel_f64(double sigma, int size, double* out, int cap);

/* SeparableConvolutionView<ImageView<float>, float, Edge>::rasterize over the whole image
 * (src/vw/Image/Convolution.h:275-328, correlate_1d_at_point :53-65), followed by SubsampleView
 * (src/vw/Image/Manipulation.h:214-293) with step `subsample` (1 = none).  nx or ny may be 0 (axis inactive).
 * cx, cy = kernel origins ((n-1)/2 for the reference's default constructor).  dst is
 * (1+(w-1)/s) x (1+(h-1)/s). */
int vwo_separable_convolution_f32(const float* src, int w, int h, const float* xk, int nx, int cx,
                                  const float* yk, int ny, int cy, int edge, int subsample, float* dst);
int vwo_separable_convolution_f64(const double* src, int w, int h, const double* xk, int nx, int cx,
                                  const double* yk, int ny, int cy, int edge, int subsample, double* dst);

/* ConvolutionView (general 2-D kernel, kw x kh, origin (ci,cj)): src/vw/Image/Convolution.h:105-170,
 * correlate_2d_at_point :66-88 with the kernel rotated by 180 degrees. */
int vwo_convolution_2d_f32(const float* src, int w, int h, const float* k, int kw, int kh, int ci, int cj,
                           int edge, float* dst);
int vwo_convolution_2d_f64(const double* src, int w, int h, const double* k, int kw, int kh, int ci, int cj,
                           int edge, double* dst);

/* subsample_mask_by_two, src/vw/Stereo/CorrelationView.cc:38-63. dst is (1+(w-1)/2) x (1+(h-1)/2). */
int vwo_subsample_mask_by_two(const uint8_t* src, int w, int h, uint8_t* dst);

/* prefilter_image, src/vw/Stereo/PreFilter.h:41-95 (LoG = laplacian(gaussian(width)); MEANSUB = I - gaussian(width)). */
int vwo_prefilter_image(const float* src, int w, int h, int mode, float width, float* dst);

/* ---- zone subdivision and parabola sub-pixel refinement ------------------------------------------------------- */

/* subdivide_regions(disparity, bounding_box(disparity), list, kernel_size), src/vw/Stereo/Correlation.cc:139-328.
 * disp3: w x h x {dx,dy,valid} int32.  Each zone is written as 8 ints
 * {region.min.x, region.min.y, region.max.x, region.max.y, range.min.x, range.min.y, range.max.x, range.max.y}.
 * Returns the number of zones (may exceed cap; only cap are written). */
int vwo_subdivide_regions(const int32_t* disp3, int w, int h, int kx, int ky, int32_t* zones, int cap);

/* Rasterises prefilter.filter(image) (src/vw/Stereo/PreFilter.h:41-74) over an arbitrary region [x0,x0+bw) x
 * [y0,y0+bh), which may extend beyond the image: the lazy views evaluate the filter of the edge-extended source
 * there (this is what ParabolaSubpixelView::prerasterize crops, ParabolaSubpixelView.cc:302-327). */
int vwo_prefilter_region(const float* src, int w, int h, int mode, float width,
                         int x0, int y0, int bw, int bh, float* dst);

/* parabola_subpixel(disparity, left, right, prefilter_mode, prefilter_width, kernel) rasterised over the whole
 * image in one block: ParabolaSubpixelView::prerasterize + evaluate, src/vw/Stereo/ParabolaSubpixelView.cc:31-330.
 * disp3f / out3f: w x h x {dx, dy, valid in {0.f,1.f}} float (PixelMask<Vector2f>); left is w x h. */
int vwo_parabola_subpixel(const float* disp3f, int w, int h, const float* left, const float* right, int rw, int rh,
                          int prefilter_mode, float prefilter_width, int kx, int ky, float* out3f);

/* The range vwo_parabola_subpixel sizes its rasters with: get_disparity_range of the truncated disparity
 * (ParabolaSubpixelView.cc:283-287) over the VALID pixels (Image/Statistics.h:283-290), zeros without any.
 * range4 = {min x, min y, max x, max y}. */
void vwo_parabola_range(const float* disp3f, int w, int h, int32_t* range4);

/* ---- pyramid block matching ------------------------------------------------------------------------------------ */

/* One tile of pyramid_correlate(...) with VW_CORRELATION_BM: PyramidCorrelationView::prerasterize(bbox),
 * src/vw/Stereo/CorrelationView.cc:273-886 (build_image_pyramids :67-239, zone loop :596-700, clean-up filters
 * :702-750 with src/vw/Stereo/DisparityMap.h:97-253,318-441, zone refinement :754-799, final cast :876-885).
 * Masks may be NULL (all valid).  search = [smin, smax) as a BBox2i.  blob_filter_area = 0, no lr_disp_diff,
 * collar 0.  corr_timeout > 0 uses the reference's estimate accounting (seconds_per_op * search volume) without the
 * wall-clock re-calibration.  out3f: bw x bh x {dx, dy, valid} float. Returns 0, or -1 on bad arguments. */
int vwo_pyramid_correlate(const float* left, int lw, int lh, const float* right, int rw, int rh,
                          const uint8_t* lmask, const uint8_t* rmask,
                          int prefilter_mode, float prefilter_width,
                          int sminx, int sminy, int smaxx, int smaxy, int kx, int ky, int cost_type,
                          int corr_timeout, double seconds_per_op, float consistency_threshold,
                          int filter_half_kernel, int max_pyramid_levels,
                          int bx, int by, int bw, int bh, float* out3f);

/* The same tile with VW_CORRELATION_SGM (SGM branch, CorrelationView.cc:391-595; final sub-pixel view :862-875).
 * kernel is square; cost_type 3 = census, 4 = ternary census. */
int vwo_pyramid_correlate_sgm(const float* left, int lw, int lh, const float* right, int rw, int rh,
                              const uint8_t* lmask, const uint8_t* rmask,
                              int sminx, int sminy, int smaxx, int smaxy, int kernel, int cost_type,
                              float consistency_threshold, int min_consistency_level, int filter_half_kernel, int max_pyramid_levels,
                              int sgm_subpixel_mode, int sgm_sbx, int sgm_sby, size_t memory_limit_mb, int num_threads,
                              int bx, int by, int bw, int bh, float* out3f);
/* algorithm of the following vwo_pyramid_correlate_sgm calls of this thread: 1 = VW_CORRELATION_SGM (default), 2 = VW_CORRELATION_MGM,
 * 3 = VW_CORRELATION_FINAL_MGM (src/vw/Stereo/CorrelationView.cc:365-366) */
void vwo_set_sgm_algorithm(int algorithm);
/* Host threads the SGM oracle may use for the lines of a path direction and the rows of the cost fill (process wide; the
 * results do not depend on it — the reference runs its PixelPassTasks on a pool as well, SGM.cc:2462-2612). */
void vwo_set_sgm_host_threads(int n);
/* Opt-in (process wide) to cost types 0 / 1 = the mean-abs-difference block cost of fill_costs_block / get_cost_block
 * (SGM.cc:1651-1738, defaults p1 = 3, p2 = 250 :128-131,156-158), which the reference keeps behind a NoImplErr (:1887-1892). */
void vwo_set_sgm_allow_block_cost(int on);

/* disparity_blob_filter (CorrelationView.cc:242-271): zero every valid pixel of an 8-connected component of valid pixels
 * with at most `area` pixels; vwo_blob_sizes = the size of each pixel's component (0 for invalid pixels), the quantity
 * get_blob_sizes reports (src/vw/Image/tests/TestBlobIndex.cxx:97-126). */
int vwo_blob_sizes(const int32_t* disp3, int w, int h, uint32_t* sizes);
int vwo_disparity_blob_filter(int32_t* disp3, int w, int h, int area);
void vwo_set_blob_filter_area(int area);
/* cross_corr_consistency_check with the optional lr_disp_diff output (Correlate.cc:1441-1502) and the pyramid's
 * m_lr_disp_diff / m_region_ul (CorrelationView.h:84; set for the following pyramid calls of the calling thread). */
int vwo_cross_corr_consistency_check_diff(int32_t* l2r, int lw, int lh, const int32_t* r2l, int rw, int rh, float thr,
                                          float* diff2, int dcols, int drows, int ulx, int uly);
void vwo_set_lr_disp_diff(float* buf, int cols, int rows, int ulx, int uly);

/* rm_outliers_using_thresh / disparity_cleanup_using_thresh / disparity_mask on whole images
 * (src/vw/Stereo/DisparityMap.h:318-441, 97-253); disp3 in place.  cleanup != 0 adds the second (1,1,3.0,0.20) pass. */
int vwo_disparity_filter(int32_t* disp3, int w, int h, int half_h, int half_v, double pixel_thr, double rej_thr, int cleanup);
int vwo_disparity_mask(int32_t* disp3, int w, int h, const uint8_t* lmask, const uint8_t* rmask, int rmw, int rmh);

/* ---- semi-global matching (vw_sgm_oracle.cc) -------------------------------------------------------------------- */

/* u8_convert: min/max stretch to [0,255] with truncation, src/vw/Image/ImageThresh.h:275-286. */
int vwo_u8_convert(const float* src, int w, int h, uint8_t* dst);
/* get_census_value_{3x3,5x5,7x7,9x9} / ternary variants at every pixel with a full window
 * (src/vw/Image/CensusTransform.h:64-340); out is (w-k+1) x (h-k+1) uint64. */
int vwo_census_transform(const uint8_t* img, int w, int h, int kernel, int ternary, int threshold, uint64_t* out);
int vwo_hamming_distance(uint64_t a, uint64_t b);          /* src/vw/Math/Functions.h:226-260 */

/* SemiGlobalMatcher (src/vw/Stereo/SGM.h:75-352): create = ctor/set_parameters, run = semi_global_matching_func +
 * create_disparity_view, subpixel = create_disparity_view_subpixel.  cost_type 3 = CENSUS_TRANSFORM, 4 = TERNARY_CENSUS.
 * Masks / prev may be NULL.  num_threads only enters the memory-cap check (calc_main_buf_size, SGM.cc:677-731). */
typedef struct vwo_sgm vwo_sgm;
vwo_sgm* vwo_sgm_create(int cost_type, int use_mgm, int min_dx, int min_dy, int max_dx, int max_dy, int kernel, int subpixel,
                        int sbx, int sby, size_t memory_limit_mb, int p1, int p2, int ternary_thr, int num_threads);
void vwo_sgm_destroy(vwo_sgm* s);
int vwo_sgm_run(vwo_sgm* s, const uint8_t* left, int lw, int lh, const uint8_t* right, int rw, int rh,
                const uint8_t* lmask, int lmw, int lmh, const uint8_t* rmask, int rmw, int rmh,
                const int32_t* prev, int pw, int ph, int32_t* out_disp, int cap_pixels);
int vwo_sgm_output_size(vwo_sgm* s, int* ow, int* oh);
int vwo_sgm_subpixel(vwo_sgm* s, const int32_t* int_disp, float* out3f);
size_t vwo_sgm_buffer_size(vwo_sgm* s);
int vwo_sgm_read(vwo_sgm* s, int32_t* bounds4, uint64_t* starts, uint8_t* cost, uint16_t* accum);
int vwo_sgm_p1p2(vwo_sgm* s, int* p1, int* p2);
/* calc_disparity_sgm (src/vw/Stereo/SGM.cc:167-229) on already cropped regions: left lw x lh, right (lw+sx) x (lh+sy). */
int vwo_calc_disparity_sgm(int cost_type, const float* left, int lw, int lh, const float* right, int rw, int rh,
                           int sx, int sy, int kernel, int subpixel, int sbx, int sby, size_t memory_limit_mb, int num_threads,
                           const uint8_t* lmask, int lmw, int lmh, const uint8_t* rmask, int rmw, int rmh,
                           const int32_t* prev, int pw, int ph, int32_t* out_disp, float* out_subpixel, int* ow, int* oh);

/* the same with user penalties (p1 / p2 = 0: the defaults) */
int vwo_calc_disparity_sgm_p(int cost_type, const float* left, int lw, int lh, const float* right, int rw, int rh,
                             int sx, int sy, int kernel, int subpixel, int sbx, int sby, size_t memory_limit_mb, int num_threads,
                             const uint8_t* lmask, int lmw, int lmh, const uint8_t* rmask, int rmw, int rmh,
                             const int32_t* prev, int pw, int ph, int p1, int p2, int32_t* out_disp, float* out_subpixel, int* ow, int* oh);

/* the same with use_mgm (accum_mgm_multithread, SGM.cc:2619-2700) */
int vwo_calc_disparity_sgm_x(int cost_type, int use_mgm, const float* left, int lw, int lh, const float* right, int rw, int rh,
                             int sx, int sy, int kernel, int subpixel, int sbx, int sby, size_t memory_limit_mb, int num_threads,
                             const uint8_t* lmask, int lmw, int lmh, const uint8_t* rmask, int rmw, int rmh,
                             const int32_t* prev, int pw, int ph, int p1, int p2, int32_t* out_disp, float* out_subpixel, int* ow, int* oh);

#ifdef __cplusplus
}
#endif
#endif
