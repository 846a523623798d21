"""Host-side mirror of the reference's stereo entry points on the block-matching hot path.

Same names, argument meaning and error behaviour as vw::stereo; every function hands
rasterised images to libvwgpu.so through the C ABI (include/vwgpu.h).  Inputs may be
  * torch CUDA tensors  -> device entry points, asynchronous on the current torch stream, result = CUDA tensor;
  * numpy arrays        -> host entry points (H2D, kernels, D2H), result = numpy array.
There is no CPU implementation here: without the HIP library or a GPU these functions raise.
"""
import ctypes

import numpy as np

from . import _lib, camera, core
from ._operands import Operands, is_tensor as _is_tensor, new_stats, put_stats
from .core import ArgumentErr, BBox2i, CostFunctionType


def calc_disparity(cost_type, left_in, right_in, left_region, search_volume, kernel_size, ctx=None):
    """vw::stereo::calc_disparity (src/vw/Stereo/Correlation.h:50-57, Correlation.cc:330-375).

    left_in / right_in: (rows, cols) float32 images (PixelGray<float>).  left_region: BBox2i inside the left
    image.  search_volume = (sx, sy) >= 1, kernel_size = (kx, ky) odd.  The right image must cover
    left_region grown by search_volume - 1 on the max side (the reference crops it so, :356-359).
    Returns (rows-ky+1, cols-kx+1, 3) int32 = PixelMask<Vector2i> {dx, dy, valid (INT32_MAX|0)}.

    Device tensors: the call is queued on the current torch stream, but by default it WAITS for the input-class flags of the data
    (one small device-to-host copy: packed integer kernels, the float64 tile kernel or the reference's summation order are chosen
    from the data, so that the result is bit-exact for any input).  Callers that queue many calls set
    ctx.set_option(core.OPT_DEFER_EXACTNESS, 1): no host round trip, ctx.last_path() reports afterwards.
    """
    kx, ky = int(kernel_size[0]), int(kernel_size[1])
    sx, sy = int(search_volume[0]), int(search_volume[1])
    if left_in.ndim != 2 or right_in.ndim != 2:
        raise ArgumentErr("calc_disparity: images must be 2-D (rows, cols)")
    x0, y0 = left_region.min
    x1, y1 = left_region.max
    if x0 < 0 or y0 < 0 or x1 > left_in.shape[1] or y1 > left_in.shape[0]:
        raise ArgumentErr("calc_disparity: Region not inside left image.")
    rx1, ry1 = x1 + sx - 1, y1 + sy - 1
    if rx1 > right_in.shape[1] or ry1 > right_in.shape[0]:
        raise ArgumentErr("calc_disparity: right image does not cover the search region")
    lw, lh = x1 - x0, y1 - y0
    ow, oh = lw - kx + 1, lh - ky + 1
    ops = Operands("calc_disparity", left_in, ctx)
    # the crops stay views of a tensor (row stride = the whole image's); a numpy crop is copied for the host entry
    l = ops.image(left_in[y0:y1, x0:x1], np.float32, rows=True)
    r = ops.image(right_in[y0:ry1, x0:rx1], np.float32, rows=True)
    out = ops.empty((max(oh, 0), max(ow, 0), 3), np.int32)
    ops.call("calc_disparity", int(cost_type), ops.ptr(l), lw, lh, ops.row_stride(l),
             ops.ptr(r), rx1 - x0, ry1 - y0, ops.row_stride(r), kx, ky, sx, sy, ops.ptr(out), 0)
    return out


def fast_box_sum(image, kernel, ctx=None):
    """vw::stereo::fast_box_sum<double>(image, kernel) (src/vw/Stereo/Algorithms.h:41-129): float64 sums of every
    kx x ky window, (rows-ky+1, cols-kx+1), formed in the reference's running-sum order (bit-identical for any float input)."""
    kx, ky = int(kernel[0]), int(kernel[1])
    if image.ndim != 2:
        raise ArgumentErr("fast_box_sum: the image must be 2-D (rows, cols)")
    h, w = image.shape
    ops = Operands("fast_box_sum", image, ctx)
    img = ops.image(image, np.float32, rows=True)
    out = ops.empty((max(h - ky + 1, 0), max(w - kx + 1, 0)), np.float64)
    ops.call("fast_box_sum", ops.ptr(img), w, h, ops.row_stride(img), kx, ky, ops.ptr(out), 0)
    return out


def cross_corr_consistency_check(l2r, r2l, cross_corr_threshold, lr_disp_diff=None, ul_corner_offset=(0, 0), ctx=None):
    """vw::stereo::cross_corr_consistency_check (src/vw/Stereo/Correlate.cc:1441-1502), IN PLACE on l2r.

    l2r, r2l: (rows, cols, 3) int32 PixelMask<Vector2i> images.  lr_disp_diff (optional, modified in place): (rows, cols, 2)
    float32 PixelMask<float> {value, valid}; every kept pixel stores its discrepancy at (c, r) + ul_corner_offset."""
    ops = Operands("cross_corr_consistency_check", l2r, ctx)
    if lr_disp_diff is not None and (lr_disp_diff.ndim != 3 or lr_disp_diff.shape[2] != 2):
        raise ArgumentErr("cross_corr_consistency_check: lr_disp_diff must be (rows, cols, 2) float32")
    ops.image(l2r, np.int32, in_place=True)
    diff = ops.image(lr_disp_diff, np.float32, in_place=True)
    r2l = ops.image(r2l, np.int32)
    args = (ops.ptr(l2r), l2r.shape[1], l2r.shape[0], 0, ops.ptr(r2l), r2l.shape[1], r2l.shape[0], 0, float(cross_corr_threshold))
    if diff is None:
        ops.call("cross_corr_consistency_check", *args)
    else:
        ops.call("cross_corr_consistency_check_diff", *args, ops.ptr(diff), diff.shape[1], diff.shape[0], 0,
                 int(ul_corner_offset[0]), int(ul_corner_offset[1]))
    return l2r


def parabola_subpixel(disparity, left_image, right_image, prefilter_mode, prefilter_width, kernel_size, ctx=None):
    """vw::stereo::parabola_subpixel (src/vw/Stereo/ParabolaSubpixelView.h:112-117) rasterised over the whole image.

    disparity: (rows, cols, 3) float32 PixelMask<Vector2f> {dx, dy, valid}; same rows/cols as left_image (the
    reference asserts this, ParabolaSubpixelView.h:67-69).  Returns the refined disparity in the same layout."""
    kx, ky = int(kernel_size[0]), int(kernel_size[1])
    if disparity.ndim != 3 or disparity.shape[2] != 3 or tuple(disparity.shape[:2]) != tuple(left_image.shape):
        raise ArgumentErr("SubpixelView: Disparity image must match left image.")
    h, w = left_image.shape
    rh, rw = right_image.shape
    ops = Operands("parabola_subpixel", left_image, ctx)
    d, l, r = (ops.image(x, np.float32) for x in (disparity, left_image, right_image))
    out = ops.empty(d.shape, np.float32)
    ops.call("parabola_subpixel", ops.ptr(d), w, h, 0, ops.ptr(l), 0, ops.ptr(r), rw, rh, 0,
             int(prefilter_mode), float(prefilter_width), kx, ky, ops.ptr(out), 0)
    return out


SUBPIXEL_LUCAS_KANADE, SUBPIXEL_FAST_AFFINE, SUBPIXEL_BAYES_EM, SUBPIXEL_PHASE = 0, 1, 2, 3   # SubpixelView.h:28-33


def subpixel_tiles(cols, rows, block_size=None):
    """The prerasterize boxes {x, y, w, h}: the whole image, or the blocks of block_write_image / block_rasterize,
    aligned to multiples of block_size = (bw, bh) from (0, 0)."""
    if block_size is None:
        return np.array([[0, 0, cols, rows]], np.int32)
    bw, bh = int(block_size[0]), int(block_size[1])
    if bw <= 0 or bh <= 0:
        raise ArgumentErr("PyramidSubpixelView: block_size must be positive")
    return np.array([[x, y, min(bw, cols - x), min(bh, rows - y)] for y in range(0, rows, bh) for x in range(0, cols, bw)],
                    np.int32).reshape(-1, 4)


def _pyramid_subpixel(name, disparity, left, right, prefilter_mode, prefilter_width, kernel_size, max_pyramid_levels,
                      algorithm, block_size, ctx, stats, phase_accuracy=None):
    # phase_accuracy given: vwgpu_phase_subpixel[_dev], which takes the accuracy where the generic entry takes algorithm
    entry = "pyramid_subpixel" if phase_accuracy is None else "phase_subpixel"
    selector = int(algorithm) if phase_accuracy is None else int(phase_accuracy)
    kx, ky = int(kernel_size[0]), int(kernel_size[1])
    if disparity.ndim != 3 or disparity.shape[2] != 3 or left.ndim != 2 or right.ndim != 2 \
            or tuple(disparity.shape[:2]) != tuple(left.shape):
        raise ArgumentErr("PyramidSubpixelView::PyramidSubpixelView(): Disparity image must match left image.")
    if kx < 1 or ky < 1 or kx % 2 != 1 or ky % 2 != 1:
        raise ArgumentErr("%s: Kernel input not sized with odd values." % name)
    if phase_accuracy is not None and (kx > PHASE_MAX_KERNEL or ky > PHASE_MAX_KERNEL or selector > PHASE_MAX_ACCURACY):
        raise core.NoImplErr("phase_subpixel: kernel %d x %d or accuracy %d above the limits %d x %d, %d"
                             % (kx, ky, selector, PHASE_MAX_KERNEL, PHASE_MAX_KERNEL, PHASE_MAX_ACCURACY))
    h, w = left.shape
    rh, rw = right.shape
    tiles = subpixel_tiles(w, h, block_size)
    st = new_stats(3)
    ops = Operands(name, left, ctx)
    d, l, r = (ops.image(x, np.float32) for x in (disparity, left, right))
    out = ops.zeros(d.shape, np.float32)     # pixels outside every tile stay 0
    ops.call(entry, ops.ptr(d), w, h, 0, ops.ptr(l), 0, ops.ptr(r), rw, rh, 0, int(prefilter_mode), float(prefilter_width),
             kx, ky, int(max_pyramid_levels), selector, tiles.ctypes.data, len(tiles), ops.ptr(out), 0, st)
    put_stats(stats, st)
    return out


def pyramid_subpixel(disparity, left, right, prefilter_mode, prefilter_width, kernel_size, max_pyramid_levels=2,
                     algorithm=SUBPIXEL_FAST_AFFINE, block_size=None, ctx=None, stats=None):
    """vw::stereo::PyramidSubpixelView (src/vw/Stereo/SubpixelView.h:36-108) with any implemented algorithm
    (SUBPIXEL_LUCAS_KANADE, SUBPIXEL_FAST_AFFINE, SUBPIXEL_BAYES_EM; SUBPIXEL_PHASE raises NoImplErr: phase refinement is
    phase_subpixel, which takes its accuracy argument), rasterised one
    prerasterize(bbox) per tile (SubpixelView.cc:33-224).

    disparity: (rows, cols, 3) float32 PixelMask<Vector2f> {dx, dy, valid}, the left image's size; each tile's disparity range
    is taken over its valid pixels, as in the reference (what an invalid pixel stores is never read).  left / right: 2-D float32 (any sizes), numpy arrays
    (host entry) or CUDA tensors (device entry, result on the device).  block_size None = one tile, the whole image
    (ImageView out = view); (bw, bh) = the blocks of block_write_image.  Returns refined {dx, dy, 1}, invalid {0, 0, 0}.
    stats (optional list) receives [fixpoint rounds summed over tiles and levels, most rounds of one tile level, window
    passes (BAYES_EM: every EM pass)]."""
    if int(algorithm) not in (SUBPIXEL_LUCAS_KANADE, SUBPIXEL_FAST_AFFINE, SUBPIXEL_BAYES_EM, SUBPIXEL_PHASE):
        raise ArgumentErr("PyramidSubpixelView: unknown algorithm %d" % int(algorithm))
    if int(algorithm) == SUBPIXEL_PHASE:
        raise core.NoImplErr("PyramidSubpixelView: SUBPIXEL_PHASE is not implemented")
    return _pyramid_subpixel("pyramid_subpixel", disparity, left, right, prefilter_mode, prefilter_width, kernel_size,
                             max_pyramid_levels, algorithm, block_size, ctx, stats)


def affine_subpixel(disparity, left, right, prefilter_mode, prefilter_width, kernel_size, max_pyramid_levels=2,
                    block_size=None, ctx=None, algorithm=SUBPIXEL_FAST_AFFINE, stats=None):
    """vw::stereo::affine_subpixel (src/vw/Stereo/SubpixelView.h:120-126): PyramidSubpixelView with SUBPIXEL_FAST_AFFINE
    (see pyramid_subpixel for the arguments).  algorithm must stay SUBPIXEL_FAST_AFFINE; the other refiners are
    lk_subpixel, bayes_em_subpixel and pyramid_subpixel."""
    if int(algorithm) != SUBPIXEL_FAST_AFFINE:
        raise core.NoImplErr("affine_subpixel: algorithm %d is not FAST_AFFINE (use lk_subpixel, bayes_em_subpixel or "
                             "pyramid_subpixel)" % int(algorithm))
    return _pyramid_subpixel("affine_subpixel", disparity, left, right, prefilter_mode, prefilter_width, kernel_size,
                             max_pyramid_levels, algorithm, block_size, ctx, stats)


def lk_subpixel(disparity, left, right, prefilter_mode, prefilter_width, kernel_size, max_pyramid_levels=2,
                block_size=None, ctx=None, stats=None):
    """vw::stereo::lk_subpixel (src/vw/Stereo/SubpixelView.h:111-117): PyramidSubpixelView with SUBPIXEL_LUCAS_KANADE
    (see pyramid_subpixel for the arguments)."""
    return _pyramid_subpixel("lk_subpixel", disparity, left, right, prefilter_mode, prefilter_width, kernel_size,
                             max_pyramid_levels, SUBPIXEL_LUCAS_KANADE, block_size, ctx, stats)


def bayes_em_subpixel(disparity, left, right, prefilter_mode, prefilter_width, kernel_size, max_pyramid_levels=2,
                      block_size=None, ctx=None, stats=None):
    """vw::stereo::bayes_em_subpixel (src/vw/Stereo/SubpixelView.h:127-133): PyramidSubpixelView with SUBPIXEL_BAYES_EM
    (see pyramid_subpixel for the arguments)."""
    return _pyramid_subpixel("bayes_em_subpixel", disparity, left, right, prefilter_mode, prefilter_width, kernel_size,
                             max_pyramid_levels, SUBPIXEL_BAYES_EM, block_size, ctx, stats)


PHASE_MAX_KERNEL, PHASE_MAX_ACCURACY = 41, 64   # include/vwgpu.h: larger sizes raise NoImplErr


def phase_subpixel(disparity, left, right, prefilter_mode, prefilter_width, kernel_size, max_pyramid_levels=0,
                   phase_subpixel_accuracy=20, block_size=None, ctx=None, stats=None):
    """vw::stereo::phase_subpixel (src/vw/Stereo/SubpixelView.h:136-144): PyramidSubpixelView with SUBPIXEL_PHASE, refined
    by subpixel_phase_2d (src/vw/Stereo/PhaseSubpixelView.cc:231-326).  Arguments and result as pyramid_subpixel, plus
    phase_subpixel_accuracy (the pad factor of the second phase correlation; the first gets accuracy // 2 rounded toward
    zero, and a factor <= 2 stops after the coarse pass).  Kernels up to 41 x 41 and accuracies up to 64; larger values
    raise NoImplErr.  stats (optional list) receives [pixels refined, pixels invalidated (|d| > 3 or NaN), tiles].
    Each patch is converted to 8 bits as the reference's get_dft does; the transforms follow the order defined in
    DESIGN.md section 4.13, not OpenCV's."""
    return _pyramid_subpixel("phase_subpixel", disparity, left, right, prefilter_mode, prefilter_width, kernel_size,
                             max_pyramid_levels, SUBPIXEL_PHASE, block_size, ctx, stats,
                             phase_accuracy=int(phase_subpixel_accuracy))


CORR_EVAL_METRICS = {"ncc": 0, "stddev": 1, "parabola_curvature": 2, "cramer_rao": 3}   # CorrEval.h:88-90
CORR_EVAL_MAX_KERNEL = 63   # include/vwgpu.h: larger kernels raise NoImplErr


def corr_eval(left, right, disparity, kernel_size, metric, sample_rate=1, round_to_int=False, prefilter_mode=0,
              prefilter_kernel_width=0.0, left_valid=None, right_valid=None, block_size=None, ctx=None, stats=None):
    """vw::stereo::corr_eval (src/vw/Stereo/CorrEval.h:117-128), rasterised one CorrEval::prerasterize(bbox) per tile
    (CorrEval.cc:139-317); the tiles follow block_size as in pyramid_subpixel (the whole image when None).

    left: (rows, cols) float32, right: any (rrows, rcols) float32; left_valid / right_valid: optional masks of the same
    shapes (nonzero = valid; None = all valid), the PixelMask<float> validity of the images.  disparity: (rows, cols, 3)
    float32 PixelMask<Vector2f> {dx, dy, valid}.  metric: "ncc", "stddev", "parabola_curvature" or "cramer_rao".
    Returns (rows, cols, 2) float32 PixelMask<float> {value, valid}; pixels outside every tile stay 0.  numpy inputs run
    the host entry, CUDA tensors the device entry (which synchronises the stream once to report argument errors).
    The quirks the result keeps (the right crop per tile, the NCC that counts invalid samples, the float neighbour
    disparities of the curvature metrics) are listed at vwgpu_corr_eval in include/vwgpu.h.  Kernels up to 63 x 63.
    stats (optional list) receives [pixels evaluated, valid results, tiles, tiles with a degenerate right box]."""
    kx, ky = int(kernel_size[0]), int(kernel_size[1])
    if disparity.ndim != 3 or disparity.shape[2] != 3 or left.ndim != 2 or right.ndim != 2 \
            or tuple(disparity.shape[:2]) != tuple(left.shape):
        raise ArgumentErr("CorrEval: Left image and disparity must have the same dimensions.")
    if kx <= 0 or ky <= 0 or kx % 2 != 1 or ky % 2 != 1:
        raise ArgumentErr("CorrEval: The kernel dimensions must be positive and odd.")
    if metric not in CORR_EVAL_METRICS:
        raise ArgumentErr("CorrEval: Invalid metric: %s." % metric)
    if (left_valid is not None and tuple(left_valid.shape) != tuple(left.shape)) \
            or (right_valid is not None and tuple(right_valid.shape) != tuple(right.shape)):
        raise ArgumentErr("corr_eval: a validity mask does not match its image")
    if kx > CORR_EVAL_MAX_KERNEL or ky > CORR_EVAL_MAX_KERNEL:
        raise core.NoImplErr("corr_eval: kernel %d x %d is larger than %d x %d"
                             % (kx, ky, CORR_EVAL_MAX_KERNEL, CORR_EVAL_MAX_KERNEL))
    h, w = left.shape
    rh, rw = right.shape
    tiles = subpixel_tiles(w, h, block_size)
    st = new_stats(4)
    ops = Operands("corr_eval", left, ctx)
    # every operand, the masks included, must live on the left image's device: the kernels read them all
    d, l, r = (ops.image(x, np.float32, same_device=True) for x in (disparity, left, right))
    lv, rv = (ops.nonzero_u8(x, same_device=True) for x in (left_valid, right_valid))
    out = ops.zeros((h, w, 2), np.float32)     # pixels outside every tile stay 0
    ops.call("corr_eval", ops.ptr(d), w, h, 0, ops.ptr(l), ops.ptr(lv), 0, ops.ptr(r), ops.ptr(rv), rw, rh, 0, kx, ky,
             CORR_EVAL_METRICS[metric], int(sample_rate), 1 if round_to_int else 0, int(prefilter_mode),
             float(prefilter_kernel_width), tiles.ctypes.data, len(tiles), ops.ptr(out), 0, st)
    put_stats(stats, st)
    return out


def _filter_call(name, disparity, hh, hv, pthr, rthr, cleanup, ctx):
    if disparity.ndim != 3 or disparity.shape[2] != 3:
        raise ArgumentErr("%s: disparity must be (rows, cols, 3) int32" % name)
    h, w = disparity.shape[:2]
    if hh <= 0 or hv <= 0:
        raise ArgumentErr("RmOutliersFunc: half kernel sizes must be non-zero.")
    ops = Operands(name, disparity, ctx)
    d = ops.image(disparity, np.int32)
    out = ops.empty(d.shape, np.int32)
    ops.call("disparity_filter", ops.ptr(d), w, h, int(hh), int(hv), float(pthr), float(rthr), int(cleanup), ops.ptr(out))
    return out


def rm_outliers_using_thresh(disparity, half_h_kernel, half_v_kernel, pixel_threshold, rejection_threshold, ctx=None):
    """vw::stereo::rm_outliers_using_thresh (src/vw/Stereo/DisparityMap.h:387-399), rasterised over the whole image
    with the reference's ConstantEdgeExtension.  disparity: (rows, cols, 3) int32 PixelMask<Vector2i>."""
    return _filter_call("rm_outliers_using_thresh", disparity, half_h_kernel, half_v_kernel, pixel_threshold,
                        rejection_threshold, 0, ctx)


def disparity_cleanup_using_thresh(disparity, h_half_kernel, v_half_kernel, threshold, rejection_threshold, ctx=None):
    """vw::stereo::disparity_cleanup_using_thresh (src/vw/Stereo/DisparityMap.h:427-441): the filter above followed
    by a second pass with the reference's fixed (1, 1, 3.0, 0.20)."""
    return _filter_call("disparity_cleanup_using_thresh", disparity, h_half_kernel, v_half_kernel, threshold,
                        rejection_threshold, 1, ctx)


def disparity_mask(disparity, left_mask, right_mask, ctx=None):
    """vw::stereo::disparity_mask (src/vw/Stereo/DisparityMap.h:236-253): invalidate pixels whose source or target
    falls on masked data.  Returns a new image; masks are (rows, cols) uint8 (0 = no data)."""
    if disparity.ndim != 3 or disparity.shape[2] != 3 or tuple(disparity.shape[:2]) != tuple(left_mask.shape):
        raise ArgumentErr("disparity_mask: left mask must match the disparity image")
    h, w = left_mask.shape
    rmh, rmw = right_mask.shape
    ops = Operands("disparity_mask", disparity, ctx)
    m1, m2 = ops.image(left_mask, np.uint8), ops.image(right_mask, np.uint8)
    out = ops.copy_of(disparity, np.int32)
    ops.call("disparity_mask", ops.ptr(out), w, h, ops.ptr(m1), ops.ptr(m2), rmw, rmh)
    return out


def disparity_blob_filter(disparity, max_blob_area, ctx=None):
    """PyramidCorrelationView::disparity_blob_filter at one level (src/vw/Stereo/CorrelationView.cc:242-271): erase every
    8-connected component of valid pixels with at most max_blob_area pixels.  Returns a new image."""
    if disparity.ndim != 3 or disparity.shape[2] != 3:
        raise ArgumentErr("disparity_blob_filter: disparity must be (rows, cols, 3) int32")
    h, w = disparity.shape[:2]
    ops = Operands("disparity_blob_filter", disparity, ctx)
    out = ops.copy_of(disparity, np.int32)
    ops.call("disparity_blob_filter", ops.ptr(out), w, h, int(max_blob_area))
    return out


def subdivide_regions(disparity, kernel_size):
    """vw::stereo::subdivide_regions(disparity, bounding_box(disparity), list, kernel_size)
    (src/vw/Stereo/Correlation.cc:139-328).  Host logic (the zone scheduler of pyramid_correlate) on a numpy
    PixelMask<Vector2i> image; returns [(region BBox2i, disparity_range BBox2i), ...] in the reference's order."""
    lib = _lib.load()
    d = np.ascontiguousarray(disparity, np.int32)
    if d.ndim != 3 or d.shape[2] != 3:
        raise ArgumentErr("subdivide_regions: disparity must be (rows, cols, 3) int32")
    h, w = d.shape[:2]
    cap = 1024
    while True:
        buf = np.empty((cap, 8), np.int32)
        n = lib.vwgpu_subdivide_regions(d.ctypes.data, w, h, int(kernel_size[0]), int(kernel_size[1]), buf.ctypes.data, cap)
        if n < 0:
            raise ArgumentErr("subdivide_regions: bad arguments")
        if n <= cap:
            break
        cap = n
    return [(BBox2i.from_corners(z[0:2], z[2:4]), BBox2i.from_corners(z[4:6], z[6:8])) for z in buf[:n].tolist()]


def _pyramid_params(prefilter_mode, prefilter_width, search_region, kernel_size, cost_type, corr_timeout, seconds_per_op,
                    consistency_threshold, min_consistency_level, filter_half_kernel, max_pyramid_levels, algorithm,
                    blob_filter_area, sgm_subpixel_mode, sgm_search_buffer, memory_limit_mb, sgm_num_threads, region_ul=(0, 0)):
    """struct vwgpu_pyramid_params, without an lr_disp_diff image."""
    return _lib.PyramidParams(
        int(prefilter_mode), float(prefilter_width),
        int(search_region.min[0]), int(search_region.min[1]), int(search_region.max[0]), int(search_region.max[1]),
        int(kernel_size[0]), int(kernel_size[1]), int(cost_type), int(corr_timeout), float(seconds_per_op),
        float(consistency_threshold), int(min_consistency_level), int(filter_half_kernel),
        int(max_pyramid_levels), int(algorithm), int(blob_filter_area), int(sgm_subpixel_mode),
        int(sgm_search_buffer[0]), int(sgm_search_buffer[1]), int(memory_limit_mb), int(sgm_num_threads),
        None, 0, 0, 0, int(region_ul[0]), int(region_ul[1]))


def _masks(ops, left_mask, right_mask):
    """The optional uint8 masks of an image pair (None = every pixel valid)."""
    return ops.image(left_mask, np.uint8), ops.image(right_mask, np.uint8)


def _pyramid_images(ops, left, right, left_mask, right_mask):
    l, r = ops.image(left, np.float32), ops.image(right, np.float32)
    lm, rm = _masks(ops, left_mask, right_mask)
    for m, shp in ((lm, l.shape), (rm, r.shape)):
        if m is not None and tuple(m.shape) != tuple(shp):
            raise ArgumentErr("pyramid_correlate: masks must have the image size")
    return l, r, lm, rm


def pyramid_correlate(left, right, left_mask, right_mask, prefilter_mode, prefilter_width, search_region, kernel_size,
                      cost_type, corr_timeout=0, seconds_per_op=0.0, consistency_threshold=-1.0,
                      min_consistency_level=0, filter_half_kernel=0, max_pyramid_levels=5, algorithm=0,
                      collar_size=0, sgm_subpixel_mode=5, sgm_search_buffer=(2, 2), memory_limit_mb=6000,
                      blob_filter_area=0, bbox=None, sgm_num_threads=1, lr_disp_diff=None, region_ul=(0, 0), ctx=None):
    """vw::stereo::pyramid_correlate (src/vw/Stereo/CorrelationView.h:195-230) rasterised over `bbox`
    (default: the whole left image as ONE tile, i.e. PyramidCorrelationView::prerasterize(bounding_box),
    src/vw/Stereo/CorrelationView.cc:273-886).  The reference rasterises per block-cache tile; pass the same
    bbox to reproduce a tile.

    left / right: (rows, cols) float32; masks: (rows, cols) uint8 or None; search_region: BBox2i (half open).
    Returns (bbox rows, bbox cols, 3) float32 PixelMask<Vector2f> {dx, dy, valid}.
    algorithm 0 = VW_CORRELATION_BM (integer disparities cast to float), 1 = VW_CORRELATION_SGM (census costs only; the
    result is the matcher's sub-pixel view, CorrelationView.cc:862-875), 2 = VW_CORRELATION_MGM, 3 = _FINAL_MGM (MGM at level 0 only).  collar_size is
    the tile rasteriser's business (CorrelationView.h:128-132): pass the collared bbox.
    lr_disp_diff (optional, modified in place): (rows, cols, 2) float32 PixelMask<float> image covering the image pixels from
    region_ul on; the level-0 consistency check stores the L-R / R-L discrepancy of the pixels it keeps there and pixels
    the filters remove are invalidated again (CorrelationView.h:84, .cc:277-283, 683-693, 846-855)."""
    if left.ndim != 2 or right.ndim != 2:
        raise ArgumentErr("pyramid_correlate: images must be 2-D (rows, cols)")
    lh, lw = left.shape
    rh, rw = right.shape
    if bbox is None:
        bbox = BBox2i(0, 0, lw, lh)
    (bx, by), (bx1, by1) = bbox.min, bbox.max
    P = _pyramid_params(prefilter_mode, prefilter_width, search_region, kernel_size, cost_type, corr_timeout, seconds_per_op,
                        consistency_threshold, min_consistency_level, filter_half_kernel, max_pyramid_levels, algorithm,
                        blob_filter_area, sgm_subpixel_mode, sgm_search_buffer, memory_limit_mb, sgm_num_threads, region_ul)
    ops = Operands("pyramid_correlate", left, ctx)
    if lr_disp_diff is not None:
        if lr_disp_diff.ndim != 3 or lr_disp_diff.shape[2] != 2:
            raise ArgumentErr("pyramid_correlate: lr_disp_diff must be (rows, cols, 2) float32")
        P.lr_disp_diff = ops.ptr(ops.image(lr_disp_diff, np.float32, in_place=True))
        P.lr_disp_diff_rows, P.lr_disp_diff_cols = int(lr_disp_diff.shape[0]), int(lr_disp_diff.shape[1])
    bw, bh = bx1 - bx, by1 - by
    l, r, lm, rm = _pyramid_images(ops, left, right, left_mask, right_mask)
    out = ops.empty((max(bh, 0), max(bw, 0), 3), np.float32)
    ops.call("pyramid_correlate", ops.ptr(l), lw, lh, 0, ops.ptr(r), rw, rh, 0, ops.ptr(lm), 0, ops.ptr(rm), 0,
             ctypes.byref(P), bx, by, bw, bh, ops.ptr(out), 0)
    return out


def pyramid_correlate_batch(left, right, left_mask, right_mask, prefilter_mode, prefilter_width, search_region, kernel_size, cost_type,
                            bboxes, corr_timeout=0, seconds_per_op=0.0, consistency_threshold=-1.0, min_consistency_level=0,
                            filter_half_kernel=0, max_pyramid_levels=5, algorithm=0, collar_size=0, sgm_subpixel_mode=5,
                            sgm_search_buffer=(2, 2), memory_limit_mb=6000, blob_filter_area=0, sgm_num_threads=1, ctx=None):
    """Several tiles (`bboxes`: a list of BBox2i) of vw::stereo::pyramid_correlate in ONE call: what the reference's block rasteriser hands
    to its tile threads one at a time (src/vw/Image/ImageIO.h:228-251).  Runs of consecutive tiles of equal size go through the pyramid
    level loop together (vwgpu_pyramid_correlate_batch[_dev], include/vwgpu.h); every tile's result is identical to pyramid_correlate on
    that tile.  Returns a list of (rows, cols, 3) float32 PixelMask<Vector2f> images: CUDA tensors for CUDA inputs, numpy arrays otherwise."""
    if left.ndim != 2 or right.ndim != 2:
        raise ArgumentErr("pyramid_correlate: images must be 2-D (rows, cols)")
    lh, lw = left.shape
    rh, rw = right.shape
    P = _pyramid_params(prefilter_mode, prefilter_width, search_region, kernel_size, cost_type, corr_timeout, seconds_per_op,
                        consistency_threshold, min_consistency_level, filter_half_kernel, max_pyramid_levels, algorithm,
                        blob_filter_area, sgm_subpixel_mode, sgm_search_buffer, memory_limit_mb, sgm_num_threads)
    n = len(bboxes)
    IA = ctypes.c_int * max(n, 1)
    bx = IA(*[int(b.min[0]) for b in bboxes]); by = IA(*[int(b.min[1]) for b in bboxes])
    bw = IA(*[int(b.max[0] - b.min[0]) for b in bboxes]); bh = IA(*[int(b.max[1] - b.min[1]) for b in bboxes])
    ops = Operands("pyramid_correlate", left, ctx)
    l, r, lm, rm = _pyramid_images(ops, left, right, left_mask, right_mask)
    outs = [ops.empty((max(bh[t], 0), max(bw[t], 0), 3), np.float32) for t in range(n)]
    ptrs = (ctypes.c_void_p * max(n, 1))(*[ops.ptr(o) for o in outs])
    ops.call("pyramid_correlate_batch", ops.ptr(l), lw, lh, 0, ops.ptr(r), rw, rh, 0, ops.ptr(lm), 0, ops.ptr(rm), 0,
             ctypes.byref(P), n, bx, by, bw, bh, ptrs, None)
    return outs


SUBPIXEL_NONE, SUBPIXEL_PARABOLA, SUBPIXEL_LINEAR, SUBPIXEL_POLY4, SUBPIXEL_COSINE, SUBPIXEL_LC_BLEND = range(6)


def calc_disparity_sgm(cost_type, left_in, right_in, left_region, search_volume, kernel_size, use_mgm=False,
                       subpixel_mode=SUBPIXEL_LC_BLEND, search_buffer=(2, 2), memory_limit_mb=6000,
                       left_mask=None, right_mask=None, prev_disparity=None, p1=0, p2=0, ternary_census_threshold=5,
                       num_threads=1, with_subpixel=False, allow_block_cost=False, ctx=None):
    """vw::stereo::calc_disparity_sgm (src/vw/Stereo/SGM.h:360-375, SGM.cc:167-229).

    allow_block_cost (not an argument of the reference's function): cost types ABSOLUTE_DIFFERENCE / SQUARED_DIFFERENCE raise
    NoImplErr exactly as compute_disparity_costs throws (SGM.cc:1887-1892) unless this is True, which runs the code behind that
    throw — fill_costs_block's mean-abs-difference block cost (SGM.cc:1651-1738; p1 = 3, p2 = 250 by default).

    left_in / right_in: (rows, cols) float32; left_region: BBox2i inside the left image; search_volume = (sx, sy) is
    INCLUSIVE like the reference's (the right crop is left_region grown by search_volume, so (sx+1) x (sy+1) disparities
    are searched); kernel_size = (k, k) with k in {3, 5, 7, 9}; cost_type CENSUS_TRANSFORM / TERNARY_CENSUS_TRANSFORM.
    Masks / prev_disparity as in SemiGlobalMatcher::semi_global_matching_func (SGM.h:149-157).
    Returns the integer disparity (rows-k+1, cols-k+1, 3) int32; with_subpixel=True also returns the matcher's
    create_disparity_view_subpixel result (the reference hands the matcher back through matcher_ptr for that)."""
    kx, ky = int(kernel_size[0]), int(kernel_size[1])
    sx, sy = int(search_volume[0]), int(search_volume[1])
    if left_in.ndim != 2 or right_in.ndim != 2:
        raise ArgumentErr("calc_disparity_sgm: images must be 2-D (rows, cols)")
    if kx % 2 != 1 or ky % 2 != 1:
        raise ArgumentErr("calc_disparity_sgm: Kernel input not sized with odd values.")
    x0, y0 = left_region.min
    x1, y1 = left_region.max
    if x0 < 0 or y0 < 0 or x1 > left_in.shape[1] or y1 > left_in.shape[0]:
        raise ArgumentErr("calc_disparity_sgm: Region not inside left image.")
    lw, lh = x1 - x0, y1 - y0
    if kx > lw or ky > lh:
        raise ArgumentErr("calc_disparity_sgm: Kernel size too large of active region.")
    rx1, ry1 = min(x1 + sx, right_in.shape[1]), min(y1 + sy, right_in.shape[0])
    P = _lib.SgmParams(int(cost_type), int(bool(use_mgm)), kx, int(subpixel_mode), int(search_buffer[0]), int(search_buffer[1]),
                       int(memory_limit_mb), int(p1), int(p2), int(ternary_census_threshold), int(num_threads),
                       int(bool(allow_block_cost)))
    ow, oh = ctypes.c_int(), ctypes.c_int()
    cap = lw * lh
    ops = Operands("calc_disparity_sgm", left_in, ctx)
    l = ops.image(left_in[y0:y1, x0:x1], np.float32)
    r = ops.image(right_in[y0:ry1, x0:rx1], np.float32)
    lm, rm = _masks(ops, left_mask, right_mask)
    pd = ops.image(prev_disparity, np.int32)
    out = ops.empty((cap, 3), np.int32)
    sub = ops.empty((cap, 3), np.float32) if with_subpixel else None

    def sized(a):
        return (ops.ptr(a), 0, 0) if a is None else (ops.ptr(a), a.shape[1], a.shape[0])
    ops.call("calc_disparity_sgm", ctypes.byref(P), ops.ptr(l), lw, lh, 0, ops.ptr(r), r.shape[1], r.shape[0], 0, sx, sy,
             *sized(lm), *sized(rm), *sized(pd), ops.ptr(out), ops.ptr(sub), cap, ctypes.byref(ow), ctypes.byref(oh))
    n = ow.value * oh.value

    def result(a):     # a tensor stays a view of its cap-sized buffer, a numpy result lets go of it
        a = a[:n].reshape(oh.value, ow.value, 3)
        return a if ops.tensor else a.copy()
    return (result(out), result(sub)) if with_subpixel else result(out)


FILTER_SEMANTICS = {"reference": 0, "snapshot": 1}   # vwgpu_filter_semantics
MEDIAN_FILTER_MAX_KERNEL = TEXTURE_MEASURE_MAX_KERNEL = TEXTURE_FILTER_MAX_KERNEL = 31


def _filter_boxes(name, cols, rows, block_size, tiles):
    if tiles is not None:
        return np.ascontiguousarray(tiles, np.int32).reshape(-1, 4)
    if block_size is not None and (int(block_size[0]) <= 0 or int(block_size[1]) <= 0):
        raise ArgumentErr("%s: block_size must be positive" % name)
    return subpixel_tiles(cols, rows, block_size)


def _post_filter(name, disparity, dtype, semantics, block_size, tiles, ctx, stats, head, texture=None):
    """One of the three disparity filters of Algorithms.h through vwgpu_<name>[_dev]: `head` are the arguments between
    the input's stride and `semantics`, the texture image (if any) is passed in front of them."""
    if semantics not in FILTER_SEMANTICS:
        raise ArgumentErr("%s: semantics must be 'reference' or 'snapshot', not %r" % (name, semantics))
    if disparity.ndim != 3 or disparity.shape[2] != 3:
        raise ArgumentErr("%s: disparity must be (rows, cols, 3) {dx, dy, valid}" % name)
    h, w = int(disparity.shape[0]), int(disparity.shape[1])
    if texture is not None and (texture.ndim != 2 or tuple(texture.shape) != (h, w)):
        raise ArgumentErr("%s: the texture image and the disparity differ in size" % name)
    boxes = _filter_boxes(name, w, h, block_size, tiles)
    st = new_stats(1)
    ops = Operands(name, disparity, ctx)
    d = ops.image(disparity, dtype)
    tex = ops.image(texture, np.float32, same_device=True)
    out = ops.empty(d.shape, dtype)
    targs = () if tex is None else (ops.ptr(tex), 0)
    ops.call(name, ops.ptr(d), w, h, 0, *targs, *head, FILTER_SEMANTICS[semantics], boxes.ctypes.data, len(boxes), ops.ptr(out), 0,
             st if stats is not None else None)
    put_stats(stats, st)
    return out


def disparity_median_filter(disparity, kernel_size, semantics="reference", block_size=None, tiles=None, ctx=None,
                            stats=None):
    """vw::stereo::disparity_median_filter (src/vw/Stereo/Algorithms.cc:26-67) on a (rows, cols, 3) float32
    PixelMask<Vector2f> image {dx, dy, valid}; returns the filtered image (the input is not modified).

    semantics="reference" (default) is the reference's result: its loops run in place (`disparity_out = disparity_in`
    shares the buffer), so a window sees the filtered values above and to its left.  "snapshot" filters every pixel from
    the unmodified input.  Every box (block_size as in pyramid_subpixel, or tiles = [[x, y, w, h], ...], which must not
    overlap) is filtered as an image of its own.  numpy in -> numpy out (host entry); CUDA tensor in -> CUDA tensor out
    on the current stream, no pixel leaves the device.  kernel_size up to 31 (NoImplErr above).  stats (optional list)
    receives [pixels changed]."""
    if int(kernel_size) > MEDIAN_FILTER_MAX_KERNEL:
        raise core.NoImplErr("disparity_median_filter: kernel_size %d is larger than %d"
                             % (int(kernel_size), MEDIAN_FILTER_MAX_KERNEL))
    return _post_filter("disparity_median_filter", disparity, np.float32, semantics, block_size, tiles, ctx, stats,
                        (int(kernel_size),))


def disparity_neighbor_filter(disparity, semantics="reference", block_size=None, tiles=None, ctx=None, stats=None):
    """vw::stereo::disparity_neighbor_filter (src/vw/Stereo/Algorithms.cc:69-110) on a (rows, cols, 3) int32
    PixelMask<Vector2i> image: a pixel five or more of whose 8 neighbours agree takes their value, whatever its own
    validity.  semantics, boxes, devices and stats as disparity_median_filter."""
    return _post_filter("disparity_neighbor_filter", disparity, np.int32, semantics, block_size, tiles, ctx, stats, ())


def texture_preserving_disparity_filter(disparity, texture, texture_max=0.15, max_kernel_size=11, semantics="reference",
                                        block_size=None, tiles=None, ctx=None, stats=None):
    """vw::stereo::texture_preserving_disparity_filter<float> (src/vw/Stereo/Algorithms.h:215-281): every valid pixel is
    replaced by the mean of the valid pixels of a window whose size grows as the texture (a (rows, cols) float32 image,
    see texture_measure) falls below texture_max, up to max_kernel_size (at most 31, NoImplErr above).  semantics,
    boxes, devices and stats as disparity_median_filter."""
    if int(max_kernel_size) > TEXTURE_FILTER_MAX_KERNEL:
        raise core.NoImplErr("texture_preserving_disparity_filter: max_kernel_size %d is larger than %d"
                             % (int(max_kernel_size), TEXTURE_FILTER_MAX_KERNEL))
    return _post_filter("texture_preserving_disparity_filter", disparity, np.float32, semantics, block_size, tiles, ctx,
                        stats, (float(texture_max), int(max_kernel_size)), texture=texture)


def texture_measure(image, kernel_size=9, gradient_weight=0.5, stddev_weight=0.5, block_size=None, tiles=None, ctx=None,
                    stats=None):
    """vw::stereo::texture_measure (src/vw/Stereo/Algorithms.h:144-209) of a plain (rows, cols) float32 image: per pixel
    gradient_weight * mean(|dx| + |dy|) / 2 + stddev_weight * stddev over the kernel window of the edge-extended image.
    Returns a (rows, cols) float32 image (zero outside the boxes); numpy or CUDA tensor as the input.  kernel_size up to
    31 (NoImplErr above).  stats (optional list) receives [largest score], from which the reference's caller scales
    texture_max."""
    if image.ndim != 2:
        raise ArgumentErr("texture_measure: the image must be (rows, cols)")
    if int(kernel_size) > TEXTURE_MEASURE_MAX_KERNEL:
        raise core.NoImplErr("texture_measure: kernel_size %d is larger than %d" % (int(kernel_size), TEXTURE_MEASURE_MAX_KERNEL))
    h, w = int(image.shape[0]), int(image.shape[1])
    boxes = _filter_boxes("texture_measure", w, h, block_size, tiles)
    mx = ctypes.c_float(0)
    want = ctypes.addressof(mx) if stats is not None else None
    ops = Operands("texture_measure", image, ctx)
    img = ops.image(image, np.float32)
    out = ops.zeros((h, w), np.float32)     # zero outside the boxes
    ops.call("texture_measure", ops.ptr(img), w, h, 0, int(kernel_size), float(gradient_weight), float(stddev_weight),
             boxes.ctypes.data, len(boxes), ops.ptr(out), 0, want)
    if stats is not None:
        stats[:] = [mx.value]
    return out


OUTLIER_METHODS = {"mean": 0, "stddev": 1, "plane": 2}   # vwgpu_outlier_method
OUTLIER_SEMANTICS = {"reference": 0, "skip": 1}          # vwgpu_outlier_semantics
OUTLIER_MAX_HALF_KERNEL = 15
STD_DEV_IMAGE_MAX_KERNEL = 31
EDGE_EXTENSIONS = {"constant": 0, "zero": 1}             # vwgpu_edge


def _typed_disparity(ops, disparity):
    """An int32 (PixelMask<Vector2i>) or float32 (PixelMask<Vector2f>) image and its vwgpu_disparity_type."""
    d = ops.image(disparity, (np.int32, np.float32))
    return d, 0 if ops.dtype_of(d) == np.int32 else 1


def _rm_outliers(name, method, disparity, hh, hv, p0, p1, cleanup, semantics, ctx, stats):
    """One of the window filters of DisparityMap.h through vwgpu_rm_outliers[_dev], on either disparity pixel type."""
    if semantics not in OUTLIER_SEMANTICS:
        raise ArgumentErr("%s: semantics must be 'reference' or 'skip', not %r" % (name, semantics))
    if disparity.ndim != 3 or disparity.shape[2] != 3:
        raise ArgumentErr("%s: disparity must be (rows, cols, 3) {dx, dy, valid}" % name)
    h, w = int(disparity.shape[0]), int(disparity.shape[1])
    if int(hh) <= 0 or int(hv) <= 0:
        raise ArgumentErr("%s: half kernel sizes must be non-zero."
                          % ("RmOutliersUsingMeanFunc" if method == "mean" else "RmOutliersFunc"))
    if int(hh) > OUTLIER_MAX_HALF_KERNEL or int(hv) > OUTLIER_MAX_HALF_KERNEL:
        raise core.NoImplErr("%s: half kernel sizes %d, %d are larger than %d" % (name, int(hh), int(hv), OUTLIER_MAX_HALF_KERNEL))
    st = new_stats(2)
    ops = Operands(name, disparity, ctx)
    d, t = _typed_disparity(ops, disparity)
    out = ops.empty(d.shape, ops.dtype_of(d))
    ops.call("rm_outliers", OUTLIER_METHODS[method], t, ops.ptr(d), w, h, 0, int(hh), int(hv), float(p0), float(p1),
             int(bool(cleanup)), OUTLIER_SEMANTICS[semantics], ops.ptr(out), 0, st if stats is not None else None)
    put_stats(stats, st)
    return out


def rm_outliers_using_mean(disparity, half_h_kernel, half_v_kernel, max_mean_diff, semantics="reference", ctx=None,
                           stats=None):
    """vw::stereo::rm_outliers_using_mean (src/vw/Stereo/DisparityMap.h:444-578), rasterised over the whole image with
    the reference's ConstantEdgeExtension: a valid pixel farther than max_mean_diff from the mean of its window's valid
    pixels, gross outliers (magnitude above twice the 75th percentile) left out, becomes {0, 0, 0}.

    disparity: (rows, cols, 3) int32 (PixelMask<Vector2i>) or float32 (PixelMask<Vector2f>) {dx, dy, valid}; numpy in ->
    numpy out (host entry), CUDA tensor in -> CUDA tensor out on the current stream.  semantics="reference" (default)
    reproduces the reference's loop, in which a window row ends at its first pixel above the cutoff (the `continue` at
    :525 skips next_col()); "skip" leaves out only that pixel, as the comment at :492-496 describes.  Half kernel sizes
    1 .. 15 (NoImplErr above).  stats (optional list) receives [pixels rejected, 0]."""
    return _rm_outliers("rm_outliers_using_mean", "mean", disparity, half_h_kernel, half_v_kernel, max_mean_diff, 0.0, 0,
                        semantics, ctx, stats)


def disparity_cleanup_using_mean(disparity, h_half_kernel, v_half_kernel, max_mean_diff, semantics="reference", ctx=None,
                                 stats=None):
    """vw::stereo::disparity_cleanup_using_mean (src/vw/Stereo/DisparityMap.h:580-598): rm_outliers_using_mean followed by
    RmOutliersUsingThreshFunc(1, 1, 3.0, 0.2) on the inner view.  stats receives [rejected by the filter, rejected by
    the second pass]."""
    return _rm_outliers("disparity_cleanup_using_mean", "mean", disparity, h_half_kernel, v_half_kernel, max_mean_diff, 0.0, 1,
                        semantics, ctx, stats)


def rm_outliers_using_stddev(disparity, half_h_kernel, half_v_kernel, pixel_threshold, rejection_threshold, ctx=None,
                             stats=None):
    """vw::stereo::rm_outliers_using_stddev (src/vw/Stereo/DisparityMap.h:600-748): a valid pixel more than
    pixel_threshold standard deviations (at least rejection_threshold each) from its window's mean in dx or dy becomes
    {0, 0, 0}.  Pixel types, devices, limits and stats as rm_outliers_using_mean."""
    return _rm_outliers("rm_outliers_using_stddev", "stddev", disparity, half_h_kernel, half_v_kernel, pixel_threshold,
                        rejection_threshold, 0, "reference", ctx, stats)


def disparity_cleanup_using_stddev(disparity, h_half_kernel, v_half_kernel, pixel_threshold, rejection_threshold, ctx=None,
                                   stats=None):
    """vw::stereo::disparity_cleanup_using_stddev (src/vw/Stereo/DisparityMap.h:750-767): rm_outliers_using_stddev followed
    by RmOutliersUsingThreshFunc(1, 1, 3.0, 0.2) on the inner view."""
    return _rm_outliers("disparity_cleanup_using_stddev", "stddev", disparity, h_half_kernel, v_half_kernel, pixel_threshold,
                        rejection_threshold, 1, "reference", ctx, stats)


def rm_outliers_using_plane(disparity, half_h_kernel, half_v_kernel, pixel_threshold, rejection_threshold, ctx=None,
                            stats=None):
    """vw::stereo::rm_outliers_using_plane (src/vw/Stereo/DisparityMap.h:769-927, DisparityMap.cc:37-118): per channel a
    plane is fitted to the window's valid pixels; a pixel farther from it than pixel_threshold times the RMS distance of
    the window's pixels (at least rejection_threshold) becomes {0, 0, 0}; a window whose fit has an exactly zero pivot
    (points on a line) keeps its pixel.  The 3 x 3 solve is the elimination include/vwgpu.h specifies.  Pixel types,
    devices, limits and stats as rm_outliers_using_mean."""
    return _rm_outliers("rm_outliers_using_plane", "plane", disparity, half_h_kernel, half_v_kernel, pixel_threshold,
                        rejection_threshold, 0, "reference", ctx, stats)


def disparity_clean_using_plane(disparity, h_half_kernel, v_half_kernel, pixel_threshold, rejection_threshold, ctx=None,
                                stats=None):
    """vw::stereo::disparity_clean_using_plane (src/vw/Stereo/DisparityMap.h:929-947, the reference's spelling):
    rm_outliers_using_plane followed by RmOutliersUsingThreshFunc(1, 1, 3.0, 0.2) on the inner view."""
    return _rm_outliers("disparity_clean_using_plane", "plane", disparity, h_half_kernel, v_half_kernel, pixel_threshold,
                        rejection_threshold, 1, "reference", ctx, stats)


def std_dev_image(image, kernel_width, kernel_height, edge="zero", ctx=None):
    """vw::stereo::std_dev_image (src/vw/Stereo/DisparityMap.h:949-1014) of a plain (rows, cols) float32 image: per pixel
    the sum of squared differences from the window mean divided by kernel_width * kernel_height - 1 (the variance,
    despite the name), float accumulators, offsets -k/2 .. k/2 (an even size reads k + 1 samples; 1 x 1 gives NaN).
    edge: "zero" (the reference's default overload) or "constant".  numpy or CUDA tensor as the input.  Kernel sizes up
    to 31 (NoImplErr above)."""
    if image.ndim != 2:
        raise ArgumentErr("std_dev_image: the image must be (rows, cols)")
    if edge not in EDGE_EXTENSIONS:
        raise ArgumentErr("std_dev_image: edge must be 'zero' or 'constant', not %r" % (edge,))
    kw, kh = int(kernel_width), int(kernel_height)
    if kw <= 0 or kh <= 0:
        raise ArgumentErr("StdDevImageFunc: kernel sizes must be non-zero.")
    if kw > STD_DEV_IMAGE_MAX_KERNEL or kh > STD_DEV_IMAGE_MAX_KERNEL:
        raise core.NoImplErr("std_dev_image: kernel size %d x %d is larger than %d" % (kw, kh, STD_DEV_IMAGE_MAX_KERNEL))
    h, w = int(image.shape[0]), int(image.shape[1])
    ops = Operands("std_dev_image", image, ctx)
    img = ops.image(image, np.float32)
    out = ops.empty(img.shape, np.float32)
    ops.call("std_dev_image", ops.ptr(img), w, h, 0, kw, kh, EDGE_EXTENSIONS[edge], ops.ptr(out), 0)
    return out


RANGE_MASK_SEMANTICS = {"reference": 0, "fixed": 1}                     # vwgpu_range_mask_semantics
TRANSFORM_MODES = {"functor": 0, "subregion": 1, "subregion_round": 2}  # vwgpu_transform_mode


class HomographyTransform(object):
    """vw::HomographyTransform(H) (src/vw/Math/Transform.h:369-389): forward applies H, reverse applies inverse(H), each
    as w = m20 x + m21 y + m22 first, then the two quotients.  The inverse is a plain 3 x 3 adjugate divided by the
    determinant (the bits of the reference's inverse() are not pinned); transform_disparities(d, HomographyTransform(H))
    applies it, as TransformDisparitiesFunc calls reverse()."""

    def __init__(self, H):
        m = np.array(H, np.float64)
        if m.shape != (3, 3):
            raise ArgumentErr("HomographyTransform: the matrix must be 3 x 3")
        self.matrix = m
        a, b, c, d, e, f, g, h, i = [float(v) for v in m.reshape(9)]
        adj = np.array([[e * i - f * h, c * h - b * i, b * f - c * e],
                        [f * g - d * i, a * i - c * g, c * d - a * f],
                        [d * h - e * g, b * g - a * h, a * e - b * d]], np.float64)
        det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
        self.inverse_matrix = adj / det

    @staticmethod
    def _apply(m, p):
        x, y = float(p[0]), float(p[1])
        w = m[2, 0] * x + m[2, 1] * y + m[2, 2]
        return ((m[0, 0] * x + m[0, 1] * y + m[0, 2]) / w, (m[1, 0] * x + m[1, 1] * y + m[1, 2]) / w)

    def forward(self, p):
        return self._apply(self.matrix, p)

    def reverse(self, p):
        return self._apply(self.inverse_matrix, p)


def _disparity_map(ops, disparity):
    """Checks a {dx, dy, valid} map; returns (contiguous map, vwgpu_disparity_type, w, h)."""
    if disparity.ndim != 3 or disparity.shape[2] != 3:
        raise ArgumentErr("%s: disparity must be (rows, cols, 3) {dx, dy, valid}" % ops.name)
    if int(disparity.shape[0]) <= 0 or int(disparity.shape[1]) <= 0:
        raise ArgumentErr("%s: empty image" % ops.name)
    d, t = _typed_disparity(ops, disparity)
    return d, t, int(d.shape[1]), int(d.shape[0])


def get_disparity_range(disparity, ctx=None, device_result=False):
    """vw::stereo::get_disparity_range (src/vw/Stereo/DisparityMap.h:48-66): the box of the VALID disparities, returned
    as float32[4] {min.x, min.y, max.x, max.y} (BBox2f(min, max)); zeros when no pixel is valid.  A NaN component counts
    only in the first valid pixel in raster order (then both extrema of that component are NaN), as the reference's
    accumulator has it.  numpy in -> numpy out; CUDA tensor in -> numpy out after one synchronisation, or with
    device_result=True a CUDA float32[4] tensor without any host round trip."""
    ops = Operands("get_disparity_range", disparity, ctx)
    d, t, w, h = _disparity_map(ops, disparity)
    host = np.zeros(4, np.float32)
    # the two entries differ: the device one takes (range on the device, range on the host), the host one a single pointer
    if device_result:
        if not ops.tensor:
            raise ArgumentErr("get_disparity_range: device_result needs a CUDA tensor")
        out = ops.empty(4, np.float32)
        ops.call("get_disparity_range", t, ops.ptr(d), w, h, 0, ops.ptr(out), None)
        return out
    if ops.tensor:
        ops.call("get_disparity_range", t, ops.ptr(d), w, h, 0, None, host.ctypes.data)
    else:
        ops.call("get_disparity_range", t, ops.ptr(d), w, h, 0, host.ctypes.data)
    return host


def disparity_range_mask(disparity, min, max, semantics="reference", x0=0, y0=0, ctx=None, stats=None):
    """vw::stereo::disparity_range_mask(d, min, max) (src/vw/Stereo/DisparityMap.h:255-300): a valid pixel whose target
    location (x0 + x + dx, y0 + y + dy) leaves [min, max - 1) becomes {0, 0, 0}; min, max are (x, y) pairs in the
    pixel's channel type.  semantics="reference" (default) keeps the reference's comparison of the lower bound of y with
    min[0] (:279), "fixed" uses min[1].  x0, y0: the image coordinates of pixel (0, 0) of `disparity` (a tile of a
    larger map).  stats (optional list) receives [pixels masked]."""
    if semantics not in RANGE_MASK_SEMANTICS:
        raise ArgumentErr("disparity_range_mask: semantics must be 'reference' or 'fixed', not %r" % (semantics,))
    ops = Operands("disparity_range_mask", disparity, ctx)
    d, t, w, h = _disparity_map(ops, disparity)
    lo, hi = np.array(min, np.float64).reshape(-1), np.array(max, np.float64).reshape(-1)
    if lo.size != 2 or hi.size != 2:
        raise ArgumentErr("disparity_range_mask: min and max must be (x, y) pairs")
    out = ops.empty(d.shape, ops.dtype_of(d))
    st = new_stats(1)
    ops.call("disparity_range_mask", t, ops.ptr(d), w, h, 0, int(x0), int(y0), lo.ctypes.data, hi.ctypes.data,
             RANGE_MASK_SEMANTICS[semantics], ops.ptr(out), 0, st if stats is not None else None)
    put_stats(stats, st)
    return out


def _transform(name, disparity, matrix, mode, x0, y0, ctx):
    ops = Operands(name, disparity, ctx)
    d, t, w, h = _disparity_map(ops, disparity)
    m = np.ascontiguousarray(np.array(matrix, np.float64))
    if m.shape != (3, 3):
        raise ArgumentErr("%s: the matrix must be 3 x 3" % name)
    out = ops.empty(d.shape, ops.dtype_of(d))
    ops.call("transform_disparities", t, ops.ptr(d), w, h, 0, int(x0), int(y0), m.ctypes.data, TRANSFORM_MODES[mode],
             ops.ptr(out), 0)
    return out


def transform_disparities(disparity, matrix, x0=0, y0=0, ctx=None):
    """vw::stereo::transform_disparities(d, transform) (src/vw/Stereo/DisparityMap.h:1016-1057): every pixel's target
    point loc + d is mapped by the transform and the disparity becomes the mapped point minus loc, converted to the
    pixel's channel type (int32: toward zero).  Validity is copied; invalid pixels carry the transformed stored values.
    matrix: a HomographyTransform (its INVERSE is applied, as the reference's functor calls reverse()), or the 3 x 3
    matrix to apply as it is (row-major; last row (0, 0, 1) for a translation or an affine transform).  x0, y0: the
    image coordinates of pixel (0, 0) of `disparity`."""
    m = matrix.inverse_matrix if isinstance(matrix, HomographyTransform) else matrix
    return _transform("transform_disparities", disparity, m, "functor", x0, y0, ctx)


def transform_disparities_subregion(do_round, subregion, T, disparity, ctx=None):
    """vw::stereo::transform_disparities(do_round, subregion, T, disparity) (src/vw/Stereo/DisparityMap.h:1190-1224):
    with beg = subregion.min + (x, y), the disparity becomes HomographyTransform(T).forward(beg + d) - beg, rounded with
    round() when do_round; invalid pixels become {0, 0, 0}.  subregion: a BBox2i of the disparity's size."""
    x0, y0 = subregion.min
    x1, y1 = subregion.max
    if x1 - x0 != int(disparity.shape[1]) or y1 - y0 != int(disparity.shape[0]):
        raise ArgumentErr("transform_disparities: The sizes of subregion and disparity don't match.")
    return _transform("transform_disparities", disparity, T, "subregion_round" if do_round else "subregion", x0, y0, ctx)


def _resample(name, disparity, shape_of, dtype, ctx):
    ops = Operands(name, disparity, ctx)
    d, t, w, h = _disparity_map(ops, disparity)
    out = ops.empty(shape_of(h, w), ops.dtype_of(d) if dtype is None else dtype)
    ops.call(name, t, ops.ptr(d), w, h, 0, ops.ptr(out), 0)
    return out


def disparity_subsample(disparity, ctx=None):
    """vw::stereo::disparity_subsample (src/vw/Stereo/DisparityMap.h:1251-1322): (1 + (rows-1)//2, 1 + (cols-1)//2, 3);
    each pixel is the weighted mean (10 / 5 / 2) of the valid ones of nine taps around (2i, 2j) of the constant-extended
    map, divided by two; accumulated in double (float pixels) or int64 with an integer division (int32 pixels)."""
    return _resample("disparity_subsample", disparity, lambda h, w: (1 + (h - 1) // 2, 1 + (w - 1) // 2, 3), None, ctx)


def disparity_upsample(disparity, ctx=None):
    """vw::stereo::disparity_upsample (src/vw/Stereo/DisparityMap.h:1324-1358): (2 rows, 2 cols, 3), pixel (i, j) is
    pixel (i >> 1, j >> 1) times 2 with its validity."""
    return _resample("disparity_upsample", disparity, lambda h, w: (2 * h, 2 * w, 3), None, ctx)


def missing_pixel_image(disparity, ctx=None):
    """vw::stereo::missing_pixel_image (src/vw/Stereo/DisparityMap.h:68-87): (rows, cols, 3) uint8, (200, 200, 200)
    where the disparity is valid and (255, 0, 0) where it is not."""
    return _resample("missing_pixel_image", disparity, lambda h, w: (h, w, 3), np.uint8, ctx)


def intersect_mask_and_data(data, mask, ctx=None):
    """vw::stereo::intersect_mask_and_data (src/vw/Stereo/DisparityMap.h:1226-1249): the data pixel where it is valid,
    else the mask pixel where that is valid, else the data pixel.  Both maps have one type and size."""
    ops = Operands("intersect_mask_and_data", data, ctx)
    d, t, w, h = _disparity_map(ops, data)
    m, tm, wm, hm = _disparity_map(ops, mask)
    if (t, w, h) != (tm, wm, hm):
        raise ArgumentErr("intersect_mask_and_data: data and mask must have the same type and size")
    out = ops.empty(d.shape, ops.dtype_of(d))
    ops.call("intersect_mask_and_data", t, ops.ptr(d), 0, ops.ptr(m), 0, w, h, ops.ptr(out), 0)
    return out


def disparity_transform_image(right, disparity, ctx=None):
    """transform(right, DisparityTransform(disparity)) (src/vw/Stereo/DisparityMap.h:1164-1187): the (rows, cols)
    float32 right image seen from the left one, bilinear over zero edge extension; a pixel without a valid disparity
    (or outside the float32 disparity map, which may have another size) samples (-1, y) and becomes 0."""
    ops = Operands("disparity_transform_image", disparity, ctx)
    d, t, dw, dh = _disparity_map(ops, disparity)
    if t != 1:
        raise ArgumentErr("disparity_transform_image: the disparity must be float32 (PixelMask<Vector2f>)")
    if right.ndim != 2:
        raise ArgumentErr("disparity_transform_image: the image must be (rows, cols), on the same side as the disparity")
    r = ops.image(right, np.float32)
    rh, rw = int(r.shape[0]), int(r.shape[1])
    if rw <= 0 or rh <= 0:
        raise ArgumentErr("disparity_transform_image: empty image")
    out = ops.empty(r.shape, np.float32)
    ops.call("disparity_warp", ops.ptr(r), rw, rh, 0, ops.ptr(d), dw, dh, 0, ops.ptr(out), 0)
    return out


TRIANGULATE_SEMANTICS = {"view": 0, "model": 1}
DISPARITY_LAYOUTS = {"dxdyv": 0x000, "dxdy": 0x100, "dv": 0x200, "d": 0x300}
_LAYOUT_WORDS = {"dxdyv": 3, "dxdy": 2, "dv": 2, "d": 1}


def _tri_disparity(ops, disparity, layout):
    """A disparity image in one of the pixel forms DispHelper accepts (src/vw/Stereo/StereoView.h:37-53); returns
    (contiguous image, vwgpu_disparity_type, layout flag, w, h).  Never copies a tensor to the host."""
    name = ops.name
    if layout is None:
        if disparity.ndim == 2:
            layout = "d"
        elif disparity.ndim == 3 and int(disparity.shape[2]) in (2, 3):
            layout = "dxdyv" if int(disparity.shape[2]) == 3 else "dxdy"
    if layout not in DISPARITY_LAYOUTS:
        raise ArgumentErr("%s: disparity must be (rows, cols, 3) {dx, dy, valid}, (rows, cols, 2) {dx, dy} or, with layout='dv', "
                          "{d, valid}, or (rows, cols) {d}" % name)
    words = _LAYOUT_WORDS[layout]
    if (disparity.ndim != 2 if words == 1 else (disparity.ndim != 3 or int(disparity.shape[2]) != words)):
        raise ArgumentErr("%s: layout %r needs %d word(s) per pixel" % (name, layout, words))
    if int(disparity.shape[0]) <= 0 or int(disparity.shape[1]) <= 0:
        raise ArgumentErr("%s: empty image" % name)
    d, t = _typed_disparity(ops, disparity)
    return d, t, DISPARITY_LAYOUTS[layout], int(d.shape[1]), int(d.shape[0])


def _triangulate(name, disparity, cam1, cam2, x0, y0, angle_tol, semantics, layout, want_error, want_errvec, stats, ctx):
    if semantics not in TRIANGULATE_SEMANTICS:
        raise ArgumentErr("%s: semantics must be 'view' or 'model', not %r" % (name, semantics))
    ops = Operands(name, disparity, ctx)
    d, t, lay, w, h = _tri_disparity(ops, disparity, layout)
    c1, c2 = camera.descriptor_of(cam1), camera.descriptor_of(cam2)
    xyz = ops.empty((h, w, 3), np.float64)
    err = ops.empty((h, w), np.float64) if want_error else None
    vec = ops.empty((h, w, 3), np.float64) if want_errvec else None
    st, st_dev = None, None
    if stats is not None:
        if _is_tensor(stats):
            if not ops.tensor or stats.numel() != 3:
                raise ArgumentErr("%s: a device stats must be a contiguous int64[3] CUDA tensor, with a CUDA disparity" % name)
            st = ops.ptr(ops.image(stats, np.int64, in_place=True))     # contiguous, int64, CUDA: or ArgumentErr
        elif ops.tensor:
            st_dev = ops.empty(3, np.int64)
            st = ops.ptr(st_dev)
        else:
            st_host = _lib.TriangulateStats()
            st = ctypes.addressof(st_host)
    ops.call("stereo_triangulate", t, ops.ptr(d), w, h, 0, int(x0), int(y0), ctypes.byref(c1), ctypes.byref(c2), float(angle_tol),
             TRIANGULATE_SEMANTICS[semantics] | lay, ops.ptr(xyz), 0, ops.ptr(err), 0, ops.ptr(vec), 0, st)
    if stats is not None and not _is_tensor(stats):
        if ops.tensor:
            words = st_dev.cpu().numpy()
            stats[:] = [int(words[0]), float(words[1:2].view(np.float64)[0]), float(words[2:3].view(np.float64)[0])]
        else:
            stats[:] = [int(st_host.point_count), float(st_host.max_error), float(st_host.sum_error)]
    return xyz, err, vec


def stereo_triangulate(disparity, cam1, cam2, x0=0, y0=0, error=False, error_vector=False, stats=None, ctx=None, layout=None,
                       angle_tol=0.0):
    """vw::stereo::stereo_triangulate(disparity, cam1, cam2) rasterised (StereoView, src/vw/Stereo/StereoView.h:56-130): the
    (rows, cols, 3) float64 point image; the right pixel of a pair is Vector2(i, j) + Vector2((double)dx, (double)dy).
    Invalid disparities, pixel pairs with fewer than two rays and nearly parallel rays give (0, 0, 0); points behind a
    camera are reflected (StereoModel::operator(), src/vw/Stereo/StereoModel.cc:97-147).  cam1, cam2: camera.PinholeModel /
    camera.CAHVModel in any combination, or two camera.CAHVORModel, or two camera.CAHVOREModel (a CAHVORE ray that does not
    converge gives (0, 0, 0); any other pair with one of these raises NoImplErr).  x0, y0: the image coordinates of pixel (0, 0) of `disparity` (a tile of a larger map).
    error=True adds the (rows, cols) ray-intersection error norm_2(error vector), error_vector=True the (rows, cols, 3)
    vector between the closest points; the result is then a tuple (xyz[, error][, error_vector]).  StereoView::error() has
    no definition behind it in the reference; the error here is StereoModel's.
    disparity: (rows, cols, 3) {dx, dy, valid}, (rows, cols, 2) {dx, dy}, (rows, cols) {d}, or with layout="dv" a masked
    scalar (rows, cols, 2) {d, valid}; int32 or float32; numpy in -> numpy out, CUDA tensor in -> CUDA tensors out on the
    current torch stream.  stats: a list that receives [point_count, max_error, sum_error] (for tensors after one
    synchronisation), or an int64[3] CUDA tensor that receives the three 8-byte words without any (the last two are
    float64 bits: stats[1:].view(torch.float64))."""
    xyz, err, vec = _triangulate("stereo_triangulate", disparity, cam1, cam2, x0, y0, angle_tol, "view", layout, error, error_vector,
                                 stats, ctx)
    out = (xyz,) + ((err,) if error else ()) + ((vec,) if error_vector else ())
    return out[0] if len(out) == 1 else out


class StereoModel(object):
    """vw::stereo::StereoModel(cam1, cam2, angle_tol) for two cameras (src/vw/Stereo/StereoModel.h)."""

    def __init__(self, cam1, cam2, angle_tol=0.0):
        self.cam1, self.cam2, self.angle_tol = cam1, cam2, float(angle_tol)

    def __call__(self, disparity, x0=0, y0=0, stats=None, ctx=None, layout=None):
        """StereoModel::operator()(disparity_map, error) (src/vw/Stereo/StereoModel.cc:254-309): (xyz, error).  The right pixel is
        x + dx with x an int32 and dx a float (a float add, widened afterwards), and a point whose error is not >= 0
        becomes zero.  stats as in stereo_triangulate: the quantities this overload prints."""
        xyz, err, _ = _triangulate("StereoModel", disparity, self.cam1, self.cam2, x0, y0, self.angle_tol, "model", layout, True,
                                   False, stats, ctx)
        return xyz, err

    def convergence_angle(self, disparity, x0=0, y0=0, semantics="model", ctx=None, layout=None):
        """StereoModel::convergence_angle (src/vw/Stereo/StereoModel.cc:174-177) for every pixel pair of a disparity map:
        (rows, cols) float64 acos(dot(ray1, ray2)); 0 at invalid pixels."""
        if semantics not in TRIANGULATE_SEMANTICS:
            raise ArgumentErr("convergence_angle: semantics must be 'view' or 'model', not %r" % (semantics,))
        ops = Operands("convergence_angle", disparity, ctx)
        d, t, lay, w, h = _tri_disparity(ops, disparity, layout)
        c1, c2 = camera.descriptor_of(self.cam1), camera.descriptor_of(self.cam2)
        out = ops.empty((h, w), np.float64)
        ops.call("convergence_angle", t, ops.ptr(d), w, h, 0, int(x0), int(y0), ctypes.byref(c1), ctypes.byref(c2),
                 TRIANGULATE_SEMANTICS[semantics] | lay, ops.ptr(out), 0)
        return out


DBL_MAX = float(np.finfo(np.float64).max)


def universe_radius(points, origin, near_radius=0.0, far_radius=DBL_MAX, stats=None, ctx=None, out=None):
    """per_pixel_filter(points, UniverseRadiusFunc(origin, near_radius, far_radius)) (src/vw/Stereo/StereoView.h:139-222) on a
    (rows, cols, 3 | 4 | 6) float64 point image (xyz; xyz + error; xyz + error vector): a pixel whose xyz is zero becomes
    all zero, one whose distance from origin is below a non-zero near_radius or above a non-zero far_radius too.  Negative
    radii or near_radius > far_radius raise ArgumentErr, as the reference's constructor asserts.  stats (optional list)
    receives [total_points, rejected_points] (one synchronisation).  out=points filters in place."""
    if points.ndim != 3 or int(points.shape[2]) not in (3, 4, 6):
        raise ArgumentErr("universe_radius: points must be (rows, cols, 3 | 4 | 6)")
    ops = Operands("universe_radius", points, ctx)
    if ops.dtype_of(points) != np.float64:     # on either side: a numpy image of another type is not converted
        raise ArgumentErr("universe_radius: the points must be float64")
    p = ops.image(points, np.float64, in_place=out is points)
    if out is points:
        res = p
    elif out is not None:
        raise ArgumentErr("universe_radius: out must be None or the points themselves")
    else:
        res = ops.empty(tuple(p.shape), np.float64)
    h, w, ch = int(p.shape[0]), int(p.shape[1]), int(p.shape[2])
    if w <= 0 or h <= 0:
        raise ArgumentErr("universe_radius: empty image")
    o = np.array(origin, np.float64).reshape(-1)
    if o.size != 3:
        raise ArgumentErr("universe_radius: the origin must have three elements")
    st = new_stats(2)
    ops.call("universe_radius", ops.ptr(p), ch, w, h, 0, o.ctypes.data, float(near_radius), float(far_radius), ops.ptr(res), 0,
             st if stats is not None else None)
    put_stats(stats, st)
    return res


def epipolar_transformed_images(left, right, cam_l, cam_r, left_mask=None, right_mask=None, edge=(0, False), sizes=None,
                                check=True, ctx=None):
    """From two raw frames and their cameras to the epipolar-aligned pair (vw::camera::epipolar_transformed_images and
    epipolar_transformed_cahv_images, src/vw/Camera/EpipolarUtils.cc:79-200, with the cameras given as models): epipolar(),
    for pinholes resize_epipolar_cameras_to_fit over the whole frames, and one camera_transform per image.  Returns
    (left_out, right_out, epi_l, epi_r), or with masks (left_out, left_out_mask, right_out, right_out_mask, epi_l, epi_r);
    epi_l, epi_r are the rectified cameras stereo_triangulate takes for a disparity map of the aligned pair.
    cam_l, cam_r: two camera.PinholeModel (null or Tsai lens), two camera.CAHVModel, two camera.CAHVORModel or two
    camera.CAHVOREModel.  A CAHVOR or CAHVORE pair takes the .cahvor / .cahvore branch of epipolar_transformed_cahv_images
    (:173-188): each model is linearised at its frame's size (linearize_camera), epipolar() aligns the two CAHV results,
    and every frame goes from its raw model straight to its rectified CAHV camera.  (A distorted pinhole against a CAHV
    pair is two camera.camera_transform calls.)  The frames start at (0, 0): there is no AdjustedCameraModel for cropped
    inputs.
    sizes: ((cols, rows), (cols, rows)) of the results; by default what resize_epipolar_cameras_to_fit returns for
    pinholes, and the frames' own sizes for the CAHV family.  edge, check: as in camera.camera_transform."""
    if left.ndim != 2 or right.ndim != 2:
        raise ArgumentErr("epipolar_transformed_images: the images must be (rows, cols)")
    distorted = (camera.CAHVORModel, camera.CAHVOREModel)
    if isinstance(cam_l, distorted) or isinstance(cam_r, distorted):
        if type(cam_l) is not type(cam_r):
            raise ArgumentErr("epipolar_transformed_images: expected two CAHVORModels or two CAHVOREModels")
        lin_l = camera.linearize_camera(cam_l, (int(left.shape[1]), int(left.shape[0])))
        lin_r = camera.linearize_camera(cam_r, (int(right.shape[1]), int(right.shape[0])))
        epi_l, epi_r = camera.epipolar(lin_l, lin_r)
    else:
        epi_l, epi_r = camera.epipolar(cam_l, cam_r)
    if isinstance(cam_l, camera.PinholeModel):
        roi_l = BBox2i(0, 0, int(left.shape[1]), int(left.shape[0]))
        roi_r = BBox2i(0, 0, int(right.shape[1]), int(right.shape[0]))
        epi_l, epi_r, size_l, size_r = camera.resize_epipolar_cameras_to_fit(cam_l, cam_r, epi_l, epi_r, roi_l, roi_r, ctx=ctx)
    else:
        size_l, size_r = (int(left.shape[1]), int(left.shape[0])), (int(right.shape[1]), int(right.shape[0]))
    if sizes is not None:
        size_l, size_r = sizes
    out_l = camera.camera_transform(left, cam_l, epi_l, size=size_l, mask=left_mask, edge=edge, check=check, ctx=ctx)
    out_r = camera.camera_transform(right, cam_r, epi_r, size=size_r, mask=right_mask, edge=edge, check=check, ctx=ctx)
    flat = lambda o: o if isinstance(o, tuple) else (o,)      # noqa: E731
    return flat(out_l) + flat(out_r) + (epi_l, epi_r)


# epipolar_transformed_images is public like fast_box_sum, and like it not listed: it is a composition of camera.py's wrappers
__all__ = [
    "affine_subpixel",
    "bayes_em_subpixel",
    "corr_eval",
    "disparity_median_filter",
    "disparity_neighbor_filter",
    "texture_measure",
    "texture_preserving_disparity_filter",
    "lk_subpixel",
    "phase_subpixel",
    "pyramid_subpixel",
    "calc_disparity",
    "calc_disparity_sgm",
    "cross_corr_consistency_check",
    "parabola_subpixel",
    "rm_outliers_using_thresh",
    "disparity_cleanup_using_thresh",
    "disparity_mask",
    "disparity_blob_filter",
    "subdivide_regions",
    "pyramid_correlate",
    "pyramid_correlate_batch",
    "rm_outliers_using_mean",
    "rm_outliers_using_stddev",
    "rm_outliers_using_plane",
    "disparity_cleanup_using_mean",
    "disparity_cleanup_using_stddev",
    "disparity_clean_using_plane",
    "std_dev_image",
    "get_disparity_range",
    "disparity_range_mask",
    "transform_disparities",
    "transform_disparities_subregion",
    "HomographyTransform",
    "disparity_subsample",
    "disparity_upsample",
    "disparity_transform_image",
    "missing_pixel_image",
    "intersect_mask_and_data",
    "StereoModel",
    "stereo_triangulate",
    "universe_radius",
    "BBox2i",
    "CostFunctionType",
]
