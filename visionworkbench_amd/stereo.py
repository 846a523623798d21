"""Host-side mirror of the reference's stereo entry points on the block-matching hot path.

Same names, argument meaning and error behaviour as vw::stereo; every function hands
rasterised images to libvwgpu.so through the C ABI (include/vwgpu.h).  Inputs may be
  * torch CUDA tensors  -> device entry points, asynchronous on the current torch stream, result = CUDA tensor;
  * numpy arrays        -> host entry points (H2D, kernels, D2H), result = numpy array.
There is no CPU implementation here: without the HIP library or a GPU these functions raise.
"""
import ctypes

import numpy as np

from . import core
from .core import ArgumentErr, BBox2i, CostFunctionType

try:  # torch is plumbing (device memory, streams); the host-pointer path works without it
    import torch
except Exception:  # pragma: no cover
    torch = None


def _is_tensor(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _ctx_for(x, ctx):
    if ctx is not None:
        return ctx
    dev = x.device.index if _is_tensor(x) and x.is_cuda else 0
    return core.default_context(dev or 0)


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
    ctx = _ctx_for(left_in, ctx)
    lib = ctx._lib
    ow, oh = lw - kx + 1, lh - ky + 1
    if _is_tensor(left_in):
        if not (left_in.is_cuda and right_in.is_cuda):
            raise ArgumentErr("calc_disparity: torch inputs must be CUDA tensors (no CPU path)")
        if left_in.dtype != torch.float32 or right_in.dtype != torch.float32:
            raise ArgumentErr("calc_disparity: images must be float32")
        if left_in.stride(1) != 1 or right_in.stride(1) != 1:
            left_in, right_in = left_in.contiguous(), right_in.contiguous()
        l = left_in[y0:y1, x0:x1]
        r = right_in[y0:ry1, x0:rx1]
        out = torch.empty((max(oh, 0), max(ow, 0), 3), dtype=torch.int32, device=left_in.device)
        ctx.set_stream(torch.cuda.current_stream(left_in.device).cuda_stream)
        rc = lib.vwgpu_calc_disparity_dev(ctx._h, int(cost_type), l.data_ptr(), lw, lh, l.stride(0),
                                          r.data_ptr(), rx1 - x0, ry1 - y0, r.stride(0),
                                          kx, ky, sx, sy, out.data_ptr(), 0)
        ctx.check(rc)
        return out
    l = np.ascontiguousarray(left_in[y0:y1, x0:x1], np.float32)
    r = np.ascontiguousarray(right_in[y0:ry1, x0:rx1], np.float32)
    out = np.empty((max(oh, 0), max(ow, 0), 3), np.int32)
    rc = lib.vwgpu_calc_disparity(ctx._h, int(cost_type), l.ctypes.data, lw, lh, lw,
                                  r.ctypes.data, r.shape[1], r.shape[0], r.shape[1],
                                  kx, ky, sx, sy, out.ctypes.data, 0)
    ctx.check(rc)
    return out


def fast_box_sum(image, kernel, ctx=None):
    """vw::stereo::fast_box_sum<double>(image, kernel) (src/vw/Stereo/Algorithms.h:41-129): float64 sums of every
    kx x ky window, (rows-ky+1, cols-kx+1), formed in the reference's running-sum order (bit-identical for any float input)."""
    kx, ky = int(kernel[0]), int(kernel[1])
    if image.ndim != 2:
        raise ArgumentErr("fast_box_sum: the image must be 2-D (rows, cols)")
    h, w = image.shape
    ctx = _ctx_for(image, ctx)
    lib = ctx._lib
    if _is_tensor(image):
        if not image.is_cuda or image.dtype != torch.float32:
            raise ArgumentErr("fast_box_sum: torch input must be a float32 CUDA tensor (no CPU path)")
        if image.stride(1) != 1:
            image = image.contiguous()
        out = torch.empty((max(h - ky + 1, 0), max(w - kx + 1, 0)), dtype=torch.float64, device=image.device)
        ctx.set_stream(torch.cuda.current_stream(image.device).cuda_stream)
        ctx.check(lib.vwgpu_fast_box_sum_dev(ctx._h, image.data_ptr(), w, h, image.stride(0), kx, ky, out.data_ptr(), 0))
        return out
    img = np.ascontiguousarray(image, np.float32)
    out = np.empty((max(h - ky + 1, 0), max(w - kx + 1, 0)), np.float64)
    ctx.check(lib.vwgpu_fast_box_sum(ctx._h, img.ctypes.data, w, h, w, kx, ky, out.ctypes.data, 0))
    return out


def cross_corr_consistency_check(l2r, r2l, cross_corr_threshold, lr_disp_diff=None, ul_corner_offset=(0, 0), ctx=None):
    """vw::stereo::cross_corr_consistency_check (src/vw/Stereo/Correlate.cc:1441-1502), IN PLACE on l2r.

    l2r, r2l: (rows, cols, 3) int32 PixelMask<Vector2i> images.  lr_disp_diff (optional, modified in place): (rows, cols, 2)
    float32 PixelMask<float> {value, valid}; every kept pixel stores its discrepancy at (c, r) + ul_corner_offset."""
    ctx = _ctx_for(l2r, ctx)
    lib = ctx._lib
    if lr_disp_diff is not None:
        ux, uy = int(ul_corner_offset[0]), int(ul_corner_offset[1])
        if lr_disp_diff.ndim != 3 or lr_disp_diff.shape[2] != 2:
            raise ArgumentErr("cross_corr_consistency_check: lr_disp_diff must be (rows, cols, 2) float32")
        dr, dc = lr_disp_diff.shape[:2]
        if _is_tensor(l2r):
            if not (l2r.is_cuda and r2l.is_cuda and lr_disp_diff.is_cuda and l2r.is_contiguous() and r2l.is_contiguous()
                    and lr_disp_diff.is_contiguous() and lr_disp_diff.dtype == torch.float32):
                raise ArgumentErr("cross_corr_consistency_check: contiguous CUDA tensors required")
            ctx.set_stream(torch.cuda.current_stream(l2r.device).cuda_stream)
            ctx.check(lib.vwgpu_cross_corr_consistency_check_diff_dev(ctx._h, l2r.data_ptr(), l2r.shape[1], l2r.shape[0], 0, r2l.data_ptr(),
                                                                      r2l.shape[1], r2l.shape[0], 0, float(cross_corr_threshold),
                                                                      lr_disp_diff.data_ptr(), dc, dr, 0, ux, uy))
            return l2r
        if not (l2r.flags.c_contiguous and l2r.dtype == np.int32 and lr_disp_diff.flags.c_contiguous and lr_disp_diff.dtype == np.float32):
            raise ArgumentErr("cross_corr_consistency_check: contiguous int32 / float32 arrays required (modified in place)")
        r2l = np.ascontiguousarray(r2l, np.int32)
        ctx.check(lib.vwgpu_cross_corr_consistency_check_diff(ctx._h, l2r.ctypes.data, l2r.shape[1], l2r.shape[0], 0, r2l.ctypes.data,
                                                              r2l.shape[1], r2l.shape[0], 0, float(cross_corr_threshold),
                                                              lr_disp_diff.ctypes.data, dc, dr, 0, ux, uy))
        return l2r
    if _is_tensor(l2r):
        if not (l2r.is_cuda and r2l.is_cuda and l2r.is_contiguous() and r2l.is_contiguous()):
            raise ArgumentErr("cross_corr_consistency_check: contiguous CUDA tensors required")
        ctx.set_stream(torch.cuda.current_stream(l2r.device).cuda_stream)
        rc = lib.vwgpu_cross_corr_consistency_check_dev(ctx._h, l2r.data_ptr(), l2r.shape[1], l2r.shape[0], 0,
                                                        r2l.data_ptr(), r2l.shape[1], r2l.shape[0], 0,
                                                        float(cross_corr_threshold))
        ctx.check(rc)
        return l2r
    if not (l2r.flags.c_contiguous and l2r.dtype == np.int32):
        raise ArgumentErr("cross_corr_consistency_check: l2r must be a contiguous int32 array (modified in place)")
    r2l = np.ascontiguousarray(r2l, np.int32)
    rc = lib.vwgpu_cross_corr_consistency_check(ctx._h, l2r.ctypes.data, l2r.shape[1], l2r.shape[0], 0,
                                                r2l.ctypes.data, r2l.shape[1], r2l.shape[0], 0,
                                                float(cross_corr_threshold))
    ctx.check(rc)
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
    ctx = _ctx_for(left_image, ctx)
    lib = ctx._lib
    if _is_tensor(left_image):
        d, l, r = disparity.contiguous(), left_image.contiguous(), right_image.contiguous()
        if not (d.is_cuda and l.is_cuda and r.is_cuda) or d.dtype != torch.float32:
            raise ArgumentErr("parabola_subpixel: float32 CUDA tensors required")
        out = torch.empty_like(d)
        ctx.set_stream(torch.cuda.current_stream(l.device).cuda_stream)
        ctx.check(lib.vwgpu_parabola_subpixel_dev(ctx._h, d.data_ptr(), w, h, 0, l.data_ptr(), 0, r.data_ptr(), rw, rh, 0,
                                                  int(prefilter_mode), float(prefilter_width), kx, ky, out.data_ptr(), 0))
        return out
    d = np.ascontiguousarray(disparity, np.float32)
    l = np.ascontiguousarray(left_image, np.float32)
    r = np.ascontiguousarray(right_image, np.float32)
    out = np.empty_like(d)
    ctx.check(lib.vwgpu_parabola_subpixel(ctx._h, d.ctypes.data, w, h, 0, l.ctypes.data, 0, r.ctypes.data, rw, rh, 0,
                                          int(prefilter_mode), float(prefilter_width), kx, ky, out.ctypes.data, 0))
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
    st = (ctypes.c_longlong * 3)()
    ctx = _ctx_for(left, ctx)
    lib = ctx._lib
    if _is_tensor(left):
        d, l, r = disparity.contiguous(), left.contiguous(), right.contiguous()
        if not (d.is_cuda and l.is_cuda and r.is_cuda) or d.dtype != torch.float32 or l.dtype != torch.float32 \
                or r.dtype != torch.float32:
            raise ArgumentErr("%s: float32 CUDA tensors required" % name)
        out = torch.zeros_like(d)
        ctx.set_stream(torch.cuda.current_stream(l.device).cuda_stream)
        ctx.check(getattr(lib, "vwgpu_%s_dev" % entry)(ctx._h, d.data_ptr(), w, h, 0, l.data_ptr(), 0, r.data_ptr(), rw, rh, 0,
                                                 int(prefilter_mode), float(prefilter_width), kx, ky, int(max_pyramid_levels),
                                                 selector, tiles.ctypes.data, len(tiles), out.data_ptr(), 0, st))
    else:
        d = np.ascontiguousarray(disparity, np.float32)
        l = np.ascontiguousarray(left, np.float32)
        r = np.ascontiguousarray(right, np.float32)
        out = np.zeros_like(d)
        ctx.check(getattr(lib, "vwgpu_" + entry)(ctx._h, d.ctypes.data, w, h, 0, l.ctypes.data, 0, r.ctypes.data, rw, rh, 0,
                                             int(prefilter_mode), float(prefilter_width), kx, ky, int(max_pyramid_levels),
                                             selector, tiles.ctypes.data, len(tiles), out.ctypes.data, 0, st))
    if stats is not None:
        stats[:] = list(st)
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
    st = (ctypes.c_longlong * 4)()
    if _is_tensor(left):
        # every operand, the masks included, must live on the left image's device: the kernels read them all
        operands = [(disparity, True), (left, True), (right, True), (left_valid, False), (right_valid, False)]
        for x, is_float in operands:
            if x is not None and (not _is_tensor(x) or not x.is_cuda or x.device != left.device
                                  or (is_float and x.dtype != torch.float32)):
                raise ArgumentErr("corr_eval: float32 images and disparity, and masks, as CUDA tensors on %s" % left.device)
    elif any(_is_tensor(x) for x in (disparity, right, left_valid, right_valid)):
        raise ArgumentErr("corr_eval: with a numpy left image every operand must be a numpy array")
    ctx = _ctx_for(left, ctx)
    lib = ctx._lib
    args = (CORR_EVAL_METRICS[metric], int(sample_rate), 1 if round_to_int else 0, int(prefilter_mode),
            float(prefilter_kernel_width), tiles.ctypes.data, len(tiles))
    if _is_tensor(left):
        d, l, r = disparity.contiguous(), left.contiguous(), right.contiguous()
        lv = None if left_valid is None else (left_valid != 0).to(torch.uint8).contiguous()
        rv = None if right_valid is None else (right_valid != 0).to(torch.uint8).contiguous()
        out = torch.zeros((h, w, 2), dtype=torch.float32, device=l.device)
        ctx.set_stream(torch.cuda.current_stream(l.device).cuda_stream)
        ctx.check(lib.vwgpu_corr_eval_dev(ctx._h, d.data_ptr(), w, h, 0, l.data_ptr(), None if lv is None else lv.data_ptr(), 0,
                                          r.data_ptr(), None if rv is None else rv.data_ptr(), rw, rh, 0, kx, ky, *args,
                                          out.data_ptr(), 0, st))
    else:
        d = np.ascontiguousarray(disparity, np.float32)
        l = np.ascontiguousarray(left, np.float32)
        r = np.ascontiguousarray(right, np.float32)
        lv = None if left_valid is None else np.ascontiguousarray(np.asarray(left_valid) != 0, np.uint8)
        rv = None if right_valid is None else np.ascontiguousarray(np.asarray(right_valid) != 0, np.uint8)
        out = np.zeros((h, w, 2), np.float32)
        ctx.check(lib.vwgpu_corr_eval(ctx._h, d.ctypes.data, w, h, 0, l.ctypes.data, None if lv is None else lv.ctypes.data, 0,
                                      r.ctypes.data, None if rv is None else rv.ctypes.data, rw, rh, 0, kx, ky, *args,
                                      out.ctypes.data, 0, st))
    if stats is not None:
        stats[:] = list(st)
    return out


def _filter_call(name, disparity, hh, hv, pthr, rthr, cleanup, ctx):
    if disparity.ndim != 3 or disparity.shape[2] != 3:
        raise ArgumentErr("%s: disparity must be (rows, cols, 3) int32" % name)
    h, w = disparity.shape[:2]
    if hh <= 0 or hv <= 0:
        raise ArgumentErr("RmOutliersFunc: half kernel sizes must be non-zero.")
    ctx = _ctx_for(disparity, ctx)
    lib = ctx._lib
    if _is_tensor(disparity):
        if not disparity.is_cuda or disparity.dtype != torch.int32:
            raise ArgumentErr("%s: int32 CUDA tensor required" % name)
        d = disparity.contiguous()
        out = torch.empty_like(d)
        ctx.set_stream(torch.cuda.current_stream(d.device).cuda_stream)
        ctx.check(lib.vwgpu_disparity_filter_dev(ctx._h, d.data_ptr(), w, h, int(hh), int(hv), float(pthr), float(rthr),
                                                 int(cleanup), out.data_ptr()))
        return out
    d = np.ascontiguousarray(disparity, np.int32)
    out = np.empty_like(d)
    ctx.check(lib.vwgpu_disparity_filter(ctx._h, d.ctypes.data, w, h, int(hh), int(hv), float(pthr), float(rthr),
                                         int(cleanup), out.ctypes.data))
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
    ctx = _ctx_for(disparity, ctx)
    lib = ctx._lib
    if _is_tensor(disparity):
        if not (disparity.is_cuda and left_mask.is_cuda and right_mask.is_cuda) or disparity.dtype != torch.int32:
            raise ArgumentErr("disparity_mask: int32 / uint8 CUDA tensors required")
        out = disparity.contiguous().clone()
        m1, m2 = left_mask.contiguous(), right_mask.contiguous()
        ctx.set_stream(torch.cuda.current_stream(out.device).cuda_stream)
        ctx.check(lib.vwgpu_disparity_mask_dev(ctx._h, out.data_ptr(), w, h, m1.data_ptr(), m2.data_ptr(), rmw, rmh))
        return out
    out = np.array(disparity, np.int32, order="C", copy=True)
    m1 = np.ascontiguousarray(left_mask, np.uint8)
    m2 = np.ascontiguousarray(right_mask, np.uint8)
    ctx.check(lib.vwgpu_disparity_mask(ctx._h, out.ctypes.data, w, h, m1.ctypes.data, m2.ctypes.data, rmw, rmh))
    return out


def disparity_blob_filter(disparity, max_blob_area, ctx=None):
    """PyramidCorrelationView::disparity_blob_filter at one level (src/vw/Stereo/CorrelationView.cc:242-271): erase every
    8-connected component of valid pixels with at most max_blob_area pixels.  Returns a new image."""
    if disparity.ndim != 3 or disparity.shape[2] != 3:
        raise ArgumentErr("disparity_blob_filter: disparity must be (rows, cols, 3) int32")
    h, w = disparity.shape[:2]
    ctx = _ctx_for(disparity, ctx)
    lib = ctx._lib
    if _is_tensor(disparity):
        if not disparity.is_cuda or disparity.dtype != torch.int32:
            raise ArgumentErr("disparity_blob_filter: int32 CUDA tensor required")
        out = disparity.contiguous().clone()
        ctx.set_stream(torch.cuda.current_stream(out.device).cuda_stream)
        ctx.check(lib.vwgpu_disparity_blob_filter_dev(ctx._h, out.data_ptr(), w, h, int(max_blob_area)))
        return out
    out = np.array(disparity, np.int32, order="C", copy=True)
    ctx.check(lib.vwgpu_disparity_blob_filter(ctx._h, out.ctypes.data, w, h, int(max_blob_area)))
    return out


def subdivide_regions(disparity, kernel_size):
    """vw::stereo::subdivide_regions(disparity, bounding_box(disparity), list, kernel_size)
    (src/vw/Stereo/Correlation.cc:139-328).  Host logic (the zone scheduler of pyramid_correlate) on a numpy
    PixelMask<Vector2i> image; returns [(region BBox2i, disparity_range BBox2i), ...] in the reference's order."""
    from . import _lib
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
    from ._lib import PyramidParams
    if left.ndim != 2 or right.ndim != 2:
        raise ArgumentErr("pyramid_correlate: images must be 2-D (rows, cols)")
    lh, lw = left.shape
    rh, rw = right.shape
    if bbox is None:
        bbox = BBox2i(0, 0, lw, lh)
    (bx, by), (bx1, by1) = bbox.min, bbox.max
    P = PyramidParams(int(prefilter_mode), float(prefilter_width),
                      int(search_region.min[0]), int(search_region.min[1]), int(search_region.max[0]), int(search_region.max[1]),
                      int(kernel_size[0]), int(kernel_size[1]), int(cost_type), int(corr_timeout), float(seconds_per_op),
                      float(consistency_threshold), int(min_consistency_level), int(filter_half_kernel),
                      int(max_pyramid_levels), int(algorithm), int(blob_filter_area), int(sgm_subpixel_mode),
                      int(sgm_search_buffer[0]), int(sgm_search_buffer[1]), int(memory_limit_mb), int(sgm_num_threads),
                      None, 0, 0, 0, int(region_ul[0]), int(region_ul[1]))
    if lr_disp_diff is not None:
        if lr_disp_diff.ndim != 3 or lr_disp_diff.shape[2] != 2:
            raise ArgumentErr("pyramid_correlate: lr_disp_diff must be (rows, cols, 2) float32")
        if _is_tensor(lr_disp_diff) != _is_tensor(left):
            raise ArgumentErr("pyramid_correlate: lr_disp_diff must live where the images live")
        ok = (lr_disp_diff.is_cuda and lr_disp_diff.is_contiguous() and lr_disp_diff.dtype == torch.float32) if _is_tensor(lr_disp_diff) \
            else (lr_disp_diff.flags.c_contiguous and lr_disp_diff.dtype == np.float32)
        if not ok:
            raise ArgumentErr("pyramid_correlate: lr_disp_diff must be contiguous float32")
        P.lr_disp_diff = lr_disp_diff.data_ptr() if _is_tensor(lr_disp_diff) else lr_disp_diff.ctypes.data
        P.lr_disp_diff_rows, P.lr_disp_diff_cols = int(lr_disp_diff.shape[0]), int(lr_disp_diff.shape[1])
    ctx = _ctx_for(left, ctx)
    lib = ctx._lib
    bw, bh = bx1 - bx, by1 - by
    if _is_tensor(left):
        if not (left.is_cuda and right.is_cuda) or left.dtype != torch.float32 or right.dtype != torch.float32:
            raise ArgumentErr("pyramid_correlate: float32 CUDA tensors required (no CPU path)")
        l, r = left.contiguous(), right.contiguous()
        lm = left_mask.contiguous() if left_mask is not None else None
        rm = right_mask.contiguous() if right_mask is not None else None
        for m, shp in ((lm, l.shape), (rm, r.shape)):
            if m is not None and (m.dtype != torch.uint8 or tuple(m.shape) != tuple(shp) or not m.is_cuda):
                raise ArgumentErr("pyramid_correlate: masks must be uint8 CUDA tensors of the image size")
        out = torch.empty((max(bh, 0), max(bw, 0), 3), dtype=torch.float32, device=l.device)
        ctx.set_stream(torch.cuda.current_stream(l.device).cuda_stream)
        ctx.check(lib.vwgpu_pyramid_correlate_dev(ctx._h, l.data_ptr(), lw, lh, 0, r.data_ptr(), rw, rh, 0,
                                                  lm.data_ptr() if lm is not None else None, 0,
                                                  rm.data_ptr() if rm is not None else None, 0,
                                                  ctypes.byref(P), bx, by, bw, bh, out.data_ptr(), 0))
        return out
    l = np.ascontiguousarray(left, np.float32)
    r = np.ascontiguousarray(right, np.float32)
    lm = np.ascontiguousarray(left_mask, np.uint8) if left_mask is not None else None
    rm = np.ascontiguousarray(right_mask, np.uint8) if right_mask is not None else None
    for m, shp in ((lm, l.shape), (rm, r.shape)):
        if m is not None and tuple(m.shape) != tuple(shp):
            raise ArgumentErr("pyramid_correlate: masks must have the image size")
    out = np.empty((max(bh, 0), max(bw, 0), 3), np.float32)
    ctx.check(lib.vwgpu_pyramid_correlate(ctx._h, l.ctypes.data, lw, lh, 0, r.ctypes.data, rw, rh, 0,
                                          lm.ctypes.data if lm is not None else None, 0,
                                          rm.ctypes.data if rm is not None else None, 0,
                                          ctypes.byref(P), bx, by, bw, bh, out.ctypes.data, 0))
    return out


def pyramid_correlate_batch(left, right, left_mask, right_mask, prefilter_mode, prefilter_width, search_region, kernel_size, cost_type,
                            bboxes, corr_timeout=0, seconds_per_op=0.0, consistency_threshold=-1.0, min_consistency_level=0,
                            filter_half_kernel=0, max_pyramid_levels=5, algorithm=0, collar_size=0, sgm_subpixel_mode=5,
                            sgm_search_buffer=(2, 2), memory_limit_mb=6000, blob_filter_area=0, sgm_num_threads=1, ctx=None):
    """Several tiles (`bboxes`: a list of BBox2i) of vw::stereo::pyramid_correlate in ONE call: what the reference's block rasteriser hands
    to its tile threads one at a time (src/vw/Image/ImageIO.h:228-251).  Runs of consecutive tiles of equal size go through the pyramid
    level loop together (vwgpu_pyramid_correlate_batch[_dev], include/vwgpu.h); every tile's result is identical to pyramid_correlate on
    that tile.  Returns a list of (rows, cols, 3) float32 PixelMask<Vector2f> images: CUDA tensors for CUDA inputs, numpy arrays otherwise."""
    from ._lib import PyramidParams
    if left.ndim != 2 or right.ndim != 2:
        raise ArgumentErr("pyramid_correlate: images must be 2-D (rows, cols)")
    lh, lw = left.shape
    rh, rw = right.shape
    P = PyramidParams(int(prefilter_mode), float(prefilter_width),
                      int(search_region.min[0]), int(search_region.min[1]), int(search_region.max[0]), int(search_region.max[1]),
                      int(kernel_size[0]), int(kernel_size[1]), int(cost_type), int(corr_timeout), float(seconds_per_op),
                      float(consistency_threshold), int(min_consistency_level), int(filter_half_kernel),
                      int(max_pyramid_levels), int(algorithm), int(blob_filter_area), int(sgm_subpixel_mode),
                      int(sgm_search_buffer[0]), int(sgm_search_buffer[1]), int(memory_limit_mb), int(sgm_num_threads),
                      None, 0, 0, 0, 0, 0)
    n = len(bboxes)
    IA = ctypes.c_int * max(n, 1)
    bx = IA(*[int(b.min[0]) for b in bboxes]); by = IA(*[int(b.min[1]) for b in bboxes])
    bw = IA(*[int(b.max[0] - b.min[0]) for b in bboxes]); bh = IA(*[int(b.max[1] - b.min[1]) for b in bboxes])
    ctx = _ctx_for(left, ctx)
    lib = ctx._lib
    PA = ctypes.c_void_p * max(n, 1)
    if _is_tensor(left):
        if not (left.is_cuda and right.is_cuda) or left.dtype != torch.float32 or right.dtype != torch.float32:
            raise ArgumentErr("pyramid_correlate: float32 CUDA tensors required (no CPU path)")
        l, r = left.contiguous(), right.contiguous()
        lm = left_mask.contiguous() if left_mask is not None else None
        rm = right_mask.contiguous() if right_mask is not None else None
        for m, shp in ((lm, l.shape), (rm, r.shape)):
            if m is not None and (m.dtype != torch.uint8 or tuple(m.shape) != tuple(shp) or not m.is_cuda):
                raise ArgumentErr("pyramid_correlate: masks must be uint8 CUDA tensors of the image size")
        outs = [torch.empty((max(bh[t], 0), max(bw[t], 0), 3), dtype=torch.float32, device=l.device) for t in range(n)]
        ptrs = PA(*[o.data_ptr() for o in outs])
        ctx.set_stream(torch.cuda.current_stream(l.device).cuda_stream)
        ctx.check(lib.vwgpu_pyramid_correlate_batch_dev(ctx._h, l.data_ptr(), lw, lh, 0, r.data_ptr(), rw, rh, 0,
                                                        lm.data_ptr() if lm is not None else None, 0, rm.data_ptr() if rm is not None else None, 0,
                                                        ctypes.byref(P), n, bx, by, bw, bh, ptrs, None))
        return outs
    l = np.ascontiguousarray(left, np.float32)
    r = np.ascontiguousarray(right, np.float32)
    lm = np.ascontiguousarray(left_mask, np.uint8) if left_mask is not None else None
    rm = np.ascontiguousarray(right_mask, np.uint8) if right_mask is not None else None
    for m, shp in ((lm, l.shape), (rm, r.shape)):
        if m is not None and tuple(m.shape) != tuple(shp):
            raise ArgumentErr("pyramid_correlate: masks must have the image size")
    outs = [np.empty((max(bh[t], 0), max(bw[t], 0), 3), np.float32) for t in range(n)]
    ptrs = PA(*[o.ctypes.data for o in outs])
    ctx.check(lib.vwgpu_pyramid_correlate_batch(ctx._h, l.ctypes.data, lw, lh, 0, r.ctypes.data, rw, rh, 0,
                                                lm.ctypes.data if lm is not None else None, 0, rm.ctypes.data if rm is not None else None, 0,
                                                ctypes.byref(P), n, bx, by, bw, bh, ptrs, None))
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
    from ._lib import SgmParams
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
    P = SgmParams(int(cost_type), int(bool(use_mgm)), kx, int(subpixel_mode), int(search_buffer[0]), int(search_buffer[1]),
                  int(memory_limit_mb), int(p1), int(p2), int(ternary_census_threshold), int(num_threads), int(bool(allow_block_cost)))
    ctx = _ctx_for(left_in, ctx)
    lib = ctx._lib
    ow, oh = ctypes.c_int(), ctypes.c_int()
    cap = lw * lh

    def shape2(a):
        return (0, 0) if a is None else (a.shape[1], a.shape[0])
    if _is_tensor(left_in):
        if not (left_in.is_cuda and right_in.is_cuda) or left_in.dtype != torch.float32 or right_in.dtype != torch.float32:
            raise ArgumentErr("calc_disparity_sgm: float32 CUDA tensors required (no CPU path)")
        l = left_in[y0:y1, x0:x1].contiguous()
        r = right_in[y0:ry1, x0:rx1].contiguous()
        lm = left_mask.contiguous() if left_mask is not None else None
        rm = right_mask.contiguous() if right_mask is not None else None
        pd = prev_disparity.contiguous() if prev_disparity is not None else None
        out = torch.empty((cap, 3), dtype=torch.int32, device=l.device)
        sub = torch.empty((cap, 3), dtype=torch.float32, device=l.device) if with_subpixel else None
        ctx.set_stream(torch.cuda.current_stream(l.device).cuda_stream)
        ptr = lambda t: t.data_ptr() if t is not None else None
        ctx.check(lib.vwgpu_calc_disparity_sgm_dev(ctx._h, ctypes.byref(P), l.data_ptr(), lw, lh, 0, r.data_ptr(), r.shape[1], r.shape[0], 0,
                                                   sx, sy, ptr(lm), *shape2(lm), ptr(rm), *shape2(rm), ptr(pd), *shape2(pd),
                                                   out.data_ptr(), ptr(sub), cap, ctypes.byref(ow), ctypes.byref(oh)))
        n = ow.value * oh.value
        res = out[:n].reshape(oh.value, ow.value, 3)
        return (res, sub[:n].reshape(oh.value, ow.value, 3)) if with_subpixel else res
    l = np.ascontiguousarray(left_in[y0:y1, x0:x1], np.float32)
    r = np.ascontiguousarray(right_in[y0:ry1, x0:rx1], np.float32)
    lm = np.ascontiguousarray(left_mask, np.uint8) if left_mask is not None else None
    rm = np.ascontiguousarray(right_mask, np.uint8) if right_mask is not None else None
    pd = np.ascontiguousarray(prev_disparity, np.int32) if prev_disparity is not None else None
    out = np.empty((cap, 3), np.int32)
    sub = np.empty((cap, 3), np.float32) if with_subpixel else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    ctx.check(lib.vwgpu_calc_disparity_sgm(ctx._h, ctypes.byref(P), l.ctypes.data, lw, lh, 0, r.ctypes.data, r.shape[1], r.shape[0], 0,
                                           sx, sy, ptr(lm), *shape2(lm), ptr(rm), *shape2(rm), ptr(pd), *shape2(pd),
                                           out.ctypes.data, ptr(sub), cap, ctypes.byref(ow), ctypes.byref(oh)))
    n = ow.value * oh.value
    res = out[:n].reshape(oh.value, ow.value, 3).copy()
    return (res, sub[:n].reshape(oh.value, ow.value, 3).copy()) if with_subpixel else res


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
    st = (ctypes.c_longlong * 1)()
    ctx = _ctx_for(disparity, ctx)
    lib = ctx._lib
    sem = FILTER_SEMANTICS[semantics]
    want_stats = st if stats is not None else None
    if _is_tensor(disparity):
        tdt = torch.float32 if dtype == np.float32 else torch.int32
        if not disparity.is_cuda or disparity.dtype != tdt:
            raise ArgumentErr("%s: the disparity must be a %s CUDA tensor" % (name, tdt))
        if texture is not None and (not _is_tensor(texture) or texture.device != disparity.device
                                    or texture.dtype != torch.float32):
            raise ArgumentErr("%s: the texture image must be a float32 CUDA tensor on %s" % (name, disparity.device))
        d = disparity.contiguous()
        out = torch.empty_like(d)
        tex = () if texture is None else (texture.contiguous(),)
        ctx.set_stream(torch.cuda.current_stream(d.device).cuda_stream)
        fn = getattr(lib, "vwgpu_%s_dev" % name)
        targs = () if texture is None else (tex[0].data_ptr(), 0)
        ctx.check(fn(ctx._h, d.data_ptr(), w, h, 0, *targs, *head, sem, boxes.ctypes.data, len(boxes), out.data_ptr(), 0,
                     want_stats))
    else:
        if _is_tensor(texture):
            raise ArgumentErr("%s: with a numpy disparity the texture image must be a numpy array" % name)
        d = np.ascontiguousarray(disparity, dtype)
        out = np.empty_like(d)
        tex = None if texture is None else np.ascontiguousarray(texture, np.float32)
        targs = () if tex is None else (tex.ctypes.data, 0)
        fn = getattr(lib, "vwgpu_%s" % name)
        ctx.check(fn(ctx._h, d.ctypes.data, w, h, 0, *targs, *head, sem, boxes.ctypes.data, len(boxes), out.ctypes.data, 0,
                     want_stats))
    if stats is not None:
        stats[:] = list(st)
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
    ctx = _ctx_for(image, ctx)
    lib = ctx._lib
    args = (int(kernel_size), float(gradient_weight), float(stddev_weight), boxes.ctypes.data, len(boxes))
    if _is_tensor(image):
        if not image.is_cuda or image.dtype != torch.float32:
            raise ArgumentErr("texture_measure: the image must be a float32 CUDA tensor")
        img = image.contiguous()
        out = torch.zeros((h, w), dtype=torch.float32, device=img.device)
        ctx.set_stream(torch.cuda.current_stream(img.device).cuda_stream)
        ctx.check(lib.vwgpu_texture_measure_dev(ctx._h, img.data_ptr(), w, h, 0, *args, out.data_ptr(), 0, want))
    else:
        img = np.ascontiguousarray(image, np.float32)
        out = np.zeros((h, w), np.float32)
        ctx.check(lib.vwgpu_texture_measure(ctx._h, img.ctypes.data, w, h, 0, *args, out.ctypes.data, 0, want))
    if stats is not None:
        stats[:] = [mx.value]
    return out


OUTLIER_METHODS = {"mean": 0, "stddev": 1, "plane": 2}   # vwgpu_outlier_method
OUTLIER_SEMANTICS = {"reference": 0, "skip": 1}          # vwgpu_outlier_semantics
OUTLIER_MAX_HALF_KERNEL = 15
STD_DEV_IMAGE_MAX_KERNEL = 31
EDGE_EXTENSIONS = {"constant": 0, "zero": 1}             # vwgpu_edge


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
    st = (ctypes.c_longlong * 2)()
    want_stats = st if stats is not None else None
    ctx = _ctx_for(disparity, ctx)
    lib = ctx._lib
    head = (OUTLIER_METHODS[method],)
    tail = (int(hh), int(hv), float(p0), float(p1), int(bool(cleanup)), OUTLIER_SEMANTICS[semantics])
    if _is_tensor(disparity):
        if not disparity.is_cuda or disparity.dtype not in (torch.int32, torch.float32):
            raise ArgumentErr("%s: the disparity must be an int32 or float32 CUDA tensor" % name)
        d = disparity.contiguous()
        out = torch.empty_like(d)
        ctx.set_stream(torch.cuda.current_stream(d.device).cuda_stream)
        ctx.check(lib.vwgpu_rm_outliers_dev(ctx._h, *head, 0 if d.dtype == torch.int32 else 1, d.data_ptr(), w, h, 0, *tail,
                                            out.data_ptr(), 0, want_stats))
    else:
        if disparity.dtype not in (np.int32, np.float32):
            raise ArgumentErr("%s: the disparity must be int32 (PixelMask<Vector2i>) or float32 (PixelMask<Vector2f>)" % name)
        d = np.ascontiguousarray(disparity)
        out = np.empty_like(d)
        ctx.check(lib.vwgpu_rm_outliers(ctx._h, *head, 0 if d.dtype == np.int32 else 1, d.ctypes.data, w, h, 0, *tail,
                                        out.ctypes.data, 0, want_stats))
    if stats is not None:
        stats[:] = list(st)
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
    ctx = _ctx_for(image, ctx)
    lib = ctx._lib
    if _is_tensor(image):
        if not image.is_cuda or image.dtype != torch.float32:
            raise ArgumentErr("std_dev_image: the image must be a float32 CUDA tensor")
        img = image.contiguous()
        out = torch.empty_like(img)
        ctx.set_stream(torch.cuda.current_stream(img.device).cuda_stream)
        ctx.check(lib.vwgpu_std_dev_image_dev(ctx._h, img.data_ptr(), w, h, 0, kw, kh, EDGE_EXTENSIONS[edge], out.data_ptr(), 0))
    else:
        img = np.ascontiguousarray(image, np.float32)
        out = np.empty_like(img)
        ctx.check(lib.vwgpu_std_dev_image(ctx._h, img.ctypes.data, w, h, 0, kw, kh, EDGE_EXTENSIONS[edge], out.ctypes.data, 0))
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


def _dm_disparity(name, disparity):
    """Checks a {dx, dy, valid} map; returns (contiguous map, vwgpu_disparity_type, w, h, is a tensor)."""
    if disparity.ndim != 3 or disparity.shape[2] != 3:
        raise ArgumentErr("%s: disparity must be (rows, cols, 3) {dx, dy, valid}" % name)
    if int(disparity.shape[0]) <= 0 or int(disparity.shape[1]) <= 0:
        raise ArgumentErr("%s: empty image" % name)
    if _is_tensor(disparity):
        if not disparity.is_cuda or disparity.dtype not in (torch.int32, torch.float32):
            raise ArgumentErr("%s: the disparity must be an int32 or float32 CUDA tensor" % name)
        d = disparity.contiguous()
        return d, (0 if d.dtype == torch.int32 else 1), int(d.shape[1]), int(d.shape[0]), True
    if disparity.dtype not in (np.int32, np.float32):
        raise ArgumentErr("%s: the disparity must be int32 (PixelMask<Vector2i>) or float32 (PixelMask<Vector2f>)" % name)
    d = np.ascontiguousarray(disparity)
    return d, (0 if d.dtype == np.int32 else 1), int(d.shape[1]), int(d.shape[0]), False


def _dm_ptr(a):
    return a.data_ptr() if _is_tensor(a) else a.ctypes.data


def _dm_empty(like, shape, dtype=None):
    if _is_tensor(like):
        return torch.empty(shape, dtype=like.dtype if dtype is None else dtype, device=like.device)
    return np.empty(shape, like.dtype if dtype is None else dtype)


def _dm_entry(ctx, name, d, tensor):
    """The _dev entry on the current torch stream for tensors, the host entry for numpy arrays."""
    if tensor:
        ctx.set_stream(torch.cuda.current_stream(d.device).cuda_stream)
        return getattr(ctx._lib, "vwgpu_%s_dev" % name)
    return getattr(ctx._lib, "vwgpu_%s" % name)


def get_disparity_range(disparity, ctx=None, device_result=False):
    """vw::stereo::get_disparity_range (src/vw/Stereo/DisparityMap.h:48-66): the box of the VALID disparities, returned
    as float32[4] {min.x, min.y, max.x, max.y} (BBox2f(min, max)); zeros when no pixel is valid.  A NaN component counts
    only in the first valid pixel in raster order (then both extrema of that component are NaN), as the reference's
    accumulator has it.  numpy in -> numpy out; CUDA tensor in -> numpy out after one synchronisation, or with
    device_result=True a CUDA float32[4] tensor without any host round trip."""
    d, t, w, h, tensor = _dm_disparity("get_disparity_range", disparity)
    ctx = _ctx_for(d, ctx)
    host = np.zeros(4, np.float32)
    if tensor:
        ctx.set_stream(torch.cuda.current_stream(d.device).cuda_stream)
        if device_result:
            out = torch.empty(4, dtype=torch.float32, device=d.device)
            ctx.check(ctx._lib.vwgpu_get_disparity_range_dev(ctx._h, t, d.data_ptr(), w, h, 0, out.data_ptr(), None))
            return out
        ctx.check(ctx._lib.vwgpu_get_disparity_range_dev(ctx._h, t, d.data_ptr(), w, h, 0, None, host.ctypes.data))
        return host
    if device_result:
        raise ArgumentErr("get_disparity_range: device_result needs a CUDA tensor")
    ctx.check(ctx._lib.vwgpu_get_disparity_range(ctx._h, t, d.ctypes.data, w, h, 0, host.ctypes.data))
    return host


def disparity_range_mask(disparity, min, max, semantics="reference", x0=0, y0=0, ctx=None, stats=None):
    """vw::stereo::disparity_range_mask(d, min, max) (src/vw/Stereo/DisparityMap.h:255-300): a valid pixel whose target
    location (x0 + x + dx, y0 + y + dy) leaves [min, max - 1) becomes {0, 0, 0}; min, max are (x, y) pairs in the
    pixel's channel type.  semantics="reference" (default) keeps the reference's comparison of the lower bound of y with
    min[0] (:279), "fixed" uses min[1].  x0, y0: the image coordinates of pixel (0, 0) of `disparity` (a tile of a
    larger map).  stats (optional list) receives [pixels masked]."""
    if semantics not in RANGE_MASK_SEMANTICS:
        raise ArgumentErr("disparity_range_mask: semantics must be 'reference' or 'fixed', not %r" % (semantics,))
    d, t, w, h, tensor = _dm_disparity("disparity_range_mask", disparity)
    lo, hi = np.array(min, np.float64).reshape(-1), np.array(max, np.float64).reshape(-1)
    if lo.size != 2 or hi.size != 2:
        raise ArgumentErr("disparity_range_mask: min and max must be (x, y) pairs")
    ctx = _ctx_for(d, ctx)
    out = _dm_empty(d, d.shape)
    st = (ctypes.c_longlong * 1)()
    ctx.check(_dm_entry(ctx, "disparity_range_mask", d, tensor)(
        ctx._h, t, _dm_ptr(d), w, h, 0, int(x0), int(y0), lo.ctypes.data, hi.ctypes.data, RANGE_MASK_SEMANTICS[semantics],
        _dm_ptr(out), 0, st if stats is not None else None))
    if stats is not None:
        stats[:] = list(st)
    return out


def _transform(name, disparity, matrix, mode, x0, y0, ctx):
    d, t, w, h, tensor = _dm_disparity(name, disparity)
    m = np.ascontiguousarray(np.array(matrix, np.float64))
    if m.shape != (3, 3):
        raise ArgumentErr("%s: the matrix must be 3 x 3" % name)
    ctx = _ctx_for(d, ctx)
    out = _dm_empty(d, d.shape)
    ctx.check(_dm_entry(ctx, "transform_disparities", d, tensor)(
        ctx._h, t, _dm_ptr(d), w, h, 0, int(x0), int(y0), m.ctypes.data, TRANSFORM_MODES[mode], _dm_ptr(out), 0))
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
    d, t, w, h, tensor = _dm_disparity(name, disparity)
    ctx = _ctx_for(d, ctx)
    out = _dm_empty(d, shape_of(h, w), dtype)
    ctx.check(_dm_entry(ctx, name, d, tensor)(ctx._h, t, _dm_ptr(d), w, h, 0, _dm_ptr(out), 0))
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
    return _resample("missing_pixel_image", disparity, lambda h, w: (h, w, 3), torch.uint8 if _is_tensor(disparity) else np.uint8, ctx)


def intersect_mask_and_data(data, mask, ctx=None):
    """vw::stereo::intersect_mask_and_data (src/vw/Stereo/DisparityMap.h:1226-1249): the data pixel where it is valid,
    else the mask pixel where that is valid, else the data pixel.  Both maps have one type and size."""
    d, t, w, h, tensor = _dm_disparity("intersect_mask_and_data", data)
    m, tm, wm, hm, mtensor = _dm_disparity("intersect_mask_and_data", mask)
    if (t, w, h, tensor) != (tm, wm, hm, mtensor):
        raise ArgumentErr("intersect_mask_and_data: data and mask must have the same type and size")
    ctx = _ctx_for(d, ctx)
    out = _dm_empty(d, d.shape)
    ctx.check(_dm_entry(ctx, "intersect_mask_and_data", d, tensor)(ctx._h, t, _dm_ptr(d), 0, _dm_ptr(m), 0, w, h, _dm_ptr(out), 0))
    return out


def disparity_transform_image(right, disparity, ctx=None):
    """transform(right, DisparityTransform(disparity)) (src/vw/Stereo/DisparityMap.h:1164-1187): the (rows, cols)
    float32 right image seen from the left one, bilinear over zero edge extension; a pixel without a valid disparity
    (or outside the float32 disparity map, which may have another size) samples (-1, y) and becomes 0."""
    d, t, dw, dh, tensor = _dm_disparity("disparity_transform_image", disparity)
    if t != 1:
        raise ArgumentErr("disparity_transform_image: the disparity must be float32 (PixelMask<Vector2f>)")
    if right.ndim != 2 or _is_tensor(right) != tensor:
        raise ArgumentErr("disparity_transform_image: the image must be (rows, cols), on the same side as the disparity")
    if tensor:
        if not right.is_cuda or right.dtype != torch.float32:
            raise ArgumentErr("disparity_transform_image: the image must be a float32 CUDA tensor")
        r = right.contiguous()
    else:
        r = np.ascontiguousarray(right, np.float32)
    rh, rw = int(r.shape[0]), int(r.shape[1])
    if rw <= 0 or rh <= 0:
        raise ArgumentErr("disparity_transform_image: empty image")
    ctx = _ctx_for(d, ctx)
    out = _dm_empty(r, r.shape)
    ctx.check(_dm_entry(ctx, "disparity_warp", d, tensor)(ctx._h, _dm_ptr(r), rw, rh, 0, _dm_ptr(d), dw, dh, 0, _dm_ptr(out), 0))
    return out


TRIANGULATE_SEMANTICS = {"view": 0, "model": 1}
DISPARITY_LAYOUTS = {"dxdyv": 0x000, "dxdy": 0x100, "dv": 0x200, "d": 0x300}
_LAYOUT_WORDS = {"dxdyv": 3, "dxdy": 2, "dv": 2, "d": 1}


def _tri_disparity(name, disparity, layout):
    """A disparity image in one of the pixel forms DispHelper accepts (src/vw/Stereo/StereoView.h:37-53); returns
    (contiguous image, vwgpu_disparity_type, layout flag, w, h, is a tensor).  Never copies a tensor to the host."""
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
    tensor = _is_tensor(disparity)
    if tensor:
        if not disparity.is_cuda or disparity.dtype not in (torch.int32, torch.float32):
            raise ArgumentErr("%s: the disparity must be an int32 or float32 CUDA tensor" % name)
        d = disparity.contiguous()
        t = 0 if d.dtype == torch.int32 else 1
    else:
        if disparity.dtype not in (np.int32, np.float32):
            raise ArgumentErr("%s: the disparity must be int32 or float32" % name)
        d = np.ascontiguousarray(disparity)
        t = 0 if d.dtype == np.int32 else 1
    return d, t, DISPARITY_LAYOUTS[layout], int(d.shape[1]), int(d.shape[0]), tensor


def _f64(like):
    return torch.float64 if _is_tensor(like) else np.float64


def _triangulate(name, disparity, cam1, cam2, x0, y0, angle_tol, semantics, layout, want_error, want_errvec, stats, ctx):
    from . import _lib, camera
    if semantics not in TRIANGULATE_SEMANTICS:
        raise ArgumentErr("%s: semantics must be 'view' or 'model', not %r" % (name, semantics))
    d, t, lay, w, h, tensor = _tri_disparity(name, disparity, layout)
    c1, c2 = camera.descriptor_of(cam1), camera.descriptor_of(cam2)
    ctx = _ctx_for(d, ctx)
    xyz = _dm_empty(d, (h, w, 3), _f64(d))
    err = _dm_empty(d, (h, w), _f64(d)) if want_error else None
    vec = _dm_empty(d, (h, w, 3), _f64(d)) if want_errvec else None
    st, st_dev = None, None
    if stats is not None:
        if _is_tensor(stats):
            if not tensor or not stats.is_cuda or stats.dtype != torch.int64 or stats.numel() != 3 or not stats.is_contiguous():
                raise ArgumentErr("%s: a device stats must be a contiguous int64[3] CUDA tensor, with a CUDA disparity" % name)
            st = stats.data_ptr()
        elif tensor:
            st_dev = torch.empty(3, dtype=torch.int64, device=d.device)
            st = st_dev.data_ptr()
        else:
            st_host = _lib.TriangulateStats()
            st = ctypes.addressof(st_host)
    ctx.check(_dm_entry(ctx, "stereo_triangulate", d, tensor)(
        ctx._h, t, _dm_ptr(d), w, h, 0, int(x0), int(y0), ctypes.byref(c1), ctypes.byref(c2), float(angle_tol),
        TRIANGULATE_SEMANTICS[semantics] | lay, _dm_ptr(xyz), 0, _dm_ptr(err) if want_error else None, 0,
        _dm_ptr(vec) if want_errvec else None, 0, st))
    if stats is not None and not _is_tensor(stats):
        if tensor:
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
    camera.CAHVModel.  x0, y0: the image coordinates of pixel (0, 0) of `disparity` (a tile of a larger map).
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
        from . import camera
        if semantics not in TRIANGULATE_SEMANTICS:
            raise ArgumentErr("convergence_angle: semantics must be 'view' or 'model', not %r" % (semantics,))
        d, t, lay, w, h, tensor = _tri_disparity("convergence_angle", disparity, layout)
        c1, c2 = camera.descriptor_of(self.cam1), camera.descriptor_of(self.cam2)
        ctx = _ctx_for(d, ctx)
        out = _dm_empty(d, (h, w), _f64(d))
        ctx.check(_dm_entry(ctx, "convergence_angle", d, tensor)(
            ctx._h, t, _dm_ptr(d), w, h, 0, int(x0), int(y0), ctypes.byref(c1), ctypes.byref(c2),
            TRIANGULATE_SEMANTICS[semantics] | lay, _dm_ptr(out), 0))
        return out


DBL_MAX = float(np.finfo(np.float64).max)


def universe_radius(points, origin, near_radius=0.0, far_radius=DBL_MAX, stats=None, ctx=None, out=None):
    """per_pixel_filter(points, UniverseRadiusFunc(origin, near_radius, far_radius)) (src/vw/Stereo/StereoView.h:139-222) on a
    (rows, cols, 3 | 4 | 6) float64 point image (xyz; xyz + error; xyz + error vector): a pixel whose xyz is zero becomes
    all zero, one whose distance from origin is below a non-zero near_radius or above a non-zero far_radius too.  Negative
    radii or near_radius > far_radius raise ArgumentErr, as the reference's constructor asserts.  stats (optional list)
    receives [total_points, rejected_points] (one synchronisation).  out=points filters in place."""
    tensor = _is_tensor(points)
    if points.ndim != 3 or int(points.shape[2]) not in (3, 4, 6):
        raise ArgumentErr("universe_radius: points must be (rows, cols, 3 | 4 | 6)")
    if tensor:
        if not points.is_cuda or points.dtype != torch.float64:
            raise ArgumentErr("universe_radius: the points must be a float64 CUDA tensor")
        p = points if out is points else points.contiguous()
    else:
        if points.dtype != np.float64:
            raise ArgumentErr("universe_radius: the points must be float64")
        p = points if out is points else np.ascontiguousarray(points)
    if out is points:
        if not (p.is_contiguous() if tensor else p.flags["C_CONTIGUOUS"]):
            raise ArgumentErr("universe_radius: an image filtered in place must be contiguous")
        res = p
    elif out is not None:
        raise ArgumentErr("universe_radius: out must be None or the points themselves")
    else:
        res = _dm_empty(p, tuple(p.shape))
    h, w, ch = int(p.shape[0]), int(p.shape[1]), int(p.shape[2])
    if w <= 0 or h <= 0:
        raise ArgumentErr("universe_radius: empty image")
    o = np.array(origin, np.float64).reshape(-1)
    if o.size != 3:
        raise ArgumentErr("universe_radius: the origin must have three elements")
    ctx = _ctx_for(p, ctx)
    st = (ctypes.c_longlong * 2)()
    ctx.check(_dm_entry(ctx, "universe_radius", p, tensor)(
        ctx._h, _dm_ptr(p), ch, w, h, 0, o.ctypes.data, float(near_radius), float(far_radius), _dm_ptr(res), 0,
        st if stats is not None else None))
    if stats is not None:
        stats[:] = list(st)
    return res


__all__ = ["affine_subpixel", "bayes_em_subpixel", "corr_eval", "disparity_median_filter", "disparity_neighbor_filter",
           "texture_measure", "texture_preserving_disparity_filter","lk_subpixel", "phase_subpixel", "pyramid_subpixel", "calc_disparity", "calc_disparity_sgm", "cross_corr_consistency_check", "parabola_subpixel", "rm_outliers_using_thresh",
           "disparity_cleanup_using_thresh", "disparity_mask", "disparity_blob_filter", "subdivide_regions", "pyramid_correlate", "pyramid_correlate_batch",
           "rm_outliers_using_mean", "rm_outliers_using_stddev", "rm_outliers_using_plane", "disparity_cleanup_using_mean",
           "disparity_cleanup_using_stddev", "disparity_clean_using_plane", "std_dev_image",
           "get_disparity_range", "disparity_range_mask", "transform_disparities", "transform_disparities_subregion",
           "HomographyTransform", "disparity_subsample", "disparity_upsample", "disparity_transform_image",
           "missing_pixel_image", "intersect_mask_and_data",
           "StereoModel", "stereo_triangulate", "universe_radius",
           "BBox2i", "CostFunctionType"]
