"""Host-side mirror of the reference's image filters on the stereo path (pyramid smoothing + decimation, Gaussian /
Laplacian prefilters, mask decimation).  Same names and argument meaning as the reference:

  generate_gaussian_kernel           src/vw/Image/Filter.tcc:37-78
  generate_pyramid_smoothing_kernel  src/vw/Image/Filter.h:89-99
  separable_convolution_filter       src/vw/Image/Filter.h:156-191   (rasterised; optional subsample(., s))
  gaussian_filter / laplacian_filter src/vw/Image/Filter.h:205-258, 320-335
  subsample_mask_by_two              src/vw/Stereo/CorrelationView.cc:38-63
  prefilter_image                    src/vw/Stereo/PreFilter.h:76-95

numpy arrays go through the host entry points, torch CUDA tensors through the device entry points (current stream).
"""
import numpy as np

from . import _lib
from ._operands import Operands
from .core import ArgumentErr

ConstantEdgeExtension, ZeroEdgeExtension = 0, 1
PREFILTER_NONE, PREFILTER_MEANSUB, PREFILTER_LOG = 0, 1, 2


def generate_gaussian_kernel(sigma, size=0):
    taps = np.zeros(4096, np.float32)
    n = _lib.load().vwgpu_generate_gaussian_kernel(float(sigma), int(size), taps.ctypes.data, taps.size)
    if n < 0:
        raise ArgumentErr("generate_gaussian_kernel: bad size")
    return taps[:n].copy()


def generate_pyramid_smoothing_kernel():
    return np.array([1.0 / 16.0, 4.0 / 16.0, 6.0 / 16.0, 4.0 / 16.0, 1.0 / 16.0], np.float32)


def separable_convolution_filter(src, x_kernel, y_kernel, cx=None, cy=None, edge=ConstantEdgeExtension, subsample=1, ctx=None):
    ops = Operands("separable_convolution_filter", src, ctx)
    src = ops.image(src, np.float32, rows=True)
    xk = np.ascontiguousarray(x_kernel, np.float32)
    yk = np.ascontiguousarray(y_kernel, np.float32)
    cx = ((len(xk) - 1) // 2 if len(xk) else 0) if cx is None else cx
    cy = ((len(yk) - 1) // 2 if len(yk) else 0) if cy is None else cy
    h, w = src.shape
    oh, ow = 1 + (h - 1) // subsample, 1 + (w - 1) // subsample
    out = ops.empty((oh, ow), np.float32)
    ops.call("separable_convolution", ops.ptr(src), w, h, ops.row_stride(src), xk.ctypes.data, len(xk), cx,
             yk.ctypes.data, len(yk), cy, edge, subsample, ops.ptr(out), 0)
    return out


def gaussian_filter(src, x_sigma, y_sigma=None, x_dim=0, y_dim=0, edge=ConstantEdgeExtension, ctx=None):
    y_sigma = x_sigma if y_sigma is None else y_sigma
    return separable_convolution_filter(src, generate_gaussian_kernel(x_sigma, x_dim), generate_gaussian_kernel(y_sigma, y_dim),
                                        edge=edge, ctx=ctx)


def convolution_filter(src, kernel, ci=None, cj=None, edge=ConstantEdgeExtension, ctx=None):
    ops = Operands("convolution_filter", src, ctx)
    src = ops.image(src, np.float32, rows=True)
    k = np.ascontiguousarray(kernel, np.float32)
    kh, kw = k.shape
    ci = (kw - 1) // 2 if ci is None else ci
    cj = (kh - 1) // 2 if cj is None else cj
    h, w = src.shape
    out = ops.empty((h, w), np.float32)
    ops.call("convolution_2d", ops.ptr(src), w, h, ops.row_stride(src), k.ctypes.data, kw, kh, ci, cj, edge, ops.ptr(out), 0)
    return out


def laplacian_filter(src, edge=ConstantEdgeExtension, ctx=None):
    return convolution_filter(src, [[0, 1, 0], [1, -4, 1], [0, 1, 0]], 1, 1, edge, ctx=ctx)


def subsample_mask_by_two(mask, ctx=None):
    ops = Operands("subsample_mask_by_two", mask, ctx)
    mask = ops.image(mask, np.uint8, rows=True)
    h, w = mask.shape
    out = ops.empty((1 + (h - 1) // 2, 1 + (w - 1) // 2), np.uint8)
    ops.call("subsample_mask_by_two", ops.ptr(mask), w, h, ops.row_stride(mask), ops.ptr(out), 0)
    return out


def prefilter_image(image, prefilter_mode, prefilter_width, ctx=None):
    ops = Operands("prefilter_image", image, ctx)
    image = ops.image(image, np.float32, rows=True)
    h, w = image.shape
    out = ops.empty((h, w), np.float32)
    ops.call("prefilter_image", ops.ptr(image), w, h, ops.row_stride(image), int(prefilter_mode), float(prefilter_width),
             ops.ptr(out), 0)
    return out


def build_gaussian_pyramid(image, levels, ctx=None):
    """The smoothing + decimation chain of build_image_pyramids (src/vw/Stereo/CorrelationView.cc:205-216):
    level i = subsample(separable_convolution_filter(level i-1, k, k), 2) with k = [1 4 6 4 1]/16."""
    k = generate_pyramid_smoothing_kernel()
    out = [image]
    for _ in range(levels):
        out.append(separable_convolution_filter(out[-1], k, k, subsample=2, ctx=ctx))
    return out
