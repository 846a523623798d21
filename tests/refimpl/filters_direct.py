"""The pyramid / prefilter family written straight from the reference's definitions, in numpy, sharing no code with oracle/.

  correlate_1d_at_point            src/vw/Image/Convolution.h:53-65     result = 0; result += kernel[n-1-i] * src[i], i = 0..n-1
  SeparableConvolutionView         src/vw/Image/Convolution.h:275-328   horizontal pass into a work image of the source's type, then vertical
  ConvolutionView                  src/vw/Image/Convolution.h:105-170   kernel rotated by 180 degrees, rows outer, columns inner
  SubsampleView                    src/vw/Image/Manipulation.h:214-293  picks (s*i, s*j)
  PreFilter                        src/vw/Stereo/PreFilter.h:41-95      NONE = image, MEANSUB = image - gaussian, LOG = laplacian(gaussian)
  subsample_mask_by_two            src/vw/Stereo/CorrelationView.cc:38-63

Where the oracle walks pixels and asks an edge-extension function for every tap, this file pads the source once (np.pad) and adds one
shifted slice per tap: acc = acc + k[n-1-i] * slice.  Every operand has the image's dtype, so with float32 each multiply and each add
rounds once to float32, in the reference's order.  Every function takes a region {x0, y0, bw, bh} in the coordinates of the source; the
region may leave the image: the filter of the edge-extended source is defined everywhere (the reference's lazy views are cropped like
this).  The default region is the image.
"""
import math

import numpy as np

EDGE_CONSTANT, EDGE_ZERO = 0, 1
PREFILTER_NONE, PREFILTER_MEANSUB, PREFILTER_LOG = 0, 1, 2


def extended(img, x0, y0, bw, bh, edge=EDGE_CONSTANT):
    """The edge-extended image over [x0, x0 + bw) x [y0, y0 + bh)."""
    h, w = img.shape
    l, t = max(0, -x0), max(0, -y0)
    r, b = max(0, x0 + bw - w), max(0, y0 + bh - h)
    p = np.pad(img, ((t, b), (l, r)), mode="edge" if edge == EDGE_CONSTANT else "constant")
    return p[y0 + t:y0 + t + bh, x0 + l:x0 + l + bw]


def _correlate(src, k, n_out, axis):
    """out[j] = sum over i, in that order, of k[n-1-i] * src[j + i] along `axis`, from a zero of the source's type."""
    n = len(k)
    shape = list(src.shape)
    shape[axis] = n_out
    acc = np.zeros(shape, src.dtype)
    for i in range(n):
        sl = src[:, i:i + n_out] if axis == 1 else src[i:i + n_out, :]
        acc = acc + k[n - 1 - i] * sl
    return acc


def separable_convolution(img, xk, yk, cx=None, cy=None, edge=EDGE_CONSTANT, subsample=1, region=None):
    """separable_convolution_filter(img, xk, yk, cx, cy, edge) over the region, then subsample(., s).  An empty kernel leaves its axis alone."""
    dt = img.dtype
    xk, yk = np.asarray(xk, dt), np.asarray(yk, dt)
    nx, ny = len(xk), len(yk)
    cx = ((nx - 1) // 2 if nx else 0) if cx is None else cx
    cy = ((ny - 1) // 2 if ny else 0) if cy is None else cy
    h, w = img.shape
    x0, y0, bw, bh = (0, 0, w, h) if region is None else region
    x_lo, y_lo = (nx - cx - 1 if nx else 0), (ny - cy - 1 if ny else 0)
    x_hi, y_hi = (cx if nx else 0), (cy if ny else 0)
    with np.errstate(all="ignore"):
        src = extended(img, x0 - x_lo, y0 - y_lo, bw + x_lo + x_hi, bh + y_lo + y_hi, edge)
        work = _correlate(src, xk, bw, 1) if nx else src
        out = _correlate(work, yk, bh, 0) if ny else work
    return np.ascontiguousarray(out[::subsample, ::subsample])


def convolution_2d(img, kernel, ci=None, cj=None, edge=EDGE_CONSTANT, region=None):
    """convolution_filter(img, kernel, ci, cj, edge) over the region; kernel is (kh, kw), row-major."""
    dt = img.dtype
    k = np.asarray(kernel, dt)
    kh, kw = k.shape
    ci = (kw - 1) // 2 if ci is None else ci
    cj = (kh - 1) // 2 if cj is None else cj
    h, w = img.shape
    x0, y0, bw, bh = (0, 0, w, h) if region is None else region
    rot = k[::-1, ::-1]                                                  # the reference correlates with the rotated kernel
    src = extended(img, x0 - (kw - 1 - ci), y0 - (kh - 1 - cj), bw + kw - 1, bh + kh - 1, edge)
    acc = np.zeros((bh, bw), dt)
    with np.errstate(all="ignore"):
        for j in range(kh):
            for i in range(kw):
                acc = acc + rot[j, i] * src[j:j + bh, i:i + bw]
    return acc


def subsample_mask_by_two(mask):
    m = np.asarray(mask) != 0
    h, w = m.shape
    p = np.pad(m, ((0, h % 2), (0, w % 2)), mode="constant").astype(np.int32)
    count = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    return np.where(count > 1, 255, 0).astype(np.uint8)


def gaussian_kernel(sigma, size=0, dtype=np.float32):
    """generate_gaussian_kernel<KernelT> (src/vw/Image/Filter.tcc:37-78): erf differences in double, stored as KernelT, then KernelT *= double."""
    if sigma == 0:
        return np.zeros(0, dtype)
    if size == 0:
        size = int(7 * sigma)
        size = 3 if size < 3 else (size - 1 if size % 2 == 0 else size)
    z = 1.0 / (math.sqrt(2.0) * sigma)
    c = size // 2
    if size % 2 == 0:
        half = [math.erf((i + 1.0) * z) - math.erf(i * z) for i in range(c)]
        taps, total = half[::-1] + half, 2.0 * _running(half)
    else:
        half = [math.erf((i + 0.5) * z) - math.erf((i - 0.5) * z) for i in range(1, c + 1)]
        mid = math.erf(0.5 * z) - math.erf(-0.5 * z)
        taps, total = half[::-1] + [mid] + half, 2.0 * _running(half) + mid
    stored = np.array(taps, np.float64).astype(dtype)
    return (stored.astype(np.float64) * (1.0 / total)).astype(dtype)


def _running(values):
    s = 0.0
    for v in values:
        s += v
    return s


LAPLACIAN = [[0, 1, 0], [1, -4, 1], [0, 1, 0]]


def prefilter_region(img, mode, width, region=None):
    """prefilter.filter(img) rasterised over the region.  MEANSUB subtracts the gaussian of the constant-extended SOURCE at the region's
    coordinates; LOG takes the Laplacian of the gaussian VIEW, whose domain is the image and which is itself constant-extended."""
    h, w = img.shape
    x0, y0, bw, bh = (0, 0, w, h) if region is None else region
    here = np.ascontiguousarray(extended(img, x0, y0, bw, bh))
    if mode not in (PREFILTER_MEANSUB, PREFILTER_LOG):
        return here
    k = gaussian_kernel(float(np.float32(width)), 0, img.dtype.type)         # the prefilter's width is a float (PreFilter.h:53-54, 67-68)
    if mode == PREFILTER_MEANSUB:
        with np.errstate(all="ignore"):
            return here - separable_convolution(img, k, k, region=(x0, y0, bw, bh))
    return convolution_2d(separable_convolution(img, k, k), LAPLACIAN, 1, 1, EDGE_CONSTANT, region=(x0, y0, bw, bh))


def prefilter_image(img, mode, width):
    return prefilter_region(img, mode, width)


def same_bits(got, want):
    """The comparison rule of the filter tests.  Where `want` is NaN, `got` must be NaN (x86 and the GPU make different default NaNs, so
    payload and sign are not compared); everywhere else the bit patterns are equal, which tells -0.0 from +0.0 and a flushed subnormal
    from the subnormal.  Returns the number of offending pixels."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return -1
    if got.dtype.kind != "f":
        return int((got != want).sum())
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), got.view(u) != want.view(u))
    return int(bad.sum())
