"""Host-side mirror of the reference's hole filling on masked images (include/vwgpu.h): grassfire
(src/vw/Image/Grassfire.h), BlobIndexThreaded, get_blob_sizes (Image/BlobIndex.h), ErodeView (Image/ErodeView.h),
inpaint, fill_holes_grass and fill_nodata_with_avg (Image/InpaintView.h).

Masked images are numpy arrays or torch CUDA tensors of one of four pixel kinds:
    (rows, cols) uint8              a mask, non-zero = valid
    (rows, cols, 2) float32         PixelMask<float> as {value, valid}
    (rows, cols, 3) int32 / float32 PixelMask<Vector2i> / PixelMask<Vector2f> as {dx, dy, valid}
A view whose rows are further apart than its width (a crop of a wider image) is passed as it is, with its row stride.

Input conditioning, on (rows, cols) float32 images with an optional `mask` (any dtype, non-zero =
valid: the PixelMask of the reference): min_max, moments, mean, stddev, median, percentile (src/vw/Image/Statistics.h,
src/vw/Math/Functors.h), histogram, otsu_threshold, percentile_scale_convert, u8_convert (src/vw/Image/ImageThresh.h),
clamp, normalize, threshold (src/vw/Image/Algorithms.h, AutoNormalize.h).
"""
import ctypes

import numpy as np

from . import _lib
from .core import ArgumentErr, CapacityErr, LogicErr
from ._operands import Operands

MASK_U8, MASKED_F32, DISPARITY_I32, DISPARITY_F32 = 0, 1, 2, 3      # vwgpu_pixel_kind
HOLE_EDGE_SEMANTICS = {"reference": 0, "fixed": 1}                   # vwgpu_hole_edge_semantics
HOLE_FILL_MAX_LEN = 64                                               # VWGPU_HOLE_FILL_MAX_LEN
_GRASSFIRE_TYPES = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1, np.dtype(np.float32): 2}
_CHANNELS = {MASK_U8: 1, MASKED_F32: 2, DISPARITY_I32: 3, DISPARITY_F32: 3}


def _strides(ops, a):
    """Element strides of an operand of either side."""
    return tuple(a.stride()) if ops.tensor else tuple(s // a.itemsize for s in a.strides)


def _rows(ops, name, a, channels):
    """The operand as the library takes it and its row stride in pixels: a itself when only its rows are strided, else
    a contiguous copy."""
    st = _strides(ops, a)
    inner = st[1:] == ((channels, 1) if a.ndim == 3 else (1,))
    if inner and st[0] >= a.shape[1] * channels and st[0] % channels == 0:
        return a, st[0] // channels
    a = a.contiguous() if ops.tensor else np.ascontiguousarray(a)
    return a, int(a.shape[1])


def _masked(ops, name, img, kinds=(MASK_U8, MASKED_F32, DISPARITY_I32, DISPARITY_F32)):
    """(operand, kind, cols, rows, row stride in pixels) of a masked image."""
    ops._side(img)
    dt = ops.dtype_of(img)
    kind = None
    if img.ndim == 2 and dt == np.uint8:
        kind = MASK_U8
    elif img.ndim == 3 and img.shape[2] == 2 and dt == np.float32:
        kind = MASKED_F32
    elif img.ndim == 3 and img.shape[2] == 3 and dt in (np.int32, np.float32):
        kind = DISPARITY_I32 if dt == np.int32 else DISPARITY_F32
    if kind is None or kind not in kinds:
        raise ArgumentErr("%s: %s %s is not a pixel kind this call takes" % (name, tuple(img.shape), getattr(img, "dtype", None)))
    h, w = int(img.shape[0]), int(img.shape[1])
    if w <= 0 or h <= 0:
        raise ArgumentErr("%s: empty image" % name)
    a, stride = _rows(ops, name, img, _CHANNELS[kind])
    return a, kind, w, h, stride


def _edge(name, semantics):
    if semantics not in HOLE_EDGE_SEMANTICS:
        raise ArgumentErr("%s: semantics must be 'reference' or 'fixed', not %r" % (name, semantics))
    return HOLE_EDGE_SEMANTICS[semantics]


def _length(name, n):
    if not 0 <= int(n) <= HOLE_FILL_MAX_LEN:
        raise ArgumentErr("%s: a hole length of %d is outside [0, %d]" % (name, n, HOLE_FILL_MAX_LEN))
    return int(n)


def _out_for(ops, name, a, out):
    """The output image of an entry that may work in place: `out` (a contiguous image like `a`, possibly `a` itself) or
    a new one.  Returns (image, row stride)."""
    if out is None:
        return ops.empty(tuple(a.shape), ops.dtype_of(a)), int(a.shape[1])
    ops._side(out)
    if tuple(out.shape) != tuple(a.shape) or ops.dtype_of(out) != ops.dtype_of(a):
        raise ArgumentErr("%s: out must have the shape and type of the image" % name)
    return _rows_exact(ops, name, out, a.shape[2] if a.ndim == 3 else 1)


def _rows_exact(ops, name, a, channels):
    b, stride = _rows(ops, name, a, channels)
    if b is not a:
        raise ArgumentErr("%s: an image that is written must have contiguous pixels" % name)
    return a, stride


def grassfire(src, ignore_borders=False, ctx=None):
    """vw::grassfire (src/vw/Image/Grassfire.h:79-228) as int32: the Manhattan distance of every pixel to the nearest
    pixel with src == 0; everything outside the image counts as zero unless ignore_borders, which caps the result at
    cols + rows.  src: (rows, cols) uint8, int32 or float32 (a NaN is non-zero).  One row or one column gives zeros."""
    ops = Operands("grassfire", src, ctx)
    ops._side(src)
    if src.ndim != 2 or ops.dtype_of(src) not in _GRASSFIRE_TYPES:
        raise ArgumentErr("grassfire: a (rows, cols) uint8, int32 or float32 image expected")
    h, w = int(src.shape[0]), int(src.shape[1])
    if w <= 0 or h <= 0:
        raise ArgumentErr("grassfire: empty image")
    s, stride = _rows(ops, "grassfire", src, 1)
    out = ops.empty((h, w), np.int32)
    ops.call("grassfire", _GRASSFIRE_TYPES[np.dtype(ops.dtype_of(s))], ops.ptr(s), w, h, stride, 1 if ignore_borders else 0, ops.ptr(out), 0)
    return out


class BlobIndex(object):
    """What blob_index returns: labels (rows, cols) int32 (the 1-based number of the kept blob a pixel belongs to, else
    0), table (count, 5) int32 {min.x, min.y, max.x, max.y, size} with half-open boxes, count.  They stay on the side
    of the image (CUDA tensors for a tensor)."""
    __slots__ = ("labels", "table", "count")

    def __init__(self, labels, table, count):
        self.labels, self.table, self.count = labels, table, count

    def num_blobs(self):
        return self.count


def blob_index(img, invert=False, max_area=0, wipe_size=0, capacity=None, ctx=None):
    """BlobIndexThreaded(img, max_area, ..) over the whole image as one tile, then wipe_big_blobs(wipe_size) when
    wipe_size > 0 (src/vw/Image/BlobIndex.h:113-306, :385-477): the 8-connected blobs of the valid pixels (invert: of the
    invalid ones) in the reference's order.  capacity: rows of the table to offer (default: as many as there are blobs,
    which costs a second call); too few raise CapacityErr, whose .count says how many it takes."""
    ops = Operands("blob_index", img, ctx)
    a, kind, w, h, stride = _masked(ops, "blob_index", img)
    labels = ops.empty((h, w), np.int32)
    n = ctypes.c_int(0)
    args = (kind, ops.ptr(a), w, h, stride, 1 if invert else 0, int(max_area), int(wipe_size))
    if capacity is None:
        ops.call("blob_index", *(args + (None, 0, None, 0, ctypes.byref(n))))
        capacity = n.value
    table = ops.zeros((max(int(capacity), 1), 5), np.int32)
    try:
        ops.call("blob_index", *(args + (ops.ptr(labels), 0, ops.ptr(table), int(capacity), ctypes.byref(n))))
    except CapacityErr as e:
        e.count = n.value
        raise
    return BlobIndex(labels, table[:n.value], n.value)


def get_blob_sizes(img, limit=0xffffffff, ctx=None):
    """vw::get_blob_sizes (src/vw/Image/BlobIndex.h:507-615) with the image as one tile: (rows, cols) uint32, min(size of
    the pixel's blob, limit) at valid pixels and 0 at invalid ones."""
    ops = Operands("get_blob_sizes", img, ctx)
    a, kind, w, h, stride = _masked(ops, "get_blob_sizes", img)
    if ops.tensor:      # torch has no uint32 arithmetic worth the name: the words travel as int32
        out = ops.empty((h, w), np.int32)
    else:
        out = ops.empty((h, w), np.uint32)
    ops.call("blob_sizes", kind, ops.ptr(a), w, h, stride, int(limit) & 0xffffffff, ops.ptr(out), 0)
    return out


def erode_blobs(img, max_area, out=None, ctx=None):
    """applyErodeView(img, BlobIndexThreaded(img, max_area, ..)) (src/vw/Image/ErodeView.h:199-221): the pixels of every
    blob of valid pixels with at most max_area pixels become the default pixel (all words 0).  out: the image to write
    (may be img itself); default a new one."""
    ops = Operands("erode_blobs", img, ctx)
    a, kind, w, h, stride = _masked(ops, "erode_blobs", img)
    o, ostride = _out_for(ops, "erode_blobs", a, out)
    ops.call("erode_blobs", kind, ops.ptr(a), w, h, stride, int(max_area), ops.ptr(o), ostride)
    return o


def inpaint(img, bindex, use_grassfire=True, default_inpaint_val=None, semantics="reference", max_len=HOLE_FILL_MAX_LEN, out=None,
            ctx=None):
    """vw::inpaint(img, bindex, use_grassfire, default_inpaint_val) (src/vw/Image/InpaintView.h:44-237) rasterised over
    the whole image.  img: a float kind; bindex: the BlobIndex of blob_index on the same side.  Blobs the edge rule skips
    (semantics 'reference': InpaintView.h:76-80 as written; 'fixed': exactly the blobs touching the border) and blobs
    wider or taller than max_len (<= 64) stay as they are.  default_inpaint_val: the pixel's words, validity last."""
    sem = _edge("inpaint", semantics)
    max_len = _length("inpaint", max_len)
    ops = Operands("inpaint", img, ctx)
    a, kind, w, h, stride = _masked(ops, "inpaint", img, (MASKED_F32, DISPARITY_F32))
    labels = ops.image(bindex.labels, np.int32)
    table = ops.image(bindex.table, np.int32)
    if tuple(labels.shape) != (h, w) or table.ndim != 2 or table.shape[1] != 5 or int(table.shape[0]) < int(bindex.count):
        raise ArgumentErr("inpaint: the blob index does not belong to this image")
    dflt = np.zeros(3, np.float32)
    if default_inpaint_val is not None:
        v = np.asarray(default_inpaint_val, np.float32).reshape(-1)
        if v.size != _CHANNELS[kind]:
            raise ArgumentErr("inpaint: default_inpaint_val must have %d words" % _CHANNELS[kind])
        dflt[:v.size] = v
    o, ostride = _out_for(ops, "inpaint", a, out)
    ops.call("inpaint", kind, ops.ptr(a), w, h, stride, ops.ptr(labels), 0, ops.ptr(table) if bindex.count else None, int(bindex.count),
             1 if use_grassfire else 0, dflt.ctypes.data, sem, max_len, ops.ptr(o), ostride)
    return o


def fill_holes_grass(img, hole_fill_len, semantics="reference", out=None, ctx=None):
    """vw::fill_holes_grass(img, hole_fill_len) (src/vw/Image/InpaintView.h:239-311) rasterised in one call over the
    whole image: the holes (blobs of invalid pixels) whose bounding box is at most hole_fill_len wide and tall are filled
    by the grassfire inpainting.  img: a float kind; hole_fill_len in [0, 64]; out may be img itself."""
    sem = _edge("fill_holes_grass", semantics)
    n = _length("fill_holes_grass", hole_fill_len)
    ops = Operands("fill_holes_grass", img, ctx)
    a, kind, w, h, stride = _masked(ops, "fill_holes_grass", img, (MASKED_F32, DISPARITY_F32))
    o, ostride = _out_for(ops, "fill_holes_grass", a, out)
    ops.call("fill_holes_grass", kind, ops.ptr(a), w, h, stride, n, sem, ops.ptr(o), ostride)
    return o


def fill_nodata_with_avg(img, kernel_size, ctx=None):
    """vw::fill_nodata_with_avg(img, kernel_size) (src/vw/Image/InpaintView.h:317-387) on PixelMask<float> {value,
    valid}: an invalid pixel becomes the mean of the valid pixels of its window, where there are any."""
    if int(kernel_size) <= 0 or int(kernel_size) % 2 == 0:
        raise ArgumentErr("fill_nodata_with_avg: Expecting odd and positive kernel size.")
    ops = Operands("fill_nodata_with_avg", img, ctx)
    a, kind, w, h, stride = _masked(ops, "fill_nodata_with_avg", img, (MASKED_F32,))
    out = ops.empty((h, w, 2), np.float32)
    ops.call("fill_nodata_with_avg", ops.ptr(a), w, h, stride, int(kernel_size), ops.ptr(out), 0)
    return out


# ---- image statistics and intensity scaling (include/vwgpu.h) ------------------------------

HISTOGRAM_MAX_BINS = 4096                                            # VWGPU_HISTOGRAM_MAX_BINS
MIN_MAX_MODES = {"find": 0, "accumulator": 1}                        # vwgpu_min_max_mode
ORDER_RANK, ORDER_MEDIAN, ORDER_PERCENTILE = 0, 1, 2                 # vwgpu_order_kind
RESCALE_CLAMP, RESCALE_NORMALIZE, RESCALE_CLAMP_NORMALIZE, RESCALE_THRESHOLD = 0, 1, 2, 3      # vwgpu_rescale_mode
PIXEL_F32, PIXEL_U8, PIXEL_U8_AS_F32 = 0, 1, 2                       # vwgpu_rescale_pixel


def _gray(ops, name, img, mask=None, sample=None):
    """The leading arguments of a statistics entry: image, cols, rows, row stride, mask, mask stride, and the sampling
    counts (sample = (num_sample_rows, num_sample_cols) as otsu_threshold orders them, None = every pixel)."""
    a = ops.image(img, np.float32, rows=True)
    if a.ndim != 2 or a.shape[0] <= 0 or a.shape[1] <= 0:
        raise ArgumentErr("%s: a non-empty (rows, cols) float32 image expected" % name)
    h, w = int(a.shape[0]), int(a.shape[1])
    m = ops.nonzero_u8(mask)
    if m is not None and tuple(m.shape) != (h, w):
        raise ArgumentErr("%s: the mask must have the image's shape" % name)
    sr, sc = (0, 0) if sample is None else (int(sample[0]), int(sample[1]))
    return a, (ops.ptr(a), w, h, ops.row_stride(a), ops.ptr(m), 0), (sc, sr), m


def min_max(img, mask=None, mode="find", sample=None, ctx=None):
    """(min, max, count, nan_count) over the valid pixels.  mode 'find': find_image_min_max (src/vw/Image/Statistics.h:
    113-127; DBL_MAX, -DBL_MAX when nothing is valid); 'accumulator': min_max_channel_values (:98-108), which raises
    ArgumentErr without a valid sample and keeps a NaN that is the first valid pixel."""
    if mode not in MIN_MAX_MODES:
        raise ArgumentErr("min_max: mode must be 'find' or 'accumulator', not %r" % (mode,))
    ops = Operands("min_max", img, ctx)
    a, lead, samp, m = _gray(ops, "min_max", img, mask, sample)
    r = _lib.ImageRange()
    if ops.tensor:
        ops.call("image_min_max", *(lead + samp + (MIN_MAX_MODES[mode], None, ctypes.byref(r))))
    else:
        ops.call("image_min_max", *(lead + samp + (MIN_MAX_MODES[mode], ctypes.byref(r))))
    return r.min, r.max, r.count, r.nan_count


def moments(img, mask=None, sample=None, ctx=None):
    """(count, sum, sum of squares) of the valid pixels in double (vwgpu_image_moments): reproducible bit for bit, the
    raster-order sums of the reference exactly on integer-valued imagery."""
    ops = Operands("moments", img, ctx)
    a, lead, samp, m = _gray(ops, "moments", img, mask, sample)
    r = (ctypes.c_double * 3)()
    if ops.tensor:
        ops.call("image_moments", *(lead + samp + (None, ctypes.addressof(r))))
    else:
        ops.call("image_moments", *(lead + samp + (ctypes.addressof(r),)))
    return r[0], r[1], r[2]


def _from_moments(name, entry, m):
    r, mom = ctypes.c_double(0), (ctypes.c_double * 3)(*m)
    if getattr(_lib.load(), entry)(ctypes.addressof(mom), ctypes.byref(r)):
        raise ArgumentErr("%s: no valid samples" % name)
    return r.value


def sum_of_channel_values(img, mask=None, ctx=None):
    """sum_of_channel_values (src/vw/Image/Statistics.h:129-137)."""
    return moments(img, mask, ctx=ctx)[1]


def mean(img, mask=None, ctx=None):
    """mean_channel_value (src/vw/Image/Statistics.h:139-148, MeanAccumulator)."""
    return _from_moments("mean", "vwgpu_moments_mean", moments(img, mask, ctx=ctx))


def stddev(img, mask=None, ctx=None):
    """stddev_channel_value (src/vw/Image/Statistics.h:166-172, StdDevAccumulator): normalised by the sample count."""
    return _from_moments("stddev", "vwgpu_moments_stddev", moments(img, mask, ctx=ctx))


def _order(name, img, mask, kind, arg, ctx):
    ops = Operands(name, img, ctx)
    a, lead, samp, m = _gray(ops, name, img, mask)
    r = ctypes.c_double(0)
    if ops.tensor:
        ops.call("image_order_statistic", *(lead + (kind, float(arg), None, ctypes.byref(r))))
    else:
        ops.call("image_order_statistic", *(lead + (kind, float(arg), ctypes.byref(r))))
    return r.value


def median(img, mask=None, ctx=None):
    """median_channel_value (src/vw/Image/Statistics.h:179-186, destructive_median) by an exact radix select, no sort."""
    return _order("median", img, mask, ORDER_MEDIAN, 0.0, ctx)


def percentile(img, p, mask=None, ctx=None):
    """destructive_percentile (src/vw/Math/Functors.h:424-444) of the valid pixels, p in [0, 100] (nearest rank)."""
    return _order("percentile", img, mask, ORDER_PERCENTILE, p, ctx)


def kth_smallest(img, k, mask=None, ctx=None):
    """sorted(valid pixels)[k], k clamped to the last one."""
    return _order("kth_smallest", img, mask, ORDER_RANK, k, ctx)


class Histogram(object):
    """vw::math::Histogram as vw::histogram fills it (saturating).  counts: num_bins + 2 words on the image's side (an
    int64 CUDA tensor or a uint64 numpy array): the bins, the total, the NaN count."""
    __slots__ = ("counts", "num_bins", "min_value", "max_value")

    def __init__(self, counts, num_bins, min_value, max_value):
        self.counts, self.num_bins = counts, int(num_bins)
        self.min_value = float(min_value)
        self.max_value = float(max_value) if max_value != min_value else float(min_value) + 1.0      # ImageThresh.h:61-62

    def host_counts(self):
        c = self.counts.cpu().numpy() if hasattr(self.counts, "cpu") else self.counts
        return np.ascontiguousarray(c).view(np.uint64)

    @property
    def bin_width(self):
        return (self.max_value - self.min_value) / self.num_bins      # Statistics.cc:48-49

    @property
    def total(self):
        return int(self.host_counts()[self.num_bins])

    @property
    def nan_count(self):
        return int(self.host_counts()[self.num_bins + 1])

    def bin_value(self, i):
        return float(self.host_counts()[:self.num_bins][i])

    def bin_center(self, i):
        return self.min_value + i * self.bin_width + self.bin_width / 2.0      # Statistics.cc:52

    def get_percentile(self, percentile):
        c = self.host_counts()
        b = ctypes.c_int(0)
        rc = _lib.load().vwgpu_histogram_percentile(c.ctypes.data, self.num_bins, int(c[self.num_bins]), float(percentile), ctypes.byref(b))
        if rc == -1:
            raise ArgumentErr("get_histogram_percentile: illegal percentile request: %r" % (percentile,))
        if rc:
            raise LogicErr("get_histogram_percentile: Illegal histogram encountered!")
        return b.value


def otsu_from_histogram(hist, overload=1):
    """The threshold either otsu_threshold overload derives from its histogram (vwgpu_otsu_from_histogram)."""
    c = hist.host_counts()
    t = ctypes.c_double(0)
    rc = _lib.load().vwgpu_otsu_from_histogram(c.ctypes.data, hist.num_bins, int(c[hist.num_bins]), hist.min_value, hist.max_value,
                                               int(overload), ctypes.byref(t))
    if rc:
        raise ArgumentErr("otsu_from_histogram: overload must be 1 or 2")
    return t.value


def histogram(img, num_bins, min_val, max_val, mask=None, sample=None, into=None, ctx=None):
    """vw::histogram(view, num_bins, min_val, max_val, hist) (src/vw/Image/ImageThresh.h:53-73).  into: a Histogram of the
    same bins and bounds to add to (the tiles or row strips of a larger image give the counts of the whole image)."""
    if not 1 <= int(num_bins) <= HISTOGRAM_MAX_BINS:
        raise ArgumentErr("histogram: num_bins %d is outside [1, %d]" % (num_bins, HISTOGRAM_MAX_BINS))
    ops = Operands("histogram", img, ctx)
    a, lead, samp, m = _gray(ops, "histogram", img, mask, sample)
    if into is None:
        counts = ops.zeros((int(num_bins) + 2,), np.int64 if ops.tensor else np.uint64)
    else:
        same = Histogram(None, num_bins, min_val, max_val)
        if into.num_bins != same.num_bins or (into.min_value, into.max_value) != (same.min_value, same.max_value):
            raise ArgumentErr("histogram: `into` has other bins or bounds")
        counts = ops.image(into.counts, np.int64 if ops.tensor else np.uint64, in_place=True)
    ops.call("image_histogram", *(lead + samp + (int(num_bins), float(min_val), float(max_val), 1, ops.ptr(counts), None)))
    return Histogram(counts, num_bins, min_val, max_val)


def otsu_threshold(img, num_sample_rows=None, num_sample_cols=None, num_bins=None, mask=None, ctx=None):
    """otsu_threshold(view) with no further argument, otsu_threshold(view, num_sample_rows, num_sample_cols, num_bins)
    with all three (src/vw/Image/ImageThresh.h:80-145, :151-239)."""
    given = [x is not None for x in (num_sample_rows, num_sample_cols, num_bins)]
    if any(given) and not all(given):
        raise ArgumentErr("otsu_threshold: num_sample_rows, num_sample_cols and num_bins go together")
    ops = Operands("otsu_threshold", img, ctx)
    sample = (num_sample_rows, num_sample_cols) if all(given) else None
    a, lead, samp, m = _gray(ops, "otsu_threshold", img, mask, sample)
    t = ctypes.c_double(0)
    ops.call("otsu_threshold", *(lead + samp + (int(num_bins) if all(given) else 256, 2 if all(given) else 1, ctypes.byref(t))))
    return t.value


def _out_type(name, dtype, as_u8):
    dt = np.dtype(dtype)
    if dt == np.uint8:
        return PIXEL_U8, np.uint8
    if dt == np.float32:
        return (PIXEL_U8_AS_F32 if as_u8 else PIXEL_F32), np.float32
    raise ArgumentErr("%s: dtype must be float32 or uint8" % name)


def _rescale(name, img, mode, params, dtype, out, ctx):
    ops = Operands(name, img, ctx)
    a, lead, samp, m = _gray(ops, name, img)
    out_type, dt = _out_type(name, dtype, False)
    if out is None:
        out = ops.empty(tuple(a.shape), dt)
    else:
        out = ops.image(out, dt, in_place=True)
        if tuple(out.shape) != tuple(a.shape):
            raise ArgumentErr("%s: out must have the image's shape" % name)
    p = (ctypes.c_double * len(params))(*[float(x) for x in params])
    ops.call("image_rescale", *(lead[:4] + (mode, ctypes.addressof(p), out_type, ops.ptr(out), 0)))
    return out


def clamp(img, low, high, dtype=np.float32, out=None, ctx=None):
    """clamp(image, low, high) (src/vw/Image/Algorithms.h:50-61).  dtype uint8: pixel_cast<uint8> of the result."""
    return _rescale("clamp", img, RESCALE_CLAMP, (low, high), dtype, out, ctx)


def threshold(img, thresh=0.0, low=0.0, high=1.0, dtype=np.float32, out=None, ctx=None):
    """threshold(image, thresh, low, high) (src/vw/Image/Algorithms.h:192-208): high where the pixel is above thresh."""
    return _rescale("threshold", img, RESCALE_THRESHOLD, (thresh, low, high), dtype, out, ctx)


def _converted(ops, name, a, dtype, as_u8):
    out_type, dt = _out_type(name, dtype, as_u8)
    return out_type, ops.empty(tuple(a.shape), dt)


def normalize(img, *bounds, **kw):
    """normalize(image, old_low, old_high, new_low, new_high) (src/vw/Image/Algorithms.h:171-188) with four bounds;
    normalize(image, low, high) and normalize(image) = (image, 0, 1) of src/vw/Image/AutoNormalize.h:33-86 with two or
    none: old_low, old_high are min_max_channel_values of the valid pixels (mask=), found on the device without a host
    round trip.  Every pixel is converted, the invalid ones too (src/vw/Image/PixelMask.h:514-523).  Keywords: mask, dtype,
    out (four bounds only), clamp=(low, high) to clamp first in the same pass, params=True to return (image, {old_low,
    old_high, low, high}) from the automatic form, ctx."""
    mask, ctx, out, dtype = kw.pop("mask", None), kw.pop("ctx", None), kw.pop("out", None), kw.pop("dtype", np.float32)
    pre, want_params = kw.pop("clamp", None), kw.pop("params", False)
    if kw:
        raise TypeError("normalize: unexpected keyword %s" % sorted(kw)[0])
    if len(bounds) == 4:
        if pre is not None:
            return _rescale("normalize", img, RESCALE_CLAMP_NORMALIZE, tuple(pre) + bounds, dtype, out, ctx)
        return _rescale("normalize", img, RESCALE_NORMALIZE, bounds, dtype, out, ctx)
    if len(bounds) not in (0, 2) or pre is not None or out is not None or np.dtype(dtype) != np.float32:
        raise ArgumentErr("normalize: (image), (image, low, high) or (image, old_low, old_high, new_low, new_high)")
    low, high = bounds if bounds else (0.0, 1.0)
    ops = Operands("normalize", img, ctx)
    a, lead, samp, m = _gray(ops, "normalize", img, mask)
    res = ops.empty(tuple(a.shape), np.float32)
    p = (ctypes.c_double * 4)()
    ops.call("auto_normalize", *(lead + (float(low), float(high), ops.ptr(res), 0, ctypes.addressof(p) if want_params else None)))
    return (res, tuple(p)) if want_params else res


def percentile_scale_convert(img, low_percentile=0.02, high_percentile=0.98, num_bins=256, mask=None, dtype=np.uint8, params=False,
                             ctx=None):
    """percentile_scale_convert (src/vw/Image/ImageThresh.h:243-270): the stretch between the histogram bins at the two
    percentiles (fractions in [0, 1]) to 0..255.  dtype uint8 as the reference, or float32 for the same integer values as
    floats (what stereo.calc_disparity takes on its packed-u8 path).  A tensor call makes no host synchronisation unless
    params=True, which returns (image, (min, max, low_value, high_value))."""
    ops = Operands("percentile_scale_convert", img, ctx)
    a, lead, samp, m = _gray(ops, "percentile_scale_convert", img, mask)
    out_type, res = _converted(ops, "percentile_scale_convert", a, dtype, True)
    p = (ctypes.c_double * 4)()
    ops.call("percentile_scale_convert", *(lead + (float(low_percentile), float(high_percentile), int(num_bins), out_type, ops.ptr(res), 0,
                                                   ctypes.addressof(p) if params else None)))
    return (res, tuple(p)) if params else res


def u8_convert(img, mask=None, dtype=np.uint8, params=False, ctx=None):
    """u8_convert (src/vw/Image/ImageThresh.h:274-286): the stretch between the minimum and the maximum to 0..255."""
    ops = Operands("u8_convert", img, ctx)
    a, lead, samp, m = _gray(ops, "u8_convert", img, mask)
    out_type, res = _converted(ops, "u8_convert", a, dtype, True)
    p = (ctypes.c_double * 4)()
    ops.call("u8_convert", *(lead + (out_type, ops.ptr(res), 0, ctypes.addressof(p) if params else None)))
    return (res, tuple(p)) if params else res
