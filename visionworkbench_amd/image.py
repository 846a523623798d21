"""Host-side mirror of the reference's hole filling on masked images (include/vwgpu.h): grassfire
(src/vw/Image/Grassfire.h), BlobIndexThreaded, get_blob_sizes (Image/BlobIndex.h), ErodeView (Image/ErodeView.h),
inpaint, fill_holes_grass and fill_nodata_with_avg (Image/InpaintView.h).

Masked images are numpy arrays or torch CUDA tensors of one of four pixel kinds:
    (rows, cols) uint8              a mask, non-zero = valid
    (rows, cols, 2) float32         PixelMask<float> as {value, valid}
    (rows, cols, 3) int32 / float32 PixelMask<Vector2i> / PixelMask<Vector2f> as {dx, dy, valid}
A view whose rows are further apart than its width (a crop of a wider image) is passed as it is, with its row stride.
"""
import ctypes

import numpy as np

from .core import ArgumentErr, CapacityErr
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
