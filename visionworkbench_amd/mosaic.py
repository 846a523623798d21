"""Host-side mirror of vw::mosaic::ImageComposite (src/vw/Mosaic/ImageComposite.h; include/vwgpu.h, DESIGN.md section
4.24): multi-band blending of positioned images with premultiplied alpha.

Images are numpy arrays or torch CUDA tensors of float32: (rows, cols, 2) is PixelGrayA<float>, (rows, cols, 4) is
PixelRGBA<float>, alpha last; draft mode also takes (rows, cols) or (rows, cols, 1).  The first image decides the side
of the composite: with tensors every call is queued on the current torch stream and patches are CUDA tensors, with
numpy arrays patches are numpy arrays.  Either way the composite keeps its own device copy of every image.
"""
import ctypes

import numpy as np

from . import core
from .core import ArgumentErr, BBox2i
from ._operands import Operands
from .image import _rows


def _box4(b):
    if isinstance(b, BBox2i):
        return (b.min[0], b.min[1], b.max[0], b.max[1])
    b = tuple(int(v) for v in b)
    if len(b) != 4:
        raise ArgumentErr("a box is a BBox2i or (min.x, min.y, max.x, max.y)")
    return b


class ImageComposite(object):
    """ImageComposite<PixelT> with the reference's method names."""

    def __init__(self, ctx=None):
        self._ctx = ctx
        self._ops = None
        self._h = None
        self._channels = 0
        self._shapes = []
        self._draft = self._fill = False

    # -- plumbing --
    def _start(self, anchor):
        self._ops = Operands("ImageComposite", anchor, self._ctx)
        if self._ops.ctx is None:
            self._ops.ctx = core.default_context((self._ops.device.index or 0) if self._ops.tensor else 0)
        self._ctx = self._ops.ctx
        h = ctypes.c_void_p()
        self._ctx.check(self._ctx._lib.vwgpu_composite_create(self._ctx._h, ctypes.byref(h)))
        self._h = h

    def _need(self):
        if self._h is None:
            raise ArgumentErr("ImageComposite: no image was inserted")

    def close(self):
        if self._h is not None and self._ctx is not None and getattr(self._ctx, "_h", None):
            self._ctx._lib.vwgpu_composite_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the reference's interface --
    def insert(self, image, x, y):
        if self._h is None:
            self._start(image)
        ops = self._ops
        ops._side(image, same_device=True)
        if ops.dtype_of(image) != np.float32 or image.ndim not in (2, 3):
            raise ArgumentErr("ImageComposite.insert: a float32 image of (rows, cols[, channels]) expected")
        channels = 1 if image.ndim == 2 else int(image.shape[2])
        a, stride = _rows(ops, "ImageComposite.insert", image, channels)
        ops.call("composite_insert", self._h, ops.ptr(a), int(image.shape[1]), int(image.shape[0]), stride, channels, int(x), int(y))
        self._channels = channels
        self._shapes.append((int(image.shape[0]), int(image.shape[1])))

    def set_draft_mode(self, draft_mode):
        self._draft = bool(draft_mode)
        if self._h is not None:
            self._ctx.check(self._ctx._lib.vwgpu_composite_set_draft_mode(self._ctx._h, self._h, int(self._draft)))

    def set_fill_holes(self, fill_holes):
        self._fill = bool(fill_holes)
        if self._h is not None:
            self._ctx.check(self._ctx._lib.vwgpu_composite_set_fill_holes(self._ctx._h, self._h, int(self._fill)))

    def prepare(self, total_bbox=None):
        self._need()
        self.set_draft_mode(self._draft)      # the flags may have been set before the first insert
        self.set_fill_holes(self._fill)
        box = None if total_bbox is None else (ctypes.c_int * 4)(*_box4(total_bbox))
        if self._ops.tensor:
            import torch
            self._ctx.set_stream(torch.cuda.current_stream(self._ops.device).cuda_stream)
        self._ctx.check(self._ctx._lib.vwgpu_composite_prepare(self._ctx._h, self._h, box))

    def cols(self):
        return 0 if self._h is None else self._ctx._lib.vwgpu_composite_cols(self._h)

    def rows(self):
        return 0 if self._h is None else self._ctx._lib.vwgpu_composite_rows(self._h)

    @property
    def levels(self):
        return 0 if self._h is None else self._ctx._lib.vwgpu_composite_levels(self._h)

    def _bbox(self, which):
        self._need()
        out = (ctypes.c_int * 4)()
        if self._ctx._lib.vwgpu_composite_bbox(self._h, which, out):
            raise ArgumentErr("ImageComposite: no box")
        return BBox2i.from_corners((out[0], out[1]), (out[2], out[3]))

    def bbox(self):
        return self._bbox(0)

    def source_data_bbox(self):
        return self._bbox(1)

    def mask(self, index):
        """The level-0 blending mask of image `index` as a numpy array of 0.0 and 1.0."""
        self._need()
        if not 0 <= int(index) < len(self._shapes):
            raise ArgumentErr("ImageComposite.mask: no image %d" % index)
        out = np.empty(self._shapes[int(index)], np.float32)
        self._ctx.check(self._ctx._lib.vwgpu_composite_mask(self._ctx._h, self._h, int(index), out.ctypes.data, out.shape[1]))
        return out

    def generate_patch(self, patch_bbox, out=None):
        """generate_patch(BBox2i or (min.x, min.y, max.x, max.y)) -> (rows, cols, channels); out: an image of that shape
        whose pixels are contiguous (its rows may be strided) to write into."""
        self._need()
        x0, y0, x1, y1 = _box4(patch_bbox)
        w, h = x1 - x0, y1 - y0
        ops = self._ops
        shape = (max(h, 0), max(w, 0), self._channels)
        if out is None:
            out = ops.empty(shape, np.float32)
            stride = w
            target = out
        else:
            ops._side(out, same_device=True)
            if tuple(out.shape) != shape or ops.dtype_of(out) != np.float32:
                raise ArgumentErr("ImageComposite.generate_patch: out must be float32 of shape %s" % (shape,))
            target, stride = _rows(ops, "ImageComposite.generate_patch", out, self._channels)
            if target is not out:
                raise ArgumentErr("ImageComposite.generate_patch: an image that is written must have contiguous pixels")
        ops.call("composite_generate_patch", self._h, x0, y0, w, h, ops.ptr(target), stride)
        return out

    def generate(self):
        """The whole view."""
        return self.generate_patch((0, 0, self.cols(), self.rows()))

    def __call__(self, x, y):
        """operator()(x, y): the 1 x 1 patch."""
        return self.generate_patch((x, y, x + 1, y + 1))[0, 0]


def blend(images, offsets, fill_holes=False, draft_mode=False, total_bbox=None, ctx=None):
    """The whole mosaic of `images` inserted at `offsets` [(x, y), ...] in one call."""
    if len(images) != len(offsets) or not len(images):
        raise ArgumentErr("blend: as many offsets as images, and at least one")
    c = ImageComposite(ctx)
    try:
        for img, (x, y) in zip(images, offsets):
            c.insert(img, x, y)
        c.set_draft_mode(draft_mode)
        c.set_fill_holes(fill_holes)
        c.prepare(total_bbox)
        return c.generate()
    finally:
        c.close()       # hipFree waits for the work that still reads the composite's memory
