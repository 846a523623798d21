"""vw::transform on the GPU: the closed-form 2-D map functors of src/vw/Math/Transform.h:231-443 and the free functions of
src/vw/Image/Transform.h:485-843 (transform, transform_nodata, resample, resize, translate, rotate) over the three
interpolations of src/vw/Image/Interpolation.h and the edge extensions of src/vw/Image/EdgeExtension.h.

Images are (rows, cols) float32, with an optional validity mask (PixelMask<float>): numpy in -> numpy out, CUDA tensors in
-> CUDA tensors out on the current torch stream.  Points are transformed on the host by the functions the kernel runs.
"""
import ctypes

import numpy as np

from . import _lib
from . import camera as _camera
from ._operands import Operands
from .core import ArgumentErr
from .stereo import HomographyTransform

IDENTITY, TRANSLATE, RESAMPLE, AFFINE, HOMOGRAPHY = range(5)
FORWARD, REVERSE = 0, 1
MAX_STEPS = 4


# ---- interpolations and edge extensions ------------------------------------------------------------------------------

class NearestPixelInterpolation(object):
    code, pixel_buffer = 0, 1


class BilinearInterpolation(object):
    code, pixel_buffer = 1, 1


class BicubicInterpolation(object):
    code, pixel_buffer = 2, 2


class _Edge(object):
    value, valid = 0.0, False


class ZeroEdgeExtension(_Edge):
    code = 0


class ValueEdgeExtension(_Edge):
    """ValueEdgeExtension<PixelT>(value); valid: the validity of that pixel where the image has a mask."""
    code = 1

    def __init__(self, value, valid=True):
        self.value, self.valid = float(value), bool(valid)


class ConstantEdgeExtension(_Edge):
    code = 2


class PeriodicEdgeExtension(_Edge):
    code = 3


class CylindricalEdgeExtension(_Edge):
    code = 4


class ReflectEdgeExtension(_Edge):
    code = 5


class LinearEdgeExtension(_Edge):
    code = 6


def _tag(x, what):
    """A tag given as a class or as an instance."""
    t = x() if isinstance(x, type) else x
    if not hasattr(t, "code"):
        raise ArgumentErr("transform: %r is no %s" % (x, what))
    return t


# ---- the map functors ----------------------------------------------------------------------------------------------------

def _make(kind, params):
    p = np.ascontiguousarray(params, np.float64).reshape(-1)
    d = _lib.Transform()
    if _lib.load().vwgpu_transform_make(kind, p.ctypes.data if p.size else None, int(p.size), ctypes.byref(d)) != 0:
        raise ArgumentErr("transform: a singular matrix, a parameter that is not finite or a resample factor of 0")
    return d


def descriptors_of(tx):
    """The chain of vwgpu_transform descriptors of a functor, in the order reverse() applies them: a functor of this
    module, a stereo.HomographyTransform (through its matrix / inverse_matrix), a descriptor, or a sequence of descriptors."""
    if hasattr(tx, "descriptors"):
        return tx.descriptors()
    if isinstance(tx, _lib.Transform):
        return [tx]
    if hasattr(tx, "matrix") and hasattr(tx, "inverse_matrix"):
        d = _lib.Transform()
        d.kind = HOMOGRAPHY
        d.fwd[:] = [float(v) for v in np.asarray(tx.matrix, np.float64).reshape(9)]
        d.rev[:] = [float(v) for v in np.asarray(tx.inverse_matrix, np.float64).reshape(9)]
        return [d]
    if isinstance(tx, (list, tuple)) and tx and all(isinstance(d, _lib.Transform) for d in tx):
        return list(tx)
    raise ArgumentErr("transform: %r is no transform functor" % (tx,))


def _steps(tx):
    steps = descriptors_of(tx)
    if not 1 <= len(steps) <= MAX_STEPS:
        raise ArgumentErr("transform: a chain has 1 to %d steps, not %d" % (MAX_STEPS, len(steps)))
    return (_lib.Transform * len(steps))(*steps), len(steps)


def _points(tx, direction, points):
    p = np.ascontiguousarray(points, np.float64)
    if p.ndim < 1 or p.shape[-1] != 2:
        raise ArgumentErr("transform: the points must be (..., 2) {x, y}")
    arr, n = _steps(tx)
    out = np.empty_like(p)
    if _lib.load().vwgpu_transform_points(arr, n, direction, p.ctypes.data, p.size // 2, out.ctypes.data) != 0:
        raise ArgumentErr("transform: the library refused the chain")
    return out


def forward(tx, points):
    """tx.forward of an array of (..., 2) points."""
    return _points(tx, FORWARD, points)


def reverse(tx, points):
    """tx.reverse of an array of (..., 2) points."""
    return _points(tx, REVERSE, points)


class _Functor(object):
    _desc = None

    def descriptors(self):
        return [self._desc]

    def forward(self, points):
        return _points(self, FORWARD, points)

    def reverse(self, points):
        return _points(self, REVERSE, points)


class IdentityTransform(_Functor):
    def __init__(self):
        self._desc = _make(IDENTITY, [])


class TranslateTransform(_Functor):
    def __init__(self, x_translation, y_translation):
        self._desc = _make(TRANSLATE, [x_translation, y_translation])


class ResampleTransform(_Functor):
    def __init__(self, x_scaling, y_scaling):
        self._desc = _make(RESAMPLE, [x_scaling, y_scaling])


class AffineTransform(_Functor):
    """AffineTransform(matrix 2 x 2, offset): forward is matrix p + offset."""

    def __init__(self, matrix, offset):
        m, o = np.asarray(matrix, np.float64), np.asarray(offset, np.float64)
        if m.shape != (2, 2) or o.shape != (2,):
            raise ArgumentErr("AffineTransform: a 2 x 2 matrix and an offset of 2")
        self._desc = _make(AFFINE, list(m.reshape(4)) + list(o))


class LinearTransform(AffineTransform):
    def __init__(self, matrix):
        AffineTransform.__init__(self, matrix, (0.0, 0.0))


class RotateTransform(_Functor):
    """RotateTransform(theta, translate): the rotation by theta about the point translate."""

    def __init__(self, theta, translate=(0.0, 0.0)):
        d = _lib.Transform()
        if _lib.load().vwgpu_transform_rotate(float(theta), float(translate[0]), float(translate[1]), ctypes.byref(d)) != 0:
            raise ArgumentErr("RotateTransform: a parameter is not finite")
        self._desc = d


class InverseTransform(_Functor):
    """InverseTransform(tx): forward and reverse change places."""

    def __init__(self, tx):
        lib, out = _lib.load(), []
        for d in reversed(descriptors_of(tx)):
            inv = _lib.Transform()
            if lib.vwgpu_transform_invert(ctypes.byref(d), ctypes.byref(inv)) != 0:
                raise ArgumentErr("InverseTransform: the library refused a descriptor")
            out.append(inv)
        self._chain = out

    def descriptors(self):
        return list(self._chain)


class CompositionTransform(_Functor):
    """CompositionTransform(tx1, tx2): forward is tx1.forward(tx2.forward(p)), reverse tx2.reverse(tx1.reverse(p))."""

    def __init__(self, tx1, tx2):
        self._chain = descriptors_of(tx1) + descriptors_of(tx2)

    def descriptors(self):
        return list(self._chain)


def compose(tx1, tx2, *more):
    """compose(tx1, tx2[, tx3[, tx4]]) (src/vw/Math/Transform.h:455-483)."""
    txs = (tx1, tx2) + more
    out = txs[-1]
    for tx in reversed(txs[:-1]):
        out = CompositionTransform(tx, out)
    return out


# ---- images ------------------------------------------------------------------------------------------------------------------

def _run(name, image, tx, w, h, x0, y0, edge, interp, mask, nodata, ctx):
    ops = Operands(name, image, ctx)
    if image.ndim != 2:
        raise ArgumentErr("%s: the image must be (rows, cols)" % name)
    img = ops.image(image, np.float32, rows=True)
    sh, sw = int(img.shape[0]), int(img.shape[1])
    m = ops.nonzero_u8(mask, same_device=True)
    if m is not None and tuple(m.shape) != (sh, sw):
        raise ArgumentErr("%s: the mask must have the image's shape" % name)
    w, h = int(w), int(h)
    if sw <= 0 or sh <= 0 or w <= 0 or h <= 0:
        raise ArgumentErr("%s: empty image" % name)
    e, it = _tag(edge, "edge extension"), _tag(interp, "interpolation")
    arr, n = _steps(tx)
    params = _lib.TransformParams(it.code, e.code, e.value, int(e.valid), 0, 0.0, 0)
    if nodata is not None:
        params.nodata, params.nodata_value, params.nodata_valid = 1, float(nodata[0]), int(bool(nodata[1]))
    out = ops.empty((h, w), np.float32)
    out_mask = ops.empty((h, w), np.uint8) if m is not None else None
    ops.call("transform_image", ops.ptr(img), sw, sh, ops.row_stride(img), ops.ptr(m), 0, arr, n, ctypes.byref(params), w, h, int(x0),
             int(y0), ops.ptr(out), 0, ops.ptr(out_mask), 0)
    return out if m is None else (out, out_mask)


def _size(name, image):
    """(cols, rows) of a (rows, cols) image."""
    if image.ndim != 2:
        raise ArgumentErr("%s: the image must be (rows, cols)" % name)
    return int(image.shape[1]), int(image.shape[0])


def _box(image, size, bbox, x0, y0):
    if bbox is not None:
        if size is not None:
            raise ArgumentErr("transform: size or bbox, not both")
        return bbox.width(), bbox.height(), bbox.min[0], bbox.min[1]
    if size is None:
        return _size("transform", image) + (x0, y0)
    return int(size[0]), int(size[1]), x0, y0


def transform(image, tx, size=None, bbox=None, edge=ZeroEdgeExtension, interp=BilinearInterpolation, mask=None, x0=0, y0=0, ctx=None):
    """transform(v, tx[, w, h | bbox][, edge[, interp]]) rasterised (src/vw/Image/Transform.h:485-601): output pixel p is the
    interpolation of the edge-extended image at tx.reverse(p).  size: (cols, rows), the image's own by default; bbox: a
    BBox2i of the transformed space instead; x0, y0: the coordinates of output pixel (0, 0), so that a tile equals that
    region of the whole.  mask: an optional validity mask; the result is then (image, uint8 mask 255 / 0), valid where
    every tap the interpolation used is."""
    w, h, x0, y0 = _box(image, size, bbox, x0, y0)
    return _run("transform", image, tx, w, h, x0, y0, edge, interp, mask, None, ctx)


def transform_nodata(image, tx, size, edge, interp, nodata_val, nodata_valid=False, mask=None, x0=0, y0=0, ctx=None):
    """transform_nodata(v, tx, w, h, edge, interp, nodata_val) (src/vw/Image/Transform.h:606-618): nodata_val where
    tx.reverse(p) comes closer to the image's border than the interpolation's pixel_buffer allows."""
    return _run("transform_nodata", image, tx, size[0], size[1], x0, y0, edge, interp, mask, (nodata_val, nodata_valid), ctx)


def resample(image, x_scale_factor, y_scale_factor=None, size=None, edge=ConstantEdgeExtension, interp=BilinearInterpolation, mask=None,
             ctx=None):
    """resample(v, xf[, yf][, w, h][, edge[, interp]]) (src/vw/Image/Transform.h:624-709): size int(.5 + cols * f)."""
    fx = float(x_scale_factor)
    fy = fx if y_scale_factor is None else float(y_scale_factor)
    if size is None:
        cols, rows = _size("resample", image)
        size = (int(.5 + (cols * fx)), int(.5 + (rows * fy)))
    return _run("resample", image, ResampleTransform(fx, fy), size[0], size[1], 0, 0, edge, interp, mask, None, ctx)


def resize(image, output_width, output_height, edge=ConstantEdgeExtension, interp=BilinearInterpolation, mask=None, ctx=None):
    """resize(v, w, h[, edge[, interp]]) (src/vw/Image/Transform.h:716-747): the factors are w / cols and h / rows."""
    cols, rows = _size("resize", image)
    tx = ResampleTransform(int(output_width) / float(cols), int(output_height) / float(rows))
    return _run("resize", image, tx, output_width, output_height, 0, 0, edge, interp, mask, None, ctx)


def translate(image, x_offset, y_offset, edge=ZeroEdgeExtension, interp=BilinearInterpolation, mask=None, ctx=None):
    """translate(v, x, y[, edge[, interp]]) (src/vw/Image/Transform.h:754-809).  The reference's overload for int offsets is
    an EdgeExtensionView shifted by (-x, -y): the same pixels, since every interpolation returns the pixel itself at an
    integer position."""
    tx = TranslateTransform(float(x_offset), float(y_offset))
    cols, rows = _size("translate", image)
    return _run("translate", image, tx, cols, rows, 0, 0, edge, interp, mask, None, ctx)


def rotate(image, theta, translate=(0.0, 0.0), edge=ZeroEdgeExtension, interp=BilinearInterpolation, mask=None, ctx=None):
    """rotate(v, theta, translate[, edge[, interp]]) (src/vw/Image/Transform.h:817-843)."""
    cols, rows = _size("rotate", image)
    return _run("rotate", image, RotateTransform(theta, translate), cols, rows, 0, 0, edge, interp, mask, None, ctx)


class _Forward(object):
    def __init__(self, tx):
        self.tx = tx

    def forward(self, points):
        return _points(self.tx, FORWARD, points)


def compute_transformed_bbox_fast(roi, tx):
    """compute_transformed_bbox_fast(roi, tx) (src/vw/Image/Transform.h:272-315): (min, max) of the BBox2f grown by the
    forward-transformed perimeter of the BBox2i roi."""
    return _camera.compute_transformed_bbox_fast(roi, _Forward(tx))


__all__ = ["IdentityTransform", "TranslateTransform", "ResampleTransform", "LinearTransform", "AffineTransform", "RotateTransform",
           "HomographyTransform", "InverseTransform", "CompositionTransform", "compose", "descriptors_of", "forward", "reverse",
           "NearestPixelInterpolation", "BilinearInterpolation", "BicubicInterpolation", "ZeroEdgeExtension", "ValueEdgeExtension",
           "ConstantEdgeExtension", "PeriodicEdgeExtension", "CylindricalEdgeExtension", "ReflectEdgeExtension", "LinearEdgeExtension",
           "transform", "transform_nodata", "resample", "resize", "translate", "rotate", "compute_transformed_bbox_fast"]
