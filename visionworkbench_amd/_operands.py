"""The operands of one library call, on whichever side the call is on.

Every wrapper of stereo.py and filters.py serves two entries of libvwgpu.so: vwgpu_<name>_dev for torch CUDA tensors
(asynchronous on the current torch stream, results are CUDA tensors) and vwgpu_<name> for numpy arrays (results are numpy
arrays).  The two take the same argument list; only the spelling of a pointer, of an allocation and of the entry's name
differs, and that spelling lives here.  One anchor operand decides the side of a call.
"""
import ctypes

import numpy as np

from . import core
from .core import ArgumentErr

try:  # torch is plumbing (device memory, streams); the host side works without it
    import torch
except Exception:  # pragma: no cover
    torch = None

_TORCH = {} if torch is None else {np.dtype(n): t for n, t in (
    (np.uint8, torch.uint8), (np.int32, torch.int32), (np.int64, torch.int64), (np.float32, torch.float32),
    (np.float64, torch.float64))}
_NUMPY = {t: n for n, t in _TORCH.items()}


_Tensor = () if torch is None else torch.Tensor


def is_tensor(x):
    return isinstance(x, _Tensor)


def new_stats(n):
    """The int64[n] a library call fills; pass it, or None where the entry skips its counting for a null pointer."""
    return (ctypes.c_longlong * n)()


def put_stats(stats, st):
    if stats is not None:
        stats[:] = list(st)


class Operands(object):
    __slots__ = ("name", "ctx", "device", "tensor")

    def __init__(self, name, anchor, ctx=None):
        """name: the wrapper's, for messages.  A tensor anchor puts the call on its device, a numpy anchor on the host.
        ctx None: the default context of the anchor's device, created when the call is made."""
        self.name, self.ctx, self.device, self.tensor = name, ctx, None, isinstance(anchor, _Tensor)
        if self.tensor:
            if not anchor.is_cuda:
                raise ArgumentErr("%s: torch inputs must be CUDA tensors (no CPU path)" % name)
            self.device = anchor.device

    def image(self, x, dtype, rows=False, in_place=False, same_device=False):
        """The operand as the library takes it; None stays None.  dtype: one numpy dtype, a tuple of allowed ones
        (dtype_of tells which was found) or None for any.
        Host: np.ascontiguousarray(x, dtype), which converts silently; with a tuple the dtype must be one of them.
        Device: a CUDA tensor of exactly that dtype (same_device: on the anchor's device), made contiguous.
        rows: a tensor whose last stride is 1 is passed as it is, with row_stride(): a slice of a wider tensor stays a
        view.  in_place: the library writes into x, so it must be contiguous and of that dtype already, on either side."""
        if x is None:
            return None
        self._side(x, same_device)
        allowed = dtype if isinstance(dtype, tuple) else (dtype,)
        strict = self.tensor or in_place or len(allowed) > 1     # one dtype: a numpy array is converted silently
        if dtype is not None and strict and self.dtype_of(x) not in allowed:
            raise ArgumentErr("%s: %s expected, not %s" % (self.name, " or ".join(np.dtype(t).name for t in allowed), x.dtype))
        if in_place:
            if not (x.is_contiguous() if self.tensor else x.flags.c_contiguous):
                raise ArgumentErr("%s: an image that is modified in place must be contiguous" % self.name)
            return x
        if not self.tensor:
            return np.ascontiguousarray(x, None if strict else dtype)
        return x if rows and x.stride(-1) == 1 else x.contiguous()

    def _side(self, x, same_device=False):
        if isinstance(x, _Tensor) != self.tensor:
            raise ArgumentErr("%s: every image must be %s, as the first one is"
                              % (self.name, "a CUDA tensor" if self.tensor else "a numpy array"))
        if self.tensor and (not x.is_cuda or (same_device and x.device != self.device)):
            raise ArgumentErr("%s: every tensor must be a CUDA tensor%s" % (self.name, " on %s" % self.device if same_device else ""))

    def nonzero_u8(self, x, same_device=False):
        """A validity mask of any dtype as uint8 1 / 0 (None stays None)."""
        if x is None:
            return None
        self._side(x, same_device)
        return (x != 0).to(torch.uint8).contiguous() if self.tensor else np.ascontiguousarray(np.asarray(x) != 0, np.uint8)

    def dtype_of(self, a):
        """The numpy dtype of an operand of either side."""
        return _NUMPY.get(a.dtype) if self.tensor else a.dtype

    def row_stride(self, a):
        """Elements between the rows of a 2-D operand prepared with rows=True."""
        return a.stride(0) if self.tensor else a.shape[1]

    def empty(self, shape, dtype):
        if self.tensor:
            return torch.empty(shape, dtype=_TORCH[np.dtype(dtype)], device=self.device)
        return np.empty(shape, dtype)

    def zeros(self, shape, dtype):
        if self.tensor:
            return torch.zeros(shape, dtype=_TORCH[np.dtype(dtype)], device=self.device)
        return np.zeros(shape, dtype)

    def copy_of(self, x, dtype):
        """A contiguous copy of x for an entry that filters in place."""
        if self.tensor:
            return self.image(x, dtype).clone()
        self._side(x)
        return np.array(x, dtype, order="C", copy=True)

    def ptr(self, a):
        if a is None:
            return None
        return a.data_ptr() if self.tensor else a.ctypes.data

    def call(self, entry, *args):
        """vwgpu_<entry>_dev on the current torch stream of the anchor's device, or vwgpu_<entry>, which never touches
        the stream; the context's handle goes in front of args."""
        ctx = self.ctx
        if ctx is None:
            ctx = self.ctx = core.default_context((self.device.index or 0) if self.tensor else 0)
        if self.tensor:
            ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
            fn = getattr(ctx._lib, "vwgpu_%s_dev" % entry)
        else:
            fn = getattr(ctx._lib, "vwgpu_" + entry)
        ctx.check(fn(ctx._h, *args))
