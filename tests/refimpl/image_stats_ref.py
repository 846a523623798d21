"""ctypes binding of the CPU restatement of the image statistics and intensity scaling (image_stats_ref.cc; test
infrastructure), the C++ program (image_stats_view.cc) and the scenes of the tests."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DBL_MAX = np.finfo(np.float64).max
OUT_DTYPE = {0: np.float32, 1: np.uint8, 2: np.float32}      # vwgpu_rescale_pixel
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "image_stats_ref.mk"])
    return os.path.join(HERE, "libimage_stats_ref.so")


def build_view_program():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "image_stats_view.mk"])
    return os.path.join(HERE, "image_stats_view")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, d, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_uint64
        img = [p, i, i, p]
        _LIB.isr_find_min_max.argtypes = img + [i, i, p, p]
        _LIB.isr_min_max_channel_values.argtypes = img + [i, i, p]
        _LIB.isr_moments.argtypes = img + [i, i, p]
        _LIB.isr_mean.argtypes = [p, p]
        _LIB.isr_stddev.argtypes = [p, p]
        _LIB.isr_histogram.argtypes = img + [i, i, i, d, d, i, p, p]
        _LIB.isr_get_percentile.argtypes = [p, i, u, d]
        _LIB.isr_otsu_counts.argtypes = [p, i, u, d, d, i]
        _LIB.isr_otsu_counts.restype = d
        _LIB.isr_otsu_threshold.argtypes = img + [i, i, i, i]
        _LIB.isr_otsu_threshold.restype = d
        _LIB.isr_order_statistic.argtypes = img + [i, d, p]
        _LIB.isr_rescale.argtypes = [p, i, i, i, p, i, p]
        _LIB.isr_percentile_scale_convert.argtypes = img + [d, d, i, i, p, p, p]
        _LIB.isr_u8_convert.argtypes = img + [i, p, p]
        _LIB.isr_auto_normalize.argtypes = img + [d, d, p, p]
    return _LIB


class NoValidSamples(ValueError):
    """Where the reference throws ("no valid samples", "Illegal histogram encountered")."""


def _img(image, mask):
    a = np.ascontiguousarray(image, np.float32)
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    return a, m, (a.ctypes.data, a.shape[1], a.shape[0], None if m is None else m.ctypes.data)


def _sample(sample):
    """(num_sample_rows, num_sample_cols) -> the (cols, rows) the C side takes."""
    return (0, 0) if sample is None else (int(sample[1]), int(sample[0]))


def find_min_max(image, mask=None, sample=None):
    """(min, max, count, nan_count) of find_image_min_max."""
    a, m, lead = _img(image, mask)
    out, cnt = np.zeros(2), np.zeros(2, np.int64)
    lib().isr_find_min_max(*(lead + _sample(sample) + (out.ctypes.data, cnt.ctypes.data)))
    return float(out[0]), float(out[1]), int(cnt[0]), int(cnt[1])


def min_max_channel_values(image, mask=None, sample=None):
    a, m, lead = _img(image, mask)
    out = np.zeros(2)
    if lib().isr_min_max_channel_values(*(lead + _sample(sample) + (out.ctypes.data,))):
        raise NoValidSamples("MinMaxAccumulator: no valid samples")
    return float(out[0]), float(out[1])


def moments(image, mask=None, sample=None):
    a, m, lead = _img(image, mask)
    out = np.zeros(3)
    lib().isr_moments(*(lead + _sample(sample) + (out.ctypes.data,)))
    return tuple(float(x) for x in out)


def _of_moments(fn, mom):
    m, out = np.asarray(mom, np.float64), np.zeros(1)
    if fn(m.ctypes.data, out.ctypes.data):
        raise NoValidSamples("no valid samples")
    return float(out[0])


def mean(image, mask=None):
    return _of_moments(lib().isr_mean, moments(image, mask))


def stddev(image, mask=None):
    return _of_moments(lib().isr_stddev, moments(image, mask))


def histogram(image, num_bins, min_val, max_val, mask=None, sample=None, into=None):
    """uint64[num_bins + 2]: the bins, the total, the NaN count; also the bin width."""
    a, m, lead = _img(image, mask)
    counts = np.zeros(num_bins + 2, np.uint64) if into is None else into
    width = np.zeros(1)
    rc = lib().isr_histogram(*(lead + _sample(sample) + (num_bins, float(min_val), float(max_val), 0 if into is None else 1,
                                                        counts.ctypes.data, width.ctypes.data)))
    if rc:
        raise ValueError("histogram: number of input bins must be positive")
    return counts, float(width[0])


def get_percentile(counts, num_bins, percentile):
    c = np.ascontiguousarray(counts, np.uint64)
    b = lib().isr_get_percentile(c.ctypes.data, num_bins, int(c[num_bins]), float(percentile))
    if b == -1:
        raise ValueError("illegal percentile request")
    if b < 0:
        raise NoValidSamples("Illegal histogram encountered!")
    return b


def otsu_counts(counts, num_bins, min_val, max_val, overload):
    c = np.ascontiguousarray(counts, np.uint64)
    return lib().isr_otsu_counts(c.ctypes.data, num_bins, int(c[num_bins]), float(min_val), float(max_val), overload)


def otsu_threshold(image, num_sample_rows=None, num_sample_cols=None, num_bins=None, mask=None):
    a, m, lead = _img(image, mask)
    if num_bins is None:
        return lib().isr_otsu_threshold(*(lead + (0, 0, 256, 1)))
    return lib().isr_otsu_threshold(*(lead + (int(num_sample_cols), int(num_sample_rows), int(num_bins), 2)))


def order_statistic(image, kind, arg=0.0, mask=None):
    a, m, lead = _img(image, mask)
    out = np.zeros(1)
    if lib().isr_order_statistic(*(lead + (kind, float(arg), out.ctypes.data))):
        raise NoValidSamples("no valid samples")
    return float(out[0])


def median(image, mask=None):
    return order_statistic(image, 1, 0.0, mask)


def percentile(image, p, mask=None):
    return order_statistic(image, 2, p, mask)


def rescale(image, mode, params, out_type=0):
    a = np.ascontiguousarray(image, np.float32)
    p = np.asarray(params, np.float64)
    out = np.empty(a.shape, OUT_DTYPE[out_type])
    if lib().isr_rescale(a.ctypes.data, a.shape[1], a.shape[0], mode, p.ctypes.data, out_type, out.ctypes.data):
        raise ValueError("rescale: mode")
    return out


def percentile_scale_convert(image, low=0.02, high=0.98, num_bins=256, mask=None, out_type=1):
    """(image, (min, max, low_value, high_value), (low_bin, high_bin))."""
    a, m, lead = _img(image, mask)
    out, params, bins = np.empty(a.shape, OUT_DTYPE[out_type]), np.zeros(4), np.zeros(2, np.int32)
    rc = lib().isr_percentile_scale_convert(*(lead + (float(low), float(high), num_bins, out_type, out.ctypes.data, params.ctypes.data,
                                                      bins.ctypes.data)))
    if rc:
        raise NoValidSamples("percentile_scale_convert: rc %d" % rc)
    return out, tuple(float(x) for x in params), (int(bins[0]), int(bins[1]))


def u8_convert(image, mask=None, out_type=1):
    a, m, lead = _img(image, mask)
    out, params = np.empty(a.shape, OUT_DTYPE[out_type]), np.zeros(4)
    if lib().isr_u8_convert(*(lead + (out_type, out.ctypes.data, params.ctypes.data))):
        raise NoValidSamples("u8_convert: no valid samples")
    return out, tuple(float(x) for x in params)


def auto_normalize(image, low=0.0, high=1.0, mask=None):
    a, m, lead = _img(image, mask)
    out, params = np.empty(a.shape, np.float32), np.zeros(4)
    if lib().isr_auto_normalize(*(lead + (float(low), float(high), out.ctypes.data, params.ctypes.data))):
        raise NoValidSamples("MinMaxAccumulator: no valid samples")
    return out, tuple(float(x) for x in params)


# ---- scenes ---------------------------------------------------------------------------------------------------------

def natural(rows, cols, seed, lo=0.0, hi=1.0):
    """A smooth float image with noise in [lo, hi]."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    v = 0.5 + 0.25 * np.sin(x / 17.0 + seed) * np.cos(y / 11.0) + 0.2 * rng.uniform(-1, 1, (rows, cols))
    v = (v - v.min()) / max(v.max() - v.min(), 1e-30)
    return (lo + (hi - lo) * v).astype(np.float32)


def random_mask(rows, cols, seed, keep=0.7):
    return (np.random.RandomState(seed + 1000).uniform(0, 1, (rows, cols)) < keep).astype(np.uint8)


def same_bits(got, want, what):
    """Equal bit for bit, except that the sign of a zero is not pinned."""
    g, w = np.asarray(got), np.asarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, "%s: %s %s, want %s %s" % (what, g.dtype, g.shape, w.dtype, w.shape)
    if g.dtype.kind == "f":
        ok = (g == w) | (np.isnan(g) & np.isnan(w))
    else:
        ok = g == w
    assert ok.all(), "%s: %d of %d differ, first at %s: %r, want %r" % (
        what, np.count_nonzero(~ok), ok.size, np.argwhere(~ok)[0].tolist(), g[~ok].ravel()[0], w[~ok].ravel()[0])
