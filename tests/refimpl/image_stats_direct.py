"""What each image statistic and intensity scaling MEANS, stated directly in numpy / float64 and independently of
image_stats_ref.cc (which follows the reference's loops): bins by the closed formula, vectorised; order statistics by
np.sort; the rescale by explicit np.float32 / np.float64 steps.  numpy's float64 +, -, *, / and its float32 <-> float64
conversions are the IEEE operations the C++ performs, one rounding each, so the two statements agree to the bit wherever
no summation order is involved."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max


def valid_values(image, mask=None, sample=None):
    """The valid pixels a pass visits, in its order.  sample = (num_sample_rows, num_sample_cols): the grid
    round(i * (rows - 1) / (n - 1)), round half away from zero."""
    a = np.asarray(image, np.float32)
    m = np.ones(a.shape, bool) if mask is None else np.asarray(mask) != 0
    if sample is not None:
        rows, cols = a.shape
        nr, nc = sample
        ri = _round_half_away(np.arange(nr) * ((rows - 1.0) / (nr - 1.0))).astype(np.int64)
        ci = _round_half_away(np.arange(nc) * ((cols - 1.0) / (nc - 1.0))).astype(np.int64)
        a, m = a[np.ix_(ri, ci)], m[np.ix_(ri, ci)]
    return a[m]


def _round_half_away(x):
    x = np.asarray(x, np.float64)
    return np.sign(x) * _floor_half(np.abs(x))


def _floor_half(x):
    """round() of a non-negative double: floor(x) + 1 where the fraction is at least one half (x + 0.5 may round up wrongly)."""
    f = np.floor(x)
    return np.where(x - f >= 0.5, f + 1.0, f)


def find_min_max(image, mask=None, sample=None):
    v = valid_values(image, mask, sample).astype(np.float64)
    v = v[~np.isnan(v)]
    mn = min(DBL_MAX, v.min()) if v.size else DBL_MAX
    mx = max(-DBL_MAX, v.max()) if v.size else -DBL_MAX
    return float(mn), float(mx)


def min_max_accumulator(image, mask=None):
    v = valid_values(image, mask)
    if not v.size:
        return None
    if np.isnan(v[0]):
        return float("nan"), float("nan")
    v = v[~np.isnan(v)]
    return float(v.min()), float(v.max())


def histogram_bins(values, num_bins, min_val, max_val):
    """(bins, nan_count) of the values by (int)round((num_bins - 1) * ((v - min) / range)), saturated."""
    v = np.asarray(values, np.float32).astype(np.float64)
    mn, mx = np.float64(min_val), np.float64(max_val)
    if mx == mn:
        mx = mn + 1.0
    with np.errstate(all="ignore"):
        arg = np.float64(num_bins - 1) * ((v - mn) / (mx - mn))
    nan = np.isnan(arg)
    r = _round_half_away(arg[~nan])
    b = np.clip(r, 0, num_bins - 1).astype(np.int64)
    return np.bincount(b, minlength=num_bins).astype(np.uint64), int(nan.sum())


def percentile_bin(bins, p):
    """The first bin at which the running sum of bins / total reaches p (the additions in bin order, as cumsum does them)."""
    q = np.asarray(bins, np.float64) / np.float64(np.asarray(bins, np.uint64).sum())
    hit = np.nonzero(np.cumsum(q) >= p)[0]
    return int(hit[0]) if hit.size else None


def median(image, mask=None):
    s = np.sort(valid_values(image, mask))
    n = s.size
    if n % 2:
        return float(s[n // 2])
    return float(np.float64(np.float32(s[n // 2 - 1] + s[n // 2])) / 2.0)


def percentile(image, p, mask=None):
    s = np.sort(valid_values(image, mask))
    idx = int(np.ceil((np.float64(p) / 100.0) * np.float64(s.size))) - 1
    return float(s[min(max(idx, 0), s.size - 1)])


def clamp(image, low, high):
    a = np.asarray(image, np.float32)
    lo, hi = np.float32(low), np.float32(high)
    return np.where(a > hi, hi, np.where(a < lo, lo, a)).astype(np.float32)


def normalize(image, old_low, old_high, new_low, new_high):
    a = np.asarray(image, np.float32)
    ol, oh, nl, nh = (np.float32(x) for x in (old_low, old_high, new_low, new_high))
    ratio = np.float64(0.0) if oh == ol else np.float64(np.float32(nh - nl)) / np.float64(np.float32(oh - ol))
    with np.errstate(all="ignore"):
        d = (a - ol).astype(np.float32).astype(np.float64)
        return (d * ratio + np.float64(nl)).astype(np.float32)


def threshold(image, thresh, low, high):
    a = np.asarray(image, np.float32)
    return np.where(a > np.float32(thresh), np.float32(high), np.float32(low)).astype(np.float32)


def to_u8(f):
    """The C truncation, 0 for a NaN or a negative value, 255 from 256 on."""
    f = np.asarray(f, np.float32)
    with np.errstate(all="ignore"):
        t = np.where(f >= 256, 255, np.where(f >= 0, np.trunc(f), 0))
    return np.where(np.isnan(f), 0, t).astype(np.uint8)


def percentile_scale_convert(image, low=0.02, high=0.98, num_bins=256, mask=None):
    """(uint8 image, (min, max, low_value, high_value), (low_bin, high_bin))."""
    mn, mx = find_min_max(image, mask)
    bins, _ = histogram_bins(valid_values(image, mask), num_bins, mn, mx)
    lb, hb = percentile_bin(bins, low), percentile_bin(bins, high)
    width = ((mn + 1.0 if mx == mn else mx) - mn) / np.float64(num_bins)
    lo, hi = np.float64(lb + 1) * width + mn, np.float64(hb + 1) * width + mn
    return to_u8(normalize(clamp(image, lo, hi), lo, hi, 0.0, 255.0)), (mn, mx, float(lo), float(hi)), (lb, hb)


def u8_convert(image, mask=None):
    mn, mx = find_min_max(image, mask)
    hi = mn + 1.0 if mx == mn else mx
    return to_u8(normalize(clamp(image, mn, hi), mn, hi, 0.0, 255.0)), (mn, mx, mn, hi)
