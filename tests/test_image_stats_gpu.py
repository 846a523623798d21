"""GPU: every entry of the image statistics and intensity scaling family (csrc/image_stats.hip), through the C ABI and the
Python wrappers, on device tensors and on host arrays, against the CPU restatement (tests/refimpl/image_stats_ref.cc).

Equal to the bit: extrema, counts, every histogram bin, the percentile bins, both Otsu thresholds, the median and the
percentiles, every pixel of clamp / normalize / threshold in float and uint8, every pixel and all four parameters of
percentile_scale_convert, u8_convert and the automatic normalize.  The moments: equal on integer-valued imagery (every
partial sum of any order is an integer below 2^53), else sum and sum of squares within
    2 (N - 1) u / (1 - (N - 1) u) * sum |term|,  u = 2^-53, N = the number of terms,
of the raster-order sums: each of the two summation orders is within (N - 1) u / (1 - (N - 1) u) * sum |term| of the exact
sum (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4: any order), and the terms themselves are the
same doubles on both sides (a float and the product of two floats are exact in double)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import image_stats_ref as ref  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import _lib, core, image, stereo, synth  # noqa: E402
from visionworkbench_amd.core import ArgumentErr  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    c = vwa.Context(0)
    yield c
    c.close()


def dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return None if x is None else np.ascontiguousarray(x)


def arr(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


SIDES = {"device": dev, "host": host}


def moments_close(got, img, mask, what):
    """Exact on integer-valued imagery, else within the bound of the module's docstring, computed from the input."""
    want = ref.moments(img, mask)
    v = np.asarray(img, np.float32)[np.ones(img.shape, bool) if mask is None else np.asarray(mask) != 0].astype(np.float64)
    print("%s: moments %r, restatement %r" % (what, got, want))
    assert got[0] == want[0] == v.size, what
    if v.size and np.all(v == np.round(v)) and np.abs(v).max() <= 4095:
        assert got == want, what
        return
    n = max(v.size - 1, 0)
    for k, terms in ((1, np.abs(v)), (2, v * v)):
        bound = 2 * n * U / (1 - n * U) * float(terms.sum())
        assert abs(got[k] - want[k]) <= bound, "%s: moment %d off by %g, bound %g" % (what, k, abs(got[k] - want[k]), bound)


def check_everything(img, mask, side, ctx, what, bins=(256,), percentiles=(0.02, 0.98), ranks=(0.0, 37.5, 100.0)):
    """Every wrapper on one image on one side against the restatement."""
    to = SIDES[side]
    a, m = to(img), to(mask)
    what = "%s %s" % (what, side)
    want = ref.find_min_max(img, mask)
    assert image.min_max(a, m, ctx=ctx) == want, what
    valid_numbers = want[2] > want[3]
    try:
        acc = ref.min_max_channel_values(img, mask)
    except ref.NoValidSamples:
        with pytest.raises(ArgumentErr):
            image.min_max(a, m, mode="accumulator", ctx=ctx)
    else:
        got = image.min_max(a, m, mode="accumulator", ctx=ctx)
        ref.same_bits(np.array(got[:2]), np.array(acc), what + " accumulator")
    got = image.moments(a, m, ctx=ctx)
    assert np.array(got).tobytes() == np.array(image.moments(a, m, ctx=ctx)).tobytes(), what + ": two calls differ"
    if want[3] == 0:
        moments_close(got, img, mask, what)
    mn, mx = want[0], want[1]
    for nb in bins:
        h = image.histogram(a, nb, mn, mx, mask=m, ctx=ctx)
        counts, width = ref.histogram(img, nb, mn, mx, mask)
        assert np.array_equal(h.host_counts(), counts), "%s: histogram of %d bins" % (what, nb)
        assert (h.bin_width == width or not valid_numbers) and h.total == counts[nb] and h.nan_count == counts[nb + 1]
        if counts[nb]:
            for p in percentiles:
                assert h.get_percentile(p) == ref.get_percentile(counts, nb, p), what
    assert image.otsu_threshold(a, mask=m, ctx=ctx) == ref.otsu_threshold(img, mask=mask), what
    rows, cols = img.shape
    if rows > 1 and cols > 1:
        for sr, sc, nb in ((rows, cols, 256), (max(2, rows // 3), max(2, cols // 2), 64)):
            assert image.otsu_threshold(a, sr, sc, nb, mask=m, ctx=ctx) == ref.otsu_threshold(img, sr, sc, nb, mask=mask), what
    if want[3] or not want[2]:
        with pytest.raises(ArgumentErr):
            image.median(a, m, ctx=ctx)
    else:
        assert image.median(a, m, ctx=ctx) == ref.median(img, mask), what
        for p in ranks:
            assert image.percentile(a, p, m, ctx=ctx) == ref.percentile(img, p, mask), "%s: percentile %r" % (what, p)
    if valid_numbers:
        lo, hi = mn + 0.2 * (mx - mn), mn + 0.7 * (mx - mn)
    else:
        lo, hi = -1.0, 1.0
    for dt, ot in ((np.float32, 0), (np.uint8, 1)):
        ref.same_bits(arr(image.clamp(a, lo, hi, dtype=dt, ctx=ctx)), ref.rescale(img, 0, [lo, hi], ot), what + " clamp")
        ref.same_bits(arr(image.normalize(a, lo, hi, -3.0, 200.5, dtype=dt, ctx=ctx)), ref.rescale(img, 1, [lo, hi, -3.0, 200.5], ot), what + " normalize")
        ref.same_bits(arr(image.normalize(a, lo, hi, 0.0, 255.0, clamp=(lo, hi), dtype=dt, ctx=ctx)),
                      ref.rescale(img, 2, [lo, hi, lo, hi, 0.0, 255.0], ot), what + " clamp + normalize")
        ref.same_bits(arr(image.threshold(a, lo, 3.0, 250.0, dtype=dt, ctx=ctx)), ref.rescale(img, 3, [lo, 3.0, 250.0], ot), what + " threshold")
    for dt, ot in ((np.uint8, 1), (np.float32, 2)):
        try:
            wimg, wparams, _ = ref.percentile_scale_convert(img, percentiles[0], percentiles[1], bins[0], mask, ot)
        except ref.NoValidSamples:
            with pytest.raises(ArgumentErr):
                image.percentile_scale_convert(a, percentiles[0], percentiles[1], bins[0], mask=m, dtype=dt, params=True, ctx=ctx)
        else:
            gimg, gparams = image.percentile_scale_convert(a, percentiles[0], percentiles[1], bins[0], mask=m, dtype=dt, params=True, ctx=ctx)
            assert gparams == wparams, "%s: percentile_scale_convert parameters %r, want %r" % (what, gparams, wparams)
            ref.same_bits(arr(gimg), wimg, what + " percentile_scale_convert")
            ref.same_bits(arr(image.percentile_scale_convert(a, percentiles[0], percentiles[1], bins[0], mask=m, dtype=dt, ctx=ctx)), wimg,
                          what + " percentile_scale_convert without parameters")
        try:
            wimg, wparams = ref.u8_convert(img, mask, ot)
        except ref.NoValidSamples:
            with pytest.raises(ArgumentErr):
                image.u8_convert(a, mask=m, dtype=dt, params=True, ctx=ctx)
        else:
            gimg, gparams = image.u8_convert(a, mask=m, dtype=dt, params=True, ctx=ctx)
            assert gparams == wparams, what
            ref.same_bits(arr(gimg), wimg, what + " u8_convert")
    try:
        wimg, wparams = ref.auto_normalize(img, -0.5, 2.0, mask)
    except ref.NoValidSamples:
        with pytest.raises(ArgumentErr):
            image.normalize(a, -0.5, 2.0, mask=m, params=True, ctx=ctx)
    else:
        gimg, gparams = image.normalize(a, -0.5, 2.0, mask=m, params=True, ctx=ctx)
        ref.same_bits(np.array(gparams), np.array(wparams), what + " normalize parameters")
        ref.same_bits(arr(gimg), wimg, what + " automatic normalize")
        ref.same_bits(arr(image.normalize(a, mask=m, ctx=ctx)), ref.auto_normalize(img, 0.0, 1.0, mask)[0], what + " normalize(image)")


# ---- shapes ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", sorted(SIDES))
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 67), (67, 1)])
def test_degenerate_sizes(ctx, rows, cols, side):
    img = ref.natural(rows, cols, rows + cols, -2.0, 5.0)
    check_everything(img, None, side, ctx, "%dx%d" % (cols, rows))
    check_everything(img, ref.random_mask(rows, cols, 3, 0.6) | (np.arange(rows * cols).reshape(rows, cols) == 0), side, ctx,
                     "%dx%d masked" % (cols, rows))


@pytest.mark.parametrize("side", sorted(SIDES))
def test_several_workgroups(ctx, side):
    """1031 x 517: several workgroups, a ragged last one and a real fold of the slabs."""
    img = ref.natural(517, 1031, 9, 100.0, 3000.0)
    check_everything(img, ref.random_mask(517, 1031, 9), side, ctx, "1031x517", bins=(256, 4096))


def test_strided_and_misaligned(ctx):
    """333 x 77 at a row stride of 340 pixels, starting 4 bytes past a 16-byte boundary: 16-byte loads with both ragged ends.
    The device side through the wrappers (a view of a wider tensor), the host side through the C ABI with its strides."""
    rows, cols, stride = 77, 333, 340
    img = ref.natural(rows, cols, 21, -7.0, 9.0)
    mask = ref.random_mask(rows, cols, 21)
    buf = torch.full((rows * stride + 8,), float("nan"), device="cuda")
    view = buf[1:1 + rows * stride].view(rows, stride)[:, :cols]
    view.copy_(dev(img))
    assert view.data_ptr() % 16 == 4 and view.stride(0) == stride
    mbuf = torch.zeros((rows * stride + 8,), dtype=torch.uint8, device="cuda")
    mview = mbuf[3:3 + rows * stride].view(rows, stride)[:, :cols]
    mview.copy_(dev(mask))
    want = ref.find_min_max(img, mask)
    assert image.min_max(view, mask=None, ctx=ctx) == ref.find_min_max(img)      # the NaN padding between the rows is never read
    assert image.min_max(view, dev(mask), ctx=ctx) == want
    assert image.moments(view, ctx=ctx) == image.moments(dev(img), ctx=ctx) == image.moments(img, ctx=ctx)      # the same bits wherever the image lies
    moments_close(image.moments(view, ctx=ctx), img, None, "strided")
    counts, _ = ref.histogram(img, 300, want[0], want[1], mask)
    assert np.array_equal(image.histogram(view, 300, want[0], want[1], mask=dev(mask), ctx=ctx).host_counts(), counts)
    assert image.median(view, dev(mask), ctx=ctx) == ref.median(img, mask)
    ref.same_bits(arr(image.percentile_scale_convert(view, mask=dev(mask), ctx=ctx)), ref.percentile_scale_convert(img, mask=mask)[0], "strided convert")
    ref.same_bits(arr(image.normalize(view, -1.0, 2.0, 0.0, 255.0, dtype=np.uint8, ctx=ctx)), ref.rescale(img, 1, [-1.0, 2.0, 0.0, 255.0], 1), "strided rescale")
    # the C ABI: strided device pointers for image, mask and output, then strided host pointers
    lib = ctx._lib
    h = ctx._h
    r = _lib.ImageRange()
    ctx.check(lib.vwgpu_image_min_max_dev(h, view.data_ptr(), cols, rows, stride, mview.data_ptr(), stride, 0, 0, 0, None, ctypes.byref(r)))
    assert (r.min, r.max, r.count, r.nan_count) == want
    out = torch.full((rows, stride), -1.0, device="cuda")
    p = (ctypes.c_double * 4)()
    ctx.check(lib.vwgpu_percentile_scale_convert_dev(h, view.data_ptr(), cols, rows, stride, mview.data_ptr(), stride, 0.02, 0.98, 256, 2,
                                                     out.data_ptr() + 4, stride, ctypes.addressof(p)))
    wimg, wparams, _ = ref.percentile_scale_convert(img, mask=mask, out_type=2)
    flat = out.cpu().numpy().reshape(-1)
    got = np.lib.stride_tricks.as_strided(flat[1:], (rows, cols), (stride * 4, 4))
    ref.same_bits(np.ascontiguousarray(got), wimg, "C ABI strided convert")
    assert tuple(p) == wparams and flat[0] == -1.0 and np.all(out.cpu().numpy()[:-1, cols + 1:] == -1.0)      # nothing written between the rows
    hbuf = np.full(rows * stride + 8, np.nan, np.float32)
    hview = np.lib.stride_tricks.as_strided(hbuf[1:], (rows, cols), (stride * 4, 4))
    hview[:] = img
    hm = np.zeros((rows, stride), np.uint8)
    hm[:, :cols] = mask
    ctx.check(lib.vwgpu_image_min_max(h, hview.ctypes.data, cols, rows, stride, hm.ctypes.data, stride, 0, 0, 0, ctypes.byref(r)))
    assert (r.min, r.max, r.count, r.nan_count) == want
    mom = (ctypes.c_double * 3)()
    ctx.check(lib.vwgpu_image_moments(h, hview.ctypes.data, cols, rows, stride, None, 0, 0, 0, ctypes.addressof(mom)))
    assert tuple(mom) == image.moments(view, ctx=ctx)
    hc = np.zeros(302, np.uint64)
    ctx.check(lib.vwgpu_image_histogram(h, hview.ctypes.data, cols, rows, stride, hm.ctypes.data, stride, 0, 0, 300, want[0], want[1], 0,
                                        hc.ctypes.data, None))
    assert np.array_equal(hc, counts)
    med = ctypes.c_double(0)
    ctx.check(lib.vwgpu_image_order_statistic(h, hview.ctypes.data, cols, rows, stride, hm.ctypes.data, stride, 1, 0.0, ctypes.byref(med)))
    assert med.value == ref.median(img, mask)
    hout = np.full((rows, stride), 7, np.uint8)
    ctx.check(lib.vwgpu_u8_convert(h, hview.ctypes.data, cols, rows, stride, hm.ctypes.data, stride, 1, hout.ctypes.data, stride, None))
    ref.same_bits(np.ascontiguousarray(hout[:, :cols]), ref.u8_convert(img, mask)[0], "C ABI strided host u8_convert")
    assert np.all(hout[:, cols:] == 7)


@pytest.mark.parametrize("side", sorted(SIDES))
def test_constant_image(ctx, side):
    """max == min becomes min + 1, and every lane of every wavefront counts into one bin."""
    img = np.full((64, 64), 12.5, np.float32)
    check_everything(img, None, side, ctx, "constant")
    h = image.histogram(SIDES[side](img), 256, 12.5, 12.5, ctx=ctx)
    assert h.bin_value(0) == 64 * 64 and h.bin_width == 1.0 / 256
    two = img.copy()
    two[:, 32:] = 12.5 + 1.0 / 255      # two neighbouring bins
    check_everything(two, None, side, ctx, "two neighbouring bins")


@pytest.mark.parametrize("side", sorted(SIDES))
def test_half_way_bins_and_saturation(ctx, side):
    """Bin arguments at exact .5 (round goes away from zero), values below min (negative arguments, which saturate to bin 0, the
    half-way ones among them) and above max."""
    nb, mn, mx = 9, 0.0, 16.0                       # max_bin * (v - 0) / 16 = v / 2: every odd v sits on a half
    v = np.arange(-20, 44, dtype=np.float32)
    img = np.tile(v, (64, 1))
    a = SIDES[side](img)
    counts, _ = ref.histogram(img, nb, mn, mx)
    assert np.array_equal(image.histogram(a, nb, mn, mx, ctx=ctx).host_counts(), counts)
    want = np.zeros(nb + 2, np.uint64)
    for x in v:
        r = np.floor(abs(x) / 2 + 0.5) * (1 if x >= 0 else -1)      # x / 2 is exact; half away from zero
        want[int(min(max(r, 0), nb - 1))] += 64
    want[nb] = img.size
    assert np.array_equal(counts, want)
    check_everything(img, None, side, ctx, "half-way bins", bins=(9, 256))


@pytest.mark.parametrize("side", sorted(SIDES))
def test_no_valid_pixel_then_one(ctx, side):
    img = ref.natural(96, 96, 4, 0.0, 1.0)
    mask = np.zeros((96, 96), np.uint8)
    check_everything(img, mask, side, ctx, "no valid pixel")
    assert image.min_max(SIDES[side](img), SIDES[side](mask), ctx=ctx) == (ref.DBL_MAX, -ref.DBL_MAX, 0, 0)
    assert image.otsu_threshold(SIDES[side](img), mask=SIDES[side](mask), ctx=ctx) == 0.0
    with pytest.raises(ArgumentErr):
        image.mean(SIDES[side](img), SIDES[side](mask), ctx=ctx)
    mask[61, 17] = 1
    check_everything(img, mask, side, ctx, "one valid pixel")
    assert image.median(SIDES[side](img), SIDES[side](mask), ctx=ctx) == float(img[61, 17])
    assert image.mean(SIDES[side](img), SIDES[side](mask), ctx=ctx) == float(img[61, 17])
    assert image.stddev(SIDES[side](img), SIDES[side](mask), ctx=ctx) == ref.stddev(img, mask)


@pytest.mark.parametrize("side", sorted(SIDES))
def test_bin_counts_up_to_the_limit(ctx, side):
    img = ref.natural(128, 128, 8, -3.0, 3.0)
    a = SIDES[side](img)
    mn, mx = ref.find_min_max(img)[:2]
    for nb in (1, 2, 256, 1000, image.HISTOGRAM_MAX_BINS):
        counts, _ = ref.histogram(img, nb, mn, mx)
        assert np.array_equal(image.histogram(a, nb, mn, mx, ctx=ctx).host_counts(), counts), nb
    ref.same_bits(arr(image.percentile_scale_convert(a, 0.1, 0.9, image.HISTOGRAM_MAX_BINS, ctx=ctx)),
                  ref.percentile_scale_convert(img, 0.1, 0.9, image.HISTOGRAM_MAX_BINS)[0], "convert at the limit")
    with pytest.raises(ArgumentErr):
        image.histogram(a, image.HISTOGRAM_MAX_BINS + 1, mn, mx, ctx=ctx)
    with pytest.raises(ArgumentErr):
        image.percentile_scale_convert(a, 0.1, 0.9, image.HISTOGRAM_MAX_BINS + 1, ctx=ctx)
    counts = np.zeros(image.HISTOGRAM_MAX_BINS + 3, np.uint64)
    rc = ctx._lib.vwgpu_image_histogram(ctx._h, img.ctypes.data, 128, 128, 0, None, 0, 0, 0, image.HISTOGRAM_MAX_BINS + 1, mn, mx, 0,
                                        counts.ctypes.data, None)
    assert rc == -1 and not counts.any()


@pytest.mark.parametrize("side", sorted(SIDES))
def test_row_strips_accumulate_to_the_whole(ctx, side):
    img = ref.natural(129, 257, 6, 0.0, 900.0)
    mask = ref.random_mask(129, 257, 6)
    mn, mx = ref.find_min_max(img, mask)[:2]
    whole, _ = ref.histogram(img, 500, mn, mx, mask)
    h = None
    for r0, r1 in ((0, 40), (40, 41), (41, 129)):
        h = image.histogram(SIDES[side](img[r0:r1]), 500, mn, mx, mask=SIDES[side](mask[r0:r1]), into=h, ctx=ctx)
    assert np.array_equal(h.host_counts(), whole)
    assert np.array_equal(image.histogram(SIDES[side](img), 500, mn, mx, mask=SIDES[side](mask), ctx=ctx).host_counts(), whole)


@pytest.mark.parametrize("side", sorted(SIDES))
def test_sampling_grids(ctx, side):
    img = ref.natural(100, 200, 2, -1.0, 1.0)
    mask = ref.random_mask(100, 200, 2, 0.8)
    a, m = SIDES[side](img), SIDES[side](mask)
    for sample in ((2, 2), (23, 17), (100, 200)):
        want = ref.find_min_max(img, mask, sample)
        assert image.min_max(a, m, sample=sample, ctx=ctx) == want, sample
        counts, _ = ref.histogram(img, 128, want[0], want[1], mask, sample)
        assert np.array_equal(image.histogram(a, 128, want[0], want[1], mask=m, sample=sample, ctx=ctx).host_counts(), counts), sample
        got = image.moments(a, m, sample=sample, ctx=ctx)
        w = ref.moments(img, mask, sample)
        n = max(w[0] - 1, 0)
        assert got[0] == w[0] and abs(got[1] - w[1]) <= 2 * n * U / (1 - n * U) * w[0] and abs(got[2] - w[2]) <= 2 * n * U / (1 - n * U) * w[0]      # |x| <= 1
        assert image.otsu_threshold(a, sample[0], sample[1], 128, mask=m, ctx=ctx) == ref.otsu_threshold(img, sample[0], sample[1], 128, mask=mask)
    assert image.min_max(a, m, sample=(100, 200), ctx=ctx) == image.min_max(a, m, ctx=ctx)            # the full grid is no sampling
    assert np.array_equal(image.histogram(a, 128, -1.0, 1.0, mask=m, sample=(100, 200), ctx=ctx).host_counts(),
                          image.histogram(a, 128, -1.0, 1.0, mask=m, ctx=ctx).host_counts())
    for bad in ((1, 5), (5, 1), (0, 5)):
        with pytest.raises(ArgumentErr):
            image.min_max(a, m, sample=bad, ctx=ctx)


@pytest.mark.parametrize("side", sorted(SIDES))
def test_nan_inputs(ctx, side):
    img = ref.natural(64, 64, 11, 0.0, 1.0)
    img[0, 0] = img[5, 63] = img[63, 1] = np.nan
    mask = np.ones((64, 64), np.uint8)
    mask[0, 0] = 0
    check_everything(img, None, side, ctx, "NaN first")         # the accumulator keeps a NaN that is its first sample
    check_everything(img, mask, side, ctx, "NaN later")         # and ignores the later ones
    a = SIDES[side](img)
    assert image.min_max(a, ctx=ctx)[3] == 3 and image.min_max(a, SIDES[side](mask), ctx=ctx)[3] == 2
    assert all(np.isnan(x) for x in image.min_max(a, mode="accumulator", ctx=ctx)[:2])
    mn, mx = ref.find_min_max(img)[:2]
    h = image.histogram(a, 100, mn, mx, ctx=ctx)
    assert h.nan_count == 3 and h.total == 64 * 64 - 3
    assert arr(image.normalize(a, mn, mx, 0.0, 255.0, dtype=np.uint8, ctx=ctx))[0, 0] == 0
    for call in (lambda: image.median(a, ctx=ctx), lambda: image.percentile(a, 50.0, ctx=ctx)):
        with pytest.raises(ArgumentErr):
            call()
    masked = mask.copy()
    masked[5, 63] = masked[63, 1] = 0
    assert image.median(a, SIDES[side](masked), ctx=ctx) == ref.median(img, masked)       # no NaN among the valid pixels: defined again


def _digit_boundary_values():
    """Floats whose order-preserving keys differ only below, only in, and across the three digits (12, 12 and 8 bits) of the
    select, on both sides of zero, with duplicates."""
    bits = []
    for base in (0x3f800000, 0x3f8000ff, 0x3f800100, 0x3f8fffff, 0x3f900000, 0x3f900001, 0x40000000, 0x00000001, 0x00000000, 0x7f7fffff):
        bits += [base, base, base | 0x80000000]
    v = np.array(bits, np.uint32).view(np.float32)
    return v[np.isfinite(v)]


@pytest.mark.parametrize("side", sorted(SIDES))
def test_median_and_the_radix_digits(ctx, side):
    vals = _digit_boundary_values()
    rng = np.random.RandomState(5)
    img = rng.choice(vals, 64 * 64).astype(np.float32).reshape(64, 64)
    to = SIDES[side]
    for name, mask in (("even count", None), ("odd count", (np.arange(4096).reshape(64, 64) != 77).astype(np.uint8)),
                       ("three pixels", (np.arange(4096).reshape(64, 64) < 3).astype(np.uint8))):
        assert image.median(to(img), to(mask), ctx=ctx) == ref.median(img, mask), name
        for p in (0.0, 0.01, 25.0, 50.0, 99.99, 100.0):
            assert image.percentile(to(img), p, to(mask), ctx=ctx) == ref.percentile(img, p, mask), (name, p)
    s = np.sort(img.reshape(-1))
    for k in (0, 1, 2047, 2048, 4095, 5000):
        assert image.kth_smallest(to(img), k, ctx=ctx) == float(s[min(k, 4095)]), k
    two = np.array([[1.0, 1.0000001]], np.float32)       # the float sum of the two middles, divided in double
    assert image.median(to(two), ctx=ctx) == ref.median(two) == float(np.float64(np.float32(two[0, 0] + two[0, 1])) / 2.0)
    with pytest.raises(ArgumentErr):
        image.percentile(to(img), 100.5, ctx=ctx)


# ---- integer-valued imagery, seeded random cases ----------------------------------------------------------------------

@pytest.mark.parametrize("top", [255, 4095])
def test_moments_are_exact_on_integer_valued_imagery(ctx, top):
    rng = np.random.RandomState(top)
    img = rng.randint(0, top + 1, (517, 1031)).astype(np.float32)
    mask = ref.random_mask(517, 1031, top)
    for m in (None, mask):
        want = ref.moments(img, m)
        assert image.moments(dev(img), dev(m), ctx=ctx) == want
        assert image.moments(img, m, ctx=ctx) == want
        assert image.mean(dev(img), dev(m), ctx=ctx) == ref.mean(img, m) and image.stddev(dev(img), dev(m), ctx=ctx) == ref.stddev(img, m)
        assert image.sum_of_channel_values(dev(img), dev(m), ctx=ctx) == want[1]


class TestSeededRandom(object):
    """Sizes up to 300 x 300; masks, ranges, bins and percentiles vary with the seed."""

    @pytest.mark.parametrize("seed", range(10))
    def test_case(self, ctx, seed):
        rng = np.random.RandomState(4000 + seed)
        rows, cols = int(rng.randint(1, 301)), int(rng.randint(1, 301))
        lo = float(rng.uniform(-1000, 1000))
        img = ref.natural(rows, cols, seed, lo, lo + float(rng.choice([1e-4, 0.8, 255.0, 65535.0])))
        if seed % 4 == 3:
            img = np.round(img)
        mask = None if seed % 3 == 0 else ref.random_mask(rows, cols, seed, float(rng.uniform(0.05, 0.95)))
        if mask is not None:
            mask[rng.randint(rows), rng.randint(cols)] = 1
        lowp = float(rng.uniform(0, 0.3))
        check_everything(img, mask, "device" if seed % 2 else "host", ctx, "seed %d %dx%d" % (seed, cols, rows),
                         bins=(int(rng.choice([16, 256, 777, 4096])),), percentiles=(lowp, float(rng.uniform(lowp, 1.0))),
                         ranks=(0.0, float(rng.uniform(0, 100)), 100.0))


# ---- no host round trip, end to end --------------------------------------------------------------------------------

def test_device_results_without_synchronising(ctx):
    """The _dev forms with device results only: what they leave in device memory equals what the host forms return."""
    img = ref.natural(200, 300, 31, 5.0, 6.0)
    a = dev(img)
    lib, h = ctx._lib, ctx._h
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d_range = torch.zeros(4, dtype=torch.float64, device="cuda")
    d_mom = torch.zeros(3, dtype=torch.float64, device="cuda")
    d_med = torch.zeros(1, dtype=torch.float64, device="cuda")
    ctx.check(lib.vwgpu_image_min_max_dev(h, a.data_ptr(), 300, 200, 0, None, 0, 0, 0, 1, d_range.data_ptr(), None))
    ctx.check(lib.vwgpu_image_moments_dev(h, a.data_ptr(), 300, 200, 0, None, 0, 0, 0, d_mom.data_ptr(), None))
    ctx.check(lib.vwgpu_image_order_statistic_dev(h, a.data_ptr(), 300, 200, 0, None, 0, 1, 0.0, d_med.data_ptr(), None))
    torch.cuda.synchronize()
    assert tuple(d_range.cpu().numpy()[:2]) == ref.min_max_channel_values(img)
    assert d_range.cpu().numpy()[2:].view(np.int64).tolist() == [img.size, 0]
    assert tuple(d_mom.cpu().numpy()) == image.moments(img, ctx=ctx)
    assert float(d_med.cpu()[0]) == ref.median(img)
    nan = img.copy()
    nan[3, 3] = np.nan
    ctx.check(lib.vwgpu_image_order_statistic_dev(h, dev(nan).data_ptr(), 300, 200, 0, None, 0, 1, 0.0, d_med.data_ptr(), None))
    torch.cuda.synchronize()
    assert np.isnan(float(d_med.cpu()[0]))


def test_converted_pair_takes_the_packed_u8_matcher(ctx):
    """Float imagery in [0.1, 0.9] goes through percentile_scale_convert on the device (float output: integer values 0..255) and
    then through calc_disparity, which takes its packed-u8 SAD path for it; the disparities are the oracle's on the
    restatement's converted pair."""
    import oracle
    left, right, _ = synth.stereo_pair(320, 96, 33, 1, block=64)
    fl = (np.float32(0.1) + np.float32(0.8) * (left / np.float32(255))).astype(np.float32)
    fr = (np.float32(0.1) + np.float32(0.8) * (right / np.float32(255))).astype(np.float32)
    assert 0.1 <= fl.min() and fl.max() <= 0.9001
    cl = image.percentile_scale_convert(dev(fl), dtype=np.float32, ctx=ctx)
    cr = image.percentile_scale_convert(dev(fr), dtype=np.float32, ctx=ctx)
    wl = ref.percentile_scale_convert(fl, out_type=2)[0]
    wr = ref.percentile_scale_convert(fr, out_type=2)[0]
    ref.same_bits(arr(cl), wl, "left")
    ref.same_bits(arr(cr), wr, "right")
    assert len(np.unique(wl)) > 200 and np.all(wl == np.round(wl))
    got = stereo.calc_disparity(0, cl, cr, vwa.bounding_box(fl), (33, 1), (7, 7), ctx=ctx)
    torch.cuda.synchronize()
    assert ctx.last_path() == core.PATH_SAD_U8
    assert np.array_equal(got.cpu().numpy(), oracle.calc_disparity(0, wl, wr, (7, 7), (33, 1)))


def test_ipfind_normalizes_on_the_device(ctx):
    """ipfind(normalize=True, nodata=) detects on apply_mask(normalize(create_mask(raw, nodata))) as tools/ipfind.cc does: the
    same points as on that image prepared by the restatement; the defaults leave the call as it was."""
    from visionworkbench_amd import interest_point as ipm
    raw = np.zeros((96, 128), np.float32) + 200.0
    for x, y in ((28, 30), (90, 50)):
        raw[y:y + 5, x:x + 5] = 1400.0
    raw[:8, :8] = -9999.0
    valid = raw != -9999.0
    want_img = ref.auto_normalize(np.where(valid, raw, 0).astype(np.float32), 0.0, 1.0, valid)[0]
    want_img[~valid] = 0
    ref.same_bits(arr(ipm.normalized_input(dev(raw), -9999.0, ctx=ctx)), want_img, "normalized input")
    ref.same_bits(ipm.normalized_input(raw, -9999.0, ctx=ctx), want_img, "normalized input, host")
    ref.same_bits(arr(ipm.normalized_input(dev(raw), ctx=ctx)), ref.auto_normalize(raw)[0], "normalized input without nodata")
    got = ipm.ipfind(dev(raw), ip_per_tile=1000, normalize=True, nodata=-9999.0, ctx=ctx)
    want = ipm.ipfind(dev(want_img), ip_per_tile=1000, ctx=ctx)
    assert len(want.x) > 0 and {(30, 32), (92, 52)} <= set(zip(want.ix.tolist(), want.iy.tolist()))
    for name in ("x", "y", "ix", "iy", "scale", "interest", "descriptor"):
        assert np.array_equal(arr(getattr(got, name)), arr(getattr(want, name))), name


# ---- the C++ surface -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nodata", [None, 0.5])
def test_cpp_surface(tmp_path, nodata):
    """image_stats_view.cc (vwlite vw/Image.h, vw/Math.h over libvwgpu.so), once, as a fresh child process: its printed numbers
    and written images equal the restatement's."""
    exe = ref.build_view_program()
    rows, cols = 90, 150
    img = ref.natural(rows, cols, 13, 0.0, 1.0)
    mask = None
    if nodata is not None:
        img[ref.random_mask(rows, cols, 13, 0.1) != 0] = nodata
        mask = (img != np.float32(nodata)).astype(np.uint8)
    img.tofile(str(tmp_path / "image.bin"))
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, str(tmp_path / "image.bin"), str(cols), str(rows), "none" if nodata is None else repr(nodata), prefix],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0 and "image_stats_view ok" in run.stdout, run.stdout
    said = dict(line.split() for line in run.stdout.splitlines() if len(line.split()) == 2)
    stored = img if mask is None else np.where(mask != 0, img, 0).astype(np.float32)      # create_mask: an invalid pixel holds the default value
    mn, mx, _, _ = ref.find_min_max(stored, mask)
    counts, width = ref.histogram(stored, 256, mn, mx, mask)
    mom = ref.moments(stored, mask)
    want = {"min": mn, "max": mx, "accumulator_min": ref.min_max_channel_values(stored, mask)[0],
            "accumulator_max": ref.min_max_channel_values(stored, mask)[1], "mean": ref.mean(stored, mask), "median": ref.median(stored, mask),
            "bin_width": width, "bin_17": float(counts[17]), "otsu": ref.otsu_threshold(stored, mask=mask),
            "otsu_sampled": ref.otsu_threshold(stored, 23, 17, 64, mask=mask)}
    for name, value in want.items():
        assert float.fromhex(said[name]) == value, "%s: %s, want %r" % (name, said[name], value)
    n = max(mom[0] - 1, 0)
    assert abs(float.fromhex(said["sum"]) - mom[1]) <= 2 * n * U / (1 - n * U) * mom[0]       # |x| <= 1: the bound of the module's docstring
    assert int(said["total"]) == counts[256]
    assert int(said["low_bin"]) == ref.get_percentile(counts, 256, 0.02) and int(said["high_bin"]) == ref.get_percentile(counts, 256, 0.98)
    ref.same_bits(np.fromfile(prefix + ".psc", np.uint8).reshape(rows, cols), ref.percentile_scale_convert(stored, mask=mask)[0], "percentile_scale_convert")
    ref.same_bits(np.fromfile(prefix + ".u8", np.uint8).reshape(rows, cols), ref.u8_convert(stored, mask)[0], "u8_convert")
    ref.same_bits(np.fromfile(prefix + ".norm", np.float32).reshape(rows, cols), ref.auto_normalize(stored, 0.0, 1.0, mask)[0], "normalize")
    ref.same_bits(np.fromfile(prefix + ".clamp", np.float32).reshape(rows, cols), ref.rescale(stored, 0, [0.25, 0.75]), "clamp")
    ref.same_bits(np.fromfile(prefix + ".thresh", np.float32).reshape(rows, cols), ref.rescale(stored, 3, [0.5, -1.0, 2.0]), "threshold")
