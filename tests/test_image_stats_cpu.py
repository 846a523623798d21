"""CPU-only: pins the restatement of the reference's image statistics and intensity scaling (tests/refimpl/image_stats_ref.cc)
with the known answers of the reference's unit tests (tests/golden/image_stats_known.json), with an independent numpy
statement of what each operation means (tests/refimpl/image_stats_direct.py) on seeded random images, and with Otsu
thresholds that follow by hand; the library's host functions on counts equal the restatement; header, binding, Python
wrappers and vwlite names agree on the new entries."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import image_stats_direct as direct  # noqa: E402
import image_stats_ref as ref  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "image_stats_known.json")) as _f:
    KNOWN = json.load(_f)

NEW_ENTRIES = ["image_min_max", "image_moments", "image_histogram", "otsu_threshold", "image_order_statistic", "image_rescale",
               "percentile_scale_convert", "u8_convert", "auto_normalize"]
HOST_ENTRIES = ["vwgpu_moments_mean", "vwgpu_moments_stddev", "vwgpu_histogram_percentile", "vwgpu_otsu_from_histogram"]
WRAPPERS = ["min_max", "moments", "mean", "stddev", "median", "percentile", "histogram", "Histogram", "otsu_threshold", "clamp",
            "normalize", "threshold", "percentile_scale_convert", "u8_convert"]
VWLITE_NAMES = ["find_image_min_max", "min_max_channel_values", "mean_channel_value", "stddev_channel_value", "median_channel_value",
                "histogram", "otsu_threshold", "percentile_scale_convert", "u8_convert", "clamp", "normalize", "threshold"]


def _f32(rows):
    return np.asarray(rows, np.float32)


# ---- known answers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", KNOWN["statistics"], ids=lambda c: c["name"])
def test_statistics_known_answers(case):
    img, mask = _f32(case["image"]), case["mask"]
    if case.get("no_valid_samples"):
        with pytest.raises(ref.NoValidSamples):
            ref.min_max_channel_values(img, mask)
        with pytest.raises(ref.NoValidSamples):
            ref.mean(img, mask)
        with pytest.raises(ref.NoValidSamples):
            ref.stddev(img, mask)
        assert ref.moments(img, mask)[1] == case["sum"]
        assert ref.find_min_max(img, mask)[:2] == (ref.DBL_MAX, -ref.DBL_MAX)
        return
    assert ref.min_max_channel_values(img, mask) == (case["min"], case["max"])
    assert ref.find_min_max(img, mask)[:2] == (case["min"], case["max"])
    assert ref.moments(img, mask)[1] == case["sum"]
    assert abs(ref.mean(img, mask) - case["mean"]) <= 1e-6       # EXPECT_NEAR(.., 1e-6) of MeanChannel
    assert ref.stddev(img, mask) == case["stddev"]               # EXPECT_EQ of StdDevChannel


def test_median_known_answer():
    for case in KNOWN["median"]:
        assert ref.median(_f32(case["image"]), case["mask"]) == case["median"]
        assert direct.median(_f32(case["image"]), case["mask"]) == case["median"]


def test_histogram_known_answers():
    case = KNOWN["image_histogram"]
    counts, _ = ref.histogram(_f32(case["image"]), case["num_bins"], case["min"], case["max"])
    for b, n in case["bins"].items():
        assert counts[int(b)] == n
    assert counts[case["num_bins"]] == sum(case["bins"].values())
    case = KNOWN["math_histogram"]
    counts, width = ref.histogram(_f32([case["values"]]), case["num_bins"], case["min"], case["max"])
    assert counts[case["num_bins"]] == case["total"]
    for b, n in case["bins"].items():
        assert counts[int(b)] == n
    assert case["min"] + 4 * width + width / 2.0 == case["bin_center_4"]       # get_bin_center(4), Statistics.cc:52


def test_rescale_known_answers():
    k = KNOWN["clamp"]
    for case in k["cases"]:
        ref.same_bits(ref.rescale(_f32(k["image"]), 0, [case["low"], case["high"]]), _f32([case["expect"]]), "clamp")
    k = KNOWN["threshold"]
    for case in k["cases"]:
        ref.same_bits(ref.rescale(_f32(k["image"]), 3, [case["thresh"], case["low"], case["high"]]), _f32([case["expect"]]), "threshold")
    k = KNOWN["normalize"]
    for case in k["cases"]:
        b = case["bounds"]
        if len(b) == 4:
            got = ref.rescale(_f32(k["image"]), 1, b)
        else:
            got, _ = ref.auto_normalize(_f32(k["image"]), *(b if b else (0.0, 1.0)))
        assert np.abs(got.astype(np.float64) - np.asarray([case["expect"]])).max() <= k["tolerance"]      # EXPECT_PIXEL_NEAR(.., 1e-7)


# ---- the restatement against the direct statement ----------------------------------------------------------------------

def _scene(seed):
    rng = np.random.RandomState(seed)
    rows, cols = int(rng.randint(1, 90)), int(rng.randint(1, 90))
    lo = float(rng.uniform(-50, 50))
    img = ref.natural(rows, cols, seed, lo, lo + float(rng.choice([1e-3, 1.0, 255.0, 4000.0])))
    mask = None if seed % 3 == 0 else ref.random_mask(rows, cols, seed, float(rng.uniform(0.2, 0.95)))
    if mask is not None and not mask.any():
        mask[0, 0] = 1
    return img, mask, rng


@pytest.mark.parametrize("seed", range(12))
def test_restatement_equals_direct(seed):
    img, mask, rng = _scene(seed)
    mn, mx, count, nan = ref.find_min_max(img, mask)
    assert (mn, mx) == direct.find_min_max(img, mask) and nan == 0 and count == direct.valid_values(img, mask).size
    assert ref.min_max_channel_values(img, mask) == direct.min_max_accumulator(img, mask)
    for nb in (1, 2, 256, 1000):
        counts, width = ref.histogram(img, nb, mn, mx, mask)
        bins, nans = direct.histogram_bins(direct.valid_values(img, mask), nb, mn, mx)
        assert np.array_equal(counts[:nb], bins) and counts[nb] == bins.sum() and counts[nb + 1] == nans == 0
        for p in (0.0, 0.02, float(rng.uniform(0, 1)), 0.98, 1.0):
            want = direct.percentile_bin(bins, p)
            if want is None:       # the running sum ended below 1.0: the reference throws
                with pytest.raises(ref.NoValidSamples):
                    ref.get_percentile(counts, nb, p)
            else:
                assert ref.get_percentile(counts, nb, p) == want
    # a narrower range than the data: both ends saturate
    counts, _ = ref.histogram(img, 64, mn + 0.25 * (mx - mn), mx - 0.25 * (mx - mn), mask)
    bins, _ = direct.histogram_bins(direct.valid_values(img, mask), 64, mn + 0.25 * (mx - mn), mx - 0.25 * (mx - mn))
    assert np.array_equal(counts[:64], bins)
    assert ref.median(img, mask) == direct.median(img, mask)
    for p in (0.0, 1.0, 50.0, float(rng.uniform(0, 100)), 100.0):
        assert ref.percentile(img, p, mask) == direct.percentile(img, p, mask)
    lo, hi = mn + 0.2 * (mx - mn), mn + 0.7 * (mx - mn)
    ref.same_bits(ref.rescale(img, 0, [lo, hi]), direct.clamp(img, lo, hi), "clamp")
    ref.same_bits(ref.rescale(img, 1, [lo, hi, -3.0, 7.5]), direct.normalize(img, lo, hi, -3.0, 7.5), "normalize")
    ref.same_bits(ref.rescale(img, 1, [lo, lo, -3.0, 7.5]), direct.normalize(img, lo, lo, -3.0, 7.5), "normalize, empty range")
    ref.same_bits(ref.rescale(img, 2, [lo, hi, lo, hi, 0.0, 255.0], 1), direct.to_u8(direct.normalize(direct.clamp(img, lo, hi), lo, hi, 0.0, 255.0)),
                  "clamp + normalize to uint8")
    ref.same_bits(ref.rescale(img, 3, [lo, -1.0, 2.0]), direct.threshold(img, lo, -1.0, 2.0), "threshold")
    got, params, bins = ref.percentile_scale_convert(img, 0.02, 0.98, 256, mask)
    want, wparams, wbins = direct.percentile_scale_convert(img, 0.02, 0.98, 256, mask)
    assert params == wparams and bins == wbins
    ref.same_bits(got, want, "percentile_scale_convert")
    as_float, _, _ = ref.percentile_scale_convert(img, 0.02, 0.98, 256, mask, out_type=2)
    ref.same_bits(as_float, want.astype(np.float32), "percentile_scale_convert as float")
    got, params = ref.u8_convert(img, mask)
    want, wparams = direct.u8_convert(img, mask)
    assert params == wparams
    ref.same_bits(got, want, "u8_convert")


def test_nan_and_sampling():
    img = ref.natural(40, 60, 5, -1.0, 1.0)
    img[0, 0] = np.nan
    img[7, 9] = np.nan
    mn, mx, count, nan = ref.find_min_max(img)
    assert (mn, mx) == direct.find_min_max(img) and nan == 2 and count == img.size
    assert all(np.isnan(x) for x in ref.min_max_channel_values(img))                      # the first sample is a NaN: it stays
    mask = np.ones(img.shape, np.uint8)
    mask[0, 0] = 0
    assert ref.min_max_channel_values(img, mask) == direct.min_max_accumulator(img, mask)    # a later NaN never enters
    counts, _ = ref.histogram(img, 32, mn, mx)
    assert counts[33] == 2 and counts[32] == img.size - 2
    assert ref.rescale(img, 1, [mn, mx, 0, 255], 1)[0, 0] == 0                            # a NaN becomes 0 in uint8
    for sample in ((2, 2), (17, 23), (40, 60)):
        v = direct.valid_values(img, None, sample)
        assert ref.find_min_max(img, None, sample)[:2] == direct.find_min_max(img, None, sample)
        counts, _ = ref.histogram(img, 50, mn, mx, None, sample)
        bins, nans = direct.histogram_bins(v, 50, mn, mx)
        assert np.array_equal(counts[:50], bins) and counts[51] == nans
    assert np.array_equal(ref.histogram(img, 50, mn, mx, None, (40, 60))[0], ref.histogram(img, 50, mn, mx)[0])


# ---- Otsu thresholds that follow by hand -------------------------------------------------------------------------------

def test_otsu_two_values_is_a_tie_plateau():
    """Half the pixels 0, half 1: min 0, max 1, 256 bins with N/2 in bin 0, N/2 in bin 255 and nothing between.
    Overload 1: for every i in 0..254 the left class is bin 0 alone: leftProb = 0.5 and leftAccum = 0 (adding 0/sum and i * 0
    changes neither), so V[i] is one and the same double for i = 0..254; at i = 255 leftProb = 0.5 + 0.5 = 1, rightProb = 0,
    V stays 0.  The maximum is reached at 255 indices, their mean is (0 + 254) / 2 = 127, threshold = 0 + 127 / 255 * (1 - 0).
    Overload 2: at i = 0, q1 = q2 = 0.5, mu1 = 0, mu2 = 127.5 / 0.5 = 255, sigma = 0.25 * 255^2 > 0: max_pos = 0.  For
    i = 1..254 p_i = 0, mu1 = 0 * 0.5 / 0.5 = 0 and sigma is that same number: not greater.  At i = 255 q2 = 0 < FLT_EPSILON:
    skipped.  threshold = (1 - 0) * (0 / 255) + 0 = 0, the first maximum."""
    img = np.zeros((6, 10), np.float32)
    img[:, 5:] = 1.0
    assert ref.otsu_threshold(img) == 0.0 + (127.0 / 255.0) * (1.0 - 0.0)
    assert ref.otsu_threshold(img, 6, 10, 256) == 0.0


def test_otsu_constant_image():
    """Every pixel 3: max == min, so max becomes 4 and every pixel lies in bin 0.  Overload 1: leftProb = 1 from i = 0 on,
    rightProb = 0, every V[i] stays 0; the maximum 0 is reached at all 256 indices, mean 127.5, threshold = 3 + 127.5 / 255 *
    (4 - 3) = 3.5.  Overload 2: q2 = 0 at every i, all skipped, max_pos = 0, threshold = (4 - 3) * 0 + 3 = 3."""
    img = np.full((5, 7), 3.0, np.float32)
    assert ref.otsu_threshold(img) == 3.5
    assert ref.otsu_threshold(img, 5, 7, 256) == 3.0


def test_otsu_all_invalid_is_zero():
    """No valid pixel: min = DBL_MAX, max = -DBL_MAX, the histogram stays empty; both overloads return 0.0 for a total of 0."""
    img, mask = np.ones((4, 4), np.float32), np.zeros((4, 4), np.uint8)
    assert ref.otsu_threshold(img, mask=mask) == 0.0
    assert ref.otsu_threshold(img, 4, 4, 256, mask=mask) == 0.0


def test_otsu_overloads_agree_on_a_clear_split():
    """"Gives the same result as the one above if num_bins=256" and every pixel is sampled (ImageThresh.h:149-150): true where
    the maximum is unique, which two overlapping classes with no empty bin between them give.  Both then scale the same bin
    index, by formulas that differ in a few roundings."""
    rng = np.random.RandomState(3)
    img = np.concatenate([rng.normal(10, 3, 30000), rng.normal(22, 3, 20000)]).astype(np.float32).reshape(200, 250)
    a, b = ref.otsu_threshold(img), ref.otsu_threshold(img, 200, 250, 256)
    assert 13 < a < 19 and abs(a - b) <= 1e-12 * abs(a)


# ---- the library's host functions, header, binding, wrappers -----------------------------------------------------------

def _lib():
    from visionworkbench_amd import _lib
    return _lib.load()


def test_abi_version_stays_3():
    assert _lib().vwgpu_abi_version() == 3
    assert "#define VWGPU_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "vwgpu.h")).read()


@pytest.mark.parametrize("seed", range(6))
def test_host_functions_equal_the_restatement(seed):
    lib = _lib()
    img, mask, rng = _scene(100 + seed)
    mn, mx, _, _ = ref.find_min_max(img, mask)
    if mx == mn:
        mx += 1
    for nb, overloads in ((256, (1, 2)), (64, (2,)), (1000, (2,))):
        counts, _ = ref.histogram(img, nb, mn, mx, mask)
        for p in (0.0, 0.02, float(rng.uniform(0, 1)), 0.98):
            b = ctypes.c_int(-1)
            assert lib.vwgpu_histogram_percentile(counts.ctypes.data, nb, int(counts[nb]), p, ctypes.byref(b)) == 0
            assert b.value == ref.get_percentile(counts, nb, p)
        for overload in overloads:
            t = ctypes.c_double(-1)
            assert lib.vwgpu_otsu_from_histogram(counts.ctypes.data, nb, int(counts[nb]), mn, mx, overload, ctypes.byref(t)) == 0
            assert t.value == ref.otsu_counts(counts, nb, mn, mx, overload)
    mom = np.asarray(ref.moments(img, mask))
    r = ctypes.c_double(0)
    assert lib.vwgpu_moments_mean(mom.ctypes.data, ctypes.byref(r)) == 0 and r.value == ref.mean(img, mask)
    assert lib.vwgpu_moments_stddev(mom.ctypes.data, ctypes.byref(r)) == 0 and r.value == ref.stddev(img, mask)


def test_host_functions_refuse_bad_arguments():
    lib = _lib()
    counts = np.array([3, 0, 5, 8, 0], np.uint64)
    b, t, zero = ctypes.c_int(0), ctypes.c_double(0), np.zeros(3)
    for p in (-0.1, 1.5, float("nan")):
        assert lib.vwgpu_histogram_percentile(counts.ctypes.data, 3, 8, p, ctypes.byref(b)) == -1
    assert lib.vwgpu_histogram_percentile(None, 3, 8, 0.5, ctypes.byref(b)) == -1
    assert lib.vwgpu_histogram_percentile(np.zeros(5, np.uint64).ctypes.data, 3, 0, 0.5, ctypes.byref(b)) == -5      # VWGPU_ERR_LOGIC: Illegal histogram
    assert lib.vwgpu_otsu_from_histogram(counts.ctypes.data, 3, 8, 0.0, 1.0, 3, ctypes.byref(t)) == -1
    assert lib.vwgpu_otsu_from_histogram(np.zeros(5, np.uint64).ctypes.data, 3, 0, 0.0, 1.0, 1, ctypes.byref(t)) == 0 and t.value == 0.0
    assert lib.vwgpu_moments_mean(zero.ctypes.data, ctypes.byref(t)) == -1
    assert lib.vwgpu_moments_stddev(zero.ctypes.data, ctypes.byref(t)) == -1


def test_surfaces_agree_on_the_new_entries():
    from visionworkbench_amd import _lib, image, interest_point
    header = open(os.path.join(ROOT, "include", "vwgpu.h")).read()
    for name in NEW_ENTRIES:
        for symbol in ("vwgpu_" + name, "vwgpu_%s_dev" % name):
            assert symbol in _lib.SYMBOLS and ("int %s(" % symbol) in header, symbol
    for symbol in HOST_ENTRIES:
        assert symbol in _lib.SYMBOLS and ("int %s(" % symbol) in header, symbol
    assert "#define VWGPU_HISTOGRAM_MAX_BINS 4096" in header and image.HISTOGRAM_MAX_BINS == 4096
    for name in WRAPPERS:
        assert callable(getattr(image, name)), name
    vwlite = os.path.join(ROOT, "visionworkbench_amd", "vwlite", "vw")
    text = open(os.path.join(vwlite, "Image.h")).read()
    for name in VWLITE_NAMES:
        assert (" %s(ImageViewBase<ViewT> const&" % name) in text, name
    assert "class Histogram" in open(os.path.join(vwlite, "Math.h")).read()
    assert "image_stats.hip" in open(os.path.join(ROOT, "visionworkbench_amd", "csrc", "Makefile")).read()
    import inspect
    sig = inspect.signature(interest_point.ipfind)
    assert sig.parameters["normalize"].default is False and sig.parameters["nodata"].default is None


def test_wrappers_refuse_bad_arguments():
    from visionworkbench_amd import image
    from visionworkbench_amd.core import ArgumentErr
    img = np.zeros((5, 7), np.float32)
    with pytest.raises(ArgumentErr):
        image.histogram(img, image.HISTOGRAM_MAX_BINS + 1, 0.0, 1.0)
    with pytest.raises(ArgumentErr):
        image.histogram(img, 0, 0.0, 1.0)
    with pytest.raises(ArgumentErr):
        image.min_max(img, mode="both")
    with pytest.raises(ArgumentErr):
        image.min_max(np.zeros((5, 7, 2), np.float32))
    with pytest.raises(ArgumentErr):
        image.min_max(img, mask=np.ones((5, 6), np.uint8))
    with pytest.raises(ArgumentErr):
        image.otsu_threshold(img, 4, 4)
    with pytest.raises(ArgumentErr):
        image.normalize(img, 1.0)
    with pytest.raises(ArgumentErr):
        image.clamp(img, 0.0, 1.0, dtype=np.int16)
