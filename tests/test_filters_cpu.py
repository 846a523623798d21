"""CPU-only: the oracle's pyramid / prefilter family against tests/refimpl/filters_direct.py, an independent numpy formulation from the
reference's definitions, on every case of tests/filter_cases.py; and that formulation against float64 under a derived bound.

Comparison rule (filters_direct.same_bits): NaN where NaN is expected, the same bit pattern everywhere else, so the sign of a zero and a
subnormal count."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "refimpl"))
import filter_cases as fc  # noqa: E402
import filters_direct as fd  # noqa: E402


def _bad(cases, got_want):
    bad = []
    for c in cases:
        got, want = got_want(c)
        n = fd.same_bits(got, want)
        if n:
            bad.append("%s: %d" % (c["id"], n))
    return bad


def test_comparison_rule_itself():
    a = np.array([0.0, -0.0, np.nan, 1e-40, 1.0, np.inf], np.float32)
    assert fd.same_bits(a, a.copy()) == 0
    assert fd.same_bits(-a, a) == 5                                   # every sign but the NaN's
    assert fd.same_bits(np.array([0.0], np.float32), np.array([1e-45], np.float32)) == 1
    assert fd.same_bits(np.array([1.0], np.float32), np.array([np.nan], np.float32)) == 1
    assert fd.same_bits(np.array([np.nan], np.float32), np.array([1.0], np.float32)) == 1
    assert fd.same_bits(a[:3], a) == -1


def test_case_table_holds_what_it_promises():
    """The properties the table is there for, so that a later edit cannot quietly lose them."""
    cases = list(fc.sepconv_cases())
    assert len({c["id"] for c in cases}) == len(cases)
    step2 = {(c["img"].shape[1], c["img"].shape[0]) for c in cases if c["id"].startswith("seam-s2-k5x5")}
    assert {(1 + (w - 1) // 2, 1 + (h - 1) // 2) for w, h in step2} == {(a, b) for a in fc.OW for b in fc.OH}
    for step, nx, ny in fc.FLOOR:                                      # the floor fits the documented budget, the next odd size does not
        lds = lambda ax, ay: ((15 * step + 1 + max(ay - 1, 0)) * ((63 * step + 1 + max(ax - 1, 0)) + 64)) * 4
        assert lds(nx, ny) <= 65536 and nx <= 160 and ny <= 160
    sp = fc.special_image()
    for v in fc.SPECIALS:
        same = np.isnan(sp) if np.isnan(v) else (sp.view(np.uint32) == np.array(v).view(np.uint32))
        assert same.sum() >= 4
    assert fd.gaussian_kernel(0.3).size == 3 and fd.gaussian_kernel(9.6).size == 67 and fd.gaussian_kernel(9.9).size == 69
    assert fd.gaussian_kernel(4.0).size == 27 and fd.gaussian_kernel(0.0).size == 0


def test_subnormal_image_gives_subnormal_outputs(oracle):
    """The 5-tap level of the rand * 1e-38 image: every output is a non-zero subnormal (a flush to zero anywhere would show)."""
    img = dict(fc.special_images())["subnormal"]
    out = oracle.separable_convolution(img, fc.K5, fc.K5)
    assert out.shape == (30, 20) and int(((out != 0) & (np.abs(out) < np.finfo(np.float32).tiny)).sum()) == 600


def test_gaussian_kernel(oracle):
    for sigma, size in [(1.0, 5), (1.0, 4), (1.5, 0), (float(np.float32(1.4)), 0), (5.0, 0), (0.3, 0), (0.0, 0), (9.6, 0), (25.0, 0), (2.0, 12)]:
        assert fd.same_bits(oracle.generate_gaussian_kernel(sigma, size), fd.gaussian_kernel(sigma, size)) == 0, (sigma, size)


def test_separable_convolution(oracle):
    bad = _bad(fc.sepconv_cases(), lambda c: (oracle.separable_convolution(c["img"], c["xk"], c["yk"], c["cx"], c["cy"], c["edge"], c["step"]),
                                              fd.separable_convolution(c["img"], c["xk"], c["yk"], c["cx"], c["cy"], c["edge"], c["step"])))
    assert not bad, bad


def test_convolution_2d(oracle):
    bad = _bad(fc.conv2d_cases(), lambda c: (oracle.convolution_2d(c["img"], c["k"], c["ci"], c["cj"], c["edge"]),
                                             fd.convolution_2d(c["img"], c["k"], c["ci"], c["cj"], c["edge"])))
    assert not bad, bad
    img, k = fc.conv2d_too_large()                                     # the oracle has no tap limit: the case the kernels refuse is still defined
    assert fd.same_bits(oracle.convolution_2d(img, k, 0, 4, 1), fd.convolution_2d(img, k, 0, 4, 1)) == 0


def test_mask_decimation(oracle):
    bad = _bad(fc.mask_cases(), lambda c: (oracle.subsample_mask_by_two(c["mask"]), fd.subsample_mask_by_two(c["mask"])))
    assert not bad, bad


def test_prefilters(oracle):
    bad = _bad(fc.prefilter_cases(), lambda c: (oracle.prefilter_image(c["img"], c["mode"], c["width"]),
                                                fd.prefilter_image(c["img"], c["mode"], c["width"])))
    assert not bad, bad


def test_prefilter_regions(oracle):
    """oracle.prefilter_region over the regions parabola_subpixel asks for, which leave the image by 20 pixels on one side, and the NONE
    form once per scene."""
    bad, seen = [], 0
    for c in fc.region_cases():
        for img, box in fc.region_boxes(c):
            for mode in (c["mode"], 0):
                n = fd.same_bits(oracle.prefilter_region(img, mode, c["width"], *box), fd.prefilter_region(img, mode, c["width"], box))
                seen += 1
                if n:
                    bad.append("%s %s mode %d: %d" % (c["id"], box, mode, n))
        h, w = c["right"].shape                                        # (box: the right region)
        assert max(-box[0], -box[1], box[0] + box[2] - w, box[1] + box[3] - h) >= 20, c["id"]
    assert seen == 2 * 2 * 96 and not bad, bad


def _bound_violations(out, ref64, mag, nx, ny):
    """|out - ref64| <= (nx + ny + 2) 2^-24 (|xk| * |yk| * |img|) + (nx + ny) 2^-149, both sides in float64: the first-order bound of a
    recursive sum (n products, n additions: at most n + 1 roundings touch a term, on each axis) plus one underflow per product."""
    lim = (nx + ny + 2) * 2.0 ** -24 * mag + (nx + ny) * 2.0 ** -149
    return int((np.abs(out.astype(np.float64) - ref64) > lim).sum())


def test_float32_result_within_the_bound_of_float64():
    """Second opinion on the formulation itself: derived, not measured.  Finite cases only (finite image, finite float32 result)."""
    bad, seen = [], 0
    for c in fc.sepconv_cases():
        out = fd.separable_convolution(c["img"], c["xk"], c["yk"], c["cx"], c["cy"], c["edge"], c["step"])
        if not (fc.is_finite_case(c) and np.isfinite(out).all()):
            continue
        i64, x64, y64 = c["img"].astype(np.float64), c["xk"].astype(np.float64), c["yk"].astype(np.float64)
        ref = fd.separable_convolution(i64, x64, y64, c["cx"], c["cy"], c["edge"], c["step"])
        mag = fd.separable_convolution(np.abs(i64), np.abs(x64), np.abs(y64), c["cx"], c["cy"], c["edge"], c["step"])
        seen += 1
        n = _bound_violations(out, ref, mag, len(x64), len(y64))
        if n:
            bad.append("%s: %d" % (c["id"], n))
    for c in fc.conv2d_cases():
        out = fd.convolution_2d(c["img"], c["k"], c["ci"], c["cj"], c["edge"])
        if not (fc.is_finite_case(c) and np.isfinite(out).all()):
            continue
        i64, k64 = c["img"].astype(np.float64), c["k"].astype(np.float64)
        ref = fd.convolution_2d(i64, k64, c["ci"], c["cj"], c["edge"])
        mag = fd.convolution_2d(np.abs(i64), np.abs(k64), c["ci"], c["cj"], c["edge"])
        seen += 1
        n = _bound_violations(out, ref, mag, k64.size, 0)              # one recursive sum of kw * kh terms
        if n:
            bad.append("%s: %d" % (c["id"], n))
    assert seen > 300 and not bad, bad
