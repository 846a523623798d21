"""CPU: the restatement tests/refimpl/outlier_filters_ref.cc of the local outlier filters of Stereo/DisparityMap.h
(rm_outliers_using_mean / _stddev / _plane, their clean-up compositions) and std_dev_image against hand-derived answers
and an independent numpy formulation; the binding's symbols.  The reference itself cannot be built here, so these tests
pin what the GPU tests compare against."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import outlier_filters_ref as ofr  # noqa: E402

from visionworkbench_amd import _lib, stereo  # noqa: E402

TYPES = [np.int32, np.float32]


def _window3(values, dtype=np.float32, dy=0):
    """a 3 x 3 image whose centre pixel's window is the image: dx = values in window order, all valid"""
    d = np.zeros((3, 3, 3), dtype)
    d[..., 0] = np.asarray(values).reshape(3, 3)
    d[..., 1] = dy
    d[..., 2] = 1
    return d


def _kept(out):
    return out[1, 1, 2] != 0


# ---- hand-derived answers ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", ["reference", "skip"])
def test_mean_cutoff_of_the_comments_example(sem):
    """Magnitudes 1 .. 8 and 1e10 (DisparityMap.h:495-496): sorted[(int)(0.75 * 9)] = sorted[6] = 7, cutoff 14, so 1e10 is
    left out and the mean is 36 / 8 = 4.5; the centre, 5, is 0.5 away.  The large value is the window's last pixel, so
    both semantics read the same pixels."""
    d = _window3([1, 2, 3, 4, 5, 6, 7, 8, 1e10])
    assert _kept(ofr.rm_outliers("mean", d, 1, 1, 0.6, semantics=sem))
    assert not _kept(ofr.rm_outliers("mean", d, 1, 1, 0.4, semantics=sem))
    # the cutoff is exactly 14: a ninth magnitude of 14 is inside (mean 50 / 9, 0.5556 away), 15 is outside (mean 4.5)
    for dtype in TYPES:
        assert not _kept(ofr.rm_outliers("mean", _window3([1, 2, 3, 4, 5, 6, 7, 8, 14], dtype), 1, 1, 0.52, semantics=sem))
        assert _kept(ofr.rm_outliers("mean", _window3([1, 2, 3, 4, 5, 6, 7, 8, 15], dtype), 1, 1, 0.52, semantics=sem))
    # |dx| + |dy|: dy = -1 lifts the ninth magnitude from 14 to 15, outside again
    e = _window3([1, 2, 3, 4, 5, 6, 7, 8, 14])
    e[2, 2, 1] = -1
    assert _kept(ofr.rm_outliers("mean", e, 1, 1, 0.52, semantics=sem))


@pytest.mark.parametrize("dtype", TYPES)
def test_mean_reference_loop_ends_a_row_at_its_first_gross_outlier(dtype):
    """Window rows [1 1 1] [1 100 2] [1 1 1]: sorted[6] = 1, cutoff 2.  `reference`: the middle row stops at 100, the 2
    behind it is never read: mean 7 / 7 = 1, the centre is 99 away.  `skip`: mean 9 / 8 = 1.125, 98.875 away.
    max_mean_diff = 98.9 separates them."""
    d = _window3([1, 1, 1, 1, 100, 2, 1, 1, 1], dtype)
    sr, ss = [], []
    assert not _kept(ofr.rm_outliers("mean", d, 1, 1, 98.9, semantics="reference", stats=sr))
    assert _kept(ofr.rm_outliers("mean", d, 1, 1, 98.9, semantics="skip", stats=ss))
    assert sr[1] == 0 and ss[1] == 0 and sr[0] == ss[0] + 1
    # no pixel matched: a 5 x 3 window whose rows all begin with a gross outlier (magnitudes 1 x 12 and 9 x 3: sorted[11] = 1,
    # cutoff 2).  `reference` reads nothing else and rejects whatever max_mean_diff is (:536); `skip` finds mean 1, error 0
    g = np.zeros((3, 5, 3), dtype)
    g[..., 0] = 1
    g[:, 0, 0] = 9
    g[..., 2] = 1
    assert ofr.rm_outliers("mean", g, 2, 1, 1e6, semantics="reference")[1, 2, 2] == 0
    assert ofr.rm_outliers("mean", g, 2, 1, 1e-3, semantics="skip")[1, 2, 2] != 0


@pytest.mark.parametrize("dtype", TYPES)
def test_invalid_centres_are_copies_and_rejected_pixels_are_zero(dtype):
    d = _window3([1, 1, 1, 1, 100, 1, 1, 1, 1], dtype, dy=7)
    for method, args in (("mean", (1.0,)), ("stddev", (1.0, 0.1)), ("plane", (1.0, 0.1))):
        out = ofr.rm_outliers(method, d, 1, 1, *args)
        assert tuple(out[1, 1]) == (0, 0, 0), method
        e = d.copy()
        e[1, 1] = (-77, 33, 0)
        out = ofr.rm_outliers(method, e, 1, 1, *args)
        assert tuple(out[1, 1]) == (-77, 33, 0), method


@pytest.mark.parametrize("method", ["stddev", "plane"])
@pytest.mark.parametrize("dtype", TYPES)
def test_flat_region_clamps_sigma_to_the_rejection_threshold(method, dtype):
    """All 50 but the centre, 53: mean 50 + 1/3 (the fitted plane is z = 50 + 1/3 by symmetry), sigma =
    sqrt((8 / 9 + 64 / 9) / 9) = 0.9428, the centre is 2.6667 away.  pixel_threshold 2: 1.8856 < 2.6667 rejects; with
    rejection_threshold 2 sigma is raised to 2 and 4 > 2.6667 keeps.  A perfectly flat window has sigma 0, error 0."""
    d = _window3([50, 50, 50, 50, 53, 50, 50, 50, 50], dtype)
    assert not _kept(ofr.rm_outliers(method, d, 1, 1, 2.0, 0.01))
    assert _kept(ofr.rm_outliers(method, d, 1, 1, 2.0, 2.0))
    flat = _window3([50] * 9, dtype, dy=-3)
    out = ofr.rm_outliers(method, flat, 1, 1, 2.0, 0.0)
    assert np.array_equal(out, flat)


@pytest.mark.parametrize("dtype", TYPES)
def test_plane_keeps_the_pixel_when_the_fit_has_a_zero_pivot(dtype):
    """Valid points that are a single pixel, one row, one column or the main diagonal make the normal matrix singular
    with an exactly zero pivot in any elimination order: the reference's `catch` keeps the pixel.  With both thresholds
    0 any solved fit with a residual rejects, as the fifth case shows."""
    vals = [0, 40, 0, 10, 90, -20, 0, 7, 0]
    masks = {
        "single": [0, 0, 0, 0, 1, 0, 0, 0, 0],
        "row": [0, 0, 0, 1, 1, 1, 0, 0, 0],
        "column": [0, 1, 0, 0, 1, 0, 0, 1, 0],
        "diagonal": [1, 0, 0, 0, 1, 0, 0, 0, 1],
    }
    for name, m in masks.items():
        d = _window3(vals, dtype)
        d[..., 2] = np.asarray(m).reshape(3, 3)
        assert _kept(ofr.rm_outliers("plane", d, 1, 1, 0.0, 0.0)), name
    d = _window3(vals, dtype)
    d[..., 2] = np.asarray([1, 1, 0, 1, 1, 0, 0, 0, 1]).reshape(3, 3)
    assert not _kept(ofr.rm_outliers("plane", d, 1, 1, 0.0, 0.0))
    # four points that lie on a plane exactly: z = 2 xk - 3 yk + 5 at (-1,-1), (1,-1), (0,0), (-1,1)
    p = _window3([6, 0, 10, 0, 5, 0, 0, 0, 0], dtype)
    p[..., 2] = np.asarray([1, 0, 1, 0, 1, 0, 1, 0, 0]).reshape(3, 3)
    assert _kept(ofr.rm_outliers("plane", p, 1, 1, 1.0, 1e-9))


def test_std_dev_image_hand_values():
    """1 x 1: 0.0f / 0 is NaN.  Size 2 reads offsets -1 .. 1, nine samples of an all-ones image: sum 9, mean 9 / 4, nine
    differences of -1.25: 14.0625 / 3 = 4.6875; at a corner with zero extension four ones and five zeros: mean 1, five
    differences of -1: 5 / 3."""
    ones = np.ones((5, 6), np.float32)
    assert np.isnan(ofr.std_dev_image(ones, 1, 1)).all()
    assert np.isnan(ofr.std_dev_image(ofr.image_scene(7, 5), 1, 1, "constant")).all()
    z = ofr.std_dev_image(ones, 2, 2, "zero")
    c = ofr.std_dev_image(ones, 2, 2, "constant")
    assert (c == np.float32(4.6875)).all() and (z[1:-1, 1:-1] == np.float32(4.6875)).all()
    assert z[0, 0] == np.float32(5.0) / np.float32(3.0)
    assert np.array_equal(ofr.std_dev_image(ones, 3, 3, "constant"), np.zeros_like(ones))     # 9 samples, mean 1
    # an even size and the next odd one read the same samples but divide differently
    img = ofr.image_scene(9, 8)
    assert not np.array_equal(ofr.std_dev_image(img, 2, 2), ofr.std_dev_image(img, 3, 3))
    # mixed sizes: kw = 1 reads one column, kh = 3 three rows: mean = sum / 3, result = sum of squares / 2
    col = np.zeros((5, 3), np.float32)
    col[:, 1] = [1, 2, 4, 8, 16]
    got = ofr.std_dev_image(col, 1, 3, "constant")
    m = np.float32(1 + 2 + 4) / np.float32(3)
    want = (((np.float32(1) - m) ** 2 + (np.float32(2) - m) ** 2) + (np.float32(4) - m) ** 2) / np.float32(2)
    assert got[1, 1] == want and got[1, 0] == 0


# ---- an independent numpy formulation ---------------------------------------------------------------------------

def _windows(d, hh, hv):
    """(y, x, window) for every pixel: the window's pixels as a (kh, kw, 3) array, coordinates clamped"""
    h, w = d.shape[:2]
    for y in range(h):
        ys = np.clip(np.arange(y - hv, y + hv + 1), 0, h - 1)
        for x in range(w):
            xs = np.clip(np.arange(x - hh, x + hh + 1), 0, w - 1)
            yield y, x, d[np.ix_(ys, xs)]


def _magnitudes(win):
    if win.dtype == np.float32:
        return (np.abs(win[..., 0]) + np.abs(win[..., 1])).astype(np.float64)       # a float32 add
    return (np.abs(win[..., 0].astype(np.int64)) + np.abs(win[..., 1].astype(np.int64))).astype(np.float64)


def np_mean(d, hh, hv, max_mean_diff, skip):
    out = d.copy()
    for y, x, win in _windows(d, hh, hv):
        if d[y, x, 2] == 0:
            continue
        valid = win[..., 2] != 0
        mag = _magnitudes(win)
        ordered = np.sort(mag[valid])
        cutoff = 2.0 * ordered[int(0.75 * ordered.size)]
        sx = sy = 0.0
        n = 0
        for r in range(win.shape[0]):
            for c in range(win.shape[1]):
                if not valid[r, c]:
                    continue
                if mag[r, c] > cutoff:
                    if skip:
                        continue
                    break
                sx += float(win[r, c, 0])
                sy += float(win[r, c, 1])
                n += 1
        limit = max_mean_diff * max_mean_diff
        err = limit + 1.0
        if n:
            mx, my = sx / n, sy / n
            tx, ty = float(d[y, x, 0]), float(d[y, x, 1])
            err = (tx - mx) * (tx - mx) + (ty - my) * (ty - my)
        if err > limit:
            out[y, x] = 0
    return out


def np_stddev(d, hh, hv, pixel_threshold, rejection_threshold):
    out = d.copy()
    for y, x, win in _windows(d, hh, hv):
        if d[y, x, 2] == 0:
            continue
        pts = [(float(p[0]), float(p[1])) for p in win.reshape(-1, 3) if p[2] != 0]
        n = len(pts)
        sx = sy = 0.0
        for a, b in pts:
            sx += a
            sy += b
        mx, my = sx / n, sy / n
        qx = qy = 0.0
        for a, b in pts:
            qx += (a - mx) * (a - mx)
            qy += (b - my) * (b - my)
        sdx = max(math.sqrt(qx / n), rejection_threshold)
        sdy = max(math.sqrt(qy / n), rejection_threshold)
        if abs(float(d[y, x, 0]) - mx) > pixel_threshold * sdx or abs(float(d[y, x, 1]) - my) > pixel_threshold * sdy:
            out[y, x] = 0
    return out


def np_plane(d, hh, hv, pixel_threshold, rejection_threshold):
    """returns (out, near): near marks pixels whose decision is a near tie in either channel"""
    out = d.copy()
    near = np.zeros(d.shape[:2], bool)
    offs = [(xk, yk) for yk in range(-hv, hv + 1) for xk in range(-hh, hh + 1)]
    for y, x, win in _windows(d, hh, hv):
        if d[y, x, 2] == 0:
            continue
        flat = win.reshape(-1, 3)
        pts = [(float(xk), float(yk), float(p[0]), float(p[1])) for (xk, yk), p in zip(offs, flat) if p[2] != 0]
        A = np.zeros((3, 3))
        B = np.zeros((3, 2))
        for xk, yk, zx, zy in pts:
            A += [[xk * xk, xk * yk, xk], [xk * yk, yk * yk, yk], [xk, yk, 0.0]]
            B += [[xk * zx, xk * zy], [yk * zx, yk * zy], [zx, zy]]
        A[2, 2] = len(pts)
        try:
            sol = np.linalg.solve(A, B)
        except np.linalg.LinAlgError:
            continue
        reject = False
        for ch in (0, 1):
            a, b, c = sol[:, ch]
            den = math.sqrt(a * a + b * b + 1.0)
            ss = 0.0
            for p in pts:
                dist = abs(a * p[0] + b * p[1] - p[2 + ch] + c) / den
                ss += dist * dist
            sigma = max(math.sqrt(ss / len(pts)), rejection_threshold)
            err = abs(-float(d[y, x, ch]) + c) / den
            bound = pixel_threshold * sigma
            if abs(err - bound) <= 1e-9 * max(1.0, bound):
                near[y, x] = True
            reject = reject or err > bound
        if reject:
            out[y, x] = 0
    return out, near


def np_thresh3(inner):
    """RmOutliersUsingThreshFunc(1, 1, 3.0, 0.2) on the interior of a padded inner view"""
    h, w = inner.shape[0] - 2, inner.shape[1] - 2
    out = inner[1:-1, 1:-1].copy()
    for y in range(h):
        for x in range(w):
            c = inner[y + 1, x + 1]
            if c[2] == 0:
                continue
            win = inner[y:y + 3, x:x + 3].reshape(-1, 3)
            if inner.dtype == np.float32:
                close = (np.abs(c[0] - win[:, 0]) <= 3.0) & (np.abs(c[1] - win[:, 1]) <= 3.0)
            else:
                close = (np.abs(int(c[0]) - win[:, 0].astype(np.int64)) <= 3) & (np.abs(int(c[1]) - win[:, 1].astype(np.int64)) <= 3)
            if float(np.count_nonzero(close & (win[:, 2] != 0))) / 9.0 < 0.2:
                out[y, x] = 0
    return out


def _same(got, want, what):
    assert got.dtype == want.dtype
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: %d pixels differ, first at %s" % (
        what, len(np.argwhere((got != want).any(axis=2))), np.argwhere((got.view(np.uint32) != want.view(np.uint32)).any(axis=2))[:1])


def _scene(dtype, w, h, seed):
    return ofr.float_scene(w, h, seed) if dtype == np.float32 else ofr.int_scene(w, h, seed)


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("half", [(1, 1), (2, 1), (1, 3), (4, 4)])
def test_mean_equals_the_numpy_formulation(dtype, half):
    d = _scene(dtype, 40, 30, 11 + half[0])
    diff = 1.0
    outs = []
    for sem in ("reference", "skip"):
        st = []
        got = ofr.rm_outliers("mean", d, half[0], half[1], diff, semantics=sem, stats=st)
        want = np_mean(d, half[0], half[1], diff, sem == "skip")
        _same(got, want, "mean %s %s" % (half, sem))
        assert st == [int(((d[..., 2] != 0) & (got[..., 2] == 0)).sum()), 0] and st[0] > 0
        outs.append(got)
    if dtype == np.int32:
        assert not np.array_equal(outs[0], outs[1])     # the planted outliers make the two semantics differ


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("half", [(1, 1), (2, 1), (1, 3), (4, 4)])
def test_stddev_equals_the_numpy_formulation(dtype, half):
    d = _scene(dtype, 40, 30, 21 + half[1])
    for thr in ((1.5, 0.3), (2.0, 1.0)):
        st = []
        got = ofr.rm_outliers("stddev", d, half[0], half[1], *thr, stats=st)
        _same(got, np_stddev(d, half[0], half[1], *thr), "stddev %s %s" % (half, thr))
        assert st == [int(((d[..., 2] != 0) & (got[..., 2] == 0)).sum()), 0] and st[0] > 0


PLANE_SCENES = [(np.float32, 31, (1, 1)), (np.float32, 32, (2, 1)), (np.float32, 33, (1, 3)), (np.float32, 34, (4, 4)),
                (np.int32, 35, (2, 2))]


@pytest.mark.parametrize("dtype,seed,half", PLANE_SCENES)
def test_plane_agrees_with_gesv_outside_near_ties(dtype, seed, half):
    """np.linalg.solve is LAPACK gesv, the reference's solver, whose bits differ from the restatement's elimination by
    rounding: decisions must agree wherever the numpy formulation's own margin |error - t sigma| exceeds
    1e-9 max(1, t sigma), and such near ties are at most 0.5 % of the scene's valid pixels."""
    d = ofr.float_scene(40, 30, seed, hole=False) if dtype == np.float32 else ofr.int_scene(40, 30, seed)
    for thr in ((1.5, 0.2), (2.0, 0.5)):
        got = ofr.rm_outliers("plane", d, half[0], half[1], *thr)
        want, near = np_plane(d, half[0], half[1], *thr)
        valid = d[..., 2] != 0
        assert near.sum() <= 0.005 * valid.sum(), "%d near ties among %d valid pixels" % (near.sum(), valid.sum())
        differ = (got.view(np.uint32) != want.view(np.uint32)).any(axis=2) & ~near
        assert not differ.any(), "plane %s %s: %d decisions differ, first at %s" % (half, thr, differ.sum(), np.argwhere(differ)[:1])
        rejected = valid & (got[..., 2] == 0)
        assert 0 < rejected.sum() < valid.sum()


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("method,args", [("mean", (2.5,)), ("stddev", (1.5, 0.3)), ("plane", (1.5, 0.2))])
def test_cleanup_is_the_filter_on_a_padded_image_then_thresh(dtype, method, args):
    """The outer functor reads the inner view one pixel outside the image, where the inner functor runs on clamped
    reads: the same as filtering the image padded by edge replication and reading that result at the padded positions."""
    d = ofr.sparse_scene(37, 29, dtype, seed=41)
    for half in ((1, 1), (3, 2)):
        st, s1 = [], []
        got = ofr.rm_outliers(method, d, half[0], half[1], *args, cleanup=True, stats=st)
        padded = np.ascontiguousarray(np.pad(d, ((1, 1), (1, 1), (0, 0)), mode="edge"))
        inner = ofr.rm_outliers(method, padded, half[0], half[1], *args)
        want = np_thresh3(inner)
        _same(got, want, "%s clean-up %s" % (method, half))
        first = ofr.rm_outliers(method, d, half[0], half[1], *args, stats=s1)
        _same(first, np.ascontiguousarray(inner[1:-1, 1:-1]), "%s inner view inside the image" % method)
        assert st[0] == s1[0] and st[1] == int(((first[..., 2] != 0) & (got[..., 2] == 0)).sum())
    # a lone valid pixel survives every filter (its window is itself) and falls to the second pass: 1 / 9 < 0.2
    lone = np.zeros((9, 9, 3), dtype)
    lone[4, 4] = (3, -2, 1)
    st = []
    out = ofr.rm_outliers(method, lone, 1, 1, *args, cleanup=True, stats=st)
    assert not out.any() and st == [0, 1]
    # ... but at a corner the padded inner view repeats it four times: 4 / 9 >= 0.2 keeps it
    lone[4, 4] = 0
    lone[0, 0] = (3, -2, 1)
    out = ofr.rm_outliers(method, lone, 1, 1, *args, cleanup=True, stats=st)
    assert tuple(out[0, 0]) == (3, -2, 1) and st == [0, 0]


@pytest.mark.parametrize("edge", ["zero", "constant"])
def test_std_dev_image_equals_the_numpy_formulation(edge):
    img = ofr.image_scene(23, 17, seed=51)
    h, w = img.shape
    for kw, kh in ((1, 1), (2, 2), (3, 3), (4, 2), (7, 3), (5, 31), (31, 31)):
        hx, hy = kw // 2, kh // 2
        pad = np.pad(img, ((hy, hy), (hx, hx)), mode="edge" if edge == "constant" else "constant")
        sum_ = np.zeros((h, w), np.float32)
        for yk in range(2 * hy + 1):
            for xk in range(2 * hx + 1):
                sum_ = sum_ + pad[yk:yk + h, xk:xk + w]
        mean = sum_ / np.float32(kw * kh)
        sq = np.zeros((h, w), np.float32)
        for yk in range(2 * hy + 1):
            for xk in range(2 * hx + 1):
                diff = pad[yk:yk + h, xk:xk + w] - mean
                sq = sq + diff * diff
        with np.errstate(invalid="ignore", divide="ignore"):
            want = sq / np.float32(kw * kh - 1)
        got = ofr.std_dev_image(img, kw, kh, edge)
        assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want)), (kw, kh)
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), (kw, kh)


# ---- arguments and the binding ------------------------------------------------------------------------------------

def test_restatement_refuses_what_the_constructors_refuse():
    d = ofr.float_scene(8, 6, 1)
    for hh, hv in ((0, 1), (1, 0), (-2, 3)):
        with pytest.raises(ValueError):
            ofr.rm_outliers("mean", d, hh, hv, 1.0)
    for kw, kh in ((0, 3), (3, 0), (-1, -1)):
        with pytest.raises(ValueError):
            ofr.std_dev_image(d[..., 0], kw, kh)


def test_binding_lists_the_new_entries_and_python_names():
    for name in ("rm_outliers", "std_dev_image"):
        assert "vwgpu_%s" % name in _lib.SYMBOLS and "vwgpu_%s_dev" % name in _lib.SYMBOLS
    for name in ("rm_outliers_using_mean", "rm_outliers_using_stddev", "rm_outliers_using_plane", "disparity_cleanup_using_mean",
                 "disparity_cleanup_using_stddev", "disparity_clean_using_plane", "std_dev_image"):
        assert callable(getattr(stereo, name)) and name in stereo.__all__
    header = open(os.path.join(ROOT, "include", "vwgpu.h")).read()
    for word in ("VWGPU_OUTLIER_MEAN", "VWGPU_OUTLIER_STDDEV", "VWGPU_OUTLIER_PLANE", "VWGPU_OUTLIER_REFERENCE", "VWGPU_OUTLIER_SKIP",
                 "VWGPU_DISPARITY_I32", "VWGPU_DISPARITY_F32"):
        assert word in header
    assert "#define VWGPU_ABI_VERSION 3" in header
