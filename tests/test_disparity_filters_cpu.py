"""CPU: the restatement tests/refimpl/disparity_filters_ref.cc of the disparity post-filters of Stereo/Algorithms.h
(median, neighbour, texture measure, texture-preserving smoothing) against hand-derived answers and an independent
plain-Python formulation, in both semantics; the aliasing of the reference's in-place form; the binding's symbols.
The reference itself cannot be built here, so these tests pin what the GPU tests compare against."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import disparity_filters_ref as dfr  # noqa: E402

from visionworkbench_amd import _lib  # noqa: E402

SEM = ["reference", "snapshot"]


def _ramp(w, h, dtype=np.float32):
    d = np.zeros((h, w, 3), dtype)
    d[..., 0] = np.arange(w)[None, :]
    d[..., 1] = np.arange(h)[:, None] * 10
    d[..., 2] = 1
    return d


# ---- hand-derived answers ----------------------------------------------------------------------------------------

def test_median_3x3_of_a_ramp_with_one_invalid_neighbour():
    """dx = column: the window of (2, 2) holds {1, 2, 3} three times; without (1, 1) eight values remain,
    1 1 2 2 2 3 3 3, whose two middle ones are 2 and 2; dy = 10 row: 10 20 20 20 | 30 30 30 without one 10 ->
    0 0 10 10 | 10 20 20 20 shifted: rows 1, 2, 3 give 10 10 20 20 20 30 30 30 -> (20 + 20) / 2."""
    d = _ramp(5, 5)
    d[1, 1] = (77, -77, 0)
    out = dfr.disparity_median_filter(d.copy(), 3, "snapshot")
    assert tuple(out[2, 2]) == (2.0, 20.0, 1.0)
    # a window whose two middle values differ: drop (3, 1) instead -> dx 1 1 1 2 | 2 2 3 3 -> 2; make it 1 1 1 2 | 3 ...
    d = _ramp(5, 5)
    d[2, 2, 0] = 9                     # window of (2, 2): 1 1 1 2 2 3 3 3 9 minus invalid (3, 3) -> 1 1 1 2 | 2 3 3 9
    d[3, 3, 2] = 0
    d[1, 2, 0] = 2.5                   # now 1 1 1 2 2.5 3 3 9 (8 values): middle 2 and 2.5 -> 2.25
    out = dfr.disparity_median_filter(d.copy(), 3, "snapshot")
    assert out[2, 2, 0] == np.float32(2.25)
    # border, invalid centres and sizes below 3 are untouched; an even size uses half = (k - 1) / 2
    assert np.array_equal(out[0], d[0]) and np.array_equal(out[:, 0], d[:, 0]) and np.array_equal(out[3, 3], d[3, 3])
    for k in (0, 1, 2):
        assert np.array_equal(dfr.disparity_median_filter(d.copy(), k, "snapshot"), d)
    assert np.array_equal(dfr.disparity_median_filter(d.copy(), 4, "snapshot"), dfr.disparity_median_filter(d.copy(), 3, "snapshot"))


def _neighbour_case():
    d = np.zeros((3, 5, 3), np.int32)
    d[..., 2] = 1
    d[..., 0] = [[7, 7, 7, 1, 2], [7, 0, 3, 4, 7], [7, 5, 7, 7, 7]]
    d[1, 1] = (99, 99, 0)              # invalid centre with five equal valid neighbours (7): filled
    return d


def test_neighbour_fill_tips_the_next_pixel_only_in_reference_semantics():
    """(1, 1) is invalid and six of its neighbours are 7: it becomes 7.  (2, 1) has the neighbours 7 7 1 | (1, 1) 4 |
    5 7 7: four 7s, five once (1, 1) holds 7 — which only the in-place recursion sees.  (3, 1) has 7 1 2 | (2, 1) 7 |
    7 7 7: five 7s already, replaced in both."""
    d = _neighbour_case()
    st = []
    snap = dfr.disparity_neighbor_filter(d.copy(), "snapshot", stats=st)
    assert [tuple(snap[1, c]) for c in (1, 2, 3)] == [(7, 0, 1), (3, 0, 1), (7, 0, 1)] and st == [2]
    ref = dfr.disparity_neighbor_filter(d.copy(), "reference", stats=st)
    assert [tuple(ref[1, c]) for c in (1, 2, 3)] == [(7, 0, 1), (7, 0, 1), (7, 0, 1)] and st == [3]
    assert np.array_equal(ref[0], d[0]) and np.array_equal(ref[2], d[2]) and np.array_equal(ref[:, ::4], d[:, ::4])


def test_texture_measure_constant_and_ramp():
    assert np.array_equal(dfr.texture_measure(np.full((20, 24), 37.5, np.float32), 9), np.zeros((20, 24), np.float32))
    k = 9
    img = np.tile(np.arange(40, dtype=np.float32), (30, 1))
    st = []
    out = dfr.texture_measure(img, k, stats=st)
    want = 0.5 * 0.5 + 0.5 * math.sqrt((k * k - 1) / 12.0)      # |dx| = 1, |dy| = 0 -> 1 / 2; stddev of 9 integers
    assert abs(want - 1.540994) < 1e-6
    inner = out[6:-6, 6:-6]
    assert np.all(np.abs(inner - np.float32(want)) <= np.spacing(np.float32(want)))
    assert st[0] == out.max()
    # non-default weights
    out2 = dfr.texture_measure(img, k, 1.0, 0.0)
    assert np.all(out2[6:-6, 6:-6] == np.float32(0.5))


def test_texture_filter_limits():
    d = dfr.float_scene(24, 20, seed=2, hole=False)
    d[np.isnan(d)] = 0
    tex = np.full((20, 24), 0.15, np.float32)
    for sem in SEM:
        assert np.array_equal(dfr.texture_preserving_disparity_filter(d.copy(), tex, 0.15, 11, sem), d)
        assert np.array_equal(dfr.texture_preserving_disparity_filter(d.copy(), tex * 3, 0.15, 11, sem), d)
        assert np.array_equal(dfr.texture_preserving_disparity_filter(d.copy(), tex * 0, 0.0, 11, sem), d)
        assert np.array_equal(dfr.texture_preserving_disparity_filter(d.copy(), tex * 0, 0.15, 2, sem), d)
        assert np.array_equal(dfr.texture_preserving_disparity_filter(d.copy(), -tex, 0.15, 11, sem), d)
    # texture 0: the mean over the valid pixels of the clamped max_kernel_size window (0.15 * (11 / 0.15) floors to 11)
    out = dfr.texture_preserving_disparity_filter(d.copy(), tex * 0, 0.15, 11, "snapshot")
    for (c, r) in [(0, 0), (12, 10), (23, 19), (3, 17)]:
        if d[r, c, 2] == 0:
            assert np.array_equal(out[r, c], d[r, c])
            continue
        sx = sy = n = 0.0
        for rr in range(r - 5, r + 6):
            for cc in range(c - 5, c + 6):
                p = d[min(max(rr, 0), 19), min(max(cc, 0), 23)]
                if p[2] != 0:
                    sx += float(p[0]); sy += float(p[1]); n += 1.0
        assert tuple(out[r, c]) == (np.float32(sx / n), np.float32(sy / n), 1.0)


# ---- an independent formulation ----------------------------------------------------------------------------------

def _py_filter(d, boxes, semantics, make):
    """make(box) -> pixel(view, c, r) -> None or (dx, dy): `view` is the box of the image being read (the output itself
    in reference semantics)."""
    src = d.copy()
    out = d.copy()
    for (x, y, w, h) in boxes:
        pixel = make((x, y, w, h))
        rd = out[y:y + h, x:x + w] if semantics == "reference" else src[y:y + h, x:x + w]
        wr = out[y:y + h, x:x + w]
        for r in range(h):
            for c in range(w):
                v = pixel(rd, c, r)
                if v is not None:
                    wr[r, c] = (v[0], v[1], 1)
    return out


def _py_median(k):
    half = (k - 1) // 2

    def pixel(v, c, r):
        h, w = v.shape[:2]
        if k < 3 or c < half or r < half or c >= w - half or r >= h - half or v[r, c, 2] == 0:
            return None
        win = v[r - half:r + half + 1, c - half:c + half + 1].reshape(-1, 3)
        win = win[win[:, 2] != 0]
        if np.isnan(win[:, :2]).any():
            return None
        return [np.float32(np.median(win[:, i].astype(np.float64))) for i in (0, 1)]
    return pixel


def _py_neighbour(v, c, r):
    h, w = v.shape[:2]
    if c < 1 or r < 1 or c >= w - 1 or r >= h - 1:
        return None
    nb = [v[r + dr, c + dc] for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr, dc) != (0, 0)]
    keys = [(int(p[0]), int(p[1])) if p[2] != 0 else None for p in nb]
    best, arg = 0, None
    for key in keys:
        if key is not None and keys.count(key) > best:
            best, arg = keys.count(key), key
    return arg if best >= 5 else None


def _py_smooth(tex, tmax, maxk, x0, y0):
    def pixel(v, c, r):
        h, w = v.shape[:2]
        t = np.float32(tex[y0 + r, x0 + c])
        if maxk < 3 or tmax <= 0 or v[r, c, 2] == 0 or t < 0 or not np.isfinite(t):
            return None
        scale = np.float32(maxk) / np.float32(tmax)
        adj = max(np.float32(tmax) - t, np.float32(0))
        prod = np.float32(adj * scale)
        if not np.isfinite(prod):
            return None
        ks = int(math.floor(prod))
        ks += 1 - ks % 2
        if ks < 3 or ks > maxk:
            return None
        half = (ks - 1) // 2
        rows = np.clip(np.arange(r - half, r + half + 1), 0, h - 1)
        cols = np.clip(np.arange(c - half, c + half + 1), 0, w - 1)
        sx = sy = n = 0.0
        for rr in rows:
            for cc in cols:
                if v[rr, cc, 2] != 0:
                    sx += float(v[rr, cc, 0]); sy += float(v[rr, cc, 1]); n += 1.0
        return None if n < 1 else (np.float32(sx / n), np.float32(sy / n))
    return pixel


def _same(a, b):
    va, vb = a[..., 2] != 0, b[..., 2] != 0
    return np.array_equal(va, vb) and np.array_equal(a[va][:, :2], b[vb][:, :2]) and \
        np.array_equal(a[~va].view(np.uint32), b[~vb].view(np.uint32))


BOXES = [None, [(0, 0, 20, 9), (20, 0, 11, 9), (0, 9, 31, 1), (0, 10, 31, 12)]]


@pytest.mark.parametrize("sem", SEM)
@pytest.mark.parametrize("k", [3, 4, 5, 7])
def test_median_equals_the_python_formulation(sem, k):
    d = dfr.float_scene(31, 22, seed=k)
    for boxes in BOXES:
        bx = boxes or [(0, 0, 31, 22)]
        want = _py_filter(d, bx, sem, lambda b: _py_median(k))
        st = []
        got = dfr.disparity_median_filter(d.copy(), k, sem, tiles=boxes, stats=st)
        assert _same(got, want)
        changed = (got[..., 2] != d[..., 2]) | ((got[..., 2] != 0) & ((got[..., 0] != d[..., 0]) | (got[..., 1] != d[..., 1])))
        if sem == "snapshot":
            assert st[0] == changed.sum()


@pytest.mark.parametrize("sem", SEM)
def test_neighbour_equals_the_python_formulation(sem):
    d = dfr.int_scene(31, 22)
    for boxes in BOXES:
        want = _py_filter(d, boxes or [(0, 0, 31, 22)], sem, lambda b: _py_neighbour)
        got = dfr.disparity_neighbor_filter(d.copy(), sem, tiles=boxes)
        assert np.array_equal(got, want)
    assert not np.array_equal(dfr.disparity_neighbor_filter(d.copy(), "reference"), dfr.disparity_neighbor_filter(d.copy(), "snapshot"))


@pytest.mark.parametrize("sem", SEM)
@pytest.mark.parametrize("maxk", [3, 6, 11])
def test_smoothing_equals_the_python_formulation(sem, maxk):
    d = dfr.float_scene(31, 22, seed=9)
    rng = np.random.RandomState(1)
    tex = rng.uniform(-0.02, 0.2, (22, 31)).astype(np.float32)
    tex[5, 5] = np.nan
    tex[6, 6] = np.inf
    for boxes in BOXES:
        want = _py_filter(d, boxes or [(0, 0, 31, 22)], sem, lambda b: _py_smooth(tex, 0.15, maxk, b[0], b[1]))
        got = dfr.texture_preserving_disparity_filter(d.copy(), tex, 0.15, maxk, sem, tiles=boxes)
        assert _same(got, want)


@pytest.mark.parametrize("k", [1, 3, 6, 9])
def test_texture_measure_equals_the_python_formulation(k):
    img = dfr.image_scene(23, 17)
    half = (k - 1) // 2
    for boxes in (None, [(0, 0, 10, 17), (10, 0, 13, 8), (10, 8, 13, 9)]):
        want = np.zeros_like(img)
        for (x, y, w, h) in (boxes or [(0, 0, 23, 17)]):
            b = img[y:y + h, x:x + w]
            pad = np.pad(b, 1, mode="edge")
            f = np.float32
            dx = (f(0) + f(-0.5) * pad[1:-1, :-2]) + f(0) * b
            dx = dx + f(0.5) * pad[1:-1, 2:]
            dy = (f(0) + f(-0.5) * pad[:-2, 1:-1]) + f(0) * b
            dy = dy + f(0.5) * pad[2:, 1:-1]
            g = (np.abs(dx) + np.abs(dy)).astype(np.float32)
            be, ge = np.pad(b, half, mode="edge"), np.pad(g, half, mode="edge")
            for r in range(h):
                for c in range(w):
                    wv = be[r:r + 2 * half + 1, c:c + 2 * half + 1].astype(np.float64).ravel()
                    wg = ge[r:r + 2 * half + 1, c:c + 2 * half + 1].astype(np.float64).ravel()
                    n = float(len(wv))
                    mean = sd = grad = 0.0
                    for v in wv.tolist():          # plain loops: the built-in sum() may compensate
                        mean += v
                    mean /= n
                    for v in wv.tolist():
                        sd += (v - mean) * (v - mean)
                    for v in wg.tolist():
                        grad += v
                    grad /= 2.0 * n
                    want[y + r, x + c] = np.float32(grad * 0.3 + math.sqrt(sd / n) * 0.7)
        got = dfr.texture_measure(img, k, 0.3, 0.7, tiles=boxes)
        assert np.array_equal(got, want)


# ---- the aliasing, the errors and the binding -------------------------------------------------------------------

def test_reference_semantics_modify_the_input_buffer():
    d = dfr.float_scene(40, 30, seed=5)
    keep = d.copy()
    out = dfr.disparity_median_filter(d, 5, "reference")
    assert out is not d and _same(out, d) and not _same(d, keep)
    d2 = keep.copy()
    out2 = dfr.disparity_median_filter(d2, 5, "snapshot")
    assert _same(d2, keep) and not _same(out2, out)
    di = dfr.int_scene(40, 30)
    ki = di.copy()
    oi = dfr.disparity_neighbor_filter(di, "reference")
    assert np.array_equal(oi, di) and not np.array_equal(di, ki)
    tex = np.zeros((30, 40), np.float32)
    d3 = keep.copy()
    o3 = dfr.texture_preserving_disparity_filter(d3, tex, 0.15, 5, "reference")
    assert _same(o3, d3) and not _same(d3, keep)


def test_restatement_rejects_bad_boxes():
    d = dfr.int_scene(16, 12)
    for boxes in ([(0, 0, 17, 12)], [(-1, 0, 4, 4)], [(0, 0, 8, 8), (7, 7, 4, 4)], [(0, 0, 0, 4)]):
        with pytest.raises(ValueError):
            dfr.disparity_neighbor_filter(d.copy(), "snapshot", tiles=boxes)


def test_binding_lists_the_new_entry_points():
    for name in ("disparity_median_filter", "disparity_neighbor_filter", "texture_measure",
                 "texture_preserving_disparity_filter"):
        assert "vwgpu_%s" % name in _lib.SYMBOLS and "vwgpu_%s_dev" % name in _lib.SYMBOLS
