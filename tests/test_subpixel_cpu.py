"""CPU: the direct-sum restatement of parabola_subpixel (tests/refimpl/parabola_direct.py: per-window float64 sums in the
kernel's specified order) against the oracle (the reference's zones and running box sums) — no GPU.

  * ORDER-FREE scenes (every scene on which tests/test_subpixel_gpu.py and the fuzz leg demand bit-equality with the oracle, from
    the same generators): the two formulations are IDENTICAL.  This is what entitles the GPU tests to np.array_equal against the
    oracle: it is established on the reference side alone.
  * ROUNDING scenes (one huge or non-finite pixel): the two formulations DIFFER — the running sums keep the rounding residue of
    the large value for the rest of a zone — while validity and invalid pixels stay identical.  The GPU tests compare the kernel
    with the restatement there.  Measured counts: profiles/parabola_parity.md.
  * hand cases of the solve that need neither formulation's sums."""
import os
import sys

import numpy as np
import pytest

import fuzz_cases
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import parabola_direct  # noqa: E402


def _both(oracle, c):
    want = oracle.parabola_subpixel(c["disp"], c["left"], c["right"], c["mode"], c["width"], c["kernel"])
    got = parabola_direct.parabola_subpixel(oracle, c["disp"], c["left"], c["right"], c["mode"], c["width"], c["kernel"])
    return got, want


@pytest.mark.parametrize("sid", scenes.parabola_order_free_ids())
def test_restatement_equals_oracle_on_order_free_scenes(oracle, sid):
    got, want = _both(oracle, scenes.parabola_scene(sid, oracle))
    assert not np.isnan(want).any()
    assert np.array_equal(got, want), "%d pixels differ, largest by %g" % ((got != want).any(-1).sum(), np.abs(got - want).max())


def test_restatement_equals_oracle_on_fuzz_sample(oracle):
    """The generator of the gpu-marked fuzz leg emits order-free scenes only."""
    bad = []
    for c in fuzz_cases.parabola_cases(40, 701):
        got, want = _both(oracle, c)
        if not np.array_equal(got, want):
            bad.append((c["it"], c["kind"], c["mode"], c["kernel"], c["left"].shape, int((got != want).any(-1).sum())))
    assert not bad, "parabola_cases(seed=701): %s" % bad


def _rounding_scene(oracle, sid):
    c = scenes.parabola_scene(sid)
    got, want = _both(oracle, c)
    assert not np.isnan(got).any() and not np.isnan(want).any()           # a NaN offset fails the `< 5` test on both sides
    assert np.array_equal(got[..., 2], want[..., 2])
    invalid = c["disp"][..., 2] == 0
    assert invalid.any() and (got[invalid] == 0).all() and (want[invalid] == 0).all()
    differing = int((got != want).any(-1).sum())
    print("%s: %d of %d pixels differ, %d by more than 1e-5, largest %g px"
          % (sid, differing, invalid.size, int((np.abs(got - want).max(-1) > 1e-5).sum()), np.abs(got - want).max()))
    return differing


@pytest.mark.parametrize("sid", ["rounding:" + s for s in scenes.parabola_rounding_ids()])
def test_restatement_differs_from_oracle_on_rounding_scenes(oracle, sid):
    """Largest differences measured: profiles/parabola_parity.md (hundreds to thousands of the 3 840 pixels, up to several pixels)."""
    assert _rounding_scene(oracle, sid) >= 1


@pytest.mark.parametrize("sid", ["edge:" + s for s in scenes.parabola_edge_ids(True)])
def test_non_finite_class_edge_scenes_keep_validity(oracle, sid):
    """The NaN / Inf pixel of the class-edge scenes: treated by the rounding scenes' rule on the GPU (kernel == restatement).  Whether the two
    formulations differ depends on where the pixel is — in the last row and column of the left image every zone meets it last and they
    agree — so no difference is demanded here, only that validity and invalid pixels are the same."""
    _rounding_scene(oracle, sid)


def test_invalid_pixels_widen_the_rasters_and_change_no_valid_pixel(oracle):
    """Invalid pixels that store values far outside the valid range: get_disparity_range takes valid pixels only
    (Image/Statistics.h:283-290), so neither the rasters nor a single pixel change.  (The name dates from a range over all pixels.)"""
    for variant in ("u8", "f01", "log"):
        c = scenes.parabola_scene("disparity:invalid_extreme-" + variant)
        tame = c["disp"].copy()
        tame[tame[..., 2] == 0] = 0
        a = parabola_direct.parabola_subpixel(oracle, c["disp"], c["left"], c["right"], c["mode"], c["width"], c["kernel"])
        b = parabola_direct.parabola_subpixel(oracle, tame, c["left"], c["right"], c["mode"], c["width"], c["kernel"])
        assert parabola_direct.disparity_range(c["disp"])[0] == parabola_direct.disparity_range(tame)[0]
        assert np.array_equal(a, b)


# ---- hand cases: 1 x 1 windows on a zero left image make the nine costs the right image's own pixels -----------------------------------

def _costs_as_image(cost):
    """A 5 x 5 pair whose centre pixel, at disparity (1, 0), sees cost(ddx, ddy) = |0 - right(3 + ddx, 2 + ddy)|."""
    left = np.zeros((5, 5), np.float32)
    right = np.full((5, 6), 1000.0, np.float32)
    for ddy in (-1, 0, 1):
        for ddx in (-1, 0, 1):
            right[2 + ddy, 3 + ddx] = cost(ddx, ddy)
    d = np.zeros((5, 5, 3), np.float32)
    d[..., 0] = 1.9                                                    # truncates to 1
    d[2, 2, 2] = 1
    return d, left, right


def test_quadric_costs_give_the_dyadic_offset(oracle):
    """cost = 5 x^2 + y^2 + 2 x y - x + y + 20: nine integers; the fitted quadric is the cost itself, its minimum at
    ((c e - 2 b d), (c d - 2 a e)) / (4 a b - c^2) = (4, -12) / 16 = (0.25, -0.75).  The float32 solve carries the rounding of 1/6, 1/3 and of
    ~40 operations of relative error 2^-24 on well-conditioned values (no cancellation beyond a factor ~10): below 1e-5."""
    d, left, right = _costs_as_image(lambda x, y: 5 * x * x + y * y + 2 * x * y - x + y + 20)
    L, R, rminx, rminy = parabola_direct.rasters(oracle, d, left, right, 0, 0.0, (1, 1))
    _, idx, idy = parabola_direct.disparity_range(d)
    patch = parabola_direct.costs(L, R, idx, idy, rminx, rminy, (1, 1))
    assert np.array_equal(patch[2, 2], np.array([5 + 1 + 2 + 1 - 1 + 20, 1 - 1 + 20, 5 + 1 - 2 - 1 - 1 + 20, 5 + 1 + 20, 20, 5 - 1 + 20,
                                                 5 + 1 - 2 + 1 + 1 + 20, 1 + 1 + 20, 5 + 1 + 2 - 1 + 1 + 20], np.float32))
    out = parabola_direct.parabola_subpixel(oracle, d, left, right, 0, 0.0, (1, 1))
    assert out[2, 2, 2] == 1 and abs(out[2, 2, 0] - 1.25) < 1e-5 and abs(out[2, 2, 1] + 0.75) < 1e-5
    assert (out[d[..., 2] == 0] == 0).all()
    assert np.array_equal(out, oracle.parabola_subpixel(d, left, right, 0, 0.0, (1, 1)))


@pytest.mark.parametrize("slope,moves", [(99, True), (101, False)])
def test_offsets_just_below_and_just_above_five_pixels(oracle, slope, moves):
    """cost = 10 x^2 + 10 y^2 - slope x + 200: the minimum is at x = slope / 20 = 4.95 (accepted) or 5.05 (rejected: the disparity stays)."""
    d, left, right = _costs_as_image(lambda x, y: 10 * x * x + 10 * y * y - slope * x + 200)
    out = parabola_direct.parabola_subpixel(oracle, d, left, right, 0, 0.0, (1, 1))
    if moves:
        assert abs(out[2, 2, 0] - (1 + slope / 20)) < 1e-4 and abs(out[2, 2, 1]) < 1e-4
    else:
        assert tuple(out[2, 2]) == (1.0, 0.0, 1.0)
    assert np.array_equal(out, oracle.parabola_subpixel(d, left, right, 0, 0.0, (1, 1)))


def test_all_equal_costs_keep_the_truncated_disparity(oracle):
    left, right = np.full((6, 7), 0.5, np.float32), np.full((6, 9), 0.6, np.float32)
    d = np.zeros((6, 7, 3), np.float32)
    d[..., 0], d[..., 1], d[..., 2] = 1.7, -0.4, 1
    out = parabola_direct.parabola_subpixel(oracle, d, left, right, 0, 0.0, (3, 3))
    assert (out[..., 0] == 1).all() and (out[..., 1] == 0).all() and (out[..., 2] == 1).all()
    assert np.array_equal(out, oracle.parabola_subpixel(d, left, right, 0, 0.0, (3, 3)))
    ox, oy, moved = parabola_direct.solve(np.full((9,), 7.0, np.float32))
    assert not moved
