"""CPU: the sequential restatement of PyramidSubpixelView with SUBPIXEL_LUCAS_KANADE and SUBPIXEL_BAYES_EM (tests/refimpl/
pyr_ref.cc), hand-derived results of both refiners, and the argument checks of stereo.pyramid_subpixel / lk_subpixel /
bayes_em_subpixel, which fail before any device work."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import pyr_ref  # noqa: E402

from visionworkbench_amd import core, stereo  # noqa: E402

LK, EM = stereo.SUBPIXEL_LUCAS_KANADE, stereo.SUBPIXEL_BAYES_EM


def test_restatement_builds():
    assert os.path.exists(pyr_ref.build())


@pytest.mark.parametrize("alg", [LK, EM])
def test_top_left_invalid_keeps_the_input(alg):
    """Both window loops weight every pixel with w(0, 0) (the weight accessor is never advanced): where the top-left window
    pixel is invalid, LK's system is all zero and EM skips every pixel (weight 0 < 1e-26), so the disparity comes back
    bit for bit."""
    left, right, d, (ys, xs) = pyr_ref.unit_top_left_hole_scene()
    out, _ = pyr_ref.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 0, algorithm=alg)
    assert len(ys) >= 20
    assert np.array_equal(out[ys, xs], d[ys, xs])
    assert np.count_nonzero(out[ys, xs + 1, 0] != d[ys, xs + 1, 0]) >= len(ys) // 2


@pytest.mark.parametrize("alg", [LK, EM])
@pytest.mark.parametrize("levels", [0, 2])
def test_equal_flat_images_keep_the_input(alg, levels):
    """Zero derivatives: the systems are zero, posv fails, the update is 0; every interior pixel stays valid and unchanged
    (border pixels lose the zero-extended half of their window)."""
    f = np.full((60, 70), 0.5, np.float32)
    d = np.zeros((60, 70, 3), np.float32)
    d[..., 0], d[..., 2] = 3, 1
    out, _ = pyr_ref.pyramid_subpixel(d, f, f, 0, 1.5, (7, 7), levels, algorithm=alg)
    inner = (slice(3, -3), slice(3, -3))
    assert np.array_equal(out[inner], d[inner])


def test_em_constant_200_100_invalidates_every_pixel():
    """left = 200, right = 100: both probabilities underflow (exponents -5e6 and -5e5 < -75), gamma = 0 / 0 = NaN enters
    the sums, posv fails on A(1,1) = NaN and d turns NaN: every evaluated pixel is invalid, written {0, 0, 0}."""
    left = np.full((50, 60), 200, np.float32)
    right = np.full((50, 60), 100, np.float32)
    d = np.zeros((50, 60, 3), np.float32)
    d[..., 0], d[..., 2] = 2, 1
    out, passes = pyr_ref.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 0, algorithm=EM)
    assert (out == 0).all()
    assert passes > 0


@pytest.mark.parametrize("alg", [LK, EM])
def test_cascade_scene_depends_on_in_place_invalidation(alg):
    left, right, d, _ = pyr_ref.unit_cascade_scene(96, 80)
    seq, _ = pyr_ref.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 2, algorithm=alg)
    par, _ = pyr_ref.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 2, inplace=False, algorithm=alg)
    assert np.any(seq != par, axis=2).sum() >= 50      # measured: 1860 pixels for both


# measured on the 128 x 96 [0, 1] stretched scene, 15 x 15, max_pyramid_levels 2: (MAE of the result, invalid share);
# the integer start has MAE 0.243.  FAST_AFFINE on the same input: 0.127 (NONE), 0.135 (LOG).
MEASURED = {(LK, 0): (0.156, 0.0050), (LK, 2): (0.138, 0.0061), (EM, 0): (0.140, 0.0050), (EM, 2): (0.140, 0.0050)}


@pytest.mark.parametrize("alg", [LK, EM])
@pytest.mark.parametrize("mode", [0, 2])
def test_unit_stretched_scene_error(alg, mode):
    left, right, d, true = pyr_ref.unit_scene(128, 96)
    out, passes = pyr_ref.pyramid_subpixel(d, left, right, mode, 1.5, (15, 15), 2, algorithm=alg)
    inner = (slice(16, -16), slice(16, -16))
    valid = out[..., 2] > 0
    mae_int = np.abs(d[..., 0] - true)[inner].mean()
    mae = np.abs(out[..., 0] - true)[inner][valid[inner]].mean()
    want_mae, want_invalid = MEASURED[(alg, mode)]
    assert abs(mae_int - 0.243) < 0.002
    assert abs(mae - want_mae) < 0.01, mae
    assert abs((1 - valid.mean()) - want_invalid) < 0.002, 1 - valid.mean()
    assert passes > 128 * 96


def test_restatement_rejects_even_kernel_and_phase():
    left, right, d, _ = pyr_ref.unit_scene(32, 24)
    with pytest.raises(ValueError):
        pyr_ref.pyramid_subpixel(d, left, right, 0, 1.5, (8, 7), 1, algorithm=EM)
    with pytest.raises(ValueError):
        pyr_ref.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 1, algorithm=3)


@pytest.mark.parametrize("fn", [stereo.lk_subpixel, stereo.bayes_em_subpixel])
def test_argument_checks_without_gpu(fn):
    left, right, d, _ = pyr_ref.unit_scene(32, 24)
    with pytest.raises(core.ArgumentErr):
        fn(d[:-1], left, right, 0, 1.5, (7, 7))
    with pytest.raises(core.ArgumentErr):
        fn(d, left, right, 0, 1.5, (8, 7))
    with pytest.raises(core.ArgumentErr):
        fn(d, left, right, 0, 1.5, (7, 6))
    with pytest.raises(core.ArgumentErr):
        fn(d, left[:, :, None], right, 0, 1.5, (7, 7))


def test_pyramid_subpixel_argument_checks_without_gpu():
    left, right, d, _ = pyr_ref.unit_scene(32, 24)
    with pytest.raises(core.NoImplErr):
        stereo.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 2, stereo.SUBPIXEL_PHASE)
    with pytest.raises(core.ArgumentErr):
        stereo.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 2, 4)
    with pytest.raises(core.ArgumentErr):
        stereo.pyramid_subpixel(d, left, right, 0, 1.5, (7, 8), 2, EM)
    with pytest.raises(core.NoImplErr):     # affine_subpixel keeps its single algorithm
        stereo.affine_subpixel(d, left, right, 0, 1.5, (7, 7), algorithm=EM)


def test_em_exp_header_on_the_host():
    """em_exp.h compiled for the host (the same operations as the device build) against the host libm's
    (float)((double)k * exp((double)e)) at every 4093rd float in [-75, 0], +-0.0, NaN and the two midpoint inputs."""
    exe = pyr_ref.build_exp_check()
    r = subprocess.run(["timeout", "-k", "10", "300", exe, "host", "4093"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
