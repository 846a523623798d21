"""CPU: the sequential restatement of PyramidSubpixelView(SUBPIXEL_FAST_AFFINE) (tests/refimpl) and the argument checks of
stereo.affine_subpixel, which fail before any device work."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import affine_ref  # noqa: E402

from visionworkbench_amd import core, stereo  # noqa: E402


def test_restatement_builds():
    assert os.path.exists(affine_ref.build())


@pytest.mark.parametrize("mode", [0, 2])
def test_stretched_scene_lowers_error(mode):
    left, right, d, true = affine_ref.stretched_scene(128, 96)
    out, iters = affine_ref.pyramid_subpixel(d, left, right, mode, 1.5, (15, 15), 2)
    inner = (slice(16, -16), slice(16, -16))
    valid = out[..., 2] > 0
    mae_int = np.abs(d[..., 0] - true)[inner].mean()
    mae_ref = np.abs(out[..., 0] - true)[inner][valid[inner]].mean()
    # measured: 0.243 -> 0.187 (NONE) / 0.196 (LOG), 0.5 % / 0.6 % invalid
    assert mae_ref < 0.85 * mae_int
    assert 1 - valid.mean() < 0.03
    assert iters > 128 * 96


def test_cascade_scene_depends_on_in_place_invalidation():
    left, right, d, _ = affine_ref.cascade_scene(96, 80)
    seq, _ = affine_ref.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 2)
    par, _ = affine_ref.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 2, inplace=False)
    assert np.any(seq != par, axis=2).sum() >= 50      # measured: 2577 pixels


def test_restatement_rejects_even_kernel_and_other_algorithms():
    left, right, d, _ = affine_ref.stretched_scene(32, 24)
    with pytest.raises(ValueError):
        affine_ref.pyramid_subpixel(d, left, right, 0, 1.5, (8, 7), 1)
    with pytest.raises(ValueError):
        affine_ref.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 1, algorithm=2)


def test_block_tiles_cover_the_image_once():
    t = stereo.subpixel_tiles(100, 37, (64, 16))
    cover = np.zeros((37, 100), int)
    for x, y, w, h in t:
        cover[y:y + h, x:x + w] += 1
    assert (cover == 1).all()
    assert stereo.subpixel_tiles(100, 37).tolist() == [[0, 0, 100, 37]]


def test_argument_checks_without_gpu():
    left, right, d, _ = affine_ref.stretched_scene(32, 24)
    with pytest.raises(core.ArgumentErr):
        stereo.affine_subpixel(d[:-1], left, right, 0, 1.5, (7, 7))
    with pytest.raises(core.ArgumentErr):
        stereo.affine_subpixel(d, left, right, 0, 1.5, (8, 7))
    with pytest.raises(core.ArgumentErr):
        stereo.affine_subpixel(d, left, right, 0, 1.5, (7, 6))
    with pytest.raises(core.NoImplErr):
        stereo.affine_subpixel(d, left, right, 0, 1.5, (7, 7), algorithm=stereo.SUBPIXEL_BAYES_EM)


def test_restatement_weights_every_window_pixel_with_the_top_left_weight():
    """Hand-derived, not a comparison: where the top-left window pixel is invalid the reference's system is all zero
    (Correlate.cc:1006-1046 never advances the weight accessor), so the disparity comes back unchanged."""
    left, right, d, (ys, xs) = affine_ref.top_left_hole_scene()
    out, _ = affine_ref.pyramid_subpixel(d, left, right, 0, 1.5, (7, 7), 0)
    assert len(ys) >= 20
    assert np.array_equal(out[ys, xs], d[ys, xs])
    # elsewhere the fit moves the disparity: the pixel to the right of each of those has a valid top-left neighbour
    assert np.count_nonzero(out[ys, xs + 1, 0] != d[ys, xs + 1, 0]) >= len(ys) // 2
