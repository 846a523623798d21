"""CPU: the search range the sub-pixel refiners take of a tile, pinned without leaning on what a restatement's author believed.

PyramidSubpixelView::prerasterize begins with get_disparity_range(crop(disparity, bbox)) (src/vw/Stereo/SubpixelView.cc:42), and that
range is taken over the tile's VALID pixels (Image/Statistics.h:283-290; TestDisparity.cxx::GetDisparityRange), zeros without any.

  a. known answers for tests/refimpl/tile_range.h, the helper the three restatements share: the reference's own test, and 50 random
     crops against disparity_map_ref's get_disparity_range (written separately, pinned by TestDisparity.cxx), truncated the same way;
  b. fill invariance of the four restatements and of the parabola's two formulations: the output must not depend on what invalid pixels
     store (tests/subpixel_range_cases.py).  Before the restatements took the range over valid pixels only, `zero` and `inrange`
     differed by up to several pixels on most of the image at two pyramid levels;
  c. the edges of the rule: an all-invalid block that stores a far value, 1 x 1 tiles, a tile whose only valid pixel is its last.

Every comparison is np.array_equal on all three channels.  The kernels meet the same cases in tests/test_subpixel_range_gpu.py."""
import os
import sys

import numpy as np
import pytest

import subpixel_range_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import affine_ref  # noqa: E402
import disparity_map_ref  # noqa: E402
import parabola_direct  # noqa: E402


# ---- a. the range itself ----------------------------------------------------------------------------------------------------------------

def test_tile_range_reference_known_answers():
    """TestDisparity.cxx::GetDisparityRange: (2, 2), (3, 5) and an invalidated (-4, -1) give min (2, 2), max (3, 5); all invalid: zeros."""
    d = np.zeros((1, 3, 3), np.float32)
    d[0, 0], d[0, 1], d[0, 2] = (2, 2, 1), (3, 5, 1), (-4, -1, 0)
    assert affine_ref.tile_range(d).tolist() == [2, 2, 3, 5]
    assert affine_ref.tile_range(d, (1, 0, 2, 1)).tolist() == [3, 5, 3, 5]
    d[..., 2] = 0
    assert affine_ref.tile_range(d).tolist() == [0, 0, 0, 0]


def test_tile_range_equals_the_disparity_map_restatement_on_random_crops():
    """50 crops, 1 x 1 to 40 x 30, 0 to 100 % invalid, invalid pixels holding values outside the valid range (finite and not); each
    corner truncated by a C cast (Math/BBox.tcc:49-50) on both sides."""
    rng = np.random.RandomState(11)
    d = np.zeros((64, 80, 3), np.float32)
    seen_empty = seen_full = 0
    for it in range(50):
        w, h = (1, 1) if it == 0 else (40, 30) if it == 1 else (rng.randint(1, 41), rng.randint(1, 31))
        x, y = rng.randint(0, 80 - w + 1), rng.randint(0, 64 - h + 1)
        share = (0.0, 1.0, 0.5)[it] if it < 3 else rng.choice([0.0, 1.0, rng.uniform()], p=[0.1, 0.1, 0.8])
        d[..., 0] = rng.uniform(-40, 40, size=d.shape[:2])
        d[..., 1] = rng.uniform(-9.9, 9.9, size=d.shape[:2])
        d[..., 2] = 1
        bad = rng.uniform(size=d.shape[:2]) < share
        bad[y, x] = share > 0.0 and (share == 1.0 or bad[y, x])
        n = int(bad.sum())
        far = np.concatenate([rc.GARBAGE, np.float32([-41, 41, 100.25, -5000])])
        d[bad, 0] = far[rng.randint(0, len(far), n)]
        d[bad, 1] = far[rng.randint(0, len(far), n)]
        d[bad, 2] = 0
        crop = np.ascontiguousarray(d[y:y + h, x:x + w])
        want = disparity_map_ref.get_disparity_range(crop)
        assert np.isfinite(want).all()
        got = affine_ref.tile_range(d, (x, y, w, h))
        assert got.tolist() == [int(v) for v in want], (it, (x, y, w, h), got, want)       # int(): toward zero, the C cast
        assert np.array_equal(got, affine_ref.tile_range(crop))
        valid = crop[..., 2] != 0
        seen_empty += not valid.any()
        seen_full += valid.all()
        if valid.any():                                   # stated once more in numpy
            assert got.tolist() == [int(crop[valid][:, 0].min()), int(crop[valid][:, 1].min()),
                                    int(crop[valid][:, 0].max()), int(crop[valid][:, 1].max())]
        else:
            assert got.tolist() == [0, 0, 0, 0]
    assert seen_empty >= 2 and seen_full >= 2


def test_parabola_range_is_over_valid_pixels():
    (mnx, mny, mxx, mxy), _, _ = parabola_direct.disparity_range(np.float32([[(2, 2, 1), (3, 5, 1), (-4, -1, 0)]]))
    assert (mnx, mny, mxx, mxy) == (2, 2, 3, 5)
    assert parabola_direct.disparity_range(np.float32([[(np.nan, 3e38, 0), (-np.inf, 7, 0)]]))[0] == (0, 0, 0, 0)


# ---- b. fill invariance -----------------------------------------------------------------------------------------------------------------

def _same(a, b, what):
    diff = (a != b).any(-1)
    assert np.array_equal(a, b), "%s: %d pixels differ (%d in validity), largest |delta| %g px, %.2f of the valid pixels by more than 1e-5" % (
        what, diff.sum(), (a[..., 2] != b[..., 2]).sum(), np.nanmax(np.abs(a[..., :2] - b[..., :2])),
        (np.abs(a[..., :2] - b[..., :2]).max(-1) > 1e-5)[a[..., 2] != 0].mean())


@pytest.mark.parametrize("cid", rc.matrix_ids())
def test_restatement_does_not_depend_on_what_invalid_pixels_store(cid):
    alg, left, right, d, levels, block, (mode, width), tiles = rc.refiner_scene(cid)
    mask = rc.hole_mask()
    out = {}
    for v in rc.VARIANTS:
        out[v] = rc.restatement(alg, rc.variant(d, tiles, v, mask), left, right, mode, width, levels, tiles)
        assert not np.isnan(out[v]).any()
        assert (out[v][out[v][..., 2] == 0] == 0).all(), "an invalid output pixel is {0, 0, 0}"
        if levels == 0:                                   # (with a pyramid, the upsampled coarser level fills holes: SubpixelView.cc:183-189)
            assert (out[v][mask] == 0).all()
        if v != "zero":
            _same(out["zero"], out[v], "zero / " + v)
    assert (out["zero"][..., 2] != 0).sum() > 0.5 * mask.size


@pytest.mark.parametrize("which", ["direct", "oracle"])
def test_parabola_does_not_depend_on_what_invalid_pixels_store(oracle, which):
    """the parabola's values do not depend on the range (the rasters move with it, the windows do not)."""
    left, right, d, mask, tiles = rc.parabola_scene()

    def run(disp):
        if which == "oracle":
            return oracle.parabola_subpixel(disp, left, right, 0, 0.0, rc.KERNEL)
        return parabola_direct.parabola_subpixel(oracle, disp, left, right, 0, 0.0, rc.KERNEL)

    zero = run(rc.variant(d, tiles, "zero", mask))
    assert (zero[mask] == 0).all() and (zero[~mask, 2] == 1).all()
    for v in ("inrange", "garbage"):
        _same(zero, run(rc.variant(d, tiles, v, mask)), "zero / " + v)


# ---- c. edges of the rule ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels", [0, 2])
@pytest.mark.parametrize("refiner", list(rc.REFINERS))
def test_an_all_invalid_block_with_a_far_value_is_zeros_and_moves_no_other_block(refiner, levels):
    """The block's range is (0, 0, 0, 0), whatever it stores.  Without a pyramid the block is zeros.  With one, the reference itself
    fills pixels along the block's edges: the patch reaches a kernel into the valid neighbours, disparity_subsample averages them and
    the upsampled level carries its validity down (SubpixelView.cc:183-189) -- so there the whole output, the block included, must
    equal the run in which the block stores zeros."""
    alg, left, right, d, _, block, (mode, width), tiles = rc.refiner_scene("%s-plus5-%d-32x24-none" % (refiner, levels))
    mask = rc.hole_mask()
    a, b = rc.variant(d, tiles, "zero", mask), rc.variant(d, tiles, "zero", mask)
    a[24:48, 32:64] = 0
    b[24:48, 32:64] = (50, -50, 0)
    assert affine_ref.tile_range(b, (32, 24, 32, 24)).tolist() == [0, 0, 0, 0]
    oa = rc.restatement(alg, a, left, right, mode, width, levels, tiles)
    ob = rc.restatement(alg, b, left, right, mode, width, levels, tiles)
    if levels == 0:
        assert (ob[24:48, 32:64] == 0).all()
    assert (ob[24 + 8:48, 32 + 8:64] == 0).all()
    assert np.array_equal(oa, ob)
    assert (ob[:24, :, 2] != 0).mean() > 0.5


@pytest.mark.parametrize("refiner", list(rc.REFINERS))
def test_one_pixel_tiles_and_a_tile_whose_only_valid_pixel_is_its_last(refiner):
    alg, left, right, d, _, _, (mode, width), _ = rc.refiner_scene(refiner + "-plus5-2-whole-none")
    d[10, 20] = (-300, 200, 0)                            # the invalid 1 x 1 tile
    last = d.copy()
    last[24:48, 32:64] = (-77, 3e38, 0)
    last[47, 63] = d[47, 63]
    tiles = [(30, 12, 1, 1), (20, 10, 1, 1)]
    for levels in (0, 2):
        out = rc.restatement(alg, d, left, right, mode, width, levels, tiles)
        if levels == 0:                                   # (with a pyramid the valid neighbours fill the pixel, as in the reference)
            assert (out[10, 20] == 0).all()
        tame = d.copy()
        tame[10, 20] = 0
        assert np.array_equal(rc.restatement(alg, tame, left, right, mode, width, levels, tiles), out)
        out[12, 30] = out[10, 20] = 0
        assert (out == 0).all()                           # nothing outside the two tiles is written
        assert np.array_equal(affine_ref.tile_range(last, (32, 24, 32, 24)), [int(d[47, 63, 0]), 0] * 2)
        got = rc.restatement(alg, last, left, right, mode, width, levels, [(32, 24, 32, 24)])
        tame = last.copy()
        tame[last[..., 2] == 0] = 0
        tame[24:48, 32:64, 0] = d[47, 63, 0]              # the block's holes store its only valid value
        assert np.array_equal(got, rc.restatement(alg, tame, left, right, mode, width, levels, [(32, 24, 32, 24)]))
        if levels == 0:                                   # (with a pyramid the neighbours' validity is carried into the block's edges)
            assert (got[24:48, 32:64][:-1] == 0).all() and (got[47, 32:63] == 0).all()
