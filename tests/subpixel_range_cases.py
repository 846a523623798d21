"""Scenes of tests/test_subpixel_range_cpu.py (the restatements, no GPU) and tests/test_subpixel_range_gpu.py (the kernels), from
one place so that the two files cannot drift.

The property they pin belongs to the reference: PyramidSubpixelView::prerasterize sizes its patches with get_disparity_range(crop(
disparity, bbox)) (src/vw/Stereo/SubpixelView.cc:42), whose accumulator takes valid pixels only (Image/Statistics.h:283-290), and no
later statement reads the value of an invalid pixel.  So the result must not depend on what invalid pixels STORE.  Every base scene is
64 x 48 with the same 5 % of its pixels punched out; the three variants differ only in what the holes store:

  zero      {0, 0, 0}: what every filter of this project writes; zero lies outside the valid range of every base scene
  inrange   dx, dy of the first valid pixel (raster order) of the SAME tile, flag 0: the tile's range is what the valid pixels give
            under either reading of get_disparity_range (a global fill, or the value the pixel had before the punch, can widen a
            tile's range: the hole may have held its tile's only extreme)
  garbage   dx, dy cycle through NaN, +-Inf, +-3e38, 1e9, -1000.5, 777, flag 0
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "refimpl"))
import affine_ref  # noqa: E402

W, H = 64, 48
KERNEL = (7, 7)
LK, AFFINE, EM, PHASE = 0, 1, 2, 3                       # SubpixelView.h:28-33
REFINERS = {"affine": AFFINE, "lk": LK, "em": EM, "phase": PHASE}
BASES = ("plus5", "minus5", "plus5_dy2")
VARIANTS = ("zero", "inrange", "garbage")
BLOCKS = {"whole": None, "32x24": (32, 24), "40x20": (40, 20)}
GARBAGE = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e9, -1000.5, 777], np.float32)


def hole_mask():
    return np.random.RandomState(1).uniform(size=(H, W)) < 0.05


def matrix_ids():
    """refiner-base-levels-tiles-prefilter: no prefilter everywhere, LoG 1.5 on the whole image at two levels."""
    ids = []
    for r in REFINERS:
        for b in BASES:
            for levels in (0, 1, 2):
                for blk in BLOCKS:
                    ids.append("%s-%s-%d-%s-none" % (r, b, levels, blk))
            ids.append("%s-%s-2-whole-log" % (r, b))
    return ids


def parse(cid):
    r, b, levels, blk, pf = cid.split("-")
    return r, b, int(levels), BLOCKS[blk], ((2, 1.5) if pf == "log" else (0, 1.5))


def base_scene(base, unit):
    """left, right, disparity (all valid).  unit: both images scaled by one affine map to [0, 1] (LK / EM / phase)."""
    left, right, d, _ = affine_ref.stretched_scene(W, H, offset=-5.0 if base == "minus5" else 5.0)
    if base == "plus5_dy2":
        d[..., 1] = 2                                    # the imagery need not match: invariance does not care
    if unit:
        lo, hi = min(left.min(), right.min()), max(left.max(), right.max())
        left, right = ((left - lo) / (hi - lo)).astype(np.float32), ((right - lo) / (hi - lo)).astype(np.float32)
    return left, right, d


def variant(d, tiles, which, mask=None):
    """The disparity with its holes filled as `which`; tiles are the {x, y, w, h} boxes the call will use."""
    mask = hole_mask() if mask is None else mask
    out = d.copy()
    out[mask] = 0
    if which == "zero":
        return out
    if which == "garbage":
        n = int(mask.sum())
        i = np.arange(n)
        out[mask, 0] = GARBAGE[i % 8]
        out[mask, 1] = GARBAGE[(i // 8 + 3 * i) % 8]
        return out
    assert which == "inrange"
    for (x, y, w, h) in tiles:
        sub, m = out[y:y + h, x:x + w], mask[y:y + h, x:x + w]
        ok = np.argwhere(sub[..., 2] != 0)
        if len(ok):                                      # (a tile without a valid pixel keeps its zeros)
            fy, fx = ok[0]                               # argwhere is in raster order
            sub[m, 0], sub[m, 1] = sub[fy, fx, 0], sub[fy, fx, 1]
    return out


def refiner_scene(cid):
    """(algorithm, left, right, disparity, levels, block, (mode, width), tiles) of one matrix id."""
    r, b, levels, block, pf = parse(cid)
    left, right, d = base_scene(b, unit=(r != "affine"))
    return REFINERS[r], left, right, d, levels, block, pf, affine_ref.tiles_for(W, H, block)


def parabola_scene():
    """An order-free parabola scene of tests/scenes.py (bytes, 7 x 7, 80 x 48, blocky disparities in [-2, 8] x [-1, 2], all valid) and its
    hole mask: the same construction, one tile (the parabola takes the range of the whole map)."""
    import scenes
    left, right, rng = scenes.parabola_pair("u8")
    d = scenes.parabola_disparity(48, 80, rng, invalid=0.0)
    mask = np.random.RandomState(1).uniform(size=(48, 80)) < 0.05
    return left, right, d, mask, [(0, 0, 80, 48)]


def restatement(alg, d, left, right, mode, width, levels, tiles, kernel=KERNEL):
    """The CPU restatement of refiner `alg` over the {x, y, w, h} tiles; pixels outside the tiles are zero."""
    if alg == PHASE:
        import phase_ref
        return phase_ref.phase_subpixel(d, left, right, mode, width, kernel, levels, 20, tiles=tiles)[0]
    if alg == AFFINE:
        return affine_ref.pyramid_subpixel(d, left, right, mode, width, kernel, levels, tiles=tiles)[0]
    import pyr_ref
    return pyr_ref.pyramid_subpixel(d, left, right, mode, width, kernel, levels, algorithm=alg, tiles=tiles)[0]
