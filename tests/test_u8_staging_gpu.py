"""Staging of float tiles as packed u8 (csrc/u8_tile.h) through the packed matchers, pixel for pixel against the CPU oracle.

The helper loads 16 bytes per row and lane whatever the alignment of the image, so the cases are about where an image starts and ends
in memory: contiguous images whose row stride is or is not a multiple of four floats, views of a wider parent cut at columns 1, 2, 3
(base off 16-byte alignment) for the left, the right or both images, a group of four pixels that straddles the right edge with valid
parent pixels behind it, tiles whose lower rows are outside the image — and the domain check: a pixel that is not an integer in
[0, 255] anywhere inside an image must take the call off the packed path, a pixel just outside it must not.

Images are integer noise in [1, 255], cut out of parents of 48 x 1200 floats; 7x7 window, search 17 x 1; 1100-odd columns are two tiles of
the 1024-column kernels (three of the 512-column one), 40 rows leave tile rows past the bottom.  Every call runs with the launcher's own
choice (a grid this small gets a tile with several wave groups, whose threads cover every column in the main part) and with one wave group
pinned (1024 columns, 256 threads: the columns from 1024 on are the remainder columns of tile 0).  Contexts are not deferred: ctx.last_path() is the
path that produced the result.  A call that follows a refused one measures the input class before it tries the packed kernel, so every
bad-pixel case runs a clean call first: the packed kernel itself must raise the flag."""
import numpy as np
import pytest

import visionworkbench_amd as vwa
from visionworkbench_amd import core

pytestmark = pytest.mark.gpu

SAD, SSD, NCC = 0, 1, 2
KERNEL, SEARCH = (7, 7), (17, 1)
PH, PW, H = 48, 1200, 40
GROUPS = (0, 1)
BAD = {"half": 0.5, "256": 256.0, "minus_one": -1.0, "nan": float("nan"), "minus_zero": -0.0}


def _parents():
    rng = np.random.default_rng(20)
    return (rng.integers(1, 256, (PH, PW)).astype(np.float32), rng.integers(1, 256, (PH, PW)).astype(np.float32))


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    c = vwa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def parents():
    """(left, right) parents on the host and on the device; never modified (tests that plant a pixel work on copies)."""
    import torch
    pl, pr = _parents()
    return pl, pr, torch.from_numpy(pl).cuda(), torch.from_numpy(pr).cuda()


@pytest.fixture(autouse=True)
def _default_options(ctx):
    yield
    ctx.set_option(core.OPT_SAD_GROUPS, 0)


_REFS = {}


def _reference(oracle, cost, left, right, key=None):
    """oracle.calc_disparity, computed once per geometry of the unmodified parents."""
    if key is None:
        return oracle.calc_disparity(cost, np.ascontiguousarray(left), np.ascontiguousarray(right), KERNEL, SEARCH)
    if key not in _REFS:
        _REFS[key] = oracle.calc_disparity(cost, np.ascontiguousarray(left), np.ascontiguousarray(right), KERNEL, SEARCH)
    return _REFS[key]


def _cut(p, k, w, h=H):
    return p[:h, k:k + w]


def _run(ctx, cost, lt, rt, groups):
    import torch
    from visionworkbench_amd import stereo
    ctx.set_option(core.OPT_SAD_GROUPS, groups)
    out = stereo.calc_disparity(cost, lt, rt, vwa.bounding_box(lt), SEARCH, KERNEL, ctx=ctx)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ctx.last_path()


def _check(ctx, oracle, cost, lt, rt, left, right, key, what, path=None):
    """Every wave-group choice gives the oracle's image on the packed path of the cost."""
    want = _reference(oracle, cost, left, right, key)
    path = path if path is not None else (core.PATH_SAD_U8 if cost == SAD else core.PATH_DOT_U8)
    for g in (GROUPS if cost == SAD else (0,)):
        got, took = _run(ctx, cost, lt, rt, g)
        assert took == path, "%s, groups %d: path %d" % (what, g, took)
        assert np.array_equal(got, want), "%s, groups %d: differs from the oracle" % (what, g)


def _geometry(parents, kl, kr, w, h=H, contiguous=False):
    """Left view at column kl and right view at column kr of the parents (w and w + 16 columns, h rows), host and device."""
    pl, pr, plt, prt = parents
    rw = w + SEARCH[0] - 1
    left, right, lt, rt = _cut(pl, kl, w, h), _cut(pr, kr, rw, h), _cut(plt, kl, w, h), _cut(prt, kr, rw, h)
    if contiguous:
        lt, rt = lt.contiguous(), rt.contiguous()
        assert lt.data_ptr() % 16 == 0 and rt.data_ptr() % 16 == 0 and lt.stride(0) == w
    else:
        assert lt.stride(0) == PW and rt.stride(0) == PW and lt.data_ptr() % 16 == (4 * kl) % 16 and rt.data_ptr() % 16 == (4 * kr) % 16
    return lt, rt, left, right


# ---- 1, 2: contiguous images ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [1100, 1101, 1102, 1103])
def test_contiguous(ctx, oracle, parents, w):
    """w = 1100: aligned base, row stride a multiple of 4 floats.  1101 .. 1103: every other row starts off 16-byte alignment and the
    last group of a row straddles the right edge."""
    lt, rt, left, right = _geometry(parents, 0, 0, w, contiguous=True)
    _check(ctx, oracle, SAD, lt, rt, left, right, ("cut", 0, 0, w, H), "contiguous w = %d" % w)


# ---- 3, 4: views of the parent ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("side", ["left", "right", "both"])
def test_view_off_alignment(ctx, oracle, parents, k, side):
    """Base 4, 8 or 12 bytes off 16-byte alignment with a row stride of 1200 floats: every group of every row is unaligned alike."""
    kl, kr = (k if side != "right" else 0), (k if side != "left" else 0)
    lt, rt, left, right = _geometry(parents, kl, kr, 1100)
    _check(ctx, oracle, SAD, lt, rt, left, right, ("cut", kl, kr, 1100, H), "view at column %d (%s)" % (k, side))


def test_view_straddling_group_with_parent_pixels_behind(ctx, oracle, parents):
    lt, rt, left, right = _geometry(parents, 4, 4, 1101)
    _check(ctx, oracle, SAD, lt, rt, left, right, ("cut", 4, 4, 1101, H), "aligned view of 1101 columns")


# ---- 5: short images ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h", [7, 23])
def test_rows_outside_the_image(ctx, oracle, parents, h):
    """h = 7: one output row, every other row of the tile is outside.  h = 23: 17 output rows, a second tile row with one."""
    lt, rt, left, right = _geometry(parents, 1, 1, 1101, h=h)
    _check(ctx, oracle, SAD, lt, rt, left, right, ("cut", 1, 1, 1101, h), "h = %d" % h)


# ---- 6: a pixel outside the domain, inside the image --------------------------------------------------------------------------------------

W6, K6, ROW6 = 1101, 1, 20
# (image, column): the main part, the remainder columns of tile 0 (1024-column tiles: groups 256 on), the group that straddles the edge
INSIDE = {"left_main": (0, 100), "left_margin": (0, 1030), "left_straddle": (0, W6 - 1),
          "right_main": (1, 100), "right_margin": (1, 1040), "right_straddle": (1, W6 + SEARCH[0] - 2)}


@pytest.mark.parametrize("value", sorted(BAD))
@pytest.mark.parametrize("where", sorted(INSIDE))
def test_bad_pixel_inside_leaves_the_packed_path(ctx, oracle, parents, where, value):
    import torch
    lt0, rt0, left0, right0 = _geometry(parents, K6, K6, W6)
    img, x = INSIDE[where]
    hp = [parents[0].copy(), parents[1].copy()]
    hp[img][ROW6, K6 + x] = BAD[value]
    dp = [torch.from_numpy(hp[0]).cuda(), torch.from_numpy(hp[1]).cuda()]
    rw = W6 + SEARCH[0] - 1
    left, right = _cut(hp[0], K6, W6), _cut(hp[1], K6, rw)
    lt, rt = _cut(dp[0], K6, W6), _cut(dp[1], K6, rw)
    want = _reference(oracle, SAD, left, right)
    for g in GROUPS:
        got, took = _run(ctx, SAD, lt0, rt0, g)                  # clean call: the next one tries the packed kernel first
        assert took == core.PATH_SAD_U8
        assert np.array_equal(got, _reference(oracle, SAD, left0, right0, ("cut", K6, K6, W6, H)))
        got, took = _run(ctx, SAD, lt, rt, g)
        assert took != core.PATH_SAD_U8, "%s = %s, groups %d: the packed kernel accepted the pixel" % (where, value, g)
        assert np.array_equal(got, want), "%s = %s, groups %d: differs from the oracle" % (where, value, g)


# ---- 7: the same pixel just outside the image ------------------------------------------------------------------------------------------------

W7, K7 = 1101, 4
OUTSIDE = {"right_of_left": (0, ROW6, K7 + W7), "below_left": (0, H, K7 + 500),
           "right_of_right": (1, ROW6, K7 + W7 + SEARCH[0] - 1), "below_right": (1, H, K7 + 500)}


def _planted(parents, places, value):
    import torch
    hp = [parents[0].copy(), parents[1].copy()]
    for name in places:
        img, y, x = OUTSIDE[name]
        hp[img][y, x] = value
    rw = W7 + SEARCH[0] - 1
    dp = [torch.from_numpy(hp[0]).cuda(), torch.from_numpy(hp[1]).cuda()]
    return _cut(dp[0], K7, W7), _cut(dp[1], K7, rw), _cut(hp[0], K7, W7), _cut(hp[1], K7, rw)


@pytest.mark.parametrize("value", sorted(BAD))
@pytest.mark.parametrize("where", sorted(OUTSIDE))
def test_bad_pixel_outside_stays_on_the_packed_path(ctx, oracle, parents, where, value):
    lt, rt, left, right = _planted(parents, [where], BAD[value])
    _check(ctx, oracle, SAD, lt, rt, left, right, ("cut", K7, K7, W7, H), "%s = %s" % (where, value))


# ---- 8: SSD and NCC through the same helper (bm_corr_u8) ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("cost", [SSD, NCC])
def test_corr_u8_contiguous(ctx, oracle, parents, cost):
    lt, rt, left, right = _geometry(parents, 0, 0, 1100, contiguous=True)
    _check(ctx, oracle, cost, lt, rt, left, right, ("cost", cost, 0, 0, 1100), "cost %d, contiguous" % cost)


@pytest.mark.parametrize("cost", [SSD, NCC])
@pytest.mark.parametrize("side", ["left", "right", "both"])
def test_corr_u8_view_off_alignment(ctx, oracle, parents, cost, side):
    kl, kr = (1 if side != "right" else 0), (1 if side != "left" else 0)
    lt, rt, left, right = _geometry(parents, kl, kr, 1100)
    _check(ctx, oracle, cost, lt, rt, left, right, ("cost", cost, kl, kr, 1100), "cost %d, view at column 1 (%s)" % (cost, side))


@pytest.mark.parametrize("cost", [SSD, NCC])
def test_corr_u8_bad_pixels_outside(ctx, oracle, parents, cost):
    lt, rt, left, right = _planted(parents, sorted(OUTSIDE), 0.5)
    _check(ctx, oracle, cost, lt, rt, left, right, ("cost", cost, K7, K7, W7), "cost %d, 0.5 right of and below both views" % cost)
