"""The round logic of the one-group packed-u8 SAD matcher — first-round hand-off and end balance — on the smallest grids that have rounds.

Both engage on grids of at least two rounds of dispatch (2 x slots tiles, slots = 2 x CUs on the device), which only a 4096^2 image
reaches.  VWGPU_OPT_SAD_ROUND_SLOTS = n makes the launcher plan for n slots instead, so that a handful of tiles run as first-round,
middle and last-round workgroups: with n slots the first n workgroups are the first round (those the index rule takes for the second of
their CU wait before they stage), the last n the last round (priorities by byte phase).  All of it is timing only: every case is compared
bit for bit with the CPU oracle and with the same call at slots = 0.

  2054 x 70 left image   -> 2048 x 64 output pixels = 2 x 4 = 8 tiles of 1024 x 16
       slots = 4: workgroups 0-3 first round, 4-7 last round;   slots = 2: four rounds, so first, middle and last all occur
  2051 x 67              -> 2045 x 61: output width no multiple of 4, ragged last tile row and column
  2054 x 262             -> 2 x 16 = 32 tiles, slots = 16: blockIdx.x >> 3 is 0 and 1 in the first round, so both arms of the index rule run
  searches of 129, 9 and 1 disparities; a constant image (every pixel invalid: the validity sweep runs in delayed workgroups too).
The tile the launcher took is read back through VWGPU_OPT_SAD_LAST_LAUNCH and asserted."""
import numpy as np
import pytest

import visionworkbench_amd as vwa
from visionworkbench_amd import core, synth

pytestmark = pytest.mark.gpu

ABS = 0
KERNEL = (7, 7)
TILE16 = (16, 1024, 1, True)        # bm_sad_u8_kernel<7,7,16,1,0,true>: the headline kernel
TILE8 = (8, 1024, 1, True)          # what the launcher takes for so few tiles on the real device


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    c = vwa.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _default_options(ctx):
    yield
    ctx.set_option(core.OPT_SAD_GROUPS, 0)
    ctx.set_option(core.OPT_SAD_ROUND_SLOTS, 0)


_CASES = {}


def _case(oracle, name, w, h, sx):
    """(left, right, oracle result), computed once per image and search and never modified."""
    key = (name, w, h, sx)
    if key not in _CASES:
        if name == "constant":
            left = np.full((h, w), 77.0, np.float32)
            right = np.full((h, w + sx - 1), 77.0, np.float32)
        else:
            left, right, _ = synth.stereo_pair(w, h, sx, 1, block=64, seeds=(91, 92, 93))
        want = oracle.calc_disparity(ABS, left, right, KERNEL, (sx, 1))
        for a in (left, right, want):
            a.setflags(write=False)
        _CASES[key] = (left, right, want)
    return _CASES[key]


def _launch(ctx):
    v = ctx.get_option(core.OPT_SAD_LAST_LAUNCH)
    return (v & 0xff, ((v >> 8) & 0xf) * 256, (v >> 12) & 0xf, bool((v >> 16) & 1))


def _run(ctx, left, right, sx, slots):
    import torch
    from visionworkbench_amd import stereo
    ctx.set_option(core.OPT_SAD_GROUPS, 1)
    ctx.set_option(core.OPT_SAD_ROUND_SLOTS, slots)
    lt, rt = torch.from_numpy(left.copy()).cuda(), torch.from_numpy(right.copy()).cuda()
    out = stereo.calc_disparity(ABS, lt, rt, vwa.bounding_box(left), (sx, 1), KERNEL, ctx=ctx)
    torch.cuda.synchronize()
    ctx.synchronize()
    assert ctx.last_path() == core.PATH_SAD_U8
    return out.cpu().numpy(), _launch(ctx)


def _check(ctx, oracle, name, w, h, sx, slots):
    left, right, want = _case(oracle, name, w, h, sx)
    plain, tile0 = _run(ctx, left, right, sx, 0)
    got, tile = _run(ctx, left, right, sx, slots)
    assert tile0 == TILE8, "slots = 0: the launcher took %s" % (tile0,)
    assert tile == TILE16, "slots = %d: the launcher took %s, the case is about %s" % (slots, tile, TILE16)
    assert np.array_equal(plain, want), "slots = 0 differs from the oracle"
    assert np.array_equal(got, want), "slots = %d differs from the oracle" % slots
    assert np.array_equal(got, plain)
    return want


def test_round_slots_option_round_trip(ctx):
    assert ctx.get_option(core.OPT_SAD_ROUND_SLOTS) == 0
    ctx.set_option(core.OPT_SAD_ROUND_SLOTS, 4)
    assert ctx.get_option(core.OPT_SAD_ROUND_SLOTS) == 4
    with pytest.raises(Exception):
        ctx.set_option(core.OPT_SAD_ROUND_SLOTS, -1)


def test_default_slots_launch_is_unchanged(ctx, oracle):
    """slots = 0: the launcher plans for the device as before — 16 tiles of 1024 x 8 for this image, one group, entry-major."""
    left, right, want = _case(oracle, "textured", 2054, 70, 129)
    got, tile = _run(ctx, left, right, 129, 0)
    assert tile == TILE8
    assert ctx.get_option(core.OPT_SAD_LAST_LAUNCH) == (8 | 4 << 8 | 1 << 12 | 1 << 16)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("sx", [129, 9, 1])
@pytest.mark.parametrize("slots", [4, 2])
def test_eight_tiles(ctx, oracle, sx, slots):
    """slots = 4: one first and one last round; slots = 2: four rounds."""
    _check(ctx, oracle, "textured", 2054, 70, sx, slots)


@pytest.mark.parametrize("sx", [129, 9, 1])
@pytest.mark.parametrize("slots", [4, 2])
def test_ragged_tiles(ctx, oracle, sx, slots):
    _check(ctx, oracle, "textured", 2051, 67, sx, slots)


@pytest.mark.parametrize("sx", [129, 9])
def test_thirty_two_tiles_both_arms_of_the_index_rule(ctx, oracle, sx):
    _check(ctx, oracle, "textured", 2054, 262, sx, 16)


@pytest.mark.parametrize("sx", [129, 9, 1])
@pytest.mark.parametrize("slots", [4, 2])
def test_constant_image(ctx, oracle, sx, slots):
    want = _check(ctx, oracle, "constant", 2054, 70, sx, slots)
    if sx > 1:
        assert (want[..., 2] == 0).all()
