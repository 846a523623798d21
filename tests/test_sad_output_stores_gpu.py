"""The output stores of the packed-u8 SAD matcher: every wave writes its 768-dword row segment as three pieces of 16-byte lane stores at
whatever 4-byte alignment the segment has, single dwords at the row end; on grids of two rounds or more they carry the non-temporal hint.

How the 16-byte stores fall on the 128-byte lines depends on the address of the segment, i.e. on the row pitch 12 * ow (dense output) or
12 * os (a view), on the row and on the start of the buffer.  Output widths (left image = ow + 6 for the 7 x 7 kernel) and 12 * ow mod 128:

  ow              256   299   310   1027   1034   1065   282   261   1045     9
  12 * ow % 128     0     4     8     36    120    108    56    60    124   108

256 is one full wave with an empty tail, 1034, 1045 and 1065 spill into a second tile column, 261 leaves the second wave 15 dwords, 282
has the pitch class of the 4090-pixel headline (56), and 9 pixels are 27 dwords: no body at all.
Image heights 22 and 35 give 16 and 29 output rows: one tile row, and two with the second ragged.  Searches of 129 and 9 disparities.

Every case is bit for bit the CPU oracle's result, in both forms the launcher offers for the call (VWGPU_OPT_SAD_LAYOUT = 0 and 1), and
the kernel the launcher took is read back through VWGPU_OPT_SAD_LAST_LAUNCH and asserted.  The launcher plans for two workgroup slots
(VWGPU_OPT_SAD_ROUND_SLOTS = 2) so that all but the single-tile images take the 1024 x 16 tile of the headline and every one-group case
runs as a grid of several rounds, i.e. the kernels with streaming stores (bit 17 of the option); the split grids run the plain ones.  The
views, the constant image (plain zero stores of the validity sweep after the streaming stores) and the split grids are cases of their own."""
import ctypes

import numpy as np
import pytest

import visionworkbench_amd as vwa
from visionworkbench_amd import core, synth

pytestmark = pytest.mark.gpu

ABS = 0
KERNEL = (7, 7)
WIDTHS = [256, 299, 310, 1027, 1034, 1065, 282, 261, 1045, 9]          # output widths
HEIGHTS = [22, 35]                                      # image heights: 16 and 29 output rows
SENTINEL = 0x5a5a5a5a


def test_widths_cover_the_pitch_classes():
    assert {0, 4, 8, 56, 60, 124} <= {12 * ow % 128 for ow in WIDTHS}
    assert 3 * min(WIDTHS) < 32


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
    ctx.set_option(core.OPT_SAD_LAYOUT, 0)


_CASES = {}


def _case(oracle, name, ow, h, sx):
    """(left, right, oracle result), computed once per image and search and never modified."""
    key = (name, ow, h, sx)
    if key not in _CASES:
        w = ow + KERNEL[0] - 1
        if name == "constant":
            left = np.full((h, w), 77.0, np.float32)
            right = np.full((h, w + sx - 1), 77.0, np.float32)
        else:
            left, right, _ = synth.stereo_pair(w, h, sx, 1, block=64, seeds=(41, 42, 43))
        want = oracle.calc_disparity(ABS, left, right, KERNEL, (sx, 1))
        assert want.shape == (h - KERNEL[1] + 1, ow, 3)
        for a in (left, right, want):
            a.setflags(write=False)
        _CASES[key] = (left, right, want)
    return _CASES[key]


def _launch(ctx):
    v = ctx.get_option(core.OPT_SAD_LAST_LAUNCH)
    return (v & 0xff, ((v >> 8) & 0xf) * 256, (v >> 12) & 0xf, bool((v >> 16) & 1), bool((v >> 17) & 1))


def _expected_tile(ow, oh, groups):
    """What the launcher's cost model takes: (tile rows, tile columns, wave groups)."""
    if groups == 2:
        return (8, 1024, 2)
    if groups == 3:
        return (16, 512, 4)
    return (8, 1024, 1) if (ow <= 1024 and oh <= 16) else (16, 1024, 1)      # two slots: only a single tile is cheaper in 8-row tiles


def _run(ctx, left, right, sx, layout, groups, view=None):
    """One call; view = (os, first pixel): the output is a view into a wider, sentinel-filled buffer, which is returned whole."""
    import torch
    ctx.set_option(core.OPT_SAD_GROUPS, groups)
    ctx.set_option(core.OPT_SAD_ROUND_SLOTS, 2 if groups == 1 else 0)
    ctx.set_option(core.OPT_SAD_LAYOUT, layout)
    lt, rt = torch.from_numpy(left.copy()).cuda(), torch.from_numpy(right.copy()).cuda()
    lh, lw = left.shape
    ow, oh = lw - KERNEL[0] + 1, lh - KERNEL[1] + 1
    if view is None:
        os_, first = ow, 0
    else:
        os_, first = view
    buf = torch.full(((oh + 2) * os_ * 3,), SENTINEL, dtype=torch.int32, device="cuda")
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(ctx._lib.vwgpu_calc_disparity_dev(ctx._h, ABS, lt.data_ptr(), lw, lh, lt.stride(0), rt.data_ptr(), rt.shape[1], rt.shape[0],
                                                rt.stride(0), KERNEL[0], KERNEL[1], sx, 1,
                                                ctypes.c_void_p(buf.data_ptr() + 4 * 3 * first), os_))
    torch.cuda.synchronize()
    ctx.synchronize()
    assert ctx.last_path() == core.PATH_SAD_U8
    tile = _launch(ctx)
    assert tile[:3] == _expected_tile(ow, oh, groups), "the launcher took %s" % (tile,)
    assert tile[3] == (layout == 0), "layout %d: the launcher took %s" % (layout, tile)
    # eight workgroups on two slots are four rounds: the one-group cases run the kernels with streaming stores, the split grids never do
    assert tile[4] == (groups == 1), "streaming stores: the launcher took %s" % (tile,)
    return buf.cpu().numpy()


def _check(ctx, oracle, name, ow, h, sx, groups=1, view=None):
    left, right, want = _case(oracle, name, ow, h, sx)
    oh = want.shape[0]
    os_, first = (ow, 0) if view is None else view
    for layout in (0, 1):
        buf = _run(ctx, left, right, sx, layout, groups, view)
        rows = np.lib.stride_tricks.as_strided(buf[3 * first:], shape=(oh, ow, 3), strides=(12 * os_, 12, 4))
        assert np.array_equal(rows, want), "layout %d differs from the oracle" % layout
        untouched = np.ones(buf.shape, bool)
        for y in range(oh):
            untouched[3 * (first + y * os_):3 * (first + y * os_ + ow)] = False
        assert (buf[untouched] == SENTINEL).all(), "layout %d: a dword outside the output rows was written" % layout
    return want


@pytest.mark.parametrize("sx", [129, 9])
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("ow", WIDTHS)
def test_dense_output(ctx, oracle, ow, h, sx):
    """Row pitch 12 * ow: the segment's alignment changes from row to row for every width but 256."""
    _check(ctx, oracle, "textured", ow, h, sx)


@pytest.mark.parametrize("sx", [129, 9])
@pytest.mark.parametrize("ow", WIDTHS)
def test_view_into_a_wider_buffer(ctx, oracle, ow, sx):
    """os > ow and a first pixel at an odd dword offset; nothing outside the view's rows may change."""
    os_ = ow + 11
    first = os_ + (1 if (3 * (os_ + 1)) % 2 else 2)
    assert (3 * first) % 2 == 1
    _check(ctx, oracle, "textured", ow, 35, sx, view=(os_, first))


@pytest.mark.parametrize("ow", [299, 1034])
def test_constant_image(ctx, oracle, ow):
    """The validity sweep's plain zero stores land after the streaming stores to the same dwords: every pixel invalid, as the oracle says."""
    want = _check(ctx, oracle, "constant", ow, 35, 9)
    assert (want[..., 2] == 0).all()
    _check(ctx, oracle, "constant", ow, 35, 9, view=(ow + 5, ow + 5 + (1 if (ow + 5 + 1) % 2 else 2)))


@pytest.mark.parametrize("name", ["textured", "constant"])
@pytest.mark.parametrize("groups", [2, 3])
def test_split_grids(ctx, oracle, groups, name):
    """Two wave groups on the 1024-column tile and four on the 512-column tile: each group stores its own rows from its own buffers."""
    _check(ctx, oracle, name, 1034, 35, 129 if name == "textured" else 9, groups=groups)
    _check(ctx, oracle, name, 299, 35, 9, groups=groups, view=(310, 311))
