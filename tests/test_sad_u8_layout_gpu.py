"""The packed-u8 SAD matcher's LDS word-group array in both layouts, bit for bit against the CPU oracle.

The matcher keeps the word groups of a byte phase entry-major ([entry][row][EW], rows padded to an odd count) wherever that array fits
the LDS budget, and row-major ([row][entry][EW]) for searches too wide for the pad; VWGPU_OPT_SAD_LAYOUT = 1 pins the row-major array.
Every kernel size, wave-group flavour, byte-phase shape (search widths around the multiples of 4 that change the step list), several
search rows, the validity sweep (constant image, flat band) and partial tiles run in both.

Which tile, how many wave groups and which layout the launcher took is read back through VWGPU_OPT_SAD_LAST_LAUNCH and asserted, so
that a change of the launcher's cost constants cannot move a case off the kernel it names.

The widths of the 7x7 wide-search cases follow from lds_bytes() of bm_sad_u8.hip for the 1024-column tile of 16 rows (NR = 22 input
rows, EW = 2 dwords per entry, NW = 2): with ne = 256 + ((sx + 2) >> 2) + 1 entries per row the workgroup needs
    (rows * ne * 2  +  22 * (ne + 3)) * 4 bytes <= 80 KiB           (entry array + RIGHT base tile; the LEFT tile borrows the former)
  row-major,   rows = 22:  66 * ne + 66 <= 20480  ->  ne <= 309  ->  (sx + 2) >> 2 <= 52  ->  sx <= 209   (what the kernel serves at all)
  entry-major, rows = 23:  68 * ne + 66 <= 20480  ->  ne <= 300  ->  (sx + 2) >> 2 <= 43  ->  sx <= 173   (widest padded search, one group)
  entry-major, two groups (+ 64 bytes of item counters):  68 * ne + 66 <= 20464  ->  ne <= 299  ->  (sx + 2) >> 2 <= 42  ->  sx <= 169
so with one group 173 is the widest search of the padded layout, 174 the first that falls back to the row-major array and 209 the widest
packed search; with two groups the boundary is 169 / 170; 210 goes to the float64 kernel.  The 8-row and the 512-column tiles are smaller
and never leave the padded layout.  The launcher's cost model (pick_launch, 256 CUs) takes the 1024 x 16 tile
  with one group pinned on 4096 x 2064 output pixels: 4 x 129 = 516 tiles, 3 on the busiest CU, 22 * 0.5 * 3 + 4.5 * 2 = 42 against
      14 * 0.5 * 5 + 4.5 * 2 = 44 for the 1032 tiles of 8 rows;
  with two groups pinned on 4096 x 1040: 260 tiles, 22 * 0.55 * 2 + 4.5 * 2 = 33.2 against 14 * 0.55 * 3 + 4.5 * 3 = 36.6 for 520 tiles of 8 rows.
Both are asserted, not assumed."""
import numpy as np
import pytest

import visionworkbench_amd as vwa
from visionworkbench_amd import core, synth

pytestmark = pytest.mark.gpu

ABS = 0
SIZES = [(3, 3), (5, 5), (7, 7), (7, 5), (9, 9), (11, 11)]                    # kLaunch of bm_sad_u8.hip
WIDTHS = list(range(1, 13)) + list(range(31, 35)) + list(range(127, 133))
LAYOUTS = [0, 1]                                                             # OPT_SAD_LAYOUT: launcher's choice, row-major


def _groups(kernel):
    """OPT_SAD_GROUPS values with a kernel of their own for this size (the split flavours exist for 7x7 only)."""
    return [0, 1, 2, 3] if kernel == (7, 7) else [1]


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
    ctx.set_option(core.OPT_SAD_LAYOUT, 0)


def _launch(ctx):
    """(tile rows, tile columns, wave groups, entry-major) of the context's last packed-u8 SAD launch."""
    v = ctx.get_option(core.OPT_SAD_LAST_LAUNCH)
    return (v & 0xff, ((v >> 8) & 0xf) * 256, (v >> 12) & 0xf, bool((v >> 16) & 1))


def _run(ctx, lt, rt, left, kernel, search, groups, layout):
    import torch
    from visionworkbench_amd import stereo
    ctx.set_option(core.OPT_SAD_GROUPS, groups)
    ctx.set_option(core.OPT_SAD_LAYOUT, layout)
    out = stereo.calc_disparity(ABS, lt, rt, vwa.bounding_box(left), search, kernel, ctx=ctx)
    torch.cuda.synchronize()
    ctx.synchronize()
    return out.cpu().numpy(), ctx.last_path()


def _check_all(ctx, oracle, left, right, kernel, search, groups=None, layouts=LAYOUTS, tile=None, em_limit=None):
    """tile: the (rows, columns, groups) the launcher must have taken; em_limit: the widest search of the padded layout on that tile (None:
    every search of the case fits, so the launcher's own choice is entry-major).  The pinned layout must always be row-major."""
    import torch
    want = oracle.calc_disparity(ABS, left, right, kernel, search)
    lt, rt = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    for g in (_groups(kernel) if groups is None else groups):
        for lay in layouts:
            got, path = _run(ctx, lt, rt, left, kernel, search, g, lay)
            assert path == core.PATH_SAD_U8, "%s search %s groups %d layout %d: path %d" % (kernel, search, g, lay, path)
            assert np.array_equal(got, want), "%s search %s groups %d layout %d differs from the oracle" % (kernel, search, g, lay)
            took = _launch(ctx)
            assert took[3] == (lay == 0 and (em_limit is None or search[0] <= em_limit)), "%s search %s groups %d layout %d: launch %s" % (kernel, search, g, lay, took)
            if tile is not None:
                assert took[:3] == tile, "%s search %s groups %d: the launcher took %s, the case is about %s" % (kernel, search, g, took, tile)
    return want


def test_layout_option_round_trip(ctx):
    assert ctx.get_option(core.OPT_SAD_LAYOUT) == 0
    with pytest.raises(Exception):
        ctx.set_option(core.OPT_SAD_LAST_LAUNCH, 0)          # read only
    ctx.set_option(core.OPT_SAD_LAYOUT, 1)
    assert ctx.get_option(core.OPT_SAD_LAYOUT) == 1
    with pytest.raises(Exception):
        ctx.set_option(core.OPT_SAD_LAYOUT, 2)


@pytest.mark.parametrize("kernel", SIZES)
@pytest.mark.parametrize("sx", WIDTHS)
def test_every_phase_shape(ctx, oracle, kernel, sx):
    """Two tile columns and two tile rows with partial tiles on both sides (1060 x 30 output pixels or so), one search row."""
    left, right, _ = synth.stereo_pair(1060 + kernel[0] - 1, 30 + kernel[1] - 1, sx, 1, block=32, seeds=(31, 32, 33))
    _check_all(ctx, oracle, left, right, kernel, (sx, 1))


@pytest.mark.parametrize("kernel", SIZES)
@pytest.mark.parametrize("sx", [1, 6, 33, 130])
def test_three_search_rows(ctx, oracle, kernel, sx):
    left, right, _ = synth.stereo_pair(600, 41, sx, 3, block=32, seeds=(41, 42, 43))
    _check_all(ctx, oracle, left, right, kernel, (sx, 3))


@pytest.mark.parametrize("kernel", SIZES)
@pytest.mark.parametrize("sx", [1, 7, 33, 130])
@pytest.mark.parametrize("sy", [1, 3])
def test_constant_image_validity_sweep(ctx, oracle, kernel, sx, sy):
    """Every cost equal everywhere: every workgroup runs the validity sweep through the same array and invalidates every pixel."""
    left = np.full((40, 700), 77.0, np.float32)
    right = np.full((40 + sy - 1, 700 + sx - 1), 77.0, np.float32)
    want = _check_all(ctx, oracle, left, right, kernel, (sx, sy))
    if sx * sy > 1:
        assert (want[..., 2] == 0).all()


@pytest.mark.parametrize("kernel", SIZES)
@pytest.mark.parametrize("sx", [7, 33, 130])
def test_flat_band_validity_sweep(ctx, oracle, kernel, sx):
    """A constant band of rows in a textured pair: invalid pixels inside the band only, in tiles that also hold valid ones."""
    left, right, _ = synth.stereo_pair(1100, 60, sx, 1, block=32, seeds=(51, 52, 53))
    left[14:44, :] = 100.0
    right[14:44, :] = 100.0
    want = _check_all(ctx, oracle, left, right, kernel, (sx, 1))
    assert (want[..., 2] == 0).any() and (want[..., 2] != 0).any()


@pytest.mark.parametrize("kernel", SIZES)
@pytest.mark.parametrize("sx", [3, 34, 129])
def test_image_narrower_than_one_tile(ctx, oracle, kernel, sx):
    left, right, _ = synth.stereo_pair(70, 25, sx, 1, block=16, seeds=(61, 62, 63))
    _check_all(ctx, oracle, left, right, kernel, (sx, 1))


@pytest.mark.parametrize("sx", [173, 174, 209])
def test_7x7_widest_searches_full_tile_one_group(ctx, oracle, sx):
    """bm_sad_u8_kernel<7,7,16,1,0,EM>, the flavour of a full-size image: the widest search of the padded layout, the first of the
    row-major fallback and the widest the kernel serves (module docstring), each in the launcher's layout and with row-major pinned."""
    left, right, _ = synth.stereo_pair(4096 + 6, 2064 + 6, sx, 1)
    _check_all(ctx, oracle, left, right, (7, 7), (sx, 1), groups=[1], tile=(16, 1024, 1), em_limit=173)


@pytest.mark.parametrize("sx", [169, 170, 173, 174, 209])
def test_7x7_widest_searches_full_tile_two_groups(ctx, oracle, sx):
    """The same tile with two wave groups: its item counters move the boundary of the padded layout to 169 / 170."""
    left, right, _ = synth.stereo_pair(4096 + 6, 1040 + 6, sx, 1)
    _check_all(ctx, oracle, left, right, (7, 7), (sx, 1), groups=[2], tile=(16, 1024, 2), em_limit=169)


@pytest.mark.parametrize("sx", [173, 174, 209])
def test_7x7_widest_searches_small_image(ctx, oracle, sx):
    """The same widths on the small tiles (8 rows, 512 columns) and the flat case, in both layouts."""
    left, right, _ = synth.stereo_pair(1100, 40, sx, 1, block=32, seeds=(71, 72, 73))
    left[20:, :] = 9.0
    right[20:, :] = 9.0
    _check_all(ctx, oracle, left, right, (7, 7), (sx, 1))


def test_7x7_search_210_leaves_the_packed_path(ctx, oracle):
    import torch
    left, right, _ = synth.stereo_pair(300, 30, 210, 1, block=32, seeds=(81, 82, 83))
    want = oracle.calc_disparity(ABS, left, right, (7, 7), (210, 1))
    got, path = _run(ctx, torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), left, (7, 7), (210, 1), 0, 0)
    assert path != core.PATH_SAD_U8
    assert np.array_equal(got, want)
