"""GPU: the sub-pixel refiners take a tile's search range over its VALID pixels only (affine_range_kernel, affine_subpixel.hip; the
parabola's prepass, subpixel.hip), as get_disparity_range does (Image/Statistics.h:283-290).  The kernels meet the cases of
tests/test_subpixel_range_cpu.py, built by the same tests/subpixel_range_cases.py:

  b. fill invariance: out(zero) == out(inrange) == out(garbage) for the four refiners x 0 / 1 / 2 pyramid levels x three tilings (LoG on
     the whole image at two levels), every call succeeds, invalid output pixels are {0, 0, 0}, and out(zero) equals the restatement;
     once per refiner through the device entry with row strides larger than the widths; the parabola on byte imagery;
  c. an all-invalid block that stores (50, -50), 1 x 1 tiles, a tile whose only valid pixel is its last; a VALID pixel holding +Inf is
     still VWGPU_ERR_ARGUMENT and one holding 3e38 still VWGPU_ERR_NOMEM, with the output untouched.

Every comparison is np.array_equal on all three channels; every scene is 64 x 48 (the parabola's 80 x 48)."""
import numpy as np
import pytest

import subpixel_range_cases as rc
import visionworkbench_amd as vwa

pytestmark = pytest.mark.gpu

OK, ERR_ARGUMENT, ERR_NOMEM = 0, -1, -4
SENTINEL = np.float32(-777.25)
ACCURACY = 20


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


def _entry(ctx, alg, dev):
    name = "vwgpu_phase_subpixel" if alg == rc.PHASE else "vwgpu_pyramid_subpixel"
    return getattr(ctx._lib, name + ("_dev" if dev else "")), (ACCURACY if alg == rc.PHASE else alg)


def _host(ctx, alg, d, left, right, mode, width, levels, tiles, out=None):
    """The host entry over the {x, y, w, h} tiles: (status, out).  `out` given: written in place (pixels outside the tiles stay)."""
    d, left, right = (np.ascontiguousarray(a, np.float32) for a in (d, left, right))
    h, w = left.shape
    t = np.ascontiguousarray(tiles, np.int32).reshape(-1, 4)
    out = np.zeros_like(d) if out is None else out
    fn, sel = _entry(ctx, alg, False)
    status = fn(ctx._h, d.ctypes.data, w, h, 0, left.ctypes.data, 0, right.ctypes.data, right.shape[1], right.shape[0], 0, mode, width,
                rc.KERNEL[0], rc.KERNEL[1], levels, sel, t.ctypes.data, len(t), out.ctypes.data, 0, None)
    return status, out


def _dev(ctx, alg, d, left, right, mode, width, levels, tiles, pad=(5, 3, 7, 9)):
    """The device entry with every image a crop of a wider buffer (row strides w + pad, in pixels): (status, out crop, out padding)."""
    import torch
    h, w = left.shape

    def wide(a, p):
        buf = torch.full((a.shape[0], a.shape[1] + p) + a.shape[2:], float(SENTINEL), dtype=torch.float32, device="cuda")
        buf[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
        return buf

    bd, bl, br = wide(d, pad[0]), wide(left, pad[1]), wide(right, pad[2])
    bo = torch.full((h, w + pad[3], 3), float(SENTINEL), dtype=torch.float32, device="cuda")
    bo[:, :w] = 0
    t = np.ascontiguousarray(tiles, np.int32).reshape(-1, 4)
    fn, sel = _entry(ctx, alg, True)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    status = fn(ctx._h, bd.data_ptr(), w, h, w + pad[0], bl.data_ptr(), w + pad[1], br.data_ptr(), right.shape[1], right.shape[0],
                right.shape[1] + pad[2], mode, width, rc.KERNEL[0], rc.KERNEL[1], levels, sel, t.ctypes.data, len(t), bo.data_ptr(),
                w + pad[3], None)
    torch.cuda.synchronize()
    o = bo.cpu().numpy()
    return status, o[:, :w].copy(), o[:, w:].copy()


def _same(got, want, what):
    diff = (got != want).any(-1)
    assert np.array_equal(got, want), "%s: %d pixels differ (%d in validity), first at (y, x) = %s: %s / %s, largest |delta| %g px" % (
        what, diff.sum(), (got[..., 2] != want[..., 2]).sum(), tuple(np.argwhere(diff)[0]), got[tuple(np.argwhere(diff)[0])],
        want[tuple(np.argwhere(diff)[0])], np.nanmax(np.abs(got[..., :2] - want[..., :2])))


# ---- b. fill invariance -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cid", rc.matrix_ids())
def test_kernel_does_not_depend_on_what_invalid_pixels_store(ctx, cid):
    alg, left, right, d, levels, block, (mode, width), tiles = rc.refiner_scene(cid)
    mask = rc.hole_mask()
    out = {}
    for v in rc.VARIANTS:
        status, out[v] = _host(ctx, alg, rc.variant(d, tiles, v, mask), left, right, mode, width, levels, tiles)
        assert status == OK, "%s: status %d, %s" % (v, status, ctx._lib.vwgpu_last_error(ctx._h).decode())
        assert not np.isnan(out[v]).any()
        assert (out[v][out[v][..., 2] == 0] == 0).all(), "an invalid output pixel is {0, 0, 0}"
        if v != "zero":
            _same(out[v], out["zero"], v + " / zero")
    _same(out["zero"], rc.restatement(alg, rc.variant(d, tiles, "zero", mask), left, right, mode, width, levels, tiles),
          "zero / restatement")


@pytest.mark.parametrize("refiner", list(rc.REFINERS))
def test_device_entry_with_row_strides(ctx, refiner):
    alg, left, right, d, levels, block, (mode, width), tiles = rc.refiner_scene(refiner + "-plus5-2-40x20-none")
    mask = rc.hole_mask()
    want = rc.restatement(alg, rc.variant(d, tiles, "zero", mask), left, right, mode, width, levels, tiles)
    for v in ("zero", "garbage"):
        status, got, padding = _dev(ctx, alg, rc.variant(d, tiles, v, mask), left, right, mode, width, levels, tiles)
        assert status == OK, "%s: status %d, %s" % (v, status, ctx._lib.vwgpu_last_error(ctx._h).decode())
        _same(got, want, v + " / restatement")
        assert (padding == SENTINEL).all()


def test_parabola_does_not_depend_on_what_invalid_pixels_store(ctx, oracle):
    import torch
    from visionworkbench_amd import stereo
    left, right, d, mask, tiles = rc.parabola_scene()
    want = oracle.parabola_subpixel(rc.variant(d, tiles, "zero", mask), left, right, 0, 0.0, rc.KERNEL)
    assert (want[mask] == 0).all() and (want[~mask, 2] == 1).all()
    for v in rc.VARIANTS:
        dv = rc.variant(d, tiles, v, mask)
        _same(stereo.parabola_subpixel(dv, left, right, 0, 0.0, rc.KERNEL, ctx=ctx), want, v + " (host) / oracle(zero)")
        got = stereo.parabola_subpixel(torch.from_numpy(dv).cuda(), torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(),
                                       0, 0.0, rc.KERNEL, ctx=ctx)
        torch.cuda.synchronize()
        _same(got.cpu().numpy(), want, v + " (device) / oracle(zero)")


def test_parabola_without_a_valid_pixel_is_zeros(ctx):
    from visionworkbench_amd import stereo
    left, right, d, mask, tiles = rc.parabola_scene()
    d[..., 0], d[..., 1], d[..., 2] = rc.GARBAGE[np.arange(80) % 8], 3e38, 0
    assert (stereo.parabola_subpixel(d, left, right, 0, 0.0, rc.KERNEL, ctx=ctx) == 0).all()


# ---- c. edges of the rule ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("levels", [0, 2])
@pytest.mark.parametrize("refiner", list(rc.REFINERS))
def test_an_all_invalid_block_with_a_far_value_is_zeros_and_moves_no_other_block(ctx, refiner, levels):
    """As the CPU test of this name: zeros without a pyramid; with one, the reference fills pixels along the block's edges from its valid
    neighbours, and the whole output must equal the run in which the block stores zeros."""
    alg, left, right, d, _, block, (mode, width), tiles = rc.refiner_scene("%s-plus5-%d-32x24-none" % (refiner, levels))
    mask = rc.hole_mask()
    a, b = rc.variant(d, tiles, "zero", mask), rc.variant(d, tiles, "zero", mask)
    a[24:48, 32:64] = 0
    b[24:48, 32:64] = (50, -50, 0)
    sa, oa = _host(ctx, alg, a, left, right, mode, width, levels, tiles)
    sb, ob = _host(ctx, alg, b, left, right, mode, width, levels, tiles)
    assert (sa, sb) == (OK, OK), ctx._lib.vwgpu_last_error(ctx._h).decode()
    if levels == 0:
        assert (ob[24:48, 32:64] == 0).all()
    assert (ob[24 + 8:48, 32 + 8:64] == 0).all()
    _same(ob, oa, "(50, -50) / zeros")
    _same(ob, rc.restatement(alg, b, left, right, mode, width, levels, tiles), "kernel / restatement")


@pytest.mark.parametrize("levels", [0, 2])
@pytest.mark.parametrize("refiner", list(rc.REFINERS))
def test_one_pixel_tiles_and_a_tile_whose_only_valid_pixel_is_its_last(ctx, refiner, levels):
    alg, left, right, d, _, _, (mode, width), _ = rc.refiner_scene(refiner + "-plus5-2-whole-none")
    d[10, 20] = (-300, 200, 0)                            # the invalid 1 x 1 tile; (30, 12) is the valid one
    tiles = [(30, 12, 1, 1), (20, 10, 1, 1)]
    status, out = _host(ctx, alg, d, left, right, mode, width, levels, tiles, out=np.full_like(d, SENTINEL))
    assert status == OK, ctx._lib.vwgpu_last_error(ctx._h).decode()
    want = rc.restatement(alg, d, left, right, mode, width, levels, tiles)
    assert np.array_equal(out[12, 30], want[12, 30]) and np.array_equal(out[10, 20], want[10, 20])
    if levels == 0:
        assert (out[10, 20] == 0).all()
    out[12, 30] = out[10, 20] = SENTINEL
    assert (out == SENTINEL).all()                        # nothing outside the two tiles is written
    last = d.copy()
    last[24:48, 32:64] = (-77, 3e38, 0)
    last[47, 63] = d[47, 63]
    status, got = _host(ctx, alg, last, left, right, mode, width, levels, [(32, 24, 32, 24)])
    assert status == OK, ctx._lib.vwgpu_last_error(ctx._h).decode()
    _same(got, rc.restatement(alg, last, left, right, mode, width, levels, [(32, 24, 32, 24)]), "kernel / restatement")


@pytest.mark.parametrize("value,want", [(np.inf, ERR_ARGUMENT), (-np.inf, ERR_ARGUMENT), (3e38, ERR_NOMEM), (-3e38, ERR_NOMEM)])
@pytest.mark.parametrize("refiner", list(rc.REFINERS))
def test_a_valid_pixel_out_of_bounds_is_still_an_error_and_leaves_the_output_untouched(ctx, refiner, value, want):
    """The bad pixel lies in the LAST tile: no earlier tile may have been written when the call fails (host and device entry)."""
    alg, left, right, d, levels, block, (mode, width), tiles = rc.refiner_scene(refiner + "-plus5-2-32x24-none")
    d = rc.variant(d, tiles, "garbage")
    for ch in (0, 1):
        bad = d.copy()
        assert bad[40, 50, 2] == 1
        bad[40, 50, ch] = value
        status, out = _host(ctx, alg, bad, left, right, mode, width, levels, tiles, out=np.full_like(d, SENTINEL))
        assert status == want, (status, ctx._lib.vwgpu_last_error(ctx._h).decode())
        assert (out == SENTINEL).all()
        status, got, padding = _dev(ctx, alg, bad, left, right, mode, width, levels, tiles)
        assert status == want
        assert (got == 0).all() and (padding == SENTINEL).all()          # the crop was zero-filled by _dev, never written
