"""GPU parity of parabola_subpixel through the C ABI — every comparison is np.array_equal on all three channels.

  * ORDER-FREE scenes (tests/scenes.py; integer imagery of every class, ordinary floats, prefiltered or not): against the oracle (the
    literal zone-based restatement of ParabolaSubpixelView::evaluate).  tests/test_subpixel_cpu.py shows on the same scenes that the
    oracle's running sums and per-window sums agree bit for bit, so the kernel has to as well.
  * ROUNDING scenes (one huge or non-finite pixel): against tests/refimpl/parabola_direct.py, the kernel's own specification (same
    sums in the same order); validity and invalid pixels also against the oracle.  The oracle's VALUES are not compared there: its
    running sums carry the rounding residue of the large value, per-window sums do not — the stated limit, not a tolerance.

The matrix reaches every form of parabola_kernel<KX, INT, KY>: widths 3 ... 15 and the run-time loop (17, 21), the float64 / 32-bit
integer / packed-byte sums, ky == kx (compile-time height) and ky != kx (run-time height); the profiler's scope names tell which
class the engine took.  Stride shapes go through the C entries directly (the Python wrapper always passes contiguous images)."""
import os
import sys

import numpy as np
import pytest

import scenes
import visionworkbench_amd as vwa

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "refimpl"))
import parabola_direct  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


def _run(ctx, disp, left, right, mode, width, kernel, scope=None):
    """Host entry and device entry; with `scope`, the kernel form both took (the names vwgpu_prof_scope records)."""
    import torch
    from visionworkbench_amd import stereo
    if scope is not None:
        ctx.profile_enable(True)
        ctx.profile_reset()
    try:
        got_h = stereo.parabola_subpixel(disp, left, right, mode, width, kernel, ctx=ctx)
        got_d = stereo.parabola_subpixel(torch.from_numpy(disp).cuda(), torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(),
                                         mode, width, kernel, ctx=ctx)
        torch.cuda.synchronize()
        if scope is not None:
            forms = [n for n, _ in ctx.profile_read() if n.startswith("parabola_subpixel")]
            assert forms == [scope, scope], (forms, scope)
    finally:
        if scope is not None:
            ctx.profile_reset()
            ctx.profile_enable(False)
    assert np.array_equal(got_h, got_d.cpu().numpy(), equal_nan=True)
    return got_h


def _run_scene(ctx, c):
    return _run(ctx, c["disp"], c["left"], c["right"], c["mode"], c["width"], c["kernel"], c["scope"])


def _oracle(oracle, c):
    return oracle.parabola_subpixel(c["disp"], c["left"], c["right"], c["mode"], c["width"], c["kernel"])


def _same(got, want):
    bad = (got != want).any(-1)
    assert np.array_equal(got, want), "%d pixels differ, first at (y, x) = %s, largest by %g" % (
        bad.sum(), tuple(np.argwhere(bad)[0]), np.nanmax(np.abs(got - want)))


@pytest.mark.parametrize("mode", [0, 2])
def test_null_test_golden(ctx, oracle, mode):
    """TestSubPixel.cxx:93-124 through the engine (the 0.1 is that test's own bound on the refined value; parity is the array_equal)."""
    left = np.full((5, 5), 0.5, np.float32)
    right = np.full((5, 5), 0.6, np.float32)
    d = np.zeros((5, 5, 3), np.float32)
    d[..., 0] = d[..., 1] = d[..., 2] = 1
    out = _run(ctx, d, left, right, mode, 1.4, (3, 3))
    assert (out[..., 2] == 1.0).all() and np.abs(out[..., :2] - 1.0).max() < 0.1
    _same(out, oracle.parabola_subpixel(d, left, right, mode, 1.4, (3, 3)))


@pytest.mark.parametrize("kernel", [(7, 7), (11, 11), (5, 3)])
@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (1.0, -100.0), (200.0, 0.0), (3000.0, -70000.0)])
def test_integer_imagery_is_bit_exact(ctx, oracle, kernel, scale, offset):
    """Integer imagery: bytes (v_sad_u8 form), negative / 16-bit / 20-bit integers (v_sad_u32 form) — all exact."""
    c = scenes.parabola_scene("legacy:integers-%dx%d-%g-%g" % (kernel + (scale, offset)), oracle)
    got = _run_scene(ctx, c)
    _same(got, _oracle(oracle, c))
    assert (got[5:9, 20:40] == 0).all()


def test_tall_window_on_large_integers_does_not_wrap(ctx, oracle):
    """15 x 69 pixels of 20-bit integers.  This scene's pixels stay below 2^20, so 1035 abs-diffs of below 2^21 still fit 32 bits and the
    integer form keeps the call (asserted through the scope name); the two sides of the wrap rule itself are the scenes wrap:67 (sums just
    below 2^32, integer form) and wrap:69 (handed to the float64 sums) of the matrix."""
    c = scenes.parabola_scene("legacy:tall", oracle)
    _same(_run_scene(ctx, c), _oracle(oracle, c))


@pytest.mark.parametrize("mode,width", [(2, 1.4), (1, 3.0), (0, 0.0)])
def test_prefiltered_and_float_imagery_within_tolerance(ctx, oracle, mode, width):
    """Smooth float texture, each prefilter.  (The name dates from a 1e-5 comparison; the scene is order-free and the comparison exact.)"""
    c = scenes.parabola_scene("legacy:smooth-%d" % mode, oracle)
    assert (c["mode"], c["width"]) == (mode, width)
    _same(_run_scene(ctx, c), _oracle(oracle, c))


def test_disparities_pointing_outside_the_right_image(ctx, oracle):
    """Windows that leave the images use the constant edge extension of the (prefiltered) views."""
    for mode in (0, 2):
        c = scenes.parabola_scene("legacy:outside-%d" % mode, oracle)
        _same(_run_scene(ctx, c), _oracle(oracle, c))


def test_argument_errors(ctx):
    from visionworkbench_amd import stereo
    d = np.zeros((10, 12, 3), np.float32)
    img = np.zeros((10, 12), np.float32)
    with pytest.raises(vwa.ArgumentErr):
        stereo.parabola_subpixel(d, img, img, 0, 0.0, (4, 3), ctx=ctx)
    with pytest.raises(vwa.ArgumentErr):
        stereo.parabola_subpixel(d[:9], img, img, 0, 0.0, (3, 3), ctx=ctx)


# ---- the matrix: widths x heights x classes, class edges, the wrap rule, disparity fields, image shapes --------------------------------

_LEGACY = ["legacy:" + s for s in scenes.parabola_legacy_ids()]


@pytest.mark.parametrize("sid", [s for s in scenes.parabola_order_free_ids() if s not in _LEGACY])
def test_order_free_scene_is_identical_to_oracle(ctx, oracle, sid):
    """A failure names the scene: `matrix:<class>-<kx>x<ky>-<prefilter>`, `edge:<pixel>-<place>-<kernel>`, `wrap:<ky>`,
    `disparity:<field>-<class>`, `shape:<w>x<h>-<kernel>` (tests/scenes.py)."""
    c = scenes.parabola_scene(sid, oracle)
    _same(_run_scene(ctx, c), _oracle(oracle, c))


def test_invalid_pixels_widen_the_rasters_and_change_no_valid_pixel(ctx, oracle):
    """Invalid pixels that store values far outside the valid disparity range (the range is over the valid pixels: they are never read)
    must not change a single valid pixel.  (The name dates from a range taken over all pixels.)"""
    for variant in ("u8", "f01"):
        c = scenes.parabola_scene("disparity:invalid_extreme-" + variant)
        tame = c["disp"].copy()
        tame[tame[..., 2] == 0] = 0
        a = _run_scene(ctx, c)
        b = _run(ctx, tame, c["left"], c["right"], c["mode"], c["width"], c["kernel"], c["scope"])
        _same(a, b)


# ---- rounding scenes: the kernel against its own specification --------------------------------------------------------------------------

@pytest.mark.parametrize("sid", scenes.parabola_rounding_scene_ids())
def test_rounding_scene_is_identical_to_direct_sums(ctx, oracle, sid):
    c = scenes.parabola_scene(sid)
    got = _run_scene(ctx, c)
    assert not np.isnan(got).any()                                   # a NaN offset is rejected by the `< 5` test
    _same(got, parabola_direct.parabola_subpixel(oracle, c["disp"], c["left"], c["right"], c["mode"], c["width"], c["kernel"]))
    want = _oracle(oracle, c)
    invalid = c["disp"][..., 2] == 0
    assert np.array_equal(got[..., 2], want[..., 2]) and np.array_equal(got[invalid], want[invalid])


# ---- strides: every image an interior crop of a larger buffer, through the C entries ---------------------------------------------------

SENTINEL = np.float32(-777.25)
# x offset of the crop in its buffer for disparity, left, right, output; the row strides are multiples of 4 elements or odd
STRIDE_SHAPES = {
    "aligned": dict(off=(4, 8, 12, 4), odd=False),                # strides % 4 == 0 and 16-byte aligned bases: the float4 walks
    "odd": dict(off=(3, 5, 2, 1), odd=True),                      # odd strides: the scalar walks
    "offset1": dict(off=(5, 5, 5, 5), odd=False),                 # aligned strides, bases off by 1, 2, 3 elements
    "offset2": dict(off=(6, 6, 6, 6), odd=False),
    "offset3": dict(off=(7, 7, 7, 7), odd=False),
}


def _embed(a, xoff, odd, fill, rows_before=2, rows_after=3):
    """A copy of image `a` (h, w[, 3]) inside a larger buffer; returns (buffer, row stride in pixels, element offset of the crop)."""
    h, w = a.shape[:2]
    stride = (w + xoff + 9) | 1 if odd else (w + xoff + 12) // 4 * 4
    buf = np.full((h + rows_before + rows_after, stride) + a.shape[2:], fill, np.float32)
    buf[rows_before:rows_before + h, xoff:xoff + w] = a
    return buf, stride, (rows_before * stride + xoff) * (a.shape[2] if a.ndim == 3 else 1)


@pytest.mark.parametrize("shape", list(STRIDE_SHAPES))
@pytest.mark.parametrize("sid", ["matrix:u8-7x7-none", "matrix:u8-13x21-none", "matrix:i16-9x9-none", "matrix:f01-17x19-none",
                                 "matrix:f01-13x13-log", "matrix:f01-7x7-mean"])
def test_strided_crops_equal_the_contiguous_call(ctx, oracle, sid, shape):
    import torch
    c = scenes.parabola_scene(sid)
    s = STRIDE_SHAPES[shape]
    h, w = c["left"].shape
    rh, rw = c["right"].shape
    kx, ky = c["kernel"]
    want = _run_scene(ctx, c)
    _same(want, _oracle(oracle, c))
    # the surroundings of the crops hold values of another class (fractions, huge, negative): a walk that leaves its crop changes the class
    bufs = [_embed(c["disp"], s["off"][0], s["odd"], 1e6), _embed(c["left"], s["off"][1], s["odd"], -0.3),
            _embed(c["right"], s["off"][2], s["odd"], 3e9), _embed(np.zeros_like(c["disp"]), s["off"][3], s["odd"], SENTINEL)]
    lib = ctx._lib

    def outside_untouched(out_buf):
        o = out_buf.copy()
        o[2:2 + h, s["off"][3]:s["off"][3] + w] = SENTINEL
        return (o == SENTINEL).all()

    # host entry
    host = [b.copy() for b, _, _ in bufs]
    ptr = [b.ctypes.data + 4 * off for b, (_, _, off) in zip(host, bufs)]
    ctx.check(lib.vwgpu_parabola_subpixel(ctx._h, ptr[0], w, h, bufs[0][1], ptr[1], bufs[1][1], ptr[2], rw, rh, bufs[2][1],
                                          c["mode"], c["width"], kx, ky, ptr[3], bufs[3][1]))
    _same(host[3][2:2 + h, s["off"][3]:s["off"][3] + w], want)
    assert outside_untouched(host[3])
    # device entry
    dev = [torch.from_numpy(b).cuda() for b, _, _ in bufs]
    ptr = [t.data_ptr() + 4 * off for t, (_, _, off) in zip(dev, bufs)]
    if shape == "aligned":
        assert all(p % 16 == 0 for p in ptr) and all(st % 4 == 0 for _, st, _ in bufs)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.check(lib.vwgpu_parabola_subpixel_dev(ctx._h, ptr[0], w, h, bufs[0][1], ptr[1], bufs[1][1], ptr[2], rw, rh, bufs[2][1],
                                              c["mode"], c["width"], kx, ky, ptr[3], bufs[3][1]))
    torch.cuda.synchronize()
    got = dev[3].cpu().numpy()
    _same(got[2:2 + h, s["off"][3]:s["off"][3] + w], want)
    assert outside_untouched(got)
    for t, (b, _, _) in zip(dev[:3], bufs[:3]):
        assert np.array_equal(t.cpu().numpy(), b)                                     # the inputs are read only
