"""GPU parity of the pyramid / prefilter family through the C ABI, against the oracle: BIT-EXACT for any float input
(the accumulation order is fixed by the reference and reproduced; no FMA contraction on either side)."""
import os
import sys

import numpy as np
import pytest

import visionworkbench_amd as vwa
from visionworkbench_amd import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "refimpl"))
from filters_direct import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


def _both(fn_gpu, fn_ref, img, *a, **k):
    """Run through the host entry (numpy) and the device entry (torch) and compare both with the oracle: NaN where the oracle has NaN,
    the same bit pattern everywhere else (the sign of a zero and a subnormal count)."""
    import torch
    want = fn_ref(img, *a, **k)
    got_h = fn_gpu(img, *a, **k)
    got_d = fn_gpu(torch.from_numpy(img).cuda(), *a, **k)
    torch.cuda.synchronize()
    assert same_bits(got_h, want) == 0, "host entry: %d mismatching pixels" % same_bits(got_h, want)
    assert same_bits(got_d.cpu().numpy(), want) == 0, "device entry differs"
    return want


def test_gaussian_kernel_matches_oracle(oracle):
    from visionworkbench_amd import filters
    for sigma, size in [(1.0, 5), (1.0, 4), (1.5, 0), (float(np.float32(1.4)), 0), (5.0, 0), (0.3, 0), (0.0, 0)]:
        assert np.array_equal(filters.generate_gaussian_kernel(sigma, size), oracle.generate_gaussian_kernel(sigma, size))
    assert np.array_equal(filters.generate_pyramid_smoothing_kernel(), oracle.pyramid_smoothing_kernel())


@pytest.mark.parametrize("shape", [(37, 53), (64, 64), (1, 9), (130, 257), (5, 3)])
@pytest.mark.parametrize("edge", [0, 1])
def test_separable_convolution_parity(ctx, oracle, shape, edge):
    from visionworkbench_amd import filters
    img = synth.noise_f32(3, shape[0], shape[1], -5.0, 300.0)      # arbitrary floats: still bit-exact
    k5 = oracle.pyramid_smoothing_kernel()
    g = oracle.generate_gaussian_kernel(2.0)
    ka = np.array([0.25, -1.5, 3.0, 0.125], np.float32)            # asymmetric, even length
    for xk, yk, cx, cy, s in [(k5, k5, None, None, 2), (k5, k5, None, None, 1), (g, g, None, None, 1), (ka, g, 1, None, 1),
                              (ka, np.array([], np.float32), 3, None, 1), (np.array([], np.float32), ka, None, 0, 3),
                              (g, ka, None, 2, 2)]:
        _both(lambda im, **kw: filters.separable_convolution_filter(im, xk, yk, cx, cy, edge, s, ctx=ctx),
              lambda im, **kw: oracle.separable_convolution(im, xk, yk, cx, cy, edge, s), img)


def test_reference_golden_cases_on_gpu(ctx, oracle):
    """TestConvolution.cxx:110-180 and TestFilter.cxx:141-150 through the engine (float versions)."""
    from visionworkbench_amd import filters
    src = np.array([[1.0, 2.0], [3.0, 4.0]], np.float32)
    krn = np.array([1.0, -1.0], np.float32)
    d = filters.separable_convolution_filter(src, krn, krn, edge=filters.ZeroEdgeExtension, ctx=ctx)
    assert d[0, 0] == 1 and d[1, 0] == 2 and d[0, 1] == 1 and d[1, 1] == 0
    d = filters.laplacian_filter(src, filters.ZeroEdgeExtension, ctx=ctx)
    assert d[0, 0] == 1 and d[0, 1] == -3 and d[1, 0] == -7 and d[1, 1] == -11
    d = filters.convolution_filter(src, [[2.0, -1.0], [0.0, 3.0]], edge=filters.ZeroEdgeExtension, ctx=ctx)
    assert d[0, 0] == 2 and d[0, 1] == 3 and d[1, 0] == 6 and d[1, 1] == 8


@pytest.mark.parametrize("mode,width", [(0, 0.0), (1, 5.0), (2, 1.4), (1, 1.5), (2, 3.0)])
def test_prefilter_parity(ctx, oracle, mode, width):
    from visionworkbench_amd import filters
    left, _, _ = synth.stereo_pair(150, 90, 9)
    _both(lambda im: filters.prefilter_image(im, mode, width, ctx=ctx), lambda im: oracle.prefilter_image(im, mode, width), left)
    _both(lambda im: filters.prefilter_image(im, mode, width, ctx=ctx), lambda im: oracle.prefilter_image(im, mode, width),
          synth.noise_f32(8, 33, 47, 0.0, 1.0))


def test_mask_decimation_parity(ctx, oracle):
    from visionworkbench_amd import filters
    rng = np.random.RandomState(4)
    for shape in [(5, 7), (64, 64), (33, 130), (1, 1), (2, 3)]:
        m = (rng.rand(*shape) < 0.45).astype(np.uint8) * rng.randint(1, 256, shape).astype(np.uint8)
        _both(lambda im: filters.subsample_mask_by_two(im, ctx=ctx), oracle.subsample_mask_by_two, m)


def test_pyramid_chain_parity(ctx, oracle):
    """5 pyramid levels (BASELINE config 5 uses max_pyramid_levels=5): every level bit-exact, device resident."""
    import torch
    from visionworkbench_amd import filters
    left, _, _ = synth.stereo_pair(700, 420, 9)
    ref = [left]
    k = oracle.pyramid_smoothing_kernel()
    for _ in range(5):
        ref.append(oracle.separable_convolution(ref[-1], k, k, subsample=2))
    got = filters.build_gaussian_pyramid(torch.from_numpy(left).cuda(), 5, ctx=ctx)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert tuple(a.shape) == b.shape
        assert np.array_equal(a.cpu().numpy(), b)


def test_filter_argument_errors(ctx):
    from visionworkbench_amd import filters
    img = np.zeros((8, 8), np.float32)
    with pytest.raises(vwa.ArgumentErr):
        filters.separable_convolution_filter(img, [1, 2, 3], [1], cx=5, ctx=ctx)
    with pytest.raises(vwa.NoImplErr):
        filters.separable_convolution_filter(img, np.ones(400, np.float32), [1.0], ctx=ctx)
