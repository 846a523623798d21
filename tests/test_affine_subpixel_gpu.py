"""GPU: stereo.affine_subpixel (libvwgpu.so, affine_subpixel.hip) bit-identical to the sequential CPU restatement of
PyramidSubpixelView(SUBPIXEL_FAST_AFFINE) in tests/refimpl, on all three channels."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import affine_ref  # noqa: E402

from visionworkbench_amd import stereo  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(d, left, right, mode, kernel, levels, block=None, width=1.5):
    want, _ = affine_ref.pyramid_subpixel(d, left, right, mode, width, kernel, levels, block_size=block)
    got = stereo.affine_subpixel(d, left, right, mode, width, kernel, levels, block_size=block)
    diff = np.any(got != want, axis=2)
    assert not diff.any(), "%d pixels differ, first at %s: got %s want %s" % (
        diff.sum(), np.argwhere(diff)[0], got[tuple(np.argwhere(diff)[0])], want[tuple(np.argwhere(diff)[0])])
    return got


@pytest.mark.parametrize("kernel", [(7, 7), (15, 15), (15, 9)])
@pytest.mark.parametrize("levels", [0, 1, 2, 3])
def test_kernels_and_levels(kernel, levels):
    left, right, d, _ = affine_ref.stretched_scene(90, 70)
    _check(d, left, right, 0, kernel, levels)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("block", [None, (64, 64), (100, 37)])
def test_prefilters_and_tiles(mode, block):
    left, right, d, _ = affine_ref.stretched_scene(160, 110)
    _check(d, left, right, mode, (7, 7), 2, block)


def test_large_kernel():
    left, right, d, _ = affine_ref.stretched_scene(96, 96)
    _check(d, left, right, 2, (35, 35), 2)


@pytest.mark.parametrize("dr", [(12, 5), (-10, -6)])
def test_right_image_larger_and_smaller(dr):
    left, _, d, _ = affine_ref.stretched_scene(100, 80)
    _, right, _, _ = affine_ref.stretched_scene(100 + dr[0], 80 + dr[1])
    _check(d, left, right, 1, (9, 9), 2, (64, 64))


def test_fractional_2d_disparities_and_invalid_values():
    left, right, d, _ = affine_ref.stretched_scene(100, 80)
    rng = np.random.RandomState(1)
    d[..., 0] += rng.uniform(-0.7, 0.7, size=d.shape[:2]).astype(np.float32)
    d[..., 1] = rng.uniform(-1.4, 1.4, size=d.shape[:2]).astype(np.float32)
    bad = rng.uniform(size=d.shape[:2]) < 0.1
    d[bad, 2] = 0
    d[bad, 0] = rng.uniform(-9, 9, size=bad.sum())
    _check(d, left, right, 0, (9, 7), 2, (100, 37))


def test_invalidation_cascade_fixpoint():
    left, right, d, _ = affine_ref.cascade_scene(96, 80)
    for kernel in [(7, 7), (15, 15)]:
        _check(d, left, right, 0, kernel, 2)
    st = []
    stereo.affine_subpixel(d, left, right, 0, 1.5, (7, 7), 0, stats=st)
    assert st[1] > 1, "the cascade scene should need more than one fixpoint round (stats %s)" % st
    print("fixpoint rounds (sum, max), iterations:", st)


def test_host_entry_equals_device_entry():
    import torch
    left, right, d, _ = affine_ref.stretched_scene(120, 90)
    host = stereo.affine_subpixel(d, left, right, 2, 1.5, (11, 11), 2, block_size=(64, 64))
    dev = stereo.affine_subpixel(torch.from_numpy(d).cuda(), torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(),
                                 2, 1.5, (11, 11), 2, block_size=(64, 64))
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), host)


def test_top_left_weight_quirk_on_gpu():
    """Hand-derived, independent of the restatement: the reference weights every window pixel with w(0, 0), so where the
    top-left window pixel is invalid the output equals the input bit for bit (max_pyramid_levels = 0)."""
    left, right, d, (ys, xs) = affine_ref.top_left_hole_scene()
    got = stereo.affine_subpixel(d, left, right, 0, 1.5, (7, 7), 0)
    assert np.array_equal(got[ys, xs], d[ys, xs])
    assert np.count_nonzero(got[ys, xs + 1, 0] != d[ys, xs + 1, 0]) >= len(ys) // 2


@pytest.mark.parametrize("block", [(64, 64), (100, 37)])
def test_cpp_view_through_block_write_image(tmp_path, block):
    """vwlite: block_write_image(affine_subpixel(...)) equals the Python call with the same block_size."""
    import subprocess
    exe = affine_ref.build_view_program()
    left, right, d, _ = affine_ref.cascade_scene(150, 90)
    paths = [str(tmp_path / n) for n in ("d.pfm", "l.pfm", "r.pfm", "out.pfm")]
    for p, img in zip(paths, (d, left, right)):
        affine_ref.write_pfm(p, img)
    r = subprocess.run([exe] + paths + ["2", "1.5", "9", "7", "2", str(block[0]), str(block[1])], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    want = stereo.affine_subpixel(d, left, right, 2, 1.5, (9, 7), 2, block_size=block)
    assert np.array_equal(affine_ref.read_pfm(paths[3]), want)


def test_4096_at_35x35_on_sampled_tiles():
    """One 4096^2 run at 35 x 35 in 1024^2 blocks; two of its tiles (a corner and an interior one) against the restatement."""
    import threading
    left, right, d, _ = affine_ref.stretched_scene(4096, 4096)
    lt = stereo.subpixel_tiles(4096, 4096, (1024, 1024))
    got = stereo.affine_subpixel(d, left, right, 2, 1.4, (35, 35), 2, block_size=(1024, 1024))
    sample = [lt[0], lt[6]]
    want = [None] * len(sample)

    def run(i):
        want[i] = affine_ref.pyramid_subpixel(d, left, right, 2, 1.4, (35, 35), 2, tiles=[sample[i]])[0]

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(sample))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for (x, y, w, h), wnt in zip(sample, want):
        assert np.array_equal(got[y:y + h, x:x + w], wnt[y:y + h, x:x + w]), "tile (%d, %d) differs" % (x, y)
