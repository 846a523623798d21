"""GPU: stereo.corr_eval (libvwgpu.so, ce_box_kernel / ce_eval_kernel in corr_eval.hip) bit-identical to the CPU
restatement tests/refimpl/corr_eval_ref.cc, values and validity; host and device entries; the C++ view; the limits and
argument errors; two sampled 1024^2 tiles of a 4096^2 run."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import corr_eval_ref  # noqa: E402
import pyr_ref  # noqa: E402

from visionworkbench_amd import core, stereo  # noqa: E402

pytestmark = pytest.mark.gpu
METRICS = ["ncc", "stddev", "parabola_curvature", "cramer_rao"]


def _check(left, right, d, kernel, metric, rate=1, rnd=False, width=0.0, lv=None, rv=None, block=None):
    want, wst = corr_eval_ref.corr_eval(left, right, d, kernel, metric, rate, rnd, 0, width, lv, rv, block_size=block)
    st = []
    got = stereo.corr_eval(left, right, d, kernel, metric, rate, rnd, 0, width, lv, rv, block_size=block, stats=st)
    diff = np.argwhere(~((got == want).all(axis=2)))
    assert len(diff) == 0, "%d pixels differ, first at %s: got %s want %s" % (
        len(diff), diff[0], got[tuple(diff[0])], want[tuple(diff[0])])
    assert st == wst, (st, wst)
    return got, st


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kernel", [(1, 1), (3, 3), (7, 7), (15, 9)])
def test_metrics_and_kernels(metric, kernel):
    left, right, d, lv, rv = corr_eval_ref.scene(90, 70, masks=True)
    _check(left, right, d, kernel, metric, lv=lv, rv=rv, block=(64, 64))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("kernel", [(35, 35), (63, 63), (63, 41)])
def test_large_kernels_and_the_maximum(metric, kernel):
    left, right, d, lv, rv = corr_eval_ref.scene(60, 48, masks=True, seed=8)
    _check(left, right, d, kernel, metric, rate=2 if kernel[0] == 63 else 1, lv=lv, rv=rv)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("rnd", [False, True])
@pytest.mark.parametrize("rate", [1, 2, 3])
def test_rounding_and_sample_rates(metric, rnd, rate):
    left, right, d, lv, rv = corr_eval_ref.scene(100, 64, masks=True, seed=rate)
    _check(left, right, d, (7, 5), metric, rate, rnd, 1.4, lv, rv, block=(100, 37))


@pytest.mark.parametrize("block", [None, (64, 64), (100, 37), (100, 1), (37, 1)])
def test_tilings(block):
    left, right, d, lv, rv = corr_eval_ref.scene(130, 90, masks=True, seed=11)
    d[40:50, :, 1] = 0.0              # one-row tiles with dy = 0 there: degenerate right boxes
    d[40:50, :, 2] = 1
    for metric in ("ncc", "parabola_curvature"):
        _, st = _check(left, right, d, (7, 7), metric, 1, False, 0.0, lv, rv, block)
    _check(left, right, d, (5, 5), "ncc", 2, True, 0.0, lv, rv, block)


@pytest.mark.parametrize("width", [0.0, 1.4, 7.0])
def test_prefilter_widths(width):
    left, right, d, lv, rv = corr_eval_ref.scene(80, 60, masks=True, seed=12)
    for metric in METRICS:
        _check(left, right, d, (9, 7), metric, 1, False, width, lv, rv, (40, 40))


def test_disparities_negative_tiny_large_and_outside():
    left, right, d, lv, rv = corr_eval_ref.scene(96, 72, masks=True, seed=13)
    rng = np.random.RandomState(2)
    d[:20, :, 0] = -7.5 + rng.uniform(-0.5, 0.5, (20, 96))
    d[20:30, :, 0] = 1e-20                 # tiny |dx|: an integer right coordinate only relative to right_box.min
    d[20:30, :, 1] = -1e-20
    d[30:40, :, 0] = 130.25                 # off the right image to the right
    d[40:50, :, 0] = -150.75                # and to the left
    d[50:60, :, 1] = 2.5 + rng.uniform(-2, 2, (10, 96))
    for metric in METRICS:
        for rnd in (False, True):
            _check(left, right, d, (7, 7), metric, 1, rnd, 1.4, lv, rv, (32, 24))


@pytest.mark.parametrize("size", [(120, 100), (70, 50)])
def test_right_image_larger_and_smaller(size):
    left, _, d, lv, _ = corr_eval_ref.scene(96, 72, masks=True, seed=14)
    _, right, _, _, rv = corr_eval_ref.scene(96, 72, size[0], size[1], masks=True, seed=14)
    for metric in METRICS:
        _check(left, right, d, (9, 9), metric, 1, False, 0.0, lv, rv, (48, 48))


def test_unstaged_left_reads():
    """Blocks whose left windows exceed the 64 KB staging budget read the left image through L1 (ce_eval_kernel<M, false>):
    63 x 63 at rate 5 (138^2 floats) and 7 x 7 at rate 9 (142^2 floats)."""
    left, right, d, lv, rv = corr_eval_ref.scene(100, 80, masks=True, seed=18)
    for metric in METRICS:
        _check(left, right, d, (63, 63), metric, 5, False, 0.0, lv, rv)
    left, right, d, lv, rv = corr_eval_ref.scene(160, 150, masks=True, seed=19)
    for metric in METRICS:
        _check(left, right, d, (7, 7), metric, 9, True, 1.4, lv, rv)


@pytest.mark.parametrize("rate", [2 ** 27, 10 ** 8, 2 ** 31 - 1])
def test_huge_sample_rates(rate):
    """One sampled pixel per tile: the staged extent is bounded by the tile, not by (CE_TX - 1) * rate."""
    left, right, d, lv, rv = corr_eval_ref.scene(90, 70, masks=True, seed=20)
    d[::64, ::64, 2] = 1
    for metric in ("ncc", "stddev"):
        _, st = _check(left, right, d, (9, 9), metric, rate, False, 0.0, lv, rv, (64, 64))
        assert st[0] == 4


def test_coordinates_near_a_million():
    """One-row tiles whose first pixel points 1e6 columns to the left: the other pixels' crop-relative coordinates are
    about 1e6, where float(i) has an ulp of 1/16, so the weights float(i) - float(floor(i)) are coarse and a coordinate a
    hair above an integer (dx = k + 2^-20) takes the bilinear path with a zero weight instead of the integer shortcut."""
    left, right, d, lv, rv = corr_eval_ref.scene(64, 8, masks=True, seed=22)
    d[..., 2] = 1
    d[:, :, 1] = np.float32(0.37) + np.arange(64, dtype=np.float32) * np.float32(0.001)
    d[:, 1:, 0] = np.float32(-3.3) + np.sin(np.arange(63) / 5.0).astype(np.float32)
    d[:, 10:20, 0] = np.float32(-3.0 + 2.0 ** -20)
    d[:, 20:30, 0] = np.float32(-3.0 + 0.99999)
    d[:, 0, 0] = np.float32(-1.0e6 - 0.37)
    for metric in METRICS:
        for rnd in (False, True):
            _, st = _check(left, right, d, (3, 3), metric, 1, rnd, -5.0, lv, rv, (64, 1))
            assert st[3] == (8 if rnd else 0)     # rounded, dy = 0 on every one-row tile: empty right boxes


def test_masks_and_disparity_must_live_on_the_device():
    """A mask (or the disparity) handed to the device path as a CPU tensor or a numpy array is refused before any launch."""
    import torch
    left, right, d, lv, rv = corr_eval_ref.scene(40, 30, masks=True, seed=23)
    lt, rt, dt = (torch.from_numpy(a).cuda() for a in (left, right, d))
    for kw in ({"left_valid": torch.from_numpy(lv)}, {"right_valid": torch.from_numpy(rv)}, {"left_valid": lv},
               {"right_valid": torch.from_numpy(rv).cuda(), "left_valid": torch.from_numpy(lv)}):
        with pytest.raises(core.ArgumentErr):
            stereo.corr_eval(lt, rt, dt, (5, 5), "stddev", **kw)
    with pytest.raises(core.ArgumentErr):
        stereo.corr_eval(lt, rt, torch.from_numpy(d), (5, 5), "stddev")
    got = stereo.corr_eval(lt, rt, dt, (5, 5), "stddev", left_valid=torch.from_numpy(lv).cuda(),
                           right_valid=torch.from_numpy(rv).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), stereo.corr_eval(left, right, d, (5, 5), "stddev", left_valid=lv, right_valid=rv))


def test_host_entry_equals_device_entry():
    import torch
    left, right, d, lv, rv = corr_eval_ref.scene(120, 90, masks=True, seed=15)
    for metric in METRICS:
        host = stereo.corr_eval(left, right, d, (11, 11), metric, 2, False, 0, 1.4, lv, rv, block_size=(64, 64))
        t = [torch.from_numpy(a).cuda() for a in (left, right, d, lv, rv)]
        dev = stereo.corr_eval(t[0], t[1], t[2], (11, 11), metric, 2, False, 0, 1.4, t[3], t[4], block_size=(64, 64))
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), host)


def test_limits_and_argument_errors():
    left, right, d, _, _ = corr_eval_ref.scene(60, 50, seed=16)
    with pytest.raises(core.NoImplErr):
        stereo.corr_eval(left, right, d, (65, 3), "ncc")
    ctx = core.default_context(0)
    tiles = stereo.subpixel_tiles(60, 50)
    out = np.zeros((50, 60, 2), np.float32)

    def call(kx=3, ky=3, metric=0, rate=1, width=0.0, disp=d):
        return ctx._lib.vwgpu_corr_eval(ctx._h, disp.ctypes.data, 60, 50, 0, left.ctypes.data, None, 0, right.ctypes.data, None,
                                        60, 50, 0, kx, ky, metric, rate, 0, 0, width, tiles.ctypes.data, 1, out.ctypes.data,
                                        0, None)
    assert call(kx=65) == -2 and call(ky=65) == -2     # VWGPU_ERR_NOIMPL
    for kw in ({"kx": 4}, {"metric": 4}, {"rate": 0}, {"width": -6.5}, {"width": float("nan")}):
        assert call(**kw) not in (0, -2), kw
    bad = d.copy()
    bad[10, 12] = (np.nan, 0.0, 1.0)
    assert call(disp=bad) not in (0, -2)
    with pytest.raises(core.ArgumentErr):
        stereo.corr_eval(left, right, bad, (3, 3), "ncc")
    stereo.corr_eval(left, right, bad, (3, 3), "ncc", sample_rate=5)    # column 12 is not sampled at rate 5
    bad[10, 12, 2] = 0
    stereo.corr_eval(left, right, bad, (3, 3), "ncc")                   # invalid: never read
    huge = d.copy()
    huge[5, 5] = (3.0e9, 0.0, 1.0)
    assert call(disp=huge) not in (0, -2)


def test_cpp_view_through_block_write_image(tmp_path):
    """vwlite: block_write_image(corr_eval(...)) equals the Python call with the same block size."""
    exe = corr_eval_ref.build_view_program()
    left, right, d, lv, rv = corr_eval_ref.scene(90, 70, masks=True, seed=17)
    paths = [str(tmp_path / n) for n in ("l.pfm", "r.pfm", "d.pfm", "out.pfm")]
    pyr_ref.write_pfm(paths[0], np.dstack([left, lv.astype(np.float32), np.zeros_like(left)]))
    pyr_ref.write_pfm(paths[1], np.dstack([right, rv.astype(np.float32), np.zeros_like(right)]))
    pyr_ref.write_pfm(paths[2], d)
    for metric, rate, rnd, block in (("ncc", 1, 0, (32, 32)), ("cramer_rao", 2, 1, (45, 29)), ("stddev", 3, 0, (90, 1))):
        r = subprocess.run([exe] + paths + ["7", "5", metric, str(rate), str(rnd), "1.4", str(block[0]), str(block[1])],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        want = stereo.corr_eval(left, right, d, (7, 5), metric, rate, bool(rnd), 0, 1.4, lv, rv, block_size=block)
        assert np.array_equal(pyr_ref.read_pfm(paths[3])[..., :2], want)
    r = subprocess.run([exe] + paths + ["65", "5", "ncc", "1", "0", "0", "32", "32"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, r.stdout + r.stderr


def test_4096_at_15x15_parabola_on_sampled_tiles():
    """One 4096^2 run at 15 x 15 with parabola_curvature in 1024^2 blocks; two of its tiles (a corner and an interior
    one) against the restatement."""
    left, right, d, _, _ = corr_eval_ref.scene(4096, 4096, seed=21)
    lt = stereo.subpixel_tiles(4096, 4096, (1024, 1024))
    got = stereo.corr_eval(left, right, d, (15, 15), "parabola_curvature", block_size=(1024, 1024))
    sample = [lt[0], lt[6]]
    want = [None] * len(sample)

    def run(i):
        want[i] = corr_eval_ref.corr_eval(left, right, d, (15, 15), "parabola_curvature", tiles=[sample[i]], threads=8)[0]

    threads = [threading.Thread(target=run, args=(i,)) for i in range(len(sample))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for (x, y, w, h), wnt in zip(sample, want):
        assert np.array_equal(got[y:y + h, x:x + w], wnt[y:y + h, x:x + w]), "tile (%d, %d) differs" % (x, y)
