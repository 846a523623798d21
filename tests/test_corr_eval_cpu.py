"""CPU: the restatement of vw::stereo::corr_eval (tests/refimpl/corr_eval_ref.cc) against an independent pure-Python
version written from CorrEval.cc (float32 bilinear in the reference's operation order, double sums c outer), against
hand-derived cases, and the argument checks of the restatement and of stereo.corr_eval that need no GPU."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import corr_eval_ref  # noqa: E402

from visionworkbench_amd import core, stereo  # noqa: E402

F = np.float32
BIG = 2 ** 31 - 2


def _roundf(v):
    """roundf: half away from zero, exact for float32 inputs."""
    v = float(v)
    return float(F(math.copysign(math.floor(abs(v) + 0.5), v)))


def py_corr_eval(left, right, disp, kernel, metric, rate, rnd, width, lv, rv, tiles):
    """CorrEval::prerasterize per tile, written from CorrEval.cc without the restatement's structure."""
    h, w = left.shape
    rh, rw = right.shape
    kx, ky = kernel
    hx, hy = kx // 2, ky // 2
    pad = int(math.ceil(float(F(width)))) + 5
    curv = metric in ("parabola_curvature", "cramer_rao")
    out = np.zeros((h, w, 2), np.float32)

    def lpix(x, y):
        if 0 <= x < w and 0 <= y < h:
            return float(left[y, x]), (lv is None or lv[y, x] != 0)
        return 0.0, False

    for (tx, ty, tw, th) in tiles:
        dd = {}
        for r in range(0, th, rate):
            for c in range(0, tw, rate):
                d = disp[ty + r, tx + c]
                if d[2] != 0:
                    dx, dy = float(d[0]), float(d[1])
                    if rnd:
                        dx, dy = _roundf(dx), _roundf(dy)
                    dd[(c, r)] = (dx, dy)
        mn, mx = [BIG, BIG], [-BIG, -BIG]
        for (c, r), (dx, dy) in dd.items():
            px, py = float(tx + c) + dx, float(ty + r) + dy
            for a, v in ((0, px), (1, py)):
                mn[a] = min(mn[a], math.floor(v))
                mx[a] = max(mx[a], math.ceil(v))
        for e in [(hx, hy), (1, 1), (2, 2), (pad, pad)] + ([(1, 1)] if curv else []):
            if mn[0] >= mx[0] or mn[1] >= mx[1]:
                break
            mn = [mn[0] - e[0], mn[1] - e[1]]
            mx = [mx[0] + e[0], mx[1] + e[1]]
        cw, ch = max(0, mx[0] - mn[0]), max(0, mx[1] - mn[1])

        def crop(x, y):
            if 0 <= x < cw and 0 <= y < ch and 0 <= x + mn[0] < rw and 0 <= y + mn[1] < rh:
                gx, gy = x + mn[0], y + mn[1]
                return F(right[gy, gx]), (rv is None or rv[gy, gx] != 0)
            return F(0), False

        def sample(i, j):
            if rnd:
                return crop(int(i), int(j))
            x, y = math.floor(i), math.floor(j)
            if x == i and y == j:
                return crop(x, y)
            nx, ny = F(i) - F(x), F(j) - F(y)
            n1x, n1y = F(1) - nx, F(1) - ny
            (a, va), (b, vb), (c, vc), (d, vd) = crop(x, y), crop(x + 1, y), crop(x, y + 1), crop(x + 1, y + 1)
            res = a * n1x
            res = res + b * nx
            res = res * n1y
            row = c * n1x
            row = row + d * nx
            res = res + row * ny
            return res, va and vb and vc and vd

        def patches(c0, r0, dx, dy):
            lp, rp = [], []
            for c in range(kx):
                for r in range(ky):
                    x, y = tx + c0 + c - hx, ty + r0 + r - hy
                    lp.append(lpix(x, y))
                    v, ok = sample((float(x) + dx) - float(mn[0]), (float(y) + dy) - float(mn[1]))
                    rp.append((float(v), ok))
            return lp, rp

        def ncc(lp, rp):
            num = den1 = den2 = 0.0
            for (a, _), (b, _) in zip(lp, rp):
                num += a * b
                den1 += a * a
                den2 += b * b
            return num / math.sqrt(den1 * den2) if den1 > 0 and den2 > 0 else -1.0

        def stddev(p):
            vals = [v for v, ok in p if ok]
            if not vals:
                return -1.0
            mean = 0.0
            for v in vals:
                mean += v
            mean /= len(vals)
            s = 0.0
            for v in vals:
                s += (v - mean) * (v - mean)
            return math.sqrt(s / len(vals))

        for (c, r), (dx, dy) in dd.items():
            lp, rp = patches(c, r, dx, dy)
            val = None
            if metric == "ncc":
                v = ncc(lp, rp)
                val = v if v >= 0 else None
            elif metric == "stddev":
                a, b = stddev(lp), stddev(rp)
                val = (a + b) / 2.0 if a >= 0 and b >= 0 else None
            else:
                C = ncc(lp, rp)
                if C >= 0:
                    nb = []
                    for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                        sdx, sdy = float(F(dx) + F(sx)), float(F(dy) + F(sy))
                        nb.append(ncc(*patches(c, r, sdx, sdy)))
                        if nb[-1] < 0:
                            break
                    if len(nb) == 4 and nb[-1] >= 0:
                        kxc, kyc = 2.0 * C - nb[0] - nb[1], 2.0 * C - nb[2] - nb[3]
                        if kxc > 0 and kyc > 0:
                            val = math.sqrt(1.0 / kxc + 1.0 / kyc)
                            if metric == "cramer_rao":
                                val *= math.sqrt(max(1.0 - C, 0.0))
            if val is not None:
                out[ty + r, tx + c] = (F(val), 1.0)
    return out


def _small(seed, masks, w=13, h=11, rw=15, rh=12):
    left, right, d, lv, rv = corr_eval_ref.scene(w, h, rw, rh, shift=(-1.3, 0.4), seed=seed, masks=masks)
    return left, right, d, lv, rv


CASES = [(m, rnd, rate) for m in ("ncc", "stddev", "parabola_curvature", "cramer_rao") for rnd in (False, True)
         for rate in (1, 2, 3)]


@pytest.mark.parametrize("metric,rnd,rate", CASES)
def test_restatement_matches_independent_version(metric, rnd, rate):
    left, right, d, lv, rv = _small(rate + (7 if rnd else 0), masks=True)
    tiles = [(0, 0, 5, 4), (5, 0, 8, 4), (0, 4, 13, 7)]    # origins that are not multiples of the sample rate
    for kernel, width in (((3, 3), 0.0), ((5, 3), 1.4)):
        want = py_corr_eval(left, right, d, kernel, metric, rate, rnd, width, lv, rv, tiles)
        got, st = corr_eval_ref.corr_eval(left, right, d, kernel, metric, rate, rnd, 0, width, lv, rv, tiles=tiles, threads=3)
        assert np.array_equal(got, want), (kernel, np.argwhere(got != want)[:4])
        assert st[0] > 0 and st[2] == 3


def test_identical_images_at_zero_disparity_give_one():
    left, _, _, _, _ = _small(1, masks=False)
    d = np.zeros(left.shape + (3,), np.float32)
    d[..., 2] = 1
    got, _ = corr_eval_ref.corr_eval(left, left, d, (5, 5), "ncc")
    assert np.all(got[..., 1] == 1) and np.all(got[..., 0] == 1.0)


def test_constant_images_at_integer_disparity_give_zero_stddev():
    c = np.full((10, 12), 7.25, np.float32)
    d = np.zeros((10, 12, 3), np.float32)
    d[..., 0], d[..., 1], d[..., 2] = -2, 1, 1
    got, _ = corr_eval_ref.corr_eval(c, c, d, (3, 5), "stddev")
    # column 0's right patch lies wholly left of the image: no valid sample, so no stddev
    assert np.all(got[:, 1:, 1] == 1) and not got[:, 0, 1].any() and np.all(got[..., 0] == 0.0)


def test_masked_left_pixel_value_still_counts():
    """calc_ncc's validity test always passes: a masked left pixel still adds its stored value a * b, a^2."""
    left = np.arange(1, 26, dtype=np.float32).reshape(5, 5)
    right = np.full((5, 5), 2.0, np.float32)
    d = np.zeros((5, 5, 3), np.float32)
    d[..., 2] = 1
    lv = np.ones((5, 5), np.uint8)
    lv[2, 1] = 0
    # a 3 x 3 tile: its sampled pixels span the right box (a 1 x 1 tile at d = 0 would leave it empty)
    got, _ = corr_eval_ref.corr_eval(left, right, d, (3, 3), "ncc", left_valid=lv, tiles=[(1, 1, 3, 3)])
    a = left[1:4, 1:4].astype(np.float64)
    want_all = (a * 2).sum() / math.sqrt((a * a).sum() * (4.0 * 9))
    b = a.copy()
    b[1, 0] = 0.0
    want_skip = (b * 2).sum() / math.sqrt((b * b).sum() * (4.0 * 8))
    assert got[2, 2, 1] == 1 and got[2, 2, 0] == np.float32(want_all) and np.float32(want_all) != np.float32(want_skip)


def test_one_row_tile_with_zero_dy_is_invalid_but_valid_in_a_taller_tile():
    left, right, d, _, _ = _small(3, masks=False, w=20, h=12, rw=20, rh=12)
    d[..., 1] = 0.0
    d[..., 2] = 1
    one_row, st = corr_eval_ref.corr_eval(left, right, d, (3, 3), "ncc", tiles=[(0, 5, 20, 1)])
    assert not one_row[5, :, 1].any() and st[3] == 1
    tall, st = corr_eval_ref.corr_eval(left, right, d, (3, 3), "ncc", tiles=[(0, 4, 20, 3)])
    assert tall[5, :, 1].sum() >= 12 and st[3] == 0
    rnd, _ = corr_eval_ref.corr_eval(left, right, d, (3, 3), "ncc", round_to_int=True, tiles=[(0, 5, 20, 1)])
    assert not rnd[5, :, 1].any()     # round_to_int on an empty crop: nodata, defined here


def test_one_by_one_kernel_gives_invalid_curvature():
    left, right, d, _, _ = _small(4, masks=False)
    for metric in ("parabola_curvature", "cramer_rao"):
        got, st = corr_eval_ref.corr_eval(left, right, d, (1, 1), metric)
        assert not got[..., 1].any() and st[0] > 0


def test_tile_without_valid_disparity_is_all_invalid():
    left, right, d, _, _ = _small(5, masks=False)
    d[:, :6, 2] = 0
    d[:, :6, 0] = np.nan       # never read: invalid
    got, st = corr_eval_ref.corr_eval(left, right, d, (3, 3), "ncc", tiles=[(0, 0, 6, 11), (6, 0, 7, 11)])
    assert not got[:, :6, 1].any() and got[:, 6:, 1].any()


def test_argument_errors():
    left, right, d, _, _ = _small(6, masks=False)
    for kw in ({"kernel_size": (4, 3)}, {"metric": "sad"}, {"sample_rate": 0}):
        args = dict(kernel_size=(3, 3), metric="ncc", sample_rate=1)
        args.update(kw)
        with pytest.raises(ValueError):
            corr_eval_ref.corr_eval(left, right, d, **args)
    with pytest.raises(ValueError):
        corr_eval_ref.corr_eval(left[:, :-1], right, d, (3, 3), "ncc")
    bad = d.copy()
    bad[4, 6, 2] = 1
    bad[4, 6, 0] = np.nan
    with pytest.raises(ValueError, match="rc 2"):
        corr_eval_ref.corr_eval(left, right, bad, (3, 3), "ncc")
    # the same NaN at an unsampled pixel (rate 2, odd column) or an invalid one is never read
    bad[4, 7], bad[4, 6] = bad[4, 6], d[4, 6]
    corr_eval_ref.corr_eval(left, right, bad, (3, 3), "ncc", sample_rate=2)
    bad[4, 7, 2] = 0
    corr_eval_ref.corr_eval(left, right, bad, (3, 3), "ncc")


def test_python_entry_rejects_arguments_before_the_gpu():
    left, right, d, _, _ = _small(6, masks=False)
    for args in [((4, 3), "ncc"), ((3, 3), "sad")]:
        with pytest.raises(core.ArgumentErr):
            stereo.corr_eval(left, right, d, *args)
    with pytest.raises(core.ArgumentErr):
        stereo.corr_eval(left[:, :-1], right, d, (3, 3), "ncc")
    with pytest.raises(core.NoImplErr):
        stereo.corr_eval(left, right, d, (65, 3), "ncc")


def test_python_entry_refuses_mixed_host_and_device_operands():
    """With a numpy left image every operand goes through the host entry, so a torch mask or disparity is refused."""
    torch = pytest.importorskip("torch")
    left, right, d, lv, rv = _small(6, masks=True)
    for kw in ({"left_valid": torch.from_numpy(lv)}, {"right_valid": torch.from_numpy(rv)}):
        with pytest.raises(core.ArgumentErr):
            stereo.corr_eval(left, right, d, (3, 3), "stddev", **kw)
    with pytest.raises(core.ArgumentErr):
        stereo.corr_eval(left, right, torch.from_numpy(d), (3, 3), "ncc")
