"""CPU: the restatement of phase_subpixel (tests/refimpl/phase_ref.cc) against independent mathematics — fftshift and
pad_fourier_transform derived by hand and against numpy.fft, phase_correlation_subpixel against a float64 numpy.fft
version of the same algorithm, a texture with a known shift — and the argument checks of stereo.phase_subpixel that need
no GPU."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import phase_ref  # noqa: E402

from visionworkbench_amd import core, stereo  # noqa: E402


@pytest.mark.parametrize("shape", [(3, 5), (4, 6), (5, 4), (1, 7), (8, 8), (7, 7)])
def test_fftshift_matches_numpy(shape):
    a = np.arange(np.prod(shape), dtype=np.float32).reshape(shape)
    assert np.array_equal(phase_ref.fftshift(a), np.fft.fftshift(a))
    assert np.array_equal(phase_ref.fftshift(a, reverse=True), np.fft.ifftshift(a))
    c = np.stack([a, -a], axis=2)
    assert np.array_equal(phase_ref.fftshift(c), np.stack([np.fft.fftshift(a), -np.fft.fftshift(a)], axis=2))


def test_fftshift_by_hand():
    """Odd size 5: the zero frequency moves to index 2, negative frequencies first; reverse undoes it."""
    a = np.array([[0, 1, 2, 3, 4]], np.float32)
    assert phase_ref.fftshift(a).tolist() == [[3, 4, 0, 1, 2]]
    assert phase_ref.fftshift(a, reverse=True).tolist() == [[2, 3, 4, 0, 1]]
    b = np.array([[0, 1, 2, 3]], np.float32)
    assert phase_ref.fftshift(b).tolist() == [[2, 3, 0, 1]] == phase_ref.fftshift(b, reverse=True).tolist()


def _pad_by_hand(x, nh, nw):
    """Zero-padding of a spectrum by frequency: index k of an n-long axis holds the signed frequency
    f(k) = ((k + n // 2) mod n) - n // 2 (an even size's Nyquist term counts as negative), which keeps its signed index
    f(k) mod N in the N-long result; every value is scaled by (nw nh) / (w h) in float."""
    h, w = x.shape
    out = np.zeros((nh, nw), np.complex64)
    scale = np.float32(nw * nh) / np.float32(w * h)
    for i in range(h):
        for j in range(w):
            fi, fj = (i + h // 2) % h - h // 2, (j + w // 2) % w - w // 2
            out[fi % nh, fj % nw] = np.complex64(x[i, j].real * scale + 1j * (x[i, j].imag * scale))
    return out


@pytest.mark.parametrize("shape,new", [((3, 5), (6, 10)), ((5, 5), (10, 10)), ((4, 6), (8, 12)), ((7, 3), (9, 8)),
                                       ((4, 4), (4, 4))])
def test_pad_fourier_transform(shape, new):
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    got = phase_ref.pad_fourier_transform(x, new[1], new[0])
    assert np.array_equal(got, _pad_by_hand(x, *new) if new != shape else x)


def test_pad_of_an_odd_spectrum_is_the_zero_padded_signal():
    """For odd sizes the padded spectrum of a real signal stays Hermitian, and its inverse samples the band-limited signal
    at half-pixel steps: every other sample is the signal itself."""
    rng = np.random.default_rng(1)
    a = rng.standard_normal((5, 7))
    p = phase_ref.pad_fourier_transform(np.fft.fft2(a).astype(np.complex64), 14, 10)
    up = np.fft.ifft2(p.astype(np.complex128))
    assert np.abs(up.imag).max() < 1e-4
    assert np.allclose(up.real[::2, ::2], a, atol=1e-4)


def _cvtt(x):
    """static_cast<int>(double) as x86 computes it: truncation, INT_MIN for NaN and out-of-range values."""
    x = np.asarray(x, np.float64)
    ok = (x >= -2.0 ** 31) & (x < 2.0 ** 31)
    return np.where(ok, np.trunc(np.where(ok, x, 0)), -2 ** 31).astype(np.int64)


def _np_percentile_u8(a):
    """percentile_scale_convert(a, 0.02, 0.98, 256) written from ImageThresh.h:244-268 with numpy: min / max skipping NaN,
    a 256-bin histogram over [min, max] (max = min + 1 when equal; bin round(255 (v - min) / range), saturated; NaN in
    bin 0), the first bins whose cumulative share reaches 2 % and 98 %, low / high = (bin + 1) width + min, clamp,
    normalize to 0..255 through float32 bounds and a double ratio, truncation to uint8 (NaN -> 0)."""
    a = np.asarray(a, np.float32).ravel()
    v = a.astype(np.float64)
    fin = v[~np.isnan(v)]
    mn = fin.min() if fin.size else np.finfo(np.float64).max
    mx = fin.max() if fin.size else -np.finfo(np.float64).max
    hmax = mn + 1.0 if mx == mn else mx
    rng = hmax - mn
    with np.errstate(invalid="ignore"):
        bins = np.clip(_cvtt(np.round(255 * ((v - mn) / rng))), 0, 255)
    counts = np.bincount(bins, minlength=256).astype(np.float64)
    run = np.cumsum(counts / a.size)          # sequential float64 sums, as get_percentile adds them
    lo_bin, hi_bin = int(np.argmax(run >= 0.02)), int(np.argmax(run >= 0.98))
    width = rng / 256
    lo, hi = np.float32((lo_bin + 1) * width + mn), np.float32((hi_bin + 1) * width + mn)
    ratio = 0.0 if hi == lo else 255.0 / np.float64(np.float32(hi - lo))
    c = np.where(a > hi, hi, np.where(a < lo, lo, a)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        norm = ((c - lo).astype(np.float32).astype(np.float64) * ratio).astype(np.float32)
    return (_cvtt(norm) & 0xFF).astype(np.float32)


@pytest.mark.parametrize("case", ["uniform", "lognormal", "constant", "two_values", "nan", "negative", "int8bit"])
def test_percentile_u8_against_numpy(case):
    rng = np.random.default_rng(11)
    for n in (49, 63, 225, 1225, 1681):
        a = {"uniform": lambda: rng.random(n), "lognormal": lambda: rng.lognormal(0, 2, n),
             "constant": lambda: np.full(n, 0.37), "two_values": lambda: np.where(rng.random(n) < 0.5, -1.0, 3.0),
             "nan": lambda: np.where(rng.random(n) < 0.05, np.nan, rng.standard_normal(n)),
             "negative": lambda: -1e3 * rng.random(n), "int8bit": lambda: rng.integers(0, 256, n).astype(float)}[case]()
        a = a.astype(np.float32)
        got = phase_ref.percentile_u8(a)
        assert np.array_equal(got, _np_percentile_u8(a)), (case, n)
        assert got.min() >= 0 and got.max() <= 255 and np.array_equal(got, np.trunc(got))


def test_percentile_u8_by_hand():
    """0..99: min 0, max 99, bin width 99 / 256; 2 % of the values lie in the bins up to 1 (values 0, 1), 98 % in the
    bins up to 252 (values up to 97), so low = 2 * 99/256 and high = 253 * 99/256; 0 maps to 0, 99 to 255."""
    a = np.arange(100, dtype=np.float32)
    got = phase_ref.percentile_u8(a)
    lo, hi = np.float32(2 * 99 / 256), np.float32(253 * 99 / 256)
    assert got[0] == 0 and got[-1] == 255
    k = 50
    assert got[k] == int(np.float32((np.float32(k - lo)) * (255.0 / np.float64(np.float32(hi - lo)))))


def _np_phase(l, r, pad):
    """phase_correlation_subpixel in float64 with numpy.fft, after get_dft's 8-bit conversion; returns (offset, relative
    gap of the top two magnitudes)."""
    l, r = _np_percentile_u8(l).reshape(l.shape), _np_percentile_u8(r).reshape(r.shape)
    l, r = l.astype(np.float64), r.astype(np.float64)
    R, C = l.shape
    X = np.fft.fft2(l) * np.conj(np.fft.fft2(r))
    P = np.zeros((2 * R, 2 * C), complex)
    P[np.ix_([u if u <= R // 2 else u + R for u in range(R)], [v if v <= C // 2 else v + C for v in range(C)])] = 4 * X
    conv = np.real(np.fft.ifft2(P))
    ly, lx = divmod(int(np.argmax(conv)), 2 * C)
    sx, sy = (lx if lx < C else lx - 2 * C) / 2.0, (ly if ly < R else ly - 2 * R) / 2.0
    if pad <= 2:
        return np.array([sx, sy]), np.inf
    sx, sy = round(sx * pad) / pad, round(sy * pad) / pad
    up = math.ceil(1.5 * pad)
    ds = up // 2
    roff, coff = int(ds - sy * pad), int(ds - sx * pad)
    fr = np.array([u if u <= R // 2 else u - R for u in range(R)])
    fc = np.array([v if v <= C // 2 else v - C for v in range(C)])
    rk = np.exp(-2j * np.pi * np.outer(np.arange(up) - roff, fr) / (R * pad))
    ck = np.exp(-2j * np.pi * np.outer(fc, np.arange(up) - coff) / (C * pad))
    mag = np.abs(rk @ np.conj(X) @ ck)
    m = np.sort(mag.ravel())
    y2, x2 = divmod(int(np.argmax(mag)), up)
    return np.array([sx + (x2 - ds) / pad, sy + (y2 - ds) / pad]), (m[-1] - m[-2]) / m[-1]


def test_phase_correlation_against_numpy_fft():
    """Random patch pairs (shifted crops with noise, and unrelated patches), windows 7x7 .. 15x15, pad factors 1 .. 64:
    at least 99 % identical to float64 numpy; every other offset one grid step (1 / pad) away, where numpy's two highest
    peaks nearly tie."""
    rng = np.random.default_rng(5)
    n = same = 0
    for t in range(800):
        R, C = [(7, 7), (9, 7), (15, 15), (11, 13)][t % 4]
        pad = [20, 10, 7, 4, 64, 2, 1][t % 7]
        base = rng.random((R + 8, C + 8))
        if t % 3 == 2:
            l, r = rng.random((R, C)), rng.random((R, C))
        else:
            dx, dy = rng.integers(-2, 3, 2)
            l = base[4:4 + R, 4:4 + C]
            r = base[4 + dy:4 + dy + R, 4 + dx:4 + dx + C] + 0.05 * rng.standard_normal((R, C))
        l, r = l.astype(np.float32), r.astype(np.float32)
        got = phase_ref.phase_correlation(l, r, pad)
        want, gap = _np_phase(l, r, pad)
        n += 1
        if np.allclose(got, want, atol=1e-6):
            same += 1
        else:
            assert np.allclose(np.abs(got - want).max(), 1.0 / pad, atol=1e-6) and gap < 1e-3, (R, C, pad, got, want, gap)
    assert same >= 0.99 * n, "%d of %d identical" % (same, n)


def test_phase_correlation_hand_cases():
    """Whole-pixel circular shifts are found exactly (the offset is minus the shift), for every pad factor."""
    rng = np.random.default_rng(2)
    a = rng.random((9, 11)).astype(np.float32)
    for sx, sy in [(1, 0), (-2, 1), (0, -3), (0, 0)]:
        b = np.roll(np.roll(a, sy, 0), sx, 1)
        for pad in (1, 2, 4, 20, 64):
            assert phase_ref.phase_correlation(a, b, pad).tolist() == [-sx, -sy]


def test_known_subpixel_shift_of_a_smooth_texture():
    """A band-limited texture moved by (-1.7, 0.6) with a fractional, negative seed disparity (-1.2, 0.3), LoG, 21 x 21:
    the refinement more than halves the error at the interior pixels.  The bar comes from the restatement: the reference
    correlates the raw (not phase-normalised) cross spectrum of non-periodic windows, which pulls the peak toward the
    window's own offset, and it subtracts the offset found at the truncated window from the fractional seed, so it does
    not reach the true shift exactly."""
    true, seed = (-1.7, 0.6), (-1.2, 0.3)
    left, right, d = phase_ref.shifted_texture(120, 120, true, seed_disparity=seed)
    out, st = phase_ref.phase_subpixel(d, left, right, 2, 1.4, (21, 21), 0, 20, threads=4)
    inner = (slice(20, -20), slice(20, -20))
    v = out[inner][..., 2] > 0
    assert v.mean() > 0.99
    err = np.hypot(out[inner][..., 0] - true[0], out[inner][..., 1] - true[1])[v]
    err0 = math.hypot(seed[0] - true[0], seed[1] - true[1])
    assert np.median(err) <= 0.25 and np.median(err) < 0.5 * err0, (np.median(err), err0)
    assert st == [120 * 120, 0, 1], st          # the tile's patch holds every window: every pixel is refined, none dropped


def test_three_pixel_rule_and_nan_in_the_restatement():
    rng = np.random.default_rng(3)
    left = rng.random((40, 40)).astype(np.float32)
    right = rng.random((40, 40)).astype(np.float32)
    d = np.zeros((40, 40, 3), np.float32)
    d[..., 2] = 1
    out, st = phase_ref.phase_subpixel(d, left, right, 0, 1.4, (9, 9), 0, 20, threads=2)
    assert st[1] > 0 and np.count_nonzero(out[..., 2] == 0) >= st[1]
    left[10, 10] = np.nan
    out2, _ = phase_ref.phase_subpixel(d, left, right, 0, 1.4, (9, 9), 0, 20, threads=2)
    assert not np.isnan(out2).any()          # a NaN patch never wins a maximum: the offset stays finite


# ---- argument checks that need no GPU --------------------------------------------------------------------------------

def test_arguments_without_gpu():
    d = np.zeros((30, 30, 3), np.float32)
    img = np.zeros((30, 30), np.float32)
    with pytest.raises(core.ArgumentErr):
        stereo.phase_subpixel(d, img, img, 0, 1.4, (8, 7))
    with pytest.raises(core.ArgumentErr):
        stereo.phase_subpixel(d, img[:20], img, 0, 1.4, (7, 7))
    for kernel, acc in [((43, 7), 20), ((7, 43), 20), ((7, 7), 65)]:
        with pytest.raises(core.NoImplErr):
            stereo.phase_subpixel(d, img, img, 0, 1.4, kernel, 0, acc)
    assert stereo.PHASE_MAX_KERNEL == 41 and stereo.PHASE_MAX_ACCURACY == 64
    with pytest.raises(core.NoImplErr):                  # the generic surface still reports PHASE as not implemented
        stereo.pyramid_subpixel(d, img, img, 0, 1.4, (7, 7), 0, stereo.SUBPIXEL_PHASE)


def test_header_states_the_limits():
    h = open(os.path.join(ROOT, "include", "vwgpu.h")).read()
    assert "vwgpu_phase_subpixel_dev" in h and "kx, ky <= 41 and phase_subpixel_accuracy <= 64" in h
