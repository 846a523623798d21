"""Synthetic scenes of the reference's own stereo tests, rebuilt without boost/vw (test infrastructure only).

  rand48_noise      boost::rand48 gen(10) + uniform_noise_view (src/vw/Image/UtilityViews.h:148-157): the LCG
                    x' = (0x5DEECE66D x + 0xB) mod 2^48 seeded (seed << 16) | 0x330E, output x >> 17 scaled by 2^-31,
                    raster order, multiplied by ChannelRange<T>::max() and truncated for integer channels.
  affine_bicubic    transform(img, AffineTransform(diag(sx, sy), (tx, ty)), ConstantEdgeExtension(),
                    BicubicInterpolation()) — src/vw/Image/Interpolation.h:138-186 (weights, 0.25 scale, exact-integer
                    shortcut, round+clamp for integer channels).
  pyramid_scene     the fixture of src/vw/Stereo/tests/TestPyramidCorrelationView.cxx:47-64.
"""
import numpy as np


def rand48_noise(cols, rows, seed=10):
    a, c, m = 0x5DEECE66D, 0xB, (1 << 48) - 1
    x = ((seed << 16) | 0x330E) & m
    out = np.empty(rows * cols, np.float64)
    for i in range(rows * cols):
        x = (a * x + c) & m
        out[i] = (x >> 17) / 2147483648.0
    return out.reshape(rows, cols)


def affine_bicubic(img, sx, sy, tx, ty, integer_max=None):
    """out(i, j) = bicubic(img, ((i - tx)/sx, (j - ty)/sy)) with constant edge extension; img is (rows, cols)."""
    rows, cols = img.shape
    src = img.astype(np.float64)
    ii = (np.arange(cols, dtype=np.float64) - tx) / sx
    jj = (np.arange(rows, dtype=np.float64) - ty) / sy
    x = np.floor(ii).astype(np.int64)
    y = np.floor(jj).astype(np.int64)
    nx, ny = ii - x, jj - y

    def weights(n):
        return [((2 - n) * n - 1) * n, (3 * n - 5) * n * n + 2, ((4 - 3 * n) * n + 1) * n, (n - 1) * n * n]

    s, t = weights(nx), weights(ny)
    res = np.zeros((rows, cols), np.float64)
    for b in range(4):
        yy = np.clip(y - 1 + b, 0, rows - 1)
        row = np.zeros((rows, cols), np.float64)
        for a_ in range(4):
            xx = np.clip(x - 1 + a_, 0, cols - 1)
            term = s[a_][None, :] * src[yy[:, None], xx[None, :]]
            row = term if a_ == 0 else row + term
        res = t[b][:, None] * row if b == 0 else res + t[b][:, None] * row
    res *= 0.25
    exact = (nx == 0)[None, :] & (ny == 0)[:, None]
    plain = src[np.clip(y, 0, rows - 1)[:, None], np.clip(x, 0, cols - 1)[None, :]]
    res = np.where(exact, plain, res)
    if integer_max is not None:
        res = np.clip(np.rint(res), 0, integer_max)
    return res


def pyramid_scene(channel="u8"):
    """(left, right, scale (sx, sy), translation (tx, ty), search box corners) as float32 images."""
    noise = rand48_noise(300, 200)
    if channel == "u8":
        left = np.floor(255.0 * noise)
        right = affine_bicubic(left, 0.9, 0.95, 15.0, 5.0, integer_max=255)
    elif channel == "i16":
        left = np.floor(32767.0 * noise)
        right = affine_bicubic(left, 0.9, 0.95, 15.0, 5.0, integer_max=32767)
    else:
        left = noise.astype(np.float32).astype(np.float64)
        right = affine_bicubic(left, 0.9, 0.95, 15.0, 5.0)
    # BBox2i(BBox2(-1.5 t, 1.5 t)): the corners are truncated towards zero
    return left.astype(np.float32), right.astype(np.float32), (0.9, 0.95), (15.0, 5.0), (-22, -7, 22, 7)


def pyramid_score(disp, scale, translation):
    """check_error of TestPyramidCorrelationView.cxx:66-84: (correct / valid, valid / all)."""
    rows, cols = disp.shape[:2]
    i = np.arange(cols, dtype=np.float64)[None, :]
    j = np.arange(rows, dtype=np.float64)[:, None]
    ox = np.rint(scale[0] * i + translation[0] - i) + 0 * j
    oy = np.rint(scale[1] * j + translation[1] - j) + 0 * i
    valid = disp[..., 2] != 0
    good = valid & (disp[..., 0] == ox) & (disp[..., 1] == oy)
    return good.sum() / max(valid.sum(), 1), valid.sum() / (rows * cols)


# ---- parabola_subpixel scenes -------------------------------------------------------------------------------------
# Shared by tests/test_subpixel_cpu.py (restatement vs oracle, no GPU) and tests/test_subpixel_gpu.py (kernel vs oracle /
# restatement), so that the two files cannot drift.  A scene is a dict {disp, left, right, mode, width, kernel, scope}:
# `scope` is the profiler scope of the kernel form the engine must choose ("parabola_subpixel_u8": packed bytes, "_int": 32-bit
# integer sums, plain: float64 sums).  ORDER-FREE scenes: no partial sum of the reference's running box sums rounds, so the
# oracle, the direct-sum restatement and the kernel agree bit for bit.  ROUNDING scenes: one huge / non-finite pixel makes the
# reference's running sums carry a residue; the kernel is compared with the restatement there.

PARABOLA_WIDTHS = (3, 5, 7, 9, 11, 13, 15, 17, 21)
PARABOLA_SHORTER = {3: 1, 5: 3, 7: 3, 9: 1, 11: 5, 13: 11, 15: 7, 17: 1, 21: 9}
PARABOLA_TALLER = {3: 7, 5: 9, 7: 9, 9: 15, 11: 13, 13: 21, 15: 17, 17: 19, 21: 23}
PARABOLA_CLASSES = ("u8", "i16", "i20", "f01")
_SCOPE = {0: "parabola_subpixel", 1: "parabola_subpixel_int", 2: "parabola_subpixel_u8"}


def parabola_scope(cls, kernel, mode=0):
    """The kernel form vwgpu_parabola_subpixel_dev chooses for imagery of class `cls` (0 float, 1 integers below 2^21, 2 bytes)."""
    if mode != 0:
        cls = 0
    if cls == 2 and not (3 <= kernel[0] <= 15):
        cls = 1                                                    # bytes, but no byte form of that width
    return _SCOPE[cls]


def _parabola_base(h, w, seed=5):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h + 8, 0:w + 24].astype(np.float64)
    tex = 120 + 50 * np.sin(xx / 3.1) * np.cos(yy / 4.3) + 40 * np.sin((xx + 2 * yy) / 5.7) + 20 * np.cos(xx / 1.9 + yy / 2.3)
    return tex + 8 * rng.rand(*xx.shape), rng


def parabola_disparity(h, w, rng, invalid=0.1):
    """Blocky fractional disparities in [-2, 8] x [-1, 2] (the 0.6 / -0.3 fractions truncate toward zero), `invalid` of them invalid."""
    d = np.zeros((h, w, 3), np.float32)
    bx = rng.randint(-2, 9, ((h + 7) // 8, (w + 7) // 8)).repeat(8, 0).repeat(8, 1)[:h, :w]
    by = rng.randint(-1, 3, ((h + 7) // 8, (w + 7) // 8)).repeat(8, 0).repeat(8, 1)[:h, :w]
    d[..., 0] = bx + 0.6
    d[..., 1] = by - 0.3
    d[..., 2] = rng.rand(h, w) >= invalid
    return d


def parabola_pair(cls, h=48, w=80, seed=5):
    """(left (h, w), right (h + 2, w + 10), rng) of one input class.
      u8   bytes that contain 0 and 255          i16  negative 16-bit integers
      i20  integers with |v| up to 2^21 - 1      f01  ordinary floats in [0, 1]        f12  floats on a 2^-12 grid"""
    base, rng = _parabola_base(h, w, seed)
    lb, rb = base[:h, :w], base[:h + 2, 3:3 + w + 10]
    if cls == "u8":
        l, r = np.clip(np.rint(lb), 0, 255), np.clip(np.rint(rb), 0, 255)
        l[h // 2, w // 3], l[h // 3, w // 2], r[h // 2, w // 2], r[h // 3, w // 3] = 0, 255, 0, 255
    elif cls == "i16":
        l, r = np.rint(lb * 100) - 30000, np.rint(rb * 100) - 30000
    elif cls == "i20":
        l, r = np.rint((lb - 120) * 12000), np.rint((rb - 120) * 12000)
        assert np.abs(l).max() < 2 ** 21 and np.abs(r).max() < 2 ** 21
        l[h // 2, w // 3], r[h // 2, w // 2] = 2 ** 21 - 1, -(2 ** 21 - 1)
    elif cls == "f01":
        l, r = lb / 255, rb / 255
    elif cls == "f12":
        l, r = np.rint(lb * 16) / 4096, np.rint(rb * 16) / 4096
    else:
        raise KeyError(cls)
    return l.astype(np.float32), r.astype(np.float32), rng


_CLS_NUM = {"u8": 2, "i16": 1, "i20": 1, "f01": 0, "f12": 0}


def _scene(disp, left, right, mode, width, kernel, cls):
    return dict(disp=disp, left=left, right=right, mode=mode, width=width, kernel=tuple(kernel),
                scope=None if cls is None else parabola_scope(cls, kernel, mode))


def parabola_matrix_ids():
    """Every width with ky == kx, one shorter and one taller ky, in every class; the two prefilters on floats at two widths."""
    ids = []
    for cls in PARABOLA_CLASSES:
        for kx in PARABOLA_WIDTHS:
            for ky in (kx, PARABOLA_SHORTER[kx], PARABOLA_TALLER[kx]):
                ids.append("%s-%dx%d-none" % (cls, kx, ky))
    for pf in ("mean", "log"):
        for kx, ky in ((7, 7), (13, 13), (13, 21), (17, 9)):
            ids.append("f01-%dx%d-%s" % (kx, ky, pf))
    return ids


_PREFILTER = {"none": (0, 0.0), "mean": (1, 3.0), "log": (2, 1.4)}


def parabola_matrix_scene(sid):
    cls, k, pf = sid.split("-")
    kernel = tuple(int(v) for v in k.split("x"))
    left, right, rng = parabola_pair(cls)
    mode, width = _PREFILTER[pf]
    return _scene(parabola_disparity(48, 80, rng), left, right, mode, width, kernel, _CLS_NUM[cls])


# One pixel that decides the class of an otherwise-byte pair: (value, class the call must take)
PARABOLA_EDGE_VALUES = {"256": (256.0, 1), "m1": (-1.0, 1), "half": (0.5, 0), "denormal": (1e-40, 0), "negzero": (-0.0, 2),
                        "nan": (np.nan, 0), "inf": (np.inf, 0)}
PARABOLA_EDGE_PLACES = ("L", "Lend", "Rend")      # left interior; last row + column of the left / of the right image only
PARABOLA_EDGE_ROUNDING = ("nan", "inf")


def parabola_edge_ids(rounding):
    return ["%s-%s-%dx%d" % (v, p, k, k) for v in PARABOLA_EDGE_VALUES if (v in PARABOLA_EDGE_ROUNDING) == rounding
            for p in PARABOLA_EDGE_PLACES for k in (7, 13)]


def parabola_edge_scene(sid):
    """83 x 47 bytes (widths 83 / 93: both images end in the scalar tail of the class measurement) with one odd pixel."""
    v, place, k = sid.split("-")
    kernel = tuple(int(t) for t in k.split("x"))
    left, right, rng = parabola_pair("u8", 47, 83)
    val, cls = PARABOLA_EDGE_VALUES[v]
    if place == "L":
        left[9, 11] = val
    elif place == "Lend":
        left[-1, -1] = val
    else:
        right[-1, -1] = val
    return _scene(parabola_disparity(47, 83, rng), left, right, 0, 0.0, kernel, cls)


def parabola_wrap_scene(ky):
    """Left +(2^21 - 1) against right -(2^21 - 1) blocks beside 20-bit texture: 15 x 67 windows sum to just below 2^32 (32-bit integer
    sums still hold), 15 x 69 could wrap (float64 sums)."""
    base, rng = _parabola_base(48, 80)
    big = float(2 ** 21 - 1)
    left, right = np.rint(base[:48, :80] * 3000).astype(np.float32), np.rint(base[:50, 3:93] * 3000).astype(np.float32)
    left[:, 20:50] = big
    right[:, 20:60] = -big
    return _scene(parabola_disparity(48, 80, rng), left, right, 0, 0.0, (15, ky), 1 if 15 * ky * 2 ** 22 < 2 ** 32 else 0)


PARABOLA_DISPARITY_KINDS = ("fractions", "one_value", "outside", "invalid_extreme", "all_invalid", "one_valid")


def parabola_disparity_ids():
    return ["%s-%s" % (kind, v) for kind in PARABOLA_DISPARITY_KINDS for v in ("u8", "f01", "log")]


def parabola_disparity_scene(sid):
    kind, variant = sid.split("-")
    cls = "u8" if variant == "u8" else "f01"
    kernel = {"u8": (7, 7), "f01": (9, 5), "log": (5, 5)}[variant]
    mode, width = (2, 1.4) if variant == "log" else (0, 0.0)
    h, w = 48, 80
    left, right, rng = parabola_pair(cls, h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.zeros((h, w, 3), np.float32)
    d[..., 2] = 1
    if kind == "fractions":                                 # -0.3 -> 0, -1.7 -> -1, 2.9 -> 2, -0.999 -> 0
        d[..., 0] = np.array([-0.3, -1.7, 2.9, 0.5, -0.999], np.float32)[(xx // 7 + yy // 5) % 5]
        d[..., 1] = np.array([-1.7, 0.99, -0.3], np.float32)[(xx // 11 + yy // 9) % 3]
        d[..., 2] = rng.rand(h, w) >= 0.1
    elif kind == "one_value":
        d[..., 0], d[..., 1] = 3, 1
    elif kind == "outside":                                 # the right raster leaves the right image on all four sides
        d[..., 0] = np.where(xx < 40, -30, 40)
        d[..., 1] = np.where(yy < 24, -20, 25)
    elif kind == "invalid_extreme":                         # invalid pixels store values far outside the valid range: never read
        d = parabola_disparity(h, w, rng, 0.0)
        d[5, 7] = (40.6, -25.3, 0)
        d[30, 60] = (-33.2, 19.9, 0)
        d[-1, -1] = (41.0, 20.0, 0)
    elif kind == "all_invalid":
        d = parabola_disparity(h, w, rng)
        d[..., 2] = 0
    elif kind == "one_valid":
        d = parabola_disparity(h, w, rng)
        d[..., 2] = 0
        d[5, 5, 2] = 1
    return _scene(d, left, right, mode, width, kernel, _CLS_NUM[cls])


PARABOLA_SHAPES = [(1, 1), (1, 9)] + [(hh, ww) for hh in (3, 4, 5) for ww in (63, 64, 65)]


def parabola_shape_ids():
    return ["%dx%d-%dx%d" % (ww, hh, kx, ky) for hh, ww in PARABOLA_SHAPES for kx, ky in ((5, 5), (9, 1))]


def parabola_shape_scene(sid):
    """Images of one pixel, one row, and around the 64 x 4 workgroup; bytes."""
    s, k = sid.split("-")
    ww, hh = (int(t) for t in s.split("x"))
    kernel = tuple(int(t) for t in k.split("x"))
    left, right, rng = parabola_pair("u8")
    d = np.zeros((hh, ww, 3), np.float32)
    d[..., 0], d[..., 2] = 2, 1
    d[hh // 2, ww // 2, 0] = 3.5
    return _scene(d, left[:hh, :ww].copy(), right[:hh, :ww + 3].copy(), 0, 0.0, kernel, 2)


PARABOLA_ROUNDING_VALUES = {"1e12": 1e12, "m1e12": -1e12, "3e38": 3e38, "nan": np.nan, "inf": np.inf}


def parabola_rounding_ids():
    return ["%s-%s-%dx%d-%s" % (v, p, kx, ky, pf) for v in PARABOLA_ROUNDING_VALUES for p in ("L", "R")
            for kx, ky in ((7, 7), (13, 13), (17, 9)) for pf in ("none", "log")]


def parabola_rounding_scene(sid):
    """The [0, 1] texture with one huge or non-finite pixel at (11, 9) of the left or of the right image."""
    v, place, k, pf = sid.split("-")
    kernel = tuple(int(t) for t in k.split("x"))
    left, right, rng = parabola_pair("f01")
    (left if place == "L" else right)[9, 11] = PARABOLA_ROUNDING_VALUES[v]
    mode, width = _PREFILTER[pf]
    return _scene(parabola_disparity(48, 80, rng), left, right, mode, width, kernel, 0)


def parabola_legacy_ids():
    """The scenes tests/test_subpixel_gpu.py compared before the matrix existed (three of them within 1e-5 then)."""
    return (["integers-%dx%d-%g-%g" % (k + so) for k in ((7, 7), (11, 11), (5, 3))
             for so in ((1.0, 0.0), (1.0, -100.0), (200.0, 0.0), (3000.0, -70000.0))]
            + ["tall"] + ["smooth-%d" % m for m in (2, 1, 0)] + ["outside-%d" % m for m in (0, 2)])


def _disp_from_bm(oracle, left, right, kernel, search):
    """Integer disparity of the block matcher, centred like ParabolaSubpixelView expects (same size as left)."""
    kx, ky = kernel
    hx, hy = kx // 2, ky // 2
    lp = np.pad(left, ((hy, hy), (hx, hx)), mode="edge")
    rp = np.pad(right, ((hy, hy + search[1] - 1), (hx, hx + search[0] - 1)), mode="edge")[:lp.shape[0] + search[1] - 1, :lp.shape[1] + search[0] - 1]
    d = oracle.calc_disparity(0, lp, rp, kernel, search)
    out = np.zeros(left.shape + (3,), np.float32)
    out[..., 0] = d[..., 0]
    out[..., 1] = d[..., 1]
    out[..., 2] = (d[..., 2] != 0)
    return out


def parabola_legacy_scene(sid, oracle):
    from visionworkbench_amd import synth
    p = sid.split("-", 1)
    if p[0] == "integers":
        k, scale, offset = p[1].split("-", 2)
        kernel = tuple(int(t) for t in k.split("x"))
        scale, offset = float(scale), float(offset)
        left, right, _ = synth.stereo_pair(160, 70, 17, 3, block=32, seeds=(41, 42, 43), smooth=True)
        left, right = left * np.float32(scale) + np.float32(offset), right * np.float32(scale) + np.float32(offset)
        right = np.ascontiguousarray(right[:70 + 2, :160 + 16])
        disp = _disp_from_bm(oracle, left, right, kernel, (17, 3))
        disp[5:9, 20:40, 2] = 0                                       # some invalid pixels
        return _scene(disp, left, right, 0, 0.0, kernel, 2 if (scale, offset) == (1.0, 0.0) else 1)
    if sid == "tall":            # 15 x 69 windows of integers up to 1 020 000 < 2^20: 1035 << 21 < 2^32, still the 32-bit sums (wrap:69 has 2^21-sized data)
        left, right, _ = synth.stereo_pair(120, 110, 9, 1, block=32, seeds=(51, 52, 53), smooth=True)
        left, right = left * np.float32(4000.0), right * np.float32(4000.0)
        right = np.ascontiguousarray(right[:110, :120 + 8])
        disp = np.zeros((110, 120, 3), np.float32)
        disp[..., 0], disp[..., 2] = 4.0, 1.0
        return _scene(disp, left, right, 0, 0.0, (15, 69), 1)
    if p[0] == "smooth":
        mode = int(p[1])
        yy, xx = np.mgrid[0:60, 0:110].astype(np.float64)

        def tex(x, y):
            return 120 + 50 * np.sin(x / 3.1) * np.cos(y / 4.3) + 40 * np.sin((x + 2 * y) / 5.7) + 20 * np.cos(x / 1.9 + y / 2.3)
        left, right = tex(xx, yy).astype(np.float32), tex(xx - 3.4, yy - 0.7).astype(np.float32)
        disp = np.zeros((60, 110, 3), np.float32)
        disp[..., 0], disp[..., 1], disp[..., 2] = 3, 1, 1
        disp[:, 60:, 0] = 4                                           # two disparity zones
        return _scene(disp, left, right, mode, {2: 1.4, 1: 3.0, 0: 0.0}[mode], (7, 7), 0)
    mode = int(p[1])                                                   # windows that leave the images: constant edge extension
    left, right, _ = synth.stereo_pair(64, 40, 9, 1, block=16)
    right = np.ascontiguousarray(right[:, :64])                        # right as small as left
    disp = np.zeros((40, 64, 3), np.float32)
    disp[..., 0], disp[..., 1], disp[..., 2] = 6, -2, 1
    disp[10:20, :, 0] = -5
    return _scene(disp, left, right, mode, 1.4 if mode else 0.0, (5, 5), 2)


def parabola_order_free_ids():
    """Every scene on which the GPU tests demand bit-equality with the oracle."""
    return (["matrix:" + s for s in parabola_matrix_ids()] + ["edge:" + s for s in parabola_edge_ids(False)]
            + ["wrap:67", "wrap:69"] + ["disparity:" + s for s in parabola_disparity_ids()]
            + ["shape:" + s for s in parabola_shape_ids()] + ["legacy:" + s for s in parabola_legacy_ids()])


def parabola_rounding_scene_ids():
    return ["rounding:" + s for s in parabola_rounding_ids()] + ["edge:" + s for s in parabola_edge_ids(True)]


def parabola_scene(sid, oracle=None):
    group, s = sid.split(":", 1)
    if group == "legacy":
        return parabola_legacy_scene(s, oracle)
    if group == "wrap":
        return parabola_wrap_scene(int(s))
    return {"matrix": parabola_matrix_scene, "edge": parabola_edge_scene, "disparity": parabola_disparity_scene,
            "shape": parabola_shape_scene, "rounding": parabola_rounding_scene}[group](s)
