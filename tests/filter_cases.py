"""Cases of tests/test_filters_cpu.py (the oracle against tests/refimpl/filters_direct.py, no GPU) and tests/test_filter_edges_gpu.py
(the kernels against the oracle), from one place so that the two files cannot drift.  Plain generators over seeded RandomStates.

Sizes are written cols x rows.  sepconv_kernel works in 64 x 16 output tiles and conv2d / mask kernels in 64 x 4 blocks, so output
extents sit at 1, 63 / 64 / 65, 129 and 1, 15 / 16 / 17, 33.  The launcher of the separable convolution takes what fits 64 KB of LDS:
    ((15 s + 1 + max(ny - 1, 0)) * ((63 s + 1 + max(nx - 1, 0)) + 64)) * 4 <= 65536,  and at most 160 taps per axis;
FLOOR lists the largest kernels that satisfies for each step.  They must be accepted; anything larger may be refused.
"""
import numpy as np

K5 = np.array([1.0 / 16.0, 4.0 / 16.0, 6.0 / 16.0, 4.0 / 16.0, 1.0 / 16.0], np.float32)     # generate_pyramid_smoothing_kernel
EMPTY = np.zeros(0, np.float32)
K_ZEROS = np.array([0.25, 0.0, 0.5, -0.0, 0.25], np.float32)
K_TINY = np.array([0.25, 1e-30, 0.5, 0.25], np.float32)
OW = (1, 63, 64, 65, 129)
OH = (1, 15, 16, 17, 33)
LENGTHS = (1, 2, 3, 4, 5, 13, 14)
FLOOR = ((1, 67, 67), (1, 160, 0), (1, 0, 113), (2, 39, 39), (3, 15, 15))                  # (step, nx, ny)
BEYOND = ((1, 69, 69), (1, 161, 0), (1, 0, 114), (2, 41, 41), (3, 17, 17), (1, 400, 1))  # refused, or right
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -1e-45, 3e38], np.float32)


def taps(rng, n):
    """n non-symmetric taps of either sign with sum |k| <= 1."""
    if n == 0:
        return EMPTY
    k = rng.uniform(-1.0, 1.0, n)
    return (k / np.abs(k).sum()).astype(np.float32)


def noise(rng, w, h, lo=-5.0, hi=300.0):
    return rng.uniform(lo, hi, (h, w)).astype(np.float32)


def origins(n):
    return sorted({0, (n - 1) // 2, n - 1}) if n else [0]


def _src_extent(rng, out, step):
    """A source extent whose decimated extent 1 + (n - 1) / step is `out`: the smallest or the largest one."""
    return (out - 1) * step + 1 + (step - 1) * int(rng.randint(2))


def _sep(cid, img, xk, yk, cx, cy, edge, step, accept="must"):
    return dict(id=cid, img=img, xk=xk, yk=yk, cx=cx, cy=cy, edge=edge, step=step, accept=accept)


def special_image():
    """40 x 70 noise with every special value at a corner, on an edge, on a tile seam (rows 15 | 16, 31 | 32) and in the interior."""
    rng = np.random.RandomState(77)
    img = noise(rng, 40, 70, -2.0, 2.0)
    spots = {"corner": [(0, 0), (39, 0), (0, 69), (39, 69), (39, 35), (0, 52), (20, 69)],           # (the last three: more edges)
             "edge": [(0, 24), (39, 8), (13, 0), (27, 69), (0, 40), (39, 60), (33, 0)],
             "seam": [(7, 15), (8, 16), (19, 31), (20, 32), (31, 47), (32, 48), (13, 63)],
             "interior": [(10, 6), (22, 10), (30, 22), (12, 26), (25, 38), (6, 44), (18, 56)]}
    for n, kind in enumerate(("corner", "edge", "seam", "interior")):
        for i, (x, y) in enumerate(spots[kind]):
            img[y, x] = SPECIALS[(i + 2 * n) % 7]
    return img


def special_images():
    rng = np.random.RandomState(78)
    yield "special", special_image()
    yield "negzero", np.full((70, 40), -0.0, np.float32)
    yield "subnormal", (rng.uniform(0.0, 1.0, (30, 20)) * 1e-38).astype(np.float32)
    yield "huge", np.where(rng.uniform(size=(33, 40)) < 0.5, -3e38, 3e38).astype(np.float32)


def sepconv_cases():
    # -- seams: every pair at step 2 with the pyramid kernel, corners + (65, 17) for the other steps and a 13 x 14 kernel
    rng = np.random.RandomState(1)
    kx13, ky14 = taps(rng, 13), taps(rng, 14)
    few = [(1, 1), (129, 1), (1, 33), (129, 33), (65, 17)]
    plans = [(2, K5, K5, 2, 2, [(a, b) for a in OW for b in OH]), (1, K5, K5, 2, 2, few), (3, K5, K5, 2, 2, few),
             (1, kx13, ky14, 3, 11, few), (2, kx13, ky14, 0, 6, few), (3, kx13, ky14, 12, 0, few)]
    for step, xk, yk, cx, cy, pairs in plans:
        for ow, oh in pairs:
            w, h = _src_extent(rng, ow, step), _src_extent(rng, oh, step)
            img = noise(rng, w, h)
            for edge in (0, 1):
                yield _sep("seam-s%d-k%dx%d-%dx%d-e%d" % (step, len(xk), len(yk), ow, oh, edge), img, xk, yk, cx, cy, edge, step)
    # -- images smaller than the kernel
    k13 = taps(rng, 13)
    for w, h in ((1, 1), (1, 9), (9, 1), (2, 2)):
        img = noise(rng, w, h)
        for step in (1, 2):
            for edge in (0, 1):
                yield _sep("small-%dx%d-s%d-e%d" % (w, h, step, edge), img, k13, k13[::-1].copy(), 4, 9, edge, step)
    # -- origins and lengths: every length on each axis, the three origins of each axis independently; 67 x 19 crosses both tile seams
    img = noise(rng, 67, 19)
    n = 0
    for i, nx in enumerate(LENGTHS):
        ny = LENGTHS[(i + 3) % len(LENGTHS)]
        xk, yk = taps(rng, nx), taps(rng, ny)
        for cx in origins(nx):
            for cy in origins(ny):
                yield _sep("origin-%dx%d-c%d,%d" % (nx, ny, cx, cy), img, xk, yk, cx, cy, n % 2, 1 + n % 3)
                n += 1
    for nk in (1, 4, 13):
        k = taps(rng, nk)
        for c in origins(nk):
            yield _sep("origin-%dx0-c%d" % (nk, c), img, k, EMPTY, c, 0, n % 2, 1 + n % 3)
            yield _sep("origin-0x%d-c%d" % (nk, c), img, EMPTY, k, 0, c, (n + 1) % 2, 1 + (n + 1) % 3)
            n += 1
    for step in (1, 2, 3):
        yield _sep("origin-0x0-s%d" % step, img, EMPTY, EMPTY, 0, 0, step % 2, step)
    # -- the acceptance floor, and what lies just beyond it
    img = noise(rng, 70, 40)
    for table, accept in ((FLOOR, "must"), (BEYOND, "may")):
        for step, nx, ny in table:
            xk, yk = taps(rng, nx), taps(rng, ny)
            yield _sep("limit-s%d-%dx%d-centre" % (step, nx, ny), img, xk, yk, None, None, 0, step, accept)
            yield _sep("limit-s%d-%dx%d-ends" % (step, nx, ny), img, xk, yk, 0, max(ny - 1, 0), 1, step, accept)
    # -- special values
    for name, img in special_images():
        for kname, k in (("k5", K5), ("k5x2", K5 * 2), ("zeros", K_ZEROS), ("tiny", K_TINY)):      # k5x2: sums of +-3e38 overflow
            for step in (1, 2):
                for edge in (0, 1):
                    yield _sep("%s-%s-s%d-e%d" % (name, kname, step, edge), img, k, k, None, None, edge, step)
        for kname, xk, yk in (("0x0", EMPTY, EMPTY), ("0xk5", EMPTY, K5), ("k5x0", K5, EMPTY), ("0xzeros", EMPTY, K_ZEROS)):
            yield _sep("%s-%s-identity" % (name, kname), img, xk, yk, None, None, 0, 1)


def is_finite_case(c):
    return bool(np.isfinite(c["img"]).all())


CONV2D_SHAPES = ((1, 1), (7, 1), (1, 7), (2, 2), (4, 3), (3, 3), (5, 9), (7, 7))          # (kw, kh)
CONV2D_IMAGES = ((1, 1), (3, 2), (63, 3), (65, 5), (130, 9))


def conv2d_cases():
    """Every kernel shape x five origins x both edges; the ten cases of a shape walk the five images twice."""
    rng = np.random.RandomState(2)
    imgs = [noise(rng, w, h) for w, h in CONV2D_IMAGES]
    for s, (kw, kh) in enumerate(CONV2D_SHAPES):
        k = rng.uniform(-1.0, 1.0, (kh, kw)).astype(np.float32)
        n = 0
        for ci, cj in ((0, 0), (kw - 1, 0), (0, kh - 1), (kw - 1, kh - 1), ((kw - 1) // 2, (kh - 1) // 2)):
            for edge in (0, 1):
                img = imgs[(n + s) % 5]
                yield dict(id="conv-%dx%d-c%d,%d-e%d-%dx%d" % (kw, kh, ci, cj, edge, img.shape[1], img.shape[0]),
                           img=img, k=k, ci=ci, cj=cj, edge=edge)
                n += 1
    sp = special_image()
    for kw, kh in ((3, 3), (4, 3)):
        k = rng.uniform(-1.0, 1.0, (kh, kw)).astype(np.float32)
        k[0, 1], k[1, 0] = 0.0, -0.0
        yield dict(id="conv-%dx%d-special" % (kw, kh), img=sp, k=k, ci=1, cj=1, edge=kw % 2)


def conv2d_too_large():
    rng = np.random.RandomState(3)
    return noise(rng, 20, 12), rng.uniform(-1.0, 1.0, (5, 10)).astype(np.float32)           # 10 x 5 = 50 taps


def mask_cases():
    rng = np.random.RandomState(4)
    values = np.array([0, 1, 128, 255], np.uint8)
    for w in (1, 2, 127, 128, 129, 130):
        for h in (1, 2, 7, 8, 9, 31, 33):
            yield dict(id="mask-%dx%d" % (w, h), mask=values[rng.randint(0, 4, (h, w))])


PREFILTER_WIDTHS = (0.0, 0.3, 1.4, 5.0, 9.6)           # 0, 3 (the minimum), 9, 35 and 67 taps (the largest accepted)
PREFILTER_BEYOND = (9.9, 25.0)                          # 69 and 175 taps: refused, or right


def prefilter_images():
    rng = np.random.RandomState(5)
    for w, h in ((1, 1), (5, 3), (33, 47), (150, 90)):
        yield "%dx%d" % (w, h), noise(rng, w, h, 0.0, 255.0)
    yield "special", special_image()


def prefilter_cases():
    for name, img in prefilter_images():
        yield dict(id="pf-none-%s" % name, img=img, mode=0, width=0.0, accept="must")
        for mode in (1, 2):
            for width in PREFILTER_WIDTHS:
                yield dict(id="pf-m%d-%g-%s" % (mode, width, name), img=img, mode=mode, width=width, accept="must")
    img = noise(np.random.RandomState(6), 33, 47, 0.0, 255.0)
    for mode in (1, 2):
        for width in PREFILTER_BEYOND:
            yield dict(id="pf-m%d-%g-beyond" % (mode, width), img=img, mode=mode, width=width, accept="may")


REGION_WIDTHS = (0.3, 4.0, 9.6)                         # 3, 27 (larger than the image) and 67 taps
REGION_WINDOWS = ((3, 3), (7, 5))
REGION_PUSH = {"left": (-20, 0), "right": (20, 0), "up": (0, -20), "down": (0, 20)}


def region_cases():
    """parabola_subpixel scenes whose RIGHT region leaves the image by 20 pixels on one side: every pixel valid, disparities at the push
    and one pixel nearer.  Ordinary floats in [0, 1], as the float scenes of tests/scenes.py."""
    rng = np.random.RandomState(7)
    for w, h in ((9, 7), (1, 1)):
        left, right = noise(rng, w, h, 0.0, 1.0), noise(rng, w, h, 0.0, 1.0)
        for side, (px, py) in sorted(REGION_PUSH.items()):
            d = np.zeros((h, w, 3), np.float32)
            d[..., 0], d[..., 1], d[..., 2] = px, py, 1
            near = rng.uniform(size=(h, w)) < 0.4
            d[near, 0] -= np.sign(px)
            d[near, 1] -= np.sign(py)
            for mode in (1, 2):
                for width in REGION_WIDTHS:
                    for kernel in REGION_WINDOWS:
                        yield dict(id="region-%dx%d-%s-m%d-%g-%dx%d" % (w, h, side, mode, width, kernel[0], kernel[1]), left=left,
                                   right=right, disp=d, mode=mode, width=width, kernel=kernel)


def region_boxes(c):
    """(image, box {x0, y0, bw, bh}) of the two regions parabola_subpixel prefilters for a case (ParabolaSubpixelView.cc:287-298): the
    left one is the image grown by the half window, the right one is moved by the smallest disparity - 1 and grown by the range + 2."""
    h, w = c["left"].shape
    hx, hy = c["kernel"][0] // 2, c["kernel"][1] // 2
    dx, dy = np.trunc(c["disp"][..., 0]).astype(int), np.trunc(c["disp"][..., 1]).astype(int)
    yield c["left"], (-hx, -hy, w + 2 * hx, h + 2 * hy)
    yield c["right"], (-hx + int(dx.min()) - 1, -hy + int(dy.min()) - 1, w + 2 * hx + int(dx.max() - dx.min()) + 3,
                       h + 2 * hy + int(dy.max() - dy.min()) + 3)
