"""The scenes the interest-point detection tests share (CPU and GPU)."""
import numpy as np

SIZES = ((96, 80), (131, 200), (257, 129))      # (cols, rows) of the three scenes


def scene(w, h, seed=0):
    """0.5 + 0.02 uniform noise + a sum of Gaussian blobs a exp(-r^2 / 2 s^2), clipped to [0, 1], float32 (h, w):
    max(6, w h / 600) blobs, a uniform in +-0.4, s = 1.2 * 1.25^u with u uniform in [0, 8): structure at every OBALoG scale."""
    rng = np.random.RandomState(1000 + seed)
    img = 0.5 + 0.02 * rng.uniform(-1, 1, (h, w))
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(max(6, w * h // 600)):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        a, s = rng.uniform(-0.4, 0.4), 1.2 * 1.25 ** rng.uniform(0, 8)
        img += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.ascontiguousarray(np.clip(img, 0, 1), np.float32)


def scenes():
    return [scene(w, h, k) for k, (w, h) in enumerate(SIZES)]
