"""ctypes binding of the CPU restatement of PyramidSubpixelView(SUBPIXEL_FAST_AFFINE) (affine_ref.cc; test infrastructure)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def build():
    subprocess.check_call(["make", "-s", "-C", HERE])
    return os.path.join(HERE, "libaffine_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        _LIB.afr_pyramid_subpixel.argtypes = [p, i, i, p, p, i, i, i, f, i, i, i, i, p, i, p, i, p]
        _LIB.afr_pyramid_subpixel.restype = i
        _LIB.afr_tile_range.argtypes = [p, i, i, p, p]
        _LIB.afr_tile_range.restype = i
    return _LIB


def tile_range(disparity, tile=None):
    """The search range of one tile {x, y, w, h} (default: the whole map), as the three restatements take it
    (tile_range.h): int32 [min x, min y, max x, max y] over the tile's valid pixels, zeros without any."""
    d = np.ascontiguousarray(disparity, np.float32)
    h, w = d.shape[:2]
    t = np.ascontiguousarray(tile if tile is not None else (0, 0, w, h), np.int32)
    out = np.zeros(4, np.int32)
    if lib().afr_tile_range(d.ctypes.data, w, h, t.ctypes.data, out.ctypes.data):
        raise ValueError("afr_tile_range: bad arguments")
    return out


def tiles_for(w, h, block_size=None):
    """{x, y, w, h} boxes: the whole image, or the blocks aligned to multiples of block_size from (0, 0)."""
    if block_size is None:
        return [(0, 0, w, h)]
    bw, bh = int(block_size[0]), int(block_size[1])
    return [(x, y, min(bw, w - x), min(bh, h - y)) for y in range(0, h, bh) for x in range(0, w, bw)]


def pyramid_subpixel(disparity, left, right, prefilter_mode, prefilter_width, kernel_size, max_pyramid_levels=2,
                     block_size=None, inplace=True, algorithm=1, tiles=None):
    """Returns (out (rows, cols, 3) float32, window-loop iterations).  Pixels outside the tiles are zero."""
    d = np.ascontiguousarray(disparity, np.float32)
    l = np.ascontiguousarray(left, np.float32)
    r = np.ascontiguousarray(right, np.float32)
    h, w = l.shape
    t = np.ascontiguousarray(tiles if tiles is not None else tiles_for(w, h, block_size), np.int32).reshape(-1, 4)
    out = np.zeros((h, w, 3), np.float32)
    it = ctypes.c_longlong(0)
    rc = lib().afr_pyramid_subpixel(d.ctypes.data, w, h, l.ctypes.data, r.ctypes.data, r.shape[1], r.shape[0],
                                    int(prefilter_mode), float(prefilter_width), int(kernel_size[0]), int(kernel_size[1]),
                                    int(max_pyramid_levels), int(algorithm), t.ctypes.data, len(t), out.ctypes.data,
                                    1 if inplace else 0, ctypes.byref(it))
    if rc:
        raise ValueError("afr_pyramid_subpixel: rc %d" % rc)
    return out, it.value


def _texture(x, y, seed=3):
    rng = np.random.RandomState(seed)
    v = np.zeros_like(x)
    for _ in range(12):
        fx, fy, ph = rng.uniform(0.05, 0.35), rng.uniform(0.05, 0.35), rng.uniform(0, 6.3)
        v += np.sin(fx * x + fy * y + ph) * rng.uniform(0.3, 1.0)
    return (v * 20 + 128).astype(np.float32)


def stretched_scene(w, h, stretch=1.03, offset=4.0, seed=3):
    """left(x, y) = T(x, y), right(x', y) = T(stretch * (x' - offset), y): the true disparity of left pixel x is
    x / stretch + offset - x (fractional, known).  Returns left, right, the rounded integer disparity (all valid), truth."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    left = _texture(x, y, seed)
    right = _texture(x * stretch - offset * stretch, y, seed)
    true = x / stretch + offset - x
    d = np.zeros((h, w, 3), np.float32)
    d[..., 0] = np.round(true)
    d[..., 2] = 1
    return left, right, d, true


def cascade_scene(w, h, seed=5):
    """The stretched scene with a flat (constant) patch, a saturated patch and a band of scattered holes whose valid
    share is close to one half: invalidations there change the windows of later pixels."""
    left, right, d, true = stretched_scene(w, h, seed=seed)
    left[h // 4:h // 4 + 12, w // 5:w // 5 + 14] = 100.0
    right[h // 4:h // 4 + 12, w // 5:w // 5 + 18] = 100.0
    left[h // 2:h // 2 + 10, w // 2:w // 2 + 10] = 255.0
    rng = np.random.RandomState(seed)
    band = rng.uniform(size=(h, w)) < 0.5
    band[:, : w // 3] = False
    band[: h // 3] = False
    band[2 * h // 3:] = False
    d[band, 2] = 0
    d[band, 0] = rng.uniform(-30, 30, size=band.sum())   # stored values of invalid pixels lie outside the valid range
    return left, right, d, true


def write_pfm(path, img):
    """PFM writer for the C++ surface test: (rows, cols) -> "Pf", (rows, cols, 3) -> "PF"; little-endian, rows bottom to top."""
    img = np.ascontiguousarray(img, np.float32)
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n-1.0\n" % (b"PF" if img.ndim == 3 else b"Pf", img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img[::-1]).astype("<f4").tobytes())


def read_pfm(path):
    with open(path, "rb") as f:
        magic = f.readline().strip()
        cols, rows = (int(v) for v in f.readline().split())
        scale = float(f.readline())
        ch = 3 if magic == b"PF" else 1
        data = np.frombuffer(f.read(), "<f4" if scale < 0 else ">f4").astype(np.float32)
    img = data.reshape((rows, cols, ch) if ch == 3 else (rows, cols))
    return np.ascontiguousarray(img[::-1])


def build_view_program():
    """Compiles affine_view.cc (vwlite headers + libvwgpu.so) with its own command."""
    root = os.path.dirname(os.path.dirname(HERE))
    exe = os.path.join(HERE, "affine_view")
    src = os.path.join(HERE, "affine_view.cc")
    lib = os.path.join(root, "visionworkbench_amd", "lib")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + os.path.join(root, "include"),
                           "-I" + os.path.join(root, "visionworkbench_amd", "vwlite"), "-o", exe, src, "-L" + lib, "-lvwgpu",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def top_left_hole_scene(w=96, h=80, kernel=(7, 7), step=11):
    """Integer disparities (all valid) with isolated invalid pixels on a grid.  The reference weights every window pixel with
    w(0, 0) (Correlate.cc:1006-1046: the weight accessor is never advanced), so a pixel whose top-left window neighbour is
    invalid gets an all-zero system: posv fails, the update is 0 and, with max_pyramid_levels = 0, the output equals the
    input bit for bit.  Returns left, right, disparity and the (rows, cols) of those pixels."""
    left, right, d, _ = stretched_scene(w, h)
    hx, hy = kernel[0] // 2, kernel[1] // 2
    ys, xs = np.mgrid[hy + 8:h - hy - 8:step, hx + 8:w - hx - 8:step]
    d[ys, xs, 2] = 0
    return left, right, d, (ys.ravel() + hy, xs.ravel() + hx)
