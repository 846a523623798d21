"""Seeded random case generators for the image and disparity kernel families, shared by tests/test_family_cases_cpu.py (which
shows, without a GPU, that the streams are deterministic, accepted by the CPU restatements and cover what they claim),
tests/test_fuzz_families_gpu.py and tools/fuzz_families.py / tools/replay_family_case.py.

The conventions of tests/fuzz_cases.py: a case is a plain dict with `it`; a case is a pure function of (seed, it) (every case
draws from its own default_rng([seed, K + it]) stream, so any single case is rebuilt without the ones before it); an option
added later takes a stream of its own with another K; no GPU import; a generator never emits a call the API refuses (a
combination that does not apply is not generated).  Pixel values are finite, except the stored values under invalid
disparities of the median and the smoothing filter, where the family's own GPU test feeds NaN too (they are copied, never
computed with).

Every case names one `entry` (the Python wrapper it calls), the operands (numpy arrays), the parameters, and how the test
passes the operands:
    layout       "host", "host_view" (a view of a wider array: row stride = width + pad, the surroundings a sentinel), "dev",
                 "dev_strided", or "inplace" (only where the wrapper has out=; `base` is then one of the four others)
    pad          1 .. 7
    side_stream  on about a third of the device cases: uploads and call on a stream of their own
"""
import numpy as np

# ---- shared samplers ---------------------------------------------------------------------------------------------------------

SIZE_CLASSES = ("one", "row", "col", "small", "tile", "uniform")      # + "scan" for the scan kernels
SIZE_P = (0.04, 0.07, 0.07, 0.12, 0.32, 0.38)
SCAN_P = 0.10                                                         # taken from "uniform" where the scan class applies
MAX_COLS, MAX_ROWS = 140, 48                                           # what the suite uses; tools/fuzz_families.py --max-size sets others
MOSAIC_MAX = 90                                                       # the largest side of an image of mosaic_cases
TILE_64x4, TILE_16x16 = (64, 4), (16, 16)


def _tile_side(rng, tile, limit):
    """A multiple of the tile side offset by -1, 0 or +1, at most limit + 1."""
    m = int(rng.integers(1, max(limit // tile, 1) + 1))
    return max(1, m * tile + int(rng.integers(-1, 2)))


def sample_size(rng, tile, scan=False):
    """(cols, rows, class): 1 x 1 (p 0.04); one row (0.07); one column (0.07); 2 .. 5 on a side (0.12); a multiple of the
    family's workgroup tile -1 / 0 / +1 on one axis or both (0.32); uniform up to 140 x 48 (0.38, or 0.28 and 0.10 for the
    scan class: one side 2047, 2048, 2049 or up to 4200, the other at most 3)."""
    names, p = list(SIZE_CLASSES), list(SIZE_P)
    if scan:
        names.append("scan")
        p[-1] -= SCAN_P
        p.append(SCAN_P)
    cls = names[int(rng.choice(len(names), p=p))]
    if cls == "one":
        return 1, 1, cls
    if cls == "row":
        return int(rng.integers(2, MAX_COLS + 1)), 1, cls
    if cls == "col":
        return 1, int(rng.integers(2, MAX_COLS + 1)), cls
    if cls == "small":
        return int(rng.integers(2, 6)), int(rng.integers(2, 6)), cls
    if cls == "tile":
        which = int(rng.integers(3))                                    # x, y, both
        cols = _tile_side(rng, tile[0], MAX_COLS) if which != 1 else int(rng.integers(1, MAX_COLS + 1))
        rows = _tile_side(rng, tile[1], MAX_ROWS) if which != 0 else int(rng.integers(1, MAX_ROWS + 1))
        return cols, rows, cls
    if cls == "scan":
        long = int(rng.choice([2047, 2048, 2049, int(rng.integers(2050, 4201))]))
        short = int(rng.integers(1, 4))
        return (long, short, cls) if rng.random() < 0.5 else (short, long, cls)
    return int(rng.integers(1, MAX_COLS + 1)), int(rng.integers(1, MAX_ROWS + 1)), cls


MASK_CLASSES = ("all", "none", "one_pixel", "one_line", "checker", "density", "rects")
MASK_P = (0.15, 0.05, 0.07, 0.10, 0.08, 0.35, 0.20)


def sample_mask(rng, cols, rows, p=MASK_P):
    """(bool (rows, cols), class): all valid; none; one valid pixel; one valid row or column; checkerboard; density 0.02, 0.5
    or 0.95; invalid rectangles touching each border of a valid field (or the inverse)."""
    cls = MASK_CLASSES[int(rng.choice(len(MASK_CLASSES), p=p))]
    m = np.zeros((rows, cols), bool)
    if cls == "all":
        m[:] = True
    elif cls == "one_pixel":
        m[int(rng.integers(rows)), int(rng.integers(cols))] = True
    elif cls == "one_line":
        if rng.random() < 0.5:
            m[int(rng.integers(rows))] = True
        else:
            m[:, int(rng.integers(cols))] = True
    elif cls == "checker":
        yy, xx = np.mgrid[0:rows, 0:cols]
        m = (xx + yy + int(rng.integers(2))) % 2 == 0
    elif cls == "density":
        m = rng.random((rows, cols)) < float(rng.choice([0.02, 0.5, 0.95]))
    elif cls == "rects":
        r = np.zeros((rows, cols), bool)
        for side in range(4):
            w, h = int(rng.integers(1, max(cols // 2, 1) + 1)), int(rng.integers(1, max(rows // 2, 1) + 1))
            x, y = int(rng.integers(0, cols - w + 1)), int(rng.integers(0, rows - h + 1))
            if side == 0:
                x = 0
            elif side == 1:
                x = cols - w
            elif side == 2:
                y = 0
            else:
                y = rows - h
            r[y:y + h, x:x + w] = True
        m = r if rng.random() < 0.3 else ~r
    return m, cls


LAYOUTS = ("host", "host_view", "dev", "dev_strided", "inplace")


def sample_layout(rng, inplace=False):
    """dict(layout, base, pad, side_stream)."""
    p = [0.25, 0.2, 0.25, 0.2, 0.1] if inplace else [0.28, 0.22, 0.28, 0.22, 0.0]
    layout = LAYOUTS[int(rng.choice(5, p=p))]
    base = LAYOUTS[int(rng.integers(4))] if layout == "inplace" else layout
    pad = int(rng.integers(1, 8))
    side = bool(rng.random() < 1.0 / 3.0) and base.startswith("dev")
    return dict(layout=layout, base=base, pad=pad, side_stream=side)


def _rng(seed, k, it):
    return np.random.default_rng([seed, k + it])


def _surface(rng, cols, rows):
    """A plane plus a wave plus noise, float64 (rows, cols)."""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    a, b, c = rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-8, 8)
    return c + a * x + b * y + rng.uniform(0, 2) * np.sin(x / rng.uniform(3, 15)) * np.cos(y / rng.uniform(3, 15)) \
        + rng.normal(0, rng.choice([0.0, 0.15, 0.6]), (rows, cols))


def _disparity(rng, cols, rows, dtype, valid, outliers=0.0, huge=40.0, stored="random", nan=0.0):
    """A (rows, cols, 3) {dx, dy, valid} map of int32 (valid word 1) or float32: two surfaces, planted outliers on a
    fraction `outliers` of the pixels, random (or zero) stored values under the invalid pixels, NaN on a fraction `nan` of
    those."""
    dx, dy = _surface(rng, cols, rows), 0.5 * _surface(rng, cols, rows)
    out = rng.random((rows, cols)) < outliers
    dx[out] += rng.choice([-1.0, 1.0], int(out.sum())) * rng.uniform(0.5 * huge, huge, int(out.sum()))
    out = rng.random((rows, cols)) < outliers / 2
    dy[out] += rng.uniform(-huge, huge, int(out.sum()))
    bad = ~valid
    n = int(bad.sum())
    if stored == "random":
        dx[bad], dy[bad] = rng.uniform(-50, 50, n), rng.uniform(-50, 50, n)
    else:
        dx[bad] = dy[bad] = 0.0
    d = np.zeros((rows, cols, 3), np.float64)
    d[..., 0], d[..., 1], d[..., 2] = dx, dy, valid
    if dtype == "int32":
        return np.round(d).astype(np.int32)
    d = d.astype(np.float32)
    if nan > 0 and n:
        d[bad & (rng.random((rows, cols)) < nan), 0] = np.nan
    return d


def _image(rng, cols, rows, integer=False):
    v = 100 + 40 * _surface(rng, cols, rows) / 8.0 + rng.normal(0, 6, (rows, cols)) * (rng.random() < 0.5)
    return (np.round(v) if integer else v).astype(np.float32)


def _partition(rng, cols, rows, limit=48):
    """Non-overlapping boxes [[x, y, w, h], ...] covering the image: a grid of random blocks, among them one-row and one-column
    blocks, with at most about `limit` boxes."""
    kind = int(rng.choice(4, p=[0.1, 0.1, 0.4, 0.4]))
    bw = int(rng.integers(1, cols + 1))
    bh = int(rng.integers(1, rows + 1))
    if kind == 3:                                      # large blocks: about a half or a third of a side
        bw, bh = (cols + int(rng.integers(1, 4)) - 1) // int(rng.integers(1, 4)) or 1, (rows + 1) // int(rng.integers(1, 3)) or 1
    if kind == 0:
        bh = 1
        bw = max(bw, (cols * rows + limit - 1) // limit)
    elif kind == 1:
        bw = 1
        bh = max(bh, (cols * rows + limit - 1) // limit)
    bw, bh = min(bw, cols), min(bh, rows)
    while ((cols + bw - 1) // bw) * ((rows + bh - 1) // bh) > limit:      # too many boxes: widen (one-row blocks stay one row while they can)
        if bw < cols and (bh >= rows or kind == 1 or rng.random() < 0.5) and kind != 1:
            bw = min(cols, bw * 2)
        elif bh < rows and kind != 0:
            bh = min(rows, bh * 2)
        elif bw < cols:
            bw = min(cols, bw * 2)
        else:
            bh = min(rows, bh * 2)
    return [[x, y, min(bw, cols - x), min(bh, rows - y)] for y in range(0, rows, bh) for x in range(0, cols, bw)], (bw, bh)


def _odd_kernel(rng, top=31):
    """An odd kernel 1 .. top: mostly small (the references' cost grows with the square), the maximum now and then."""
    r = rng.random()
    if r < 0.6:
        return int(rng.integers(0, 5)) * 2 + 1
    if r < 0.92:
        return int(rng.integers(5, 9)) * 2 + 1
    return int(rng.integers(9, top // 2 + 1)) * 2 + 1


# ---- the disparity post-filters of Stereo/Algorithms.h -----------------------------------------------------------------------

DISPARITY_FILTER_ENTRIES = ("disparity_median_filter", "disparity_neighbor_filter", "texture_measure",
                            "texture_preserving_disparity_filter")


def _fitting_kernel(rng, box, top=31):
    """An odd kernel of at least 3: seven times in ten one that leaves the box (cols, rows) an interior, where there is one."""
    room = min(box[0], box[1], top)
    if room >= 3 and rng.random() < 0.7:
        return int(rng.integers(1, min((room - 1) // 2, 4) + 1)) * 2 + 1
    return max(_odd_kernel(rng, top), 3) if rng.random() < 0.9 else 1


def disparity_filter_cases(n, seed, start=0):
    for it in range(start, n):
        rng = _rng(seed, 11000003, it)
        entry = DISPARITY_FILTER_ENTRIES[int(rng.integers(4))]
        cols, rows, size_class = sample_size(rng, TILE_16x16)
        valid, mask_class = sample_mask(rng, cols, rows, p=(0.35, 0.03, 0.03, 0.05, 0.05, 0.27, 0.22))
        c = dict(it=it, entry=entry, size=(cols, rows), size_class=size_class, mask_class=mask_class, **sample_layout(rng))
        c["semantics"] = ("reference", "snapshot")[int(rng.integers(2))]
        tiles, block = _partition(rng, cols, rows)
        how = int(rng.choice(3, p=[0.5, 0.25, 0.25]))   # the whole image, block_size, an explicit list of boxes
        c["block_size"] = block if how == 1 else None
        c["tiles"] = tiles if how == 2 else None
        box = (cols, rows) if how == 0 else block
        if entry == "disparity_median_filter":
            c["disparity"] = _disparity(rng, cols, rows, "float32", valid, outliers=0.06, nan=float(rng.choice([0.0, 0.2])))
            c["kernel_size"] = _fitting_kernel(rng, box)
        elif entry == "disparity_neighbor_filter":      # nearly constant stretches (five of eight neighbours agree) with outliers
            f = _disparity(rng, cols, rows, "float32", valid, outliers=0.08, huge=60.0)
            d = np.zeros((rows, cols, 3), np.int32)
            d[..., :2] = np.round(f[..., :2] * np.float32(0.08))
            d[..., 2] = valid
            if rng.random() < 0.5:                      # a checkerboard stretch where two candidates tie
                y0 = int(rng.integers(rows))
                yy, xx = np.mgrid[0:rows, 0:cols]
                band = (yy >= y0) & (yy < y0 + 6)
                d[band, 0] = np.where((xx + yy)[band] % 2 == 0, 3, 4)
                d[band, 1] = 0
            c["disparity"] = d
        elif entry == "texture_measure":
            c["image"] = _image(rng, cols, rows, integer=bool(rng.random() < 0.4))
            c["kernel_size"] = _odd_kernel(rng)
            c["gradient_weight"], c["stddev_weight"] = [(0.5, 0.5), (1.0, 0.0), (0.0, 1.0), (0.3, 1.7)][int(rng.integers(4))]
            if how == 2 and len(tiles) > 1 and rng.random() < 0.5:          # boxes that leave part of the image out: zeros there
                c["tiles"] = [t for t in tiles if rng.random() < 0.7] or tiles[:1]
        else:
            c["disparity"] = _disparity(rng, cols, rows, "float32", valid, outliers=0.04, nan=float(rng.choice([0.0, 0.2])))
            c["texture"] = np.abs(rng.normal(0, 0.12, (rows, cols))).astype(np.float32) * (rng.random((rows, cols)) < 0.8)
            c["texture_max"] = float(rng.choice([0.0, 0.05, 0.15, 0.15, 0.5, 0.5, 1e9]))
            c["max_kernel_size"] = int(rng.choice([1, 3, 5, 7, 11, 11, 15, 21, 31]))
        yield c


# ---- the local outlier filters of Stereo/DisparityMap.h ----------------------------------------------------------------------

OUTLIER_ENTRIES = ("rm_outliers_using_mean", "rm_outliers_using_stddev", "rm_outliers_using_plane", "disparity_cleanup_using_mean",
                   "disparity_cleanup_using_stddev", "disparity_clean_using_plane", "std_dev_image")


def _half_kernel(rng):
    """1 .. 15 (the wrappers refuse 0, as the reference's functors throw on it), mostly small."""
    return int(rng.integers(1, 5)) if rng.random() < 0.7 else int(rng.integers(5, 16))


def outlier_filter_cases(n, seed, start=0):
    for it in range(start, n):
        rng = _rng(seed, 12000017, it)
        entry = OUTLIER_ENTRIES[int(rng.choice(7, p=[0.15, 0.15, 0.15, 0.13, 0.13, 0.13, 0.16]))]
        cols, rows, size_class = sample_size(rng, TILE_16x16)
        valid, mask_class = sample_mask(rng, cols, rows, p=(0.2, 0.04, 0.05, 0.08, 0.08, 0.35, 0.2))
        c = dict(it=it, entry=entry, size=(cols, rows), size_class=size_class, mask_class=mask_class, **sample_layout(rng))
        if entry == "std_dev_image":
            c["image"] = _image(rng, cols, rows)
            c["kernel"] = (int(rng.integers(1, 32)) if rng.random() < 0.3 else int(rng.integers(1, 8)),
                           int(rng.integers(1, 32)) if rng.random() < 0.3 else int(rng.integers(1, 8)))
            c["edge"] = ("zero", "constant")[int(rng.integers(2))]
            yield c
            continue
        dtype = ("int32", "float32")[int(rng.integers(2))]
        huge = float(rng.choice([25.0, 500.0, 1e6])) if dtype == "int32" else float(rng.choice([8.0, 25.0, 300.0]))
        d = _disparity(rng, cols, rows, dtype, valid, outliers=float(rng.choice([0.0, 0.03, 0.1])), huge=huge)
        if rng.random() < 0.4:                          # an exactly planar patch: zero residuals, sigma 0
            w, h = int(rng.integers(1, cols + 1)), int(rng.integers(1, rows + 1))
            x, y = int(rng.integers(0, cols - w + 1)), int(rng.integers(0, rows - h + 1))
            yy, xx = np.mgrid[y:y + h, x:x + w]
            a, b = int(rng.integers(-2, 3)), int(rng.integers(-2, 3))
            d[y:y + h, x:x + w, 0] = (a * xx + b * yy - 3).astype(d.dtype)
            d[y:y + h, x:x + w, 1] = (b * xx - a * yy + 1).astype(d.dtype)
        c["disparity"] = d
        c["half"] = (_half_kernel(rng), _half_kernel(rng))
        thr = lambda: float(rng.choice([0.0, 0.05, 0.4, 1.0, 1.5, 3.0, 1e30]))      # noqa: E731
        if entry.endswith("mean"):
            c["args"] = (thr(),)
            c["semantics"] = ("reference", "skip")[int(rng.integers(2))]
        else:
            c["args"] = (thr(), float(rng.choice([0.0, 0.05, 0.2, 0.3, 1e30])))
            c["semantics"] = "reference"
        yield c


# ---- the rest of Stereo/DisparityMap.h -----------------------------------------------------------------------------------------

DISPARITY_MAP_ENTRIES = ("get_disparity_range", "disparity_range_mask", "transform_disparities", "transform_disparities_subregion",
                         "disparity_subsample", "disparity_upsample", "missing_pixel_image", "intersect_mask_and_data",
                         "disparity_transform_image")


def _origin(rng, far=100000):
    r = rng.random()
    if r < 0.3:
        return 0
    if r < 0.7:
        return int(rng.integers(-40, 41))
    return int(rng.choice([-1, 1])) * int(rng.integers(1000, far + 1))


def _matrix(rng):
    """(kind, 3 x 3): a translation, an affine map near the identity, or a projective one whose w stays above 0.5 for the
    coordinates these cases reach (|x|, |y| < 2300)."""
    kind = ("translation", "affine", "projective")[int(rng.integers(3))]
    m = np.eye(3)
    m[0, 2], m[1, 2] = rng.uniform(-120, 120), rng.uniform(-40, 40)
    if rng.random() < 0.3:
        m[0, 2], m[1, 2] = np.round(m[0, 2]), np.round(m[1, 2])
    if kind != "translation":
        m[:2, :2] += rng.uniform(-0.05, 0.05, (2, 2))
    if kind == "projective":
        m[2, 0], m[2, 1] = rng.uniform(-1e-4, 1e-4, 2)
    return kind, m


def disparity_map_cases(n, seed, start=0):
    for it in range(start, n):
        rng = _rng(seed, 13000027, it)
        entry = DISPARITY_MAP_ENTRIES[int(rng.integers(9))]
        cols, rows, size_class = sample_size(rng, TILE_64x4)
        valid, mask_class = sample_mask(rng, cols, rows)
        dtype = "float32" if entry == "disparity_transform_image" else ("int32", "float32")[int(rng.integers(2))]
        c = dict(it=it, entry=entry, size=(cols, rows), size_class=size_class, mask_class=mask_class, dtype=dtype, **sample_layout(rng))
        d = _disparity(rng, cols, rows, dtype, valid, outliers=0.03)
        c["disparity"] = d
        if entry == "disparity_range_mask":
            c["x0"], c["y0"] = _origin(rng), _origin(rng)
            lo = np.array([c["x0"] + rng.integers(-10, cols // 2 + 1), c["y0"] + rng.integers(-10, rows // 2 + 1)], np.float64)
            hi = lo + np.array([rng.integers(0, cols + 20), rng.integers(0, rows + 20)], np.float64)
            if dtype == "float32" and rng.random() < 0.5:
                lo, hi = lo + rng.uniform(-1, 1, 2), hi + rng.uniform(-1, 1, 2)
            if rng.random() < 0.1:
                lo, hi = np.array([-1e9, -1e9]), np.array([1e9, 1e9])
            c["min"], c["max"] = tuple(lo.tolist()), tuple(hi.tolist())
            c["semantics"] = ("reference", "fixed")[int(rng.integers(2))]
        elif entry in ("transform_disparities", "transform_disparities_subregion"):
            c["matrix_kind"], c["matrix"] = _matrix(rng)
            far = 2000 if c["matrix_kind"] == "projective" else 100000
            c["x0"], c["y0"] = _origin(rng, far), _origin(rng, far)
            c["do_round"] = bool(rng.random() < 0.5)
        elif entry == "intersect_mask_and_data":
            other, _ = sample_mask(rng, cols, rows)
            c["mask"] = _disparity(rng, cols, rows, dtype, other)
        elif entry == "disparity_transform_image":
            rel = int(rng.integers(3))                                  # the right image larger, equal, smaller
            rw = max(1, cols + (int(rng.integers(1, 30)), 0, -int(rng.integers(1, 30)))[rel])
            rh = max(1, rows + (int(rng.integers(1, 12)), 0, -int(rng.integers(1, 12)))[rel])
            c["right"] = _image(rng, rw, rh)
            c["right_relation"] = ("larger", "equal", "smaller")[rel]
            kind = rng.integers(0, 8, (rows, cols))                     # integer offsets (one coordinate or both), offsets off the image
            for k, ch in ((0, (0, 1)), (1, (0,)), (2, (1,))):
                for a in ch:
                    d[kind == k, a] = np.round(d[kind == k, a])
            d[kind == 3, 0] += rng.choice([-3000.0, 3000.0], int((kind == 3).sum())).astype(np.float32)
            d[kind == 4, 1] += rng.choice([-3000.0, 3000.0], int((kind == 4).sum())).astype(np.float32)
        yield c


# ---- vw::transform -------------------------------------------------------------------------------------------------------------

TRANSFORM_INTERPS = ("nearest", "bilinear", "bicubic")
TRANSFORM_EDGES = ("zero", "value", "constant", "periodic", "cylindrical", "reflect", "linear")
T_IDENTITY, T_TRANSLATE, T_RESAMPLE, T_AFFINE, T_HOMOGRAPHY = range(5)


def _step(rng, cx, cy):
    """One step of a chain as a specification the test turns into a descriptor with the restatement's own make / rotate /
    invert: ("make", kind, params), ("rotate", theta, cx, cy) or ("invert", specification)."""
    k = int(rng.integers(7))
    if k == 0:
        s = ("make", T_IDENTITY, ())
    elif k == 1:
        t = rng.uniform(-6, 6, 2)
        if rng.random() < 0.4:
            t = np.round(t)
        s = ("make", T_TRANSLATE, tuple(t.tolist()))
    elif k == 2:
        s = ("make", T_RESAMPLE, tuple(float(v) for v in rng.choice([0.5, 2.0, 1.25, 0.8, 1.0, 51 / 37.0, 3.0], 2)))
    elif k == 3:
        m = np.eye(2) + rng.uniform(-0.25, 0.25, (2, 2))
        s = ("make", T_AFFINE, tuple(m.reshape(4).tolist()) + tuple(rng.uniform(-5, 5, 2).tolist()))
    elif k == 4:
        m = np.eye(3)
        m[:2, :2] += rng.uniform(-0.05, 0.05, (2, 2))
        m[:2, 2] = rng.uniform(-3, 3, 2)
        m[2, :2] = rng.uniform(-3e-4, 3e-4, 2)
        s = ("make", T_HOMOGRAPHY, tuple(m.reshape(9).tolist()))
    else:
        s = ("rotate", float(rng.uniform(-0.6, 0.6)), float(cx), float(cy))
    if k in (3, 4, 5, 6) and rng.random() < 0.25:
        s = ("invert", s)
    return s


def transform_cases(n, seed, start=0):
    for it in range(start, n):
        rng = _rng(seed, 14000029, it)
        sw, sh, size_class = sample_size(rng, TILE_64x4)
        w, h, out_class = sample_size(rng, TILE_64x4)
        valid, mask_class = sample_mask(rng, sw, sh)
        c = dict(it=it, size=(sw, sh), size_class=size_class, out_size=(w, h), out_class=out_class, mask_class=mask_class,
                 **sample_layout(rng))
        c["image"] = _image(rng, sw, sh)
        c["mask"] = (valid.astype(np.uint8) * 255) if rng.random() < 0.5 else None
        c["interp"] = TRANSFORM_INTERPS[int(rng.integers(3))]
        c["edge"] = TRANSFORM_EDGES[int(rng.integers(7))]
        if c["edge"] in ("reflect", "linear") and min(sw, sh) < 2:      # refused on a source of one row or column
            c["edge"] = TRANSFORM_EDGES[int(rng.integers(5))]
        if c["edge"] == "linear":                                       # ... and LinearEdgeExtension has no masked form
            c["mask"] = None
        c["edge_value"] = (float(rng.choice([7.5, -3.0, 0.0])), bool(rng.random() < 0.5))
        nodata = rng.random() < 0.3
        c["entry"] = "transform_nodata" if nodata else "transform"
        c["nodata"] = (float(rng.choice([-32768.0, 0.0, 1.5])), bool(rng.random() < 0.5)) if nodata else None
        place = ("inside", "straddle", "outside", "free")[int(rng.choice(4, p=[0.25, 0.3, 0.15, 0.3]))]
        c["place"] = place
        if place == "inside":                                         # a translation; the output box maps into the source
            ti = rng.integers(-9, 10, 2)
            frac = rng.random(2) * (rng.random(2) < 0.5)
            f = [1 if (frac[0] > 0) else 0, 1 if (frac[1] > 0) else 0]
            if sw - f[0] < 1:
                frac[0], f[0] = 0.0, 0
            if sh - f[1] < 1:
                frac[1], f[1] = 0.0, 0
            w, h = min(w, sw - f[0]), min(h, sh - f[1])
            ax, ay = int(rng.integers(0, sw - f[0] - w + 1)), int(rng.integers(0, sh - f[1] - h + 1))
            c["steps"] = [("make", T_TRANSLATE, (float(ti[0] + frac[0]), float(ti[1] + frac[1])))]
            c["out_size"] = (w, h)
            c["x0"], c["y0"] = int(ti[0] + f[0] + ax), int(ti[1] + f[1] + ay)
        else:
            c["steps"] = [_step(rng, sw / 2.0, sh / 2.0) for _ in range(int(rng.integers(1, 5)))]
            if place == "straddle":
                c["x0"], c["y0"] = int(rng.integers(-w, sw + 1)) if w > 1 or sw > 1 else 0, int(rng.integers(-h // 2 - 1, sh // 2 + 1))
            elif place == "outside":
                c["x0"] = int(rng.choice([-1, 1])) * int(rng.integers(3000, 100000))
                c["y0"] = int(rng.integers(-50, 50))
                c["steps"] = [s for s in c["steps"] if s[0] == "make" and s[1] in (T_IDENTITY, T_TRANSLATE)] or [("make", T_IDENTITY, ())]
            else:
                c["x0"], c["y0"] = int(rng.integers(-60, 61)), int(rng.integers(-25, 26))
        yield c


# ---- vw::stereo::corr_eval -------------------------------------------------------------------------------------------------------

CORR_EVAL_METRICS = ("ncc", "stddev", "parabola_curvature", "cramer_rao")


def corr_eval_cases(n, seed, start=0):
    for it in range(start, n):
        rng = _rng(seed, 15000017, it)
        cols, rows, size_class = sample_size(rng, TILE_16x16)
        valid, mask_class = sample_mask(rng, cols, rows, p=(0.3, 0.03, 0.05, 0.07, 0.05, 0.35, 0.15))
        c = dict(it=it, entry="corr_eval", size=(cols, rows), size_class=size_class, mask_class=mask_class, **sample_layout(rng))
        c["metric"] = CORR_EVAL_METRICS[int(rng.integers(4))]
        big = rng.random() < 0.1                                        # at most one case in ten above 35
        side = lambda: (int(rng.integers(18, 32)) * 2 + 1) if big and rng.random() < 0.7 else (          # noqa: E731
            int(rng.integers(0, 6)) * 2 + 1 if rng.random() < 0.75 else int(rng.integers(6, 18)) * 2 + 1)
        c["kernel"] = (side(), side())
        c["sample_rate"] = int(rng.choice([1, 1, 1, 2, 3, 4, 5, 7, 9, 2 ** 27]))
        c["round_to_int"] = bool(rng.random() < 0.4)
        c["prefilter_width"] = float(rng.choice([0.0, 0.0, 1.4, 2.0, 7.0]))
        rel = int(rng.integers(3))
        rw = max(1, cols + (int(rng.integers(1, 30)), 0, -int(rng.integers(1, 30)))[rel])
        rh = max(1, rows + (int(rng.integers(1, 12)), 0, -int(rng.integers(1, 12)))[rel])
        c["right_relation"] = ("larger", "equal", "smaller")[rel]
        H, W = max(rows, rh) + 8, max(cols, rw) + 12
        tex = 100 + 20 * _surface(rng, W, H) + rng.normal(0, 8, (H, W))
        shift = (int(rng.integers(0, 8)), int(rng.integers(0, 4)))
        c["left"] = tex[4:4 + rows, 6:6 + cols].astype(np.float32)
        c["right"] = (tex[4 - shift[1] + 2:, 6 - shift[0] + 3:][:rh, :rw] + rng.normal(0, 0.5, (rh, rw))).astype(np.float32)
        d = _disparity(rng, cols, rows, "float32", valid, outliers=0.03, huge=160.0)
        d[..., 0] = d[..., 0] * np.float32(0.3) + np.float32(shift[0] - 3)
        d[..., 1] = d[..., 1] * np.float32(0.3) + np.float32(shift[1] - 2)
        kind = rng.integers(0, 10, (rows, cols))
        d[kind == 0, :2] = np.round(d[kind == 0, :2])                   # integer disparities: the one-tap shortcut
        d[kind == 1, 0] = np.float32(rng.choice([130.25, -150.75, 3000.5]))      # pointing off the right image
        c["disparity"] = d
        lv, _ = sample_mask(rng, cols, rows, p=(0.1, 0.02, 0.03, 0.05, 0.05, 0.55, 0.2))
        rv, _ = sample_mask(rng, rw, rh, p=(0.1, 0.02, 0.03, 0.05, 0.05, 0.55, 0.2))
        masks = int(rng.integers(4))                                    # none, left, right, both
        c["left_valid"] = lv.astype(np.uint8) if masks in (1, 3) else None
        c["right_valid"] = rv.astype(np.uint8) if masks in (2, 3) else None
        _, block = _partition(rng, cols, rows, limit=24)
        c["block_size"] = block if rng.random() < 0.6 else None
        yield c


# ---- hole filling ----------------------------------------------------------------------------------------------------------------

HOLE_FILL_ENTRIES = ("grassfire", "blob_index", "get_blob_sizes", "erode_blobs", "inpaint", "fill_holes_grass", "fill_nodata_with_avg")
SCAN_ENTRIES = ("grassfire", "blob_index", "get_blob_sizes")
PIXEL_KINDS = ("mask_u8", "masked_f32", "disparity_i32", "disparity_f32")


def _plant_holes(rng, valid, L):
    """Holes (False) planted into a validity field: lines, a diagonal, rings around islands, holes on and one pixel inside each
    border, holes of exactly L and L + 1 on a side."""
    rows, cols = valid.shape
    m = valid.copy()

    def at(w, h):
        return int(rng.integers(0, max(cols - w, 0) + 1)), int(rng.integers(0, max(rows - h, 0) + 1))

    for _ in range(int(rng.integers(0, 4))):
        k = int(rng.integers(5))
        n = int(rng.integers(1, 10))
        if k == 0:
            x, y = at(n, 1)
            m[y, x:x + n] = False
        elif k == 1:
            x, y = at(1, n)
            m[y:y + n, x] = False
        elif k == 2:
            x, y = at(n, n)
            for j in range(min(n, rows - y, cols - x)):
                m[y + j, x + j] = False
        elif k == 3:
            s = min(int(rng.integers(3, 8)), cols, rows)
            x, y = at(s, s)
            m[y:y + s, x:x + s] = False
            m[y + 1:y + s - 1, x + 1:x + s - 1] = True
            if rng.random() < 0.5 and s >= 5:
                m[y + s // 2, x + s // 2] = False
        else:
            d = int(rng.integers(0, 2))                                 # on the border, or one pixel inside
            side = int(rng.integers(4))
            x, y = at(1, 1)
            if side == 0:
                x = min(d, cols - 1)
            elif side == 1:
                x = max(cols - 1 - d, 0)
            elif side == 2:
                y = min(d, rows - 1)
            else:
                y = max(rows - 1 - d, 0)
            m[y, x] = False
    if L >= 1 and rng.random() < 0.8:
        for w, h in ((L, L), (L + 1, L), (L, L + 1)):
            if rng.random() < 0.75 and w + 2 <= cols and h + 2 <= rows:
                x, y = int(rng.integers(1, cols - w)), int(rng.integers(1, rows - h))
                m[max(y - 1, 0):y + h + 1, max(x - 1, 0):x + w + 1] = True
                m[y:y + h, x:x + w] = False
    return m


def _as_kind(rng, valid, kind, stored):
    """An image of the given pixel kind with the given validity; stored: "random" or "zero" values under invalid pixels."""
    rows, cols = valid.shape
    if kind == "mask_u8":
        return np.where(valid, rng.integers(1, 256, (rows, cols)), 0).astype(np.uint8)
    if kind == "disparity_i32":
        d = _disparity(rng, cols, rows, "int32", valid, stored=stored)
        d[..., 2] = np.where(valid, 0x7fffffff, 0)
        return d
    d = _disparity(rng, cols, rows, "float32", valid, stored=stored)
    if kind == "masked_f32":
        return np.ascontiguousarray(d[..., [0, 2]])
    return d


def hole_fill_cases(n, seed, start=0):
    for it in range(start, n):
        rng = _rng(seed, 16000057, it)
        entry = HOLE_FILL_ENTRIES[int(rng.choice(7, p=[0.13, 0.15, 0.1, 0.12, 0.15, 0.25, 0.1]))]
        cols, rows, size_class = sample_size(rng, TILE_64x4, scan=entry in SCAN_ENTRIES)
        valid, mask_class = sample_mask(rng, cols, rows)
        c = dict(it=it, entry=entry, size=(cols, rows), size_class=size_class, mask_class=mask_class,
                 **sample_layout(rng, inplace=entry in ("erode_blobs", "inpaint", "fill_holes_grass")))
        stored = ("random", "zero")[int(rng.integers(2))]
        c["stored"] = stored
        L = int(rng.integers(0, 17))
        if entry == "grassfire":
            dtype = (np.uint8, np.int32, np.float32)[int(rng.integers(3))]
            v = rng.integers(1, 100, (rows, cols)) if dtype != np.float32 else rng.uniform(0.5, 5, (rows, cols)) * rng.choice([-1, 1], (rows, cols))
            c["image"] = (valid * v).astype(dtype)
            c["pixel_kind"] = np.dtype(dtype).name
            c["ignore_borders"] = bool(rng.random() < 0.5)
            yield c
            continue
        if entry in ("inpaint", "fill_holes_grass"):
            kind = ("masked_f32", "disparity_f32")[int(rng.integers(2))]
            if rng.random() < 0.6:                      # a mostly valid field, so that there is something to fill from
                valid = np.ones((rows, cols), bool) if rng.random() < 0.5 else rng.random((rows, cols)) < 0.97
                mask_class = "planted"
            valid = _plant_holes(rng, valid, L)
        elif entry == "fill_nodata_with_avg":
            kind = "masked_f32"
        else:
            kind = PIXEL_KINDS[int(rng.integers(4))]
        c["mask_class"] = mask_class
        c["pixel_kind"] = kind
        c["image"] = _as_kind(rng, valid, kind, stored)
        c["semantics"] = ("reference", "fixed")[int(rng.integers(2))]
        if entry == "blob_index":
            c["invert"] = bool(rng.random() < 0.5)
            c["max_area"] = int(rng.choice([0, 0, 1, 4, L * L, 60]))
            c["wipe_size"] = int(rng.choice([0, 0, L, 1, 3]))
        elif entry == "get_blob_sizes":
            c["limit"] = int(rng.choice([0xffffffff, 1, 5, 1000]))
        elif entry == "erode_blobs":
            c["max_area"] = int(rng.choice([0, 1, 4, 9, 60, 100000]))
        elif entry == "inpaint":
            # the index the inpainting works on: the holes of at most L on a side (L >= 1: no blob is wider than the 64 the GPU
            # inpaints), or islands of at most 9 valid pixels
            L = max(L, 1)
            c["islands"] = bool(rng.random() < 0.2)
            c["index"] = dict(invert=False, max_area=int(rng.integers(1, 10)), wipe_size=0) if c["islands"] else \
                dict(invert=True, max_area=int(rng.choice([0, L * L])), wipe_size=L)
            c["use_grassfire"] = bool(rng.random() < 0.7)
            ch = 2 if kind == "masked_f32" else 3
            c["default"] = None if rng.random() < 0.5 else [float(v) for v in rng.uniform(-9, 9, ch - 1)] + [float(rng.integers(2))]
        elif entry == "fill_nodata_with_avg":
            c["kernel_size"] = _odd_kernel(rng)
        c["L"] = L
        yield c


# ---- the multi-band blend ----------------------------------------------------------------------------------------------------------

def mosaic_cases(n, seed, start=0):
    for it in range(start, n):
        rng = _rng(seed, 17000023, it)
        draft = bool(rng.random() < 0.25)
        channels = int(rng.choice([1, 2, 4])) if draft else int(rng.choice([2, 4]))
        count = int(rng.integers(1, 7))
        lay = sample_layout(rng)
        c = dict(it=it, entry="ImageComposite", draft=draft, fill_holes=bool(rng.random() < 0.5) and not draft, channels=channels, **lay)
        lo = int(rng.choice([8, 8, 16, 32, 64]))                         # the smallest side decides the number of levels
        sizes, offsets, images = [], [], []
        alpha_kind = ("one", "fraction", "rect_zero")[int(rng.integers(3))]
        x, y = int(rng.integers(-20, 21)), int(rng.integers(-20, 21))
        for k in range(count):
            w, h = int(rng.integers(lo, MOSAIC_MAX + 1)), int(rng.integers(lo, MOSAIC_MAX + 1))
            if k:
                pw, ph = sizes[-1]
                px, py = offsets[-1]
                rel = ("overlap", "touch", "gap", "inside", "free")[int(rng.choice(5, p=[0.4, 0.15, 0.15, 0.15, 0.15]))]
                if rel == "overlap":
                    x, y = px + int(rng.integers(1, pw)), py + int(rng.integers(-ph // 2, ph // 2 + 1))
                elif rel == "touch":
                    x, y = px + pw, py + int(rng.integers(-5, 6))
                elif rel == "gap":
                    x, y = px + pw + int(rng.integers(1, 12)), py + int(rng.integers(-5, 6))
                elif rel == "inside" and pw - 2 >= lo and ph - 2 >= lo:
                    w, h = int(rng.integers(lo, pw - 1)), int(rng.integers(lo, ph - 1))
                    x, y = px + int(rng.integers(1, pw - w)), py + int(rng.integers(1, ph - h))
                else:
                    x, y = px + int(rng.integers(-30, 31)), py + int(rng.integers(-30, 31))
            img = np.empty((h, w, channels), np.float32)
            yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
            for ch in range(channels):
                img[..., ch] = 0.5 + 0.3 * np.sin(xx / (5.0 + ch) + k) * np.cos(yy / (7.0 - ch)) + rng.uniform(-0.1, 0.1, (h, w))
            if channels > 1:
                a = np.ones((h, w)) if alpha_kind == "one" else 0.25 + 0.75 * rng.random((h, w))
                img[..., -1] = a
                img[..., :-1] *= img[..., -1:]
                if alpha_kind == "rect_zero":
                    rw_, rh_ = int(rng.integers(1, w // 2 + 1)), int(rng.integers(1, h // 2 + 1))
                    rx, ry = int(rng.integers(0, w - rw_ + 1)), int(rng.integers(0, h - rh_ + 1))
                    img[ry:ry + rh_, rx:rx + rw_] = 0
            sizes.append((w, h))
            offsets.append((x, y))
            images.append(img)
        c.update(images=images, offsets=offsets, sizes=sizes, alpha=alpha_kind)
        x0, y0 = min(o[0] for o in offsets), min(o[1] for o in offsets)
        x1 = max(o[0] + s[0] for o, s in zip(offsets, sizes))
        y1 = max(o[1] + s[1] for o, s in zip(offsets, sizes))
        c["total_bbox"] = None
        if rng.random() < 0.3:
            c["total_bbox"] = (x0 - int(rng.integers(0, 6)), y0 - int(rng.integers(0, 6)), x1 + int(rng.integers(0, 6)), y1 + int(rng.integers(0, 6)))
            x0, y0, x1, y1 = c["total_bbox"]
        cols, rows = x1 - x0, y1 - y0
        c["view"] = (cols, rows)
        patches = []
        for _ in range(2):                                              # (min.x, min.y, max.x, max.y) in view coordinates, down to 1 x 1
            pw = 1 if rng.random() < 0.2 else int(rng.integers(1, cols + 1))
            ph = 1 if rng.random() < 0.2 else int(rng.integers(1, rows + 1))
            px, py = int(rng.integers(0, cols - pw + 1)), int(rng.integers(0, rows - ph + 1))
            patches.append((px, py, px + pw, py + ph))
        c["patches"] = patches
        yield c


GENERATORS = {"disparity_filter_cases": disparity_filter_cases, "outlier_filter_cases": outlier_filter_cases,
              "disparity_map_cases": disparity_map_cases, "transform_cases": transform_cases, "corr_eval_cases": corr_eval_cases,
              "hole_fill_cases": hole_fill_cases, "mosaic_cases": mosaic_cases}


def case_at(generator, seed, it):
    """The case (generator, seed, it) without the ones before it."""
    return next(GENERATORS[generator](it + 1, seed, it))


# ---- the CPU restatement's answer to a case ------------------------------------------------------------------------------------

def _refimpl(name):
    import importlib
    import os
    import sys
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "refimpl")
    if here not in sys.path:
        sys.path.insert(0, here)
    return importlib.import_module(name)


def transform_steps(case):
    """The descriptors of a transform case, made by the restatement's own tfr_make / tfr_rotate / tfr_invert."""
    ref = _refimpl("transform_ref")

    def one(s):
        if s[0] == "make":
            return ref.made(s[1], s[2])
        if s[0] == "rotate":
            return ref.rotate(s[1], s[2], s[3])
        return ref.invert(one(s[1]))

    return [one(s) for s in case["steps"]]


def reference(generator, c):
    """name -> array: every output of the case's call as tests/refimpl computes it.  Raises where the restatement refuses."""
    e = c.get("entry")
    if generator == "disparity_filter_cases":
        ref, st = _refimpl("disparity_filters_ref"), []
        kw = dict(block_size=c["block_size"], tiles=c["tiles"], stats=st)
        if e == "disparity_median_filter":
            out = ref.disparity_median_filter(c["disparity"].copy(), c["kernel_size"], c["semantics"], **kw)
        elif e == "disparity_neighbor_filter":
            out = ref.disparity_neighbor_filter(c["disparity"].copy(), c["semantics"], **kw)
        elif e == "texture_measure":
            out = ref.texture_measure(c["image"], c["kernel_size"], c["gradient_weight"], c["stddev_weight"], **kw)
            return {"out": out, "stats": np.array(st, np.float32)}
        else:
            out = ref.texture_preserving_disparity_filter(c["disparity"].copy(), c["texture"], c["texture_max"], c["max_kernel_size"],
                                                          c["semantics"], **kw)
        return {"out": out, "stats": np.array(st, np.int64)}
    if generator == "outlier_filter_cases":
        ref, st = _refimpl("outlier_filters_ref"), []
        if e == "std_dev_image":
            return {"out": ref.std_dev_image(c["image"], c["kernel"][0], c["kernel"][1], c["edge"])}
        method = e.rsplit("_", 1)[1]
        args = c["args"] + ((0.0,) if method == "mean" else ())
        out = ref.rm_outliers(method, c["disparity"], c["half"][0], c["half"][1], args[0], args[1], cleanup=not e.startswith("rm_"),
                              semantics=c["semantics"], stats=st)
        return {"out": out, "stats": np.array(st, np.int64)}
    if generator == "disparity_map_cases":
        ref, d = _refimpl("disparity_map_ref"), c["disparity"]
        if e == "get_disparity_range":
            return {"out": ref.get_disparity_range(d)}
        if e == "disparity_range_mask":
            st = []
            out = ref.disparity_range_mask(d, c["min"], c["max"], c["semantics"], c["x0"], c["y0"], stats=st)
            return {"out": out, "stats": np.array(st, np.int64)}
        if e == "transform_disparities":
            return {"out": ref.transform_disparities(d, c["matrix"], "functor", c["x0"], c["y0"])}
        if e == "transform_disparities_subregion":
            return {"out": ref.transform_disparities(d, c["matrix"], "subregion_round" if c["do_round"] else "subregion", c["x0"], c["y0"])}
        if e == "intersect_mask_and_data":
            return {"out": ref.intersect_mask_and_data(d, c["mask"])}
        if e == "disparity_transform_image":
            return {"out": ref.disparity_transform_image(c["right"], d)}
        return {"out": getattr(ref, e)(d)}
    if generator == "transform_cases":
        ref = _refimpl("transform_ref")
        r = ref.image(c["image"], transform_steps(c), c["out_size"], c["x0"], c["y0"], interp=ref.INTERPS[c["interp"]], edge=ref.EDGES[c["edge"]],
                      edge_value=c["edge_value"][0], edge_valid=c["edge_value"][1], mask=c["mask"], nodata=c["nodata"])
        if r["rc"]:
            raise ValueError("tfr_image: rc %d" % r["rc"])
        out = {"out": r["out"]}
        if c["mask"] is not None:
            out["mask"] = r["mask"]
        return out
    if generator == "corr_eval_cases":
        ref = _refimpl("corr_eval_ref")
        out, st = ref.corr_eval(c["left"], c["right"], c["disparity"], c["kernel"], c["metric"], c["sample_rate"], c["round_to_int"], 0,
                                c["prefilter_width"], c["left_valid"], c["right_valid"], block_size=c["block_size"])
        return {"out": out, "stats": np.array(st, np.int64)}
    if generator == "hole_fill_cases":
        ref, img = _refimpl("hole_fill_ref"), c["image"]
        if e == "grassfire":
            return {"out": ref.grassfire(img, c["ignore_borders"])}
        if e == "blob_index":
            labels, table = ref.blob_index(img, invert=c["invert"], max_area=c["max_area"], wipe_size=c["wipe_size"])
            return {"labels": labels, "table": table, "count": np.array([len(table)])}
        if e == "get_blob_sizes":
            return {"out": ref.blob_sizes(img, c["limit"])}
        if e == "erode_blobs":
            return {"out": ref.erode_blobs(img, c["max_area"])}
        if e == "inpaint":
            labels, table = ref.blob_index(img, **c["index"])
            return {"out": ref.inpaint(img, labels, table, c["use_grassfire"], c["default"], c["semantics"]), "count": np.array([len(table)])}
        if e == "fill_holes_grass":
            return {"out": ref.fill_holes_grass(img, c["L"], c["semantics"])}
        return {"out": ref.fill_nodata_with_avg(img, c["kernel_size"])}
    if generator == "mosaic_cases":
        ref = _refimpl("mosaic_ref")
        comp = ref.compose(c["images"], c["offsets"], fill_holes=c["fill_holes"], draft=c["draft"], total_bbox=c["total_bbox"])
        out = {"geometry": np.array((comp.cols(), comp.rows(), comp.levels) + comp.bbox() + comp.source_data_bbox()), "whole": comp.generate()}
        if not c["draft"]:
            for k in range(len(c["images"])):
                out["mask%d" % k] = comp.mask(k)
        for k, (x0, y0, x1, y1) in enumerate(c["patches"]):
            out["patch%d" % k] = comp.generate_patch(x0, y0, x1 - x0, y1 - y0)
        return out
    raise KeyError(generator)


def differing(got, want):
    """The number of words of `got` that differ from `want` (==; two NaNs, or two words of the same bits, are equal), or -1
    for another shape or type."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return -1
    ne = got != want
    if got.dtype.kind == "f":
        ne &= ~(np.isnan(got) & np.isnan(want))
    return int(ne.sum())


# what the suite runs: generator -> (cases per seed, seeds).  N is chosen so that the restatements' pass over both seeds stays
# well under the 5 s that tests/test_family_cases_cpu.py allows; profiles/fuzz_families.md has the measured times.
SUITE = {"disparity_filter_cases": (300, (1101, 1102)), "outlier_filter_cases": (300, (1201, 1202)),
         "disparity_map_cases": (400, (1301, 1302)), "transform_cases": (400, (1401, 1402)), "corr_eval_cases": (150, (1501, 1502)),
         "hole_fill_cases": (400, (1601, 1602)), "mosaic_cases": (120, (1701, 1702))}
