"""CPU-only: pins the restatement of the reference's hole filling (tests/refimpl/hole_fill_ref.cc) with the known answers
of the reference's unit tests (tests/golden/hole_fill_known.json), the oracle's blob sizes, a brute-force L1 distance and
a float64 direct solve of the inpainting system; header, binding and the Python wrappers agree on the new names."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import hole_fill_ref as ref  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "hole_fill_known.json")) as _f:
    KNOWN = json.load(_f)

NEW_ENTRIES = ["grassfire", "blob_index", "blob_sizes", "erode_blobs", "inpaint", "fill_holes_grass", "fill_nodata_with_avg"]

# Twice the largest difference between the float32 Gauss-Seidel of the restatement and the float64 direct solve over the
# cases of test_inpaint_converges_to_the_direct_solve, measured on the CPU (profiles/hole_fill.md): the stagnation error
# of float32 Gauss-Seidel, which cannot be derived in advance.  Largest difference measured: 7.63e-06.
CONVERGENCE_TOL = 2 * 7.63e-06


# ---- known answers ------------------------------------------------------------------------------------------------------

def test_grassfire_known_answers():
    k = KNOWN["grassfire_border"]
    im = np.zeros((k["rows"], k["cols"]), np.uint8)
    x, y, w, h = k["nonzero_box"]
    im[y:y + h, x:x + w] = 255
    g = ref.grassfire(im)
    for col, row, want in k["expect"]:
        assert g[row, col] == want
    k = KNOWN["grassfire_no_border"]
    im = np.full((k["rows"], k["cols"]), 255, np.int32)
    im[k["zero_at"][1], k["zero_at"][0]] = 0
    g = ref.grassfire(im, True)
    r, c = np.mgrid[0:5, 0:5]
    assert np.array_equal(g, abs(2 - r) + abs(2 - c))


def _mask_from(k):
    m = np.zeros((k["rows"], k["cols"]), np.uint8)
    for x, y, w, h in k.get("valid_boxes", []):
        m[y:y + h, x:x + w] = 255
    for x, y in k.get("valid_pixels", []):
        m[y, x] = 5
    return m


def test_blob_index_known_answers():
    k = KNOWN["blob_index"]
    labels, table = ref.blob_index(_mask_from(k))
    assert len(table) == k["count"] and labels.max() == k["count"]
    for (ax, ay), (bx, by) in k["same"] + k["same_in_blob_2"]:
        assert labels[ay, ax] == labels[by, bx]
    for (ax, ay), (bx, by) in k["different"]:
        assert labels[ay, ax] != labels[by, bx]
    # the reference's order: by the first pixel in raster order; half-open boxes and sizes
    assert table.tolist() == [[1, 1, 4, 2, 3], [5, 1, 7, 4, 4], [2, 3, 4, 4, 2]]
    k = KNOWN["inpaint_blobs"]
    assert len(ref.blob_index(_mask_from(k))[1]) == k["count"]


def test_blob_sizes_known_answers():
    k = KNOWN["blob_sizes"]
    image = np.array(k["image_rows"], np.float32)
    masked = np.stack([image, (image != 0).astype(np.float32)], axis=2)      # create_mask(image): zero pixels are masked
    sizes = ref.blob_sizes(masked, 256)
    for col, row, want in k["expect"]:
        assert sizes[row, col] == want
    assert sorted(set(sizes[sizes > 0].tolist())) == [2, 3, 7]


def test_blob_sizes_equal_the_oracle(oracle):
    rng = np.random.RandomState(12)
    for w, h, density in ((37, 29, 0.45), (70, 45, 0.6), (64, 64, 0.3)):
        d = rng.randint(-9, 9, (h, w, 3)).astype(np.int32)
        d[..., 2] = rng.uniform(size=(h, w)) < density
        assert np.array_equal(ref.blob_sizes(d), oracle.blob_sizes(d))
        for area in (1, 3, 50):
            assert np.array_equal(ref.erode_blobs(d, area), oracle.disparity_blob_filter(d, area))


def test_filters_and_capacity():
    m = np.zeros((9, 12), np.uint8)
    m[1, 1:5] = 1          # 4 x 1, size 4
    m[3:6, 7:9] = 1        # 2 x 3, size 6
    m[7, 0] = 1            # 1 x 1
    _, t = ref.blob_index(m)
    assert t[:, 4].tolist() == [4, 6, 1]
    assert ref.blob_index(m, max_area=4)[1][:, 4].tolist() == [4, 1]          # size == max_area stays
    assert ref.blob_index(m, max_area=3)[1][:, 4].tolist() == [1]
    assert ref.blob_index(m, wipe_size=4)[1][:, 4].tolist() == [4, 6, 1]      # width == n stays
    assert ref.blob_index(m, wipe_size=3)[1][:, 4].tolist() == [6, 1]
    assert ref.blob_index(m, wipe_size=2)[1][:, 4].tolist() == [1]
    labels, _ = ref.blob_index(m, wipe_size=3)
    assert labels[1, 1] == 0 and labels[3, 7] == 1 and labels[7, 0] == 2
    assert ref.blob_index(m, capacity=2) == (-6, 3)
    inv_labels, inv = ref.blob_index(m, invert=True)
    assert len(inv) == 1 and inv[0, 4] == 9 * 12 - 11


# ---- grassfire against a brute-force search --------------------------------------------------------------------------------

def brute_grassfire(src, ignore_borders):
    h, w = src.shape
    if w <= 1 or h <= 1:
        return np.zeros((h, w), np.int32)
    zy, zx = np.nonzero(src == 0)
    y, x = np.mgrid[0:h, 0:w]
    if len(zy):
        d = (abs(y[..., None] - zy) + abs(x[..., None] - zx)).min(axis=2)
    else:
        d = np.full((h, w), w + h)
    if not ignore_borders:
        d = np.minimum(d, np.minimum(np.minimum(x + 1, w - x), np.minimum(y + 1, h - y)))
    return np.minimum(d, w + h).astype(np.int32)


@pytest.mark.parametrize("w,h", [(1, 7), (7, 1), (2, 2), (9, 6), (23, 17)])
@pytest.mark.parametrize("ignore_borders", [False, True])
def test_grassfire_equals_brute_force(w, h, ignore_borders):
    rng = np.random.RandomState(w * 100 + h)
    for density in (0.0, 0.05, 0.5, 1.0):
        src = (rng.uniform(size=(h, w)) >= density).astype(np.uint8) * 200       # density of zeros; 0.0: no zero at all
        want = brute_grassfire(src, ignore_borders)
        assert np.array_equal(ref.grassfire(src, ignore_borders), want)
        assert np.array_equal(ref.grassfire(src.astype(np.int32) * -3, ignore_borders), want)
        f = src.astype(np.float32)
        f[f != 0] = np.nan                                                      # a NaN is non-zero
        f[f == 0] = -0.0                                                        # -0.0f is zero
        assert np.array_equal(ref.grassfire(f, ignore_borders), want)
    if w > 1 and h > 1:
        assert ref.grassfire(np.ones((h, w), np.uint8), True).max() == w + h     # the cap of an image without any zero


# ---- the inpainting against a float64 direct solve ---------------------------------------------------------------------------

W8 = ((-1, -1, .176765), (0, -1, .073235), (1, -1, .176765), (-1, 0, .073235), (1, 0, .073235), (-1, 1, .176765), (0, 1, .073235),
      (1, 1, .176765))


def direct_solve(values, hole):
    """The fixed point of the 8-neighbour averaging over the pixels of `hole` in float64."""
    ys, xs = np.nonzero(hole)
    index = {(x, y): k for k, (y, x) in enumerate(zip(ys, xs))}
    A, b = np.eye(len(index)), np.zeros(len(index))
    for (x, y), k in index.items():
        for dx, dy, wt in W8:
            q = (x + dx, y + dy)
            if q in index:
                A[k, index[q]] -= wt
            else:
                b[k] += wt * float(values[q[1], q[0]])
    return ys, xs, np.linalg.solve(A, b)


def convergence_cases():
    for side in range(1, 13):                      # max_distance = ceil(side / 2) = 1 .. 6
        for a, b, c in ((1.0, 0.0, 0.0), (0.5, -0.75, 20.0), (-1.25, 0.875, -30.0)):
            for stored in (0.0, 1e3):
                yield side, (a, b, c), stored


def convergence_error(side, abc, stored):
    n = side + 8
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    ramp = abc[0] * x + abc[1] * y + abc[2]
    assert abs(ramp).max() <= 100
    img = np.stack([ramp, np.ones_like(ramp)], axis=2).astype(np.float32)
    hole = np.zeros((n, n), bool)
    hole[4:4 + side, 4:4 + side] = True
    got = ref.fill_holes_grass(ref.punch(img, hole, stored), side)
    assert got[..., 1].all()
    ys, xs, sol = direct_solve(img[..., 0], hole)
    # the ramp is the exact solution because the weights sum to 1
    assert abs(sol - img[ys, xs, 0].astype(np.float64)).max() < 1e-9
    return abs(got[ys, xs, 0].astype(np.float64) - sol).max()


def test_inpaint_converges_to_the_direct_solve():
    """The reading of InpaintView (order, weights, 10 d^2 sweeps, stored values as the initial guess) converges to the
    float64 solution of the same system within CONVERGENCE_TOL = 2 x 7.63e-06, twice the largest difference measured on the
    CPU over these cases (planar ramps of amplitude <= 100, square holes of max_distance 1 .. 6, stored 0 and 1e3)."""
    worst = max(convergence_error(*case) for case in convergence_cases())
    print("largest difference to the float64 solve: %.3g" % worst)
    assert worst <= CONVERGENCE_TOL


def test_edge_rule_and_default_value():
    img = ref.float_map(12, 10, 1)
    hole = np.zeros((10, 12), bool)
    hole[4, 10] = True         # column cols - 2: its ring ends at the last column; skipped as written, filled when fixed
    hole[1, 1] = True          # ring starts at 0: filled by both
    hole[5, 0] = True          # touches the border: skipped by both
    src = ref.punch(img, hole, 0.0)
    a, b = ref.fill_holes_grass(src, 3, "reference"), ref.fill_holes_grass(src, 3, "fixed")
    assert a[4, 10, 1] == 0 and b[4, 10, 1] == 1 and a[1, 1, 1] == 1 and b[1, 1, 1] == 1 and a[5, 0, 1] == 0 and b[5, 0, 1] == 0
    labels, table = ref.blob_index(src, invert=True)
    c = ref.inpaint(src, labels, table, False, (7.5, 0.0), "fixed")
    assert c[4, 10].tolist() == [7.5, 0.0] and c[1, 1].tolist() == [7.5, 0.0] and np.array_equal(c[5, 0], src[5, 0])
    avg = ref.fill_nodata_with_avg(src, 3)
    ring = [img[y, x, 0] for x in (0, 1, 2) for y in (0, 1, 2) if (x, y) != (1, 1)]
    s = np.float32(0)
    for v in ring:
        s = np.float32(s + v)
    assert avg[1, 1, 0] == np.float32(s / np.float32(8)) and avg[1, 1, 1] == 1


# ---- bindings ----------------------------------------------------------------------------------------------------------------

def test_binding_lists_the_new_entries():
    from visionworkbench_amd import _lib
    for name in NEW_ENTRIES:
        assert "vwgpu_" + name in _lib.SYMBOLS and "vwgpu_%s_dev" % name in _lib.SYMBOLS
    header = open(os.path.join(ROOT, "include", "vwgpu.h")).read()
    assert "#define VWGPU_ABI_VERSION 3" in header and "VWGPU_HOLE_FILL_MAX_LEN 64" in header


def test_wrappers_refuse_bad_arguments():
    from visionworkbench_amd import image
    from visionworkbench_amd.core import ArgumentErr
    masked = ref.float_map(9, 7, 1)
    with pytest.raises(ArgumentErr):
        image.fill_holes_grass(np.zeros((7, 9, 3), np.int32), 3)                  # integer pixels are not inpainted
    with pytest.raises(ArgumentErr):
        image.blob_index(np.zeros((7, 9, 4), np.float32))                         # not a pixel kind
    with pytest.raises(ArgumentErr):
        image.grassfire(np.zeros((7, 9), np.float64))
    with pytest.raises(ArgumentErr):
        image.fill_nodata_with_avg(masked, 4)                                     # even kernel
    with pytest.raises(ArgumentErr):
        image.fill_nodata_with_avg(masked, 0)
    with pytest.raises(ArgumentErr):
        image.fill_holes_grass(masked, image.HOLE_FILL_MAX_LEN + 1)
    with pytest.raises(ArgumentErr):
        image.fill_holes_grass(masked, 3, semantics="tiled")
    assert image.HOLE_FILL_MAX_LEN >= 64
