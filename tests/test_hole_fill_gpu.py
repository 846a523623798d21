"""GPU: grassfire, blob_index, get_blob_sizes, erode_blobs, inpaint, fill_holes_grass and fill_nodata_with_avg
(libvwgpu.so, hole_fill.hip) equal to the CPU restatement tests/refimpl/hole_fill_ref.cc word for word (== on values and
validity, no tolerance, no pixel left out): every pixel kind, sizes with partial and several workgroups, host and device
entries, strided buffers, in-place and out-of-place calls, both edge semantics, the largest hole, a device-resident chain,
the C++ surface and argument errors.  Finite values only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import hole_fill_ref as ref  # noqa: E402
from affine_ref import read_pfm, write_pfm  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import core, image, stereo  # noqa: E402

pytestmark = pytest.mark.gpu
ERR_ARGUMENT = -1
KIND_IDS = ["mask", "masked_float", "disparity_int", "disparity_float"]


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d words differ, first at %s: got %s want %s" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def wide(a, pad=5, fill=77):
    """`a` as a view of a wider array: rows further apart than the width."""
    big = np.full((a.shape[0], a.shape[1] + pad) + a.shape[2:], fill, a.dtype)
    big[:, :a.shape[1]] = a
    return big[:, :a.shape[1]]


def dev_wide(a, pad=5):
    import torch
    big = torch.full((a.shape[0], a.shape[1] + pad) + a.shape[2:], 77, dtype=dev(a[:1]).dtype, device="cuda")
    big[:, :a.shape[1]] = dev(a)
    return big[:, :a.shape[1]]


# ---- grassfire ------------------------------------------------------------------------------------------------------------

GRASS_SIZES = [(1, 7), (7, 1), (2, 2), (37, 29), (70, 45), (300, 5)]


@pytest.mark.parametrize("size", GRASS_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.float32], ids=["u8", "i32", "f32"])
def test_grassfire(ctx, size, dtype):
    w, h = size
    rng = np.random.RandomState(w * 7 + h)
    sources = [np.zeros((h, w), dtype), np.full((h, w), 3, dtype)]
    for density in (0.02, 0.3):
        s = (rng.uniform(size=(h, w)) >= density).astype(dtype)
        sources.append((s * (rng.randint(1, 100, (h, w)) if dtype != np.float32 else rng.uniform(-5, 5, (h, w)))).astype(dtype))
    blob = np.zeros((h, w), dtype)
    blob[h // 5:h - h // 5, w // 5:w - w // 5] = 1           # one large non-zero region: long chains in both scans
    sources.append(blob)
    for k, s in enumerate(sources):
        for ib in (False, True):
            want = ref.grassfire(s, ib)
            what = "grassfire %dx%d %s source %d ignore_borders %d" % (w, h, np.dtype(dtype).name, k, ib)
            same(image.grassfire(s, ib, ctx=ctx), want, what + " host")
            same(host(image.grassfire(dev(s), ib, ctx=ctx)), want, what + " device")
    s = sources[3]
    same(image.grassfire(wide(s), False, ctx=ctx), ref.grassfire(s, False), "grassfire strided host")
    same(host(image.grassfire(dev_wide(s), True, ctx=ctx)), ref.grassfire(s, True), "grassfire strided device")


# ---- blob_index, blob_sizes, erode_blobs -------------------------------------------------------------------------------------

def spiral(w, h):
    m = np.zeros((h, w), bool)
    x0, y0, x1, y1 = 0, 0, w - 1, h - 1
    while x1 - x0 >= 1 and y1 - y0 >= 1:
        m[y0, x0:x1 + 1] = True          # right
        m[y0:y1 + 1, x1] = True          # down
        m[y1, x0 + 2:x1 + 1] = True      # left, stopping two short of the arm that came down
        m[y0 + 2:y1 + 1, x0 + 2] = True  # up
        x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
    return m


def validity_cases(w, h):
    rng = np.random.RandomState(w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    cases = {"spiral": spiral(w, h), "checkerboard": (xx + yy) % 2 == 0, "isolated": (xx % 2 == 0) & (yy % 2 == 0),
             "random": rng.uniform(size=(h, w)) < 0.45, "none": np.zeros((h, w), bool), "all": np.ones((h, w), bool)}
    borders = np.zeros((h, w), bool)
    borders[0, 3:9] = borders[h - 1, 5:8] = borders[4:9, 0] = borders[6:8, w - 1] = True
    borders[h // 2, w // 2 - 2:w // 2 + 2] = True
    cases["borders"] = borders
    return cases


def check_index(got, img, what, **kw):
    labels, table = ref.blob_index(img, **kw)
    assert got.count == len(table), what
    same(host(got.labels), labels, what + " labels")
    same(host(got.table), table, what + " table")


@pytest.mark.parametrize("size", [(37, 29), (70, 45)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=KIND_IDS)
def test_blob_index_sizes_erode(ctx, size, kind):
    w, h = size
    for name, valid in validity_cases(w, h).items():
        img = ref.as_kind(valid, kind)
        what = "%s %dx%d kind %d" % (name, w, h, kind)
        on_device = name in ("spiral", "random", "borders")
        arg = dev(img) if on_device else img
        for invert in (False, True):
            check_index(image.blob_index(arg, invert=invert, ctx=ctx), img, what + " invert %d" % invert, invert=invert)
        same(host(image.get_blob_sizes(arg, ctx=ctx)).astype(np.uint32), ref.blob_sizes(img), what + " sizes")
        same(host(image.get_blob_sizes(arg, 5, ctx=ctx)).astype(np.uint32), ref.blob_sizes(img, 5), what + " sizes limit")
        for area in (1, 4, 60):
            same(host(image.erode_blobs(arg, area, ctx=ctx)), ref.erode_blobs(img, area), what + " erode %d" % area)
    assert image.blob_index(ref.as_kind(validity_cases(w, h)["isolated"], kind), ctx=ctx).count == ((w + 1) // 2) * ((h + 1) // 2)
    assert image.blob_index(ref.as_kind(validity_cases(w, h)["checkerboard"], kind), ctx=ctx).count == 1
    # strided and in place
    img = ref.as_kind(validity_cases(w, h)["random"], kind)
    check_index(image.blob_index(wide(img), ctx=ctx), img, "strided host")
    check_index(image.blob_index(dev_wide(img), invert=True, ctx=ctx), img, "strided device", invert=True)
    t = dev(img)
    assert image.erode_blobs(t, 4, out=t, ctx=ctx) is t
    same(host(t), ref.erode_blobs(img, 4), "erode in place, device")
    v = wide(img)
    image.erode_blobs(v, 4, out=v, ctx=ctx)
    same(np.ascontiguousarray(v), ref.erode_blobs(img, 4), "erode in place, strided host")


def test_blob_filters_at_their_boundaries(ctx):
    m = np.zeros((29, 37), np.uint8)
    m[1, 1:5] = 1          # 4 x 1, size 4
    m[3:6, 7:9] = 1        # 2 x 3, size 6
    m[7, 0] = 1            # 1 x 1
    m[10:14, 20:24] = 1    # 4 x 4, size 16
    for kw in ({"max_area": 4}, {"max_area": 3}, {"max_area": 16}, {"max_area": 15}, {"wipe_size": 4}, {"wipe_size": 3}, {"wipe_size": 2},
               {"max_area": 6, "wipe_size": 2}):
        check_index(image.blob_index(m, ctx=ctx, **kw), m, str(kw), **kw)
        check_index(image.blob_index(dev(m), ctx=ctx, **kw), m, str(kw) + " device", **kw)
    assert image.blob_index(m, max_area=4, ctx=ctx).table[:, 4].tolist() == [4, 1]       # size == max_area stays
    assert image.blob_index(m, wipe_size=4, ctx=ctx).count == 4                           # width == n stays
    for arg in (m, dev(m)):
        with pytest.raises(core.CapacityErr) as e:
            image.blob_index(arg, capacity=3, ctx=ctx)
        assert e.value.count == 4
    assert image.blob_index(m, capacity=4, ctx=ctx).count == 4


def test_erode_equals_the_blob_filter(ctx):
    rng = np.random.RandomState(3)
    d = rng.randint(-9, 9, (45, 70, 3)).astype(np.int32)
    d[..., 2] = np.where(rng.uniform(size=(45, 70)) < 0.5, core.VALID_I32, 0)
    for area in (0, 1, 5, 40):
        same(image.erode_blobs(d, area, ctx=ctx), stereo.disparity_blob_filter(d, area, ctx=ctx), "area %d" % area)


def test_blob_index_large(ctx):
    rng = np.random.RandomState(8)
    w, h = 1024, 768
    valid = rng.uniform(size=(h, w)) < 0.55
    valid[100:400, 200:900] = True                 # one blob of hundreds of thousands of pixels: the aggregated atomics
    img = ref.as_kind(valid, 3)
    t = dev(img)
    check_index(image.blob_index(t, ctx=ctx), img, "1024x768")
    check_index(image.blob_index(t, invert=True, max_area=30, wipe_size=6, ctx=ctx), img, "1024x768 inverted", invert=True, max_area=30,
                wipe_size=6)
    same(host(image.get_blob_sizes(t, 1000, ctx=ctx)).astype(np.uint32), ref.blob_sizes(img, 1000), "1024x768 sizes")
    same(host(image.erode_blobs(t, 50, ctx=ctx)), ref.erode_blobs(img, 50), "1024x768 erode")


# ---- inpaint and fill_holes_grass -------------------------------------------------------------------------------------------

def planted_holes(w, h, L):
    """The holes of the issue in 70 x 45 (True = hole)."""
    assert (w, h) == (70, 45) and L <= 12
    m = np.zeros((h, w), bool)
    m[5, 5] = True                                             # one pixel
    m[3, 10:19] = True                                         # 1 x 9 line: one dependent chain
    m[3:12, 22] = True                                         # 9 x 1 line
    for k in range(7):
        m[3 + k, 26 + k] = True                                # a diagonal: 8-connected, every distance 1
    m[3:10, 36] = True                                         # an L
    m[9, 36:42] = True
    m[3:8, 44:49] = True                                       # a ring around a valid island
    m[4:7, 45:48] = False
    m[3:10, 52:59] = True                                      # a ring that encloses a second, separate hole
    m[4:9, 53:58] = False
    m[6, 55] = True
    for x, y in ((5, 14), (6, 14), (7, 14), (5, 15), (5, 16)):  # two unconnected holes with interleaved bounding boxes
        m[y, x] = True
    for x, y in ((7, 16), (8, 16), (9, 16), (9, 15), (9, 14)):
        m[y, x] = True
    m[14:14 + L, 14:14 + L] = True                             # L x L: filled
    m[14:14 + L, 30:30 + L + 1] = True                         # (L + 1) x L: left alone
    m[14:14 + L + 1, 46:46 + L] = True                         # L x (L + 1): left alone
    for x, y in ((64, 0), (20, 44), (0, 30), (69, 32)):        # on each border
        m[y, x] = True
    for x, y in ((62, 1), (26, 43), (1, 34), (68, 36)):        # one pixel inside each border
        m[y, x] = True
    for x, y in ((66, 2), (32, 42), (2, 40), (67, 40)):        # two pixels inside each border
        m[y, x] = True
    return m


@pytest.mark.parametrize("L", [1, 2, 3, 7, 12])
@pytest.mark.parametrize("kind", [1, 3], ids=["masked_float", "disparity_float"])
def test_fill_holes_grass(ctx, L, kind):
    w, h = 70, 45
    base = ref.float_map(w, h, kind)
    hole = planted_holes(w, h, L)
    for stored in (0.0, None):
        src = ref.punch(base, hole, stored)
        results = {}
        for sem in ("reference", "fixed"):
            want = results[sem] = ref.fill_holes_grass(src, L, sem)
            what = "fill_holes_grass L %d kind %d stored %s %s" % (L, kind, stored, sem)
            same(image.fill_holes_grass(src, L, sem, ctx=ctx), want, what + " host")
            same(host(image.fill_holes_grass(dev(src), L, sem, ctx=ctx)), want, what + " device")
            t = dev_wide(src)
            assert image.fill_holes_grass(t, L, sem, out=t, ctx=ctx) is t
            same(host(t.contiguous()), want, what + " device, strided, in place")
            a = src.copy()
            image.fill_holes_grass(a, L, sem, out=a, ctx=ctx)
            same(a, want, what + " host, in place")
            # the two steps a caller can take apart: the index of the holes, then inpaint over it
            bi = image.blob_index(dev(src), invert=True, max_area=L * L, wipe_size=L, ctx=ctx)
            same(host(image.inpaint(dev(src), bi, True, None, sem, L, ctx=ctx)), want, what + " blob_index + inpaint")
        c = base.shape[2] - 1
        ref_valid, fixed_valid = results["reference"][..., c] != 0, results["fixed"][..., c] != 0
        assert ref_valid[5, 5] and fixed_valid[5, 5]
        assert not ref_valid[36, 68] and fixed_valid[36, 68] and not ref_valid[43, 26] and fixed_valid[43, 26]     # one pixel inside: they differ
        assert ref_valid[34, 1] and ref_valid[1, 62] and ref_valid[40, 67] and ref_valid[42, 32]
        assert not fixed_valid[0, 64] and not fixed_valid[32, 69]
        assert ref_valid[14:14 + L, 14:14 + L].all() and not ref_valid[14:14 + L, 30:30 + L + 1].any() and not ref_valid[14:14 + L + 1, 46:46 + L].any()


def test_sweeps_without_overlap(ctx):
    """VWGPU_OPT_INPAINT_OVERLAP = 0 (a sweep starts when the previous one has ended) gives the same words."""
    src = ref.punch(ref.float_map(70, 45, 3), planted_holes(70, 45, 12), None)
    want = ref.fill_holes_grass(src, 12)
    ctx.set_option(core.OPT_INPAINT_OVERLAP, 0)
    try:
        same(image.fill_holes_grass(src, 12, ctx=ctx), want, "no overlap")
    finally:
        ctx.set_option(core.OPT_INPAINT_OVERLAP, 1)
    same(image.fill_holes_grass(src, 12, ctx=ctx), want, "overlap")


def test_largest_hole(ctx):
    """One 64 x 64 hole, the documented maximum, in 70 x 70: 10240 sweeps over 4096 pixels, compared in full."""
    base = ref.float_map(70, 70, 1)
    hole = np.zeros((70, 70), bool)
    hole[3:67, 3:67] = True
    src = ref.punch(base, hole, None)
    want = ref.fill_holes_grass(src, 64)
    assert want[..., 1].all()
    same(host(image.fill_holes_grass(dev(src), 64, ctx=ctx)), want, "64 x 64")


def test_inpaint_with_a_default_value(ctx):
    for kind in (1, 3):
        src = ref.punch(ref.float_map(70, 45, kind), planted_holes(70, 45, 7), None)
        c = src.shape[2] - 1
        labels, table = ref.blob_index(src, invert=True, wipe_size=7)
        bi = image.blob_index(src, invert=True, wipe_size=7, ctx=ctx)
        for default in ([2.5, -4.0][:c] + [1.0], [9.0, 8.0][:c] + [0.0]):
            for sem in ("reference", "fixed"):
                want = ref.inpaint(src, labels, table, False, default, sem)
                same(image.inpaint(src, bi, False, default, sem, ctx=ctx), want, "default %s %s kind %d" % (default, sem, kind))
        # a selection of blobs of VALID pixels is as good as one of holes: islands of at most 9 pixels, re-estimated from around them
        labels, table = ref.blob_index(src, max_area=9)
        bi = image.blob_index(dev(src), max_area=9, ctx=ctx)
        assert bi.count == len(table) > 0
        same(host(image.inpaint(dev(src), bi, ctx=ctx)), ref.inpaint(src, labels, table), "islands kind %d" % kind)


def test_fill_holes_grass_large(ctx):
    rng = np.random.RandomState(17)
    w, h = 1024, 768
    hole = np.zeros((h, w), bool)
    for _ in range(300):
        bw, bh = rng.randint(1, 11, 2)
        x, y = rng.randint(0, w - bw + 1), rng.randint(0, h - bh + 1)
        hole[y:y + bh, x:x + bw] |= rng.uniform(size=(bh, bw)) < 0.8
    src = ref.punch(ref.float_map(w, h, 3), hole, None)
    want = ref.fill_holes_grass(src, 8)
    assert (want[..., 2] != src[..., 2]).sum() > 1000
    same(host(image.fill_holes_grass(dev(src), 8, ctx=ctx)), want, "1024x768")


def test_device_chain(ctx):
    """disparity_cleanup -> fill_holes_grass -> stereo_triangulate without a host copy equals the same chain with the fill
    done by the restatement."""
    import torch
    import triangulate_ref
    rng = np.random.RandomState(23)
    w, h = 70, 45
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.zeros((h, w, 3), np.int32)
    d[..., 0] = -8 + xx // 9
    d[..., 1] = yy // 20
    d[..., 2] = core.VALID_I32
    noise = rng.uniform(size=(h, w)) < 0.06
    d[noise, 0] += rng.randint(20, 40, noise.sum())             # outliers the cleanup removes: the holes
    clean = stereo.disparity_cleanup_using_thresh(dev(d), 3, 3, 2.0, 0.5, ctx=ctx)
    f = clean.to(torch.float32)
    f[..., 2] = (clean[..., 2] != 0).to(torch.float32)
    holes = int((f[..., 2] == 0).sum().item())
    assert 0 < holes < w * h // 2
    filled = image.fill_holes_grass(f, 5, "fixed", ctx=ctx)
    c1, c2 = triangulate_ref.pinhole_pair(w, h)
    xyz = stereo.stereo_triangulate(filled, c1, c2, ctx=ctx)
    assert filled.is_cuda and xyz.is_cuda
    want_filled = ref.fill_holes_grass(f.cpu().numpy(), 5, "fixed")
    assert (want_filled[..., 2] != 0).sum() > (f[..., 2] != 0).sum().item()
    same(filled.cpu().numpy(), want_filled, "filled")
    same(xyz.cpu().numpy(), stereo.stereo_triangulate(dev(want_filled), c1, c2, ctx=ctx).cpu().numpy(), "xyz")


# ---- fill_nodata_with_avg -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel_size", [1, 3, 7, 31])
def test_fill_nodata_with_avg(ctx, kernel_size):
    w, h = 37, 29
    rng = np.random.RandomState(kernel_size)
    hole = rng.uniform(size=(h, w)) < 0.3
    hole[5:25, 8:30] = True                        # windows without a valid pixel for the small kernels
    src = ref.punch(ref.float_map(w, h, 1), hole, None)
    want = ref.fill_nodata_with_avg(src, kernel_size)
    if kernel_size <= 7:
        assert (want[..., 1] == 0).any()
    same(image.fill_nodata_with_avg(src, kernel_size, ctx=ctx), want, "host")
    same(host(image.fill_nodata_with_avg(dev_wide(src), kernel_size, ctx=ctx)), want, "device, strided")


# ---- the C++ surface ----------------------------------------------------------------------------------------------------------

def test_cpp_surface(ctx, tmp_path):
    """vw::grassfire, BlobIndexThreaded, inpaint, fill_holes_grass, fill_nodata_with_avg, get_blob_sizes and applyErodeView of
    vwlite (tests/refimpl/hole_fill_view.cc) give the Python call's words."""
    exe = ref.build_view_program()
    w, h = 70, 45
    src = ref.punch(ref.float_map(w, h, 3), planted_holes(w, h, 7), None)
    masked = np.ascontiguousarray(src[..., [0, 2]])
    paths = {k: str(tmp_path / (k + ".pfm")) for k in ("disp", "masked", "out")}
    write_pfm(paths["disp"], src)
    write_pfm(paths["masked"], np.concatenate([masked, np.zeros((h, w, 1), np.float32)], axis=2))

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    run("fill_holes", paths["disp"], paths["out"], 7)
    same(read_pfm(paths["out"]), image.fill_holes_grass(src, 7, ctx=ctx), "fill_holes_grass")
    run("inpaint", paths["disp"], paths["out"], 7)
    bi = image.blob_index(src, invert=True, max_area=49, wipe_size=7, ctx=ctx)
    same(read_pfm(paths["out"]), image.inpaint(src, bi, ctx=ctx), "inpaint")
    out = run("blobs", paths["disp"], 7)
    assert out.split()[0] == str(bi.count)
    boxes = np.array([int(v) for v in out.split()[1:1 + 4 * bi.count]]).reshape(-1, 4)
    same(boxes.astype(np.int32), np.ascontiguousarray(bi.table[:, :4]), "blob_bbox")
    run("avg", paths["masked"], paths["out"], 3)
    same(read_pfm(paths["out"])[..., :2], image.fill_nodata_with_avg(masked, 3, ctx=ctx), "fill_nodata_with_avg")
    run("erode", paths["disp"], paths["out"], 30)
    same(read_pfm(paths["out"]), image.erode_blobs(src, 30, ctx=ctx), "applyErodeView")
    run("sizes", paths["disp"], paths["out"], 100)
    same(read_pfm(paths["out"])[..., 0].astype(np.uint32), image.get_blob_sizes(src, 100, ctx=ctx), "get_blob_sizes")
    run("grassfire", paths["disp"], paths["out"], 0)
    same(read_pfm(paths["out"])[..., 0].astype(np.int32), image.grassfire(np.ascontiguousarray(src[..., 2]), ctx=ctx), "grassfire")


# ---- argument errors ----------------------------------------------------------------------------------------------------------

def test_argument_errors(ctx):
    lib, hnd = ctx._lib, ctx._h
    w, h = 9, 7
    img = ref.float_map(w, h, 3)
    out = np.empty_like(img)
    labels = np.zeros((h, w), np.int32)
    table = np.zeros((4, 5), np.int32)
    n = ctypes.c_int(0)
    u8 = np.ones((h, w), np.uint8)
    i32 = np.zeros((h, w), np.int32)
    p = lambda a: a.ctypes.data      # noqa: E731
    for sfx in ("", "_dev"):          # the checks come before any device work: host pointers never reach a kernel
        g = lambda name: getattr(lib, "vwgpu_" + name + sfx)      # noqa: E731
        assert g("grassfire")(hnd, 0, None, w, h, 0, 0, p(i32), 0) == ERR_ARGUMENT
        assert g("grassfire")(hnd, 0, p(u8), 0, h, 0, 0, p(i32), 0) == ERR_ARGUMENT
        assert g("grassfire")(hnd, 0, p(u8), w, h, w - 1, 0, p(i32), 0) == ERR_ARGUMENT
        assert g("grassfire")(hnd, 3, p(u8), w, h, 0, 0, p(i32), 0) == ERR_ARGUMENT
        assert g("blob_index")(hnd, 4, p(img), w, h, 0, 0, 0, 0, p(labels), 0, p(table), 4, ctypes.byref(n)) == ERR_ARGUMENT
        assert g("blob_index")(hnd, 3, None, w, h, 0, 0, 0, 0, p(labels), 0, p(table), 4, ctypes.byref(n)) == ERR_ARGUMENT
        assert g("blob_index")(hnd, 3, p(img), w, -1, 0, 0, 0, 0, p(labels), 0, p(table), 4, ctypes.byref(n)) == ERR_ARGUMENT
        assert g("blob_index")(hnd, 3, p(img), w, h, 0, 0, 0, 0, p(labels), w - 1, p(table), 4, ctypes.byref(n)) == ERR_ARGUMENT
        assert g("blob_index")(hnd, 3, p(img), w, h, 0, 0, 0, 0, p(labels), 0, p(table), 4, None) == ERR_ARGUMENT
        assert g("blob_sizes")(hnd, 3, p(img), w, h, 0, 5, None, 0) == ERR_ARGUMENT
        assert g("blob_sizes")(hnd, -1, p(img), w, h, 0, 5, p(labels), 0) == ERR_ARGUMENT
        assert g("erode_blobs")(hnd, 3, p(img), w, h, 2, 5, p(out), 0) == ERR_ARGUMENT
        assert g("erode_blobs")(hnd, 3, p(img), w, h, 0, 5, None, 0) == ERR_ARGUMENT
        assert g("inpaint")(hnd, 2, p(img), w, h, 0, p(labels), 0, p(table), 0, 1, None, 0, 8, p(out), 0) == ERR_ARGUMENT
        assert g("inpaint")(hnd, 3, p(img), w, h, 0, None, 0, p(table), 0, 1, None, 0, 8, p(out), 0) == ERR_ARGUMENT
        assert g("inpaint")(hnd, 3, p(img), w, h, 0, p(labels), 0, None, 2, 1, None, 0, 8, p(out), 0) == ERR_ARGUMENT
        assert g("inpaint")(hnd, 3, p(img), w, h, 0, p(labels), 0, p(table), 0, 1, None, 2, 8, p(out), 0) == ERR_ARGUMENT
        assert g("inpaint")(hnd, 3, p(img), w, h, 0, p(labels), 0, p(table), 0, 1, None, 0, 65, p(out), 0) == ERR_ARGUMENT
        assert g("fill_holes_grass")(hnd, 3, p(img), w, h, 0, 65, 0, p(out), 0) == ERR_ARGUMENT
        assert g("fill_holes_grass")(hnd, 3, p(img), w, h, 0, -1, 0, p(out), 0) == ERR_ARGUMENT
        assert g("fill_holes_grass")(hnd, 3, p(img), w, h, 0, 5, 7, p(out), 0) == ERR_ARGUMENT
        assert g("fill_holes_grass")(hnd, 0, p(img), w, h, 0, 5, 0, p(out), 0) == ERR_ARGUMENT
        assert g("fill_holes_grass")(hnd, 3, p(img), w, h, 0, 5, 0, p(out), w - 1) == ERR_ARGUMENT
        assert g("fill_holes_grass")(hnd, 3, None, w, h, 0, 5, 0, p(out), 0) == ERR_ARGUMENT
        assert g("fill_nodata_with_avg")(hnd, p(img), w, h, 0, 4, p(out), 0) == ERR_ARGUMENT
        assert g("fill_nodata_with_avg")(hnd, p(img), w, h, 0, 0, p(out), 0) == ERR_ARGUMENT
        assert g("fill_nodata_with_avg")(hnd, p(img), w, h, 0, 3, p(img), 0) == ERR_ARGUMENT
        assert g("fill_nodata_with_avg")(hnd, None, w, h, 0, 3, p(out), 0) == ERR_ARGUMENT
    # the context still works
    same(image.fill_holes_grass(img, 5, ctx=ctx), img, "nothing to fill")
