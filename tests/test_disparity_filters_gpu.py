"""GPU: stereo.disparity_median_filter / disparity_neighbor_filter / texture_measure /
texture_preserving_disparity_filter (libvwgpu.so, disparity_filters.hip) equal to the CPU restatement
tests/refimpl/disparity_filters_ref.cc at every pixel, values (==) and validity, no tolerance, in both semantics; host
and device entries; a device-resident chain; the C++ surface; limits and argument errors; one 4096^2 run per filter with
two sampled 1024^2 boxes against the restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import disparity_filters_ref as dfr  # noqa: E402
from affine_ref import read_pfm, write_pfm  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import core, stereo, synth  # noqa: E402

pytestmark = pytest.mark.gpu
SEM = ["reference", "snapshot"]
MAX_KERNEL = 31     # the documented maximum of the median, the texture measure and the smoothing window


def _equal(got, want, what=""):
    """values (==) at valid pixels, validity everywhere; stored values of invalid pixels are copies of the input's"""
    assert got.shape == want.shape and got.dtype == want.dtype
    vg, vw = got[..., 2] != 0, want[..., 2] != 0
    bad = (vg != vw) | (vg & vw & ((got[..., 0] != want[..., 0]) | (got[..., 1] != want[..., 1])))
    diff = np.argwhere(bad)
    assert len(diff) == 0, "%s: %d pixels differ, first at %s: got %s want %s" % (
        what, len(diff), diff[0], got[tuple(diff[0])], want[tuple(diff[0])])
    assert np.array_equal(got[~vg].view(np.uint32), want[~vw].view(np.uint32)), what + ": invalid pixels are not copies"


def _median(d, k, sem, **kw):
    sw, sg = [], []
    want = dfr.disparity_median_filter(d.copy(), k, sem, stats=sw, **kw)
    got = stereo.disparity_median_filter(d, k, sem, stats=sg, **kw)
    _equal(got, want, "median k=%d %s %s" % (k, sem, kw))
    assert sg == sw
    return got


def _neighbor(d, sem, **kw):
    sw, sg = [], []
    want = dfr.disparity_neighbor_filter(d.copy(), sem, stats=sw, **kw)
    got = stereo.disparity_neighbor_filter(d, sem, stats=sg, **kw)
    _equal(got, want, "neighbour %s %s" % (sem, kw))
    assert sg == sw
    return got


def _smooth(d, tex, tmax, maxk, sem, **kw):
    sw, sg = [], []
    want = dfr.texture_preserving_disparity_filter(d.copy(), tex, tmax, maxk, sem, stats=sw, **kw)
    got = stereo.texture_preserving_disparity_filter(d, tex, tmax, maxk, sem, stats=sg, **kw)
    _equal(got, want, "smoothing max=%d %s %s" % (maxk, sem, kw))
    assert sg == sw
    return got


def _texture(img, k, gw=0.5, sw_=0.5, **kw):
    sw, sg = [], []
    want = dfr.texture_measure(img, k, gw, sw_, stats=sw, **kw)
    got = stereo.texture_measure(img, k, gw, sw_, stats=sg, **kw)
    diff = np.argwhere(got != want)
    assert len(diff) == 0, "texture k=%d: %d pixels differ, first at %s: got %r want %r" % (
        k, len(diff), diff[0], got[tuple(diff[0])], want[tuple(diff[0])])
    assert sg == sw
    return got


# ---- median ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEM)
@pytest.mark.parametrize("k", [3, 4, 5, 7, 9, 15, MAX_KERNEL])
def test_median_kernels(sem, k):
    w, h = (70, 52) if k > 15 else (90, 70)
    d = dfr.float_scene(w, h, seed=k)
    _median(d, k, sem)
    _median(d, k, sem, block_size=(64, 64))


@pytest.mark.parametrize("sem", SEM)
def test_median_sparse_windows_small_images_and_nan(sem):
    d = dfr.float_scene(48, 40, seed=30, hole=False)
    d[8:30, 6:30, 2] = 0                    # a fully invalid region ...
    d[15, 12] = (3.25, -1.5, 1)             # ... with windows that hold exactly one valid pixel
    d[20, 20] = (-7.0, 0.0, 1)
    for k in (3, 5, 9):
        _median(d, k, sem)
    for (w, h) in ((4, 30), (30, 4), (9, 9), (8, 8), (1, 1), (10, 11)):   # sides smaller than (or just at) the window
        _median(dfr.float_scene(w, h, seed=w + h, hole=False), 9, sem)
    n = dfr.float_scene(40, 30, seed=31, hole=False)
    n[10, 10] = (np.nan, 1.0, 1)            # NaN among the valid disparities: those windows stay as they are
    got = stereo.disparity_median_filter(n, 5, sem)
    want = dfr.disparity_median_filter(n.copy(), 5, sem)
    assert np.isnan(got[10, 10, 0]) and got[10, 10, 2] == 1 and np.isnan(want[10, 10, 0])
    got[10, 10, 0] = want[10, 10, 0] = 0    # NaN != NaN; every other pixel compares as usual
    _equal(got, want, "median with a valid NaN")
    near = got[8:13, 8:13][n[8:13, 8:13, 2] != 0]
    assert np.array_equal(near, np.where(np.isnan(n[8:13, 8:13]), 0, n[8:13, 8:13])[n[8:13, 8:13, 2] != 0])
    z = np.zeros((20, 20, 3), np.float32)   # zeros of both signs: equal as values
    z[..., 2] = 1
    z[::2, :, 0] = -0.0
    _median(z, 3, sem)


# ---- neighbour ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEM)
def test_neighbour_outliers_holes_and_ties(sem):
    for seed in (4, 5):
        d = dfr.int_scene(120, 90, seed=seed)
        _neighbor(d, sem)
        _neighbor(d, sem, block_size=(64, 64))
        _neighbor(d, sem, block_size=(120, 1))
    t = np.zeros((3, 3, 3), np.int32)       # a tie: four 5s then four 6s never reach five; five 6s do
    t[..., 2] = 1
    t[..., 0] = [[5, 5, 5], [5, 0, 6], [6, 6, 6]]
    assert stereo.disparity_neighbor_filter(t, sem)[1, 1, 0] == 0
    t[0, 0, 0] = 6
    assert tuple(_neighbor(t, sem)[1, 1]) == (6, 0, 1)
    t[1, 1, 2] = 0                          # whatever the centre's own validity
    assert tuple(_neighbor(t, sem)[1, 1]) == (6, 0, 1)


# ---- texture measure --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("k", [3, 9, 15, MAX_KERNEL])
def test_texture_measure_kernels(k, integer):
    img = dfr.image_scene(100, 76, seed=k, integer=integer)
    _texture(img, k)
    _texture(img, k, 0.2, 1.7, block_size=(64, 64))
    _texture(img[:9, :7].copy(), k, 1.0, 0.0)      # an image smaller than the window


# ---- texture-preserving smoothing ----------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEM)
@pytest.mark.parametrize("maxk", [3, 11, 13, 10, MAX_KERNEL])
def test_smoothing_window_sizes(sem, maxk):
    w, h = 80, 60
    d = dfr.float_scene(w, h, seed=maxk)
    rng = np.random.RandomState(maxk)
    tmax = np.float32(0.15)
    tex = rng.uniform(-0.02, 0.2, (h, w)).astype(np.float32)
    # textures exactly on the window-size steps: tmax - s * tmax / maxk, and their float neighbours
    steps = np.float32(tmax) - np.arange(0, maxk + 2, dtype=np.float32) * (np.float32(tmax) / np.float32(maxk))
    tex[0:3, :len(steps)] = np.stack([steps, np.nextafter(steps, np.float32(1)), np.nextafter(steps, np.float32(-1))])
    tex[30:33, 20:20 + len(steps)] = tex[0:3, :len(steps)]
    tex[40, 40], tex[41, 41] = np.nan, np.inf
    _smooth(d, tex, tmax, maxk, sem)
    _smooth(d, tex, tmax, maxk, sem, block_size=(64, 64))
    _smooth(d, np.zeros_like(tex), tmax, maxk, sem, block_size=(33, 17))


@pytest.mark.parametrize("sem", SEM)
def test_smoothing_degenerate_parameters(sem):
    d = dfr.float_scene(50, 40, seed=41)
    tex = np.random.RandomState(3).uniform(-0.05, 0.1, (40, 50)).astype(np.float32)
    for tmax, maxk in ((0.0, 11), (-0.3, 11), (0.15, 2), (0.15, 0), (1e-42, 11), (3e38, 5)):
        got = _smooth(d, tex, tmax, maxk, sem)
        if tmax <= 0 or maxk < 3:
            _equal(got, d)
    _smooth(d, -np.abs(tex) - 1e-3, 0.15, 11, sem)     # negative textures everywhere: untouched


# ---- tilings, entries, the chain --------------------------------------------------------------------------------

@pytest.mark.parametrize("sem", SEM)
@pytest.mark.parametrize("block", [None, (64, 64), (50, 37), (130, 1), (37, 1)])
def test_tilings(sem, block):
    d = dfr.float_scene(130, 90, seed=50)
    tex = (dfr.image_scene(130, 90, seed=51) / 1000).astype(np.float32)
    _median(d, 5, sem, block_size=block)
    _neighbor(dfr.int_scene(130, 90, seed=52), sem, block_size=block)
    _smooth(d, tex, 0.15, 7, sem, block_size=block)
    _texture(dfr.image_scene(130, 90, seed=53), 5, block_size=block)
    # boxes that leave part of the image out: the rest is copied
    _median(d, 3, sem, tiles=[(5, 6, 40, 30), (60, 10, 33, 64)])


@pytest.mark.parametrize("sem", SEM)
def test_host_entry_equals_device_entry(sem):
    import torch
    d = dfr.float_scene(120, 90, seed=60)
    di = dfr.int_scene(120, 90, seed=61)
    img = dfr.image_scene(120, 90, seed=62)
    tex = (img / 1000).astype(np.float32)
    dt, dit, it, tt = (torch.from_numpy(a).cuda() for a in (d, di, img, tex))
    keep = dt.clone()
    pairs = [
        (stereo.disparity_median_filter(d, 7, sem, block_size=(64, 64)), stereo.disparity_median_filter(dt, 7, sem, block_size=(64, 64))),
        (stereo.disparity_neighbor_filter(di, sem), stereo.disparity_neighbor_filter(dit, sem)),
        (stereo.texture_preserving_disparity_filter(d, tex, 0.15, 9, sem), stereo.texture_preserving_disparity_filter(dt, tt, 0.15, 9, sem)),
    ]
    torch.cuda.synchronize()
    for host, dev in pairs:
        assert dev.is_cuda
        _equal(dev.cpu().numpy(), host)
    assert torch.equal(dt.view(torch.int32), keep.view(torch.int32))     # the Python surface leaves its input alone
    sh, sd = [], []
    th = stereo.texture_measure(img, 9, stats=sh)
    td = stereo.texture_measure(it, 9, stats=sd)
    assert np.array_equal(td.cpu().numpy(), th) and sh == sd and sh[0] == th.max()
    with pytest.raises(core.ArgumentErr):
        stereo.texture_preserving_disparity_filter(dt, tex, 0.15, 9, sem)       # the texture must live on the device too


def test_device_resident_chain_sgm_median_smoothing():
    """calc_disparity_sgm -> median -> texture smoothing on device tensors equals the chain through host arrays."""
    import torch
    left, right, _ = synth.stereo_pair(256, 128, 17, 1, block=64)
    small_r = right[:128, :256 + 16].copy()
    box = vwa.bounding_box(left)

    def chain(l, r):
        _, sub = stereo.calc_disparity_sgm(3, l, r, box, (16, 0), (5, 5), with_subpixel=True)
        h, w = sub.shape[:2]
        img = l[2:2 + h, 2:2 + w]
        st = []
        tex = stereo.texture_measure(img if isinstance(img, np.ndarray) else img.contiguous(), 9, stats=st)
        med = stereo.disparity_median_filter(sub, 5)
        return stereo.texture_preserving_disparity_filter(med, tex, 0.15 * max(st[0], 1e-6), 11), med

    host, host_med = chain(left, small_r)
    dev, dev_med = chain(torch.from_numpy(left).cuda(), torch.from_numpy(small_r).cuda())
    torch.cuda.synchronize()
    assert dev.is_cuda and dev_med.is_cuda
    _equal(dev_med.cpu().numpy(), host_med)
    _equal(dev.cpu().numpy(), host)
    _equal(host_med, dfr.disparity_median_filter(stereo.calc_disparity_sgm(3, left, small_r, box, (16, 0), (5, 5), with_subpixel=True)[1], 5))


# ---- limits and errors through the raw C entry -----------------------------------------------------------------

def test_limits_and_argument_errors():
    d = dfr.float_scene(40, 30, seed=70)
    di = dfr.int_scene(40, 30, seed=71)
    img = dfr.image_scene(40, 30, seed=72)
    out, outi, outf = np.empty_like(d), np.empty_like(di), np.empty_like(img)
    ctx = core.default_context(0)
    L, H = ctx._lib, ctx._h
    whole = np.array([[0, 0, 40, 30]], np.int32)

    def median(k=5, sem=0, boxes=whole, n=None, src=d, dst=out, w=40, h=30, stride=0):
        return L.vwgpu_disparity_median_filter(H, None if src is None else src.ctypes.data, w, h, stride, k, sem,
                                               boxes.ctypes.data, len(boxes) if n is None else n,
                                               None if dst is None else dst.ctypes.data, 0, None)

    def smooth(maxk=11, tmax=0.15, tex=img, sem=0):
        return L.vwgpu_texture_preserving_disparity_filter(H, d.ctypes.data, 40, 30, 0, None if tex is None else tex.ctypes.data,
                                                           0, tmax, maxk, sem, whole.ctypes.data, 1, out.ctypes.data, 0, None)

    def texture(k=9, gw=0.5, dst=outf):
        return L.vwgpu_texture_measure(H, img.ctypes.data, 40, 30, 0, k, gw, 0.5, whole.ctypes.data, 1, dst.ctypes.data, 0, None)

    assert median() == 0 and smooth() == 0 and texture() == 0
    assert median(k=MAX_KERNEL) == 0 and smooth(maxk=MAX_KERNEL) == 0 and texture(k=MAX_KERNEL) == 0
    assert median(k=MAX_KERNEL + 1) == -2 and smooth(maxk=MAX_KERNEL + 1) == -2 and texture(k=MAX_KERNEL + 1) == -2   # NOIMPL
    bad_boxes = [np.array([[0, 0, 41, 30]], np.int32), np.array([[-1, 0, 10, 10]], np.int32), np.array([[0, 0, 0, 10]], np.int32),
                 np.array([[0, 0, 20, 20], [19, 19, 10, 10]], np.int32)]
    for b in bad_boxes:
        assert median(boxes=b) not in (0, -2), b
        assert L.vwgpu_disparity_neighbor_filter(H, di.ctypes.data, 40, 30, 0, 0, b.ctypes.data, len(b), outi.ctypes.data, 0,
                                                 None) not in (0, -2)
    for kw in ({"k": -1}, {"sem": 2}, {"n": -1}, {"src": None}, {"dst": None}, {"w": 0}, {"h": -3}, {"stride": 39},
               {"dst": d, "sem": 1}):
        assert median(**kw) not in (0, -2), kw
    assert median(dst=d.copy(), sem=0) == 0
    for kw in ({"maxk": -1}, {"tmax": float("nan")}, {"tex": None}, {"sem": -1}):
        assert smooth(**kw) not in (0, -2), kw
    for kw in ({"k": 0}, {"k": -9}, {"gw": float("nan")}, {"dst": img}):
        assert texture(**kw) not in (0, -2), kw
    with pytest.raises(core.NoImplErr):
        stereo.disparity_median_filter(d, MAX_KERNEL + 2)
    with pytest.raises(core.ArgumentErr):
        stereo.disparity_median_filter(d, 5, "inplace")
    with pytest.raises(core.ArgumentErr):
        stereo.texture_preserving_disparity_filter(d, img[:, :-1], 0.15, 11)
    with pytest.raises(core.ArgumentErr):
        stereo.disparity_neighbor_filter(di, tiles=[(0, 0, 30, 30), (29, 0, 11, 30)])
    # in place through the C entry: out == in is the reference's aliasing
    inplace = d.copy()
    assert L.vwgpu_disparity_median_filter(H, inplace.ctypes.data, 40, 30, 0, 5, 0, whole.ctypes.data, 1, inplace.ctypes.data, 0,
                                           None) == 0
    _equal(inplace, dfr.disparity_median_filter(d.copy(), 5, "reference"))


# ---- the C++ surface ---------------------------------------------------------------------------------------------

def test_cpp_surface_and_buffer_sharing(tmp_path):
    """vwlite's four functions equal the Python calls; the program itself exits with 4 unless disparity_out shares
    disparity_in's buffer exactly in reference semantics."""
    exe = dfr.build_view_program()
    d = dfr.float_scene(70, 50, seed=80)
    d[np.isnan(d)] = 0
    di = dfr.int_scene(70, 50, seed=81)
    img = dfr.image_scene(70, 50, seed=82)
    tex = (img / 1000).astype(np.float32)
    p = {n: str(tmp_path / (n + ".pfm")) for n in ("d", "di", "img", "tex", "out")}
    write_pfm(p["d"], d)
    write_pfm(p["di"], di.astype(np.float32))
    write_pfm(p["img"], img)
    write_pfm(p["tex"], tex)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout + r.stderr

    def same(got, want):
        v = want[..., 2] != 0
        return np.array_equal(got[..., 2] != 0, v) and np.array_equal(got[v][:, :2], want[v][:, :2].astype(np.float32))

    for snap, sem in ((0, "reference"), (1, "snapshot")):
        rc, msg = run("median", p["d"], p["out"], 9, snap)
        assert rc == 0, msg
        assert same(read_pfm(p["out"]), stereo.disparity_median_filter(d, 9, sem))
        rc, msg = run("neighbor", p["di"], p["out"], snap)
        assert rc == 0, msg
        assert same(read_pfm(p["out"]), stereo.disparity_neighbor_filter(di, sem))
        rc, msg = run("smooth", p["d"], p["out"], p["tex"], 0.15, 11, snap)
        assert rc == 0, msg
        assert same(read_pfm(p["out"]), stereo.texture_preserving_disparity_filter(d, tex, 0.15, 11, sem))
    rc, msg = run("texture", p["img"], p["out"], 9, 0.5, 0.5)
    assert rc == 0, msg
    assert np.array_equal(read_pfm(p["out"]), stereo.texture_measure(img, 9))
    assert run("median", p["d"], p["out"], MAX_KERNEL + 2, 0)[0] == 3


# ---- 4096^2 ------------------------------------------------------------------------------------------------------

def _sampled_boxes():
    boxes = stereo.subpixel_tiles(4096, 4096, (1024, 1024))
    return boxes, [tuple(boxes[0]), tuple(boxes[6])]      # a corner and an interior box


def _tile(img, shape):
    reps = [-(-shape[0] // img.shape[0]), -(-shape[1] // img.shape[1])] + [1] * (img.ndim - 2)
    return np.ascontiguousarray(np.tile(img, reps)[:shape[0], :shape[1]])


@pytest.mark.parametrize("sem", SEM)
def test_4096_median_and_smoothing_on_sampled_boxes(sem):
    d = _tile(dfr.float_scene(1111, 1033, seed=90), (4096, 4096))
    tex = _tile((dfr.image_scene(1111, 1033, seed=91) / 1000).astype(np.float32), (4096, 4096))
    _, sample = _sampled_boxes()
    got_m = stereo.disparity_median_filter(d, 5, sem, block_size=(1024, 1024))
    got_s = stereo.texture_preserving_disparity_filter(d, tex, 0.15, 11, sem, block_size=(1024, 1024))
    for (x, y, w, h) in sample:
        crop = np.ascontiguousarray(d[y:y + h, x:x + w])
        _equal(np.ascontiguousarray(got_m[y:y + h, x:x + w]), dfr.disparity_median_filter(crop.copy(), 5, sem), "median box (%d, %d)" % (x, y))
        want = dfr.texture_preserving_disparity_filter(crop.copy(), np.ascontiguousarray(tex[y:y + h, x:x + w]), 0.15, 11, sem)
        _equal(np.ascontiguousarray(got_s[y:y + h, x:x + w]), want, "smoothing box (%d, %d)" % (x, y))


@pytest.mark.parametrize("sem", SEM)
def test_4096_neighbour_on_sampled_boxes(sem):
    d = _tile(dfr.int_scene(1111, 1033, seed=92), (4096, 4096))
    _, sample = _sampled_boxes()
    got = stereo.disparity_neighbor_filter(d, sem, block_size=(1024, 1024))
    for (x, y, w, h) in sample:
        want = dfr.disparity_neighbor_filter(np.ascontiguousarray(d[y:y + h, x:x + w]), sem)
        _equal(np.ascontiguousarray(got[y:y + h, x:x + w]), want, "neighbour box (%d, %d)" % (x, y))


def test_4096_texture_measure_on_sampled_boxes():
    img = _tile(dfr.image_scene(1111, 1033, seed=93), (4096, 4096))
    _, sample = _sampled_boxes()
    got = stereo.texture_measure(img, 9, block_size=(1024, 1024))
    for (x, y, w, h) in sample:
        want = dfr.texture_measure(np.ascontiguousarray(img[y:y + h, x:x + w]), 9)
        assert np.array_equal(got[y:y + h, x:x + w], want), "texture box (%d, %d)" % (x, y)
