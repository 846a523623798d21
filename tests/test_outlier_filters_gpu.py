"""GPU: stereo.rm_outliers_using_mean / _stddev / _plane, their clean-up compositions and std_dev_image (libvwgpu.so,
outlier_filters.hip) equal to the CPU restatement tests/refimpl/outlier_filters_ref.cc at every pixel, values (==) and
validity, no tolerance: both pixel types, both mean semantics, with and without clean-up, the rejection counts; host
and device entries; strided images; a device-resident chain; the C++ surface; limits and argument errors; one
1024 x 768 run per method compared in full."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import outlier_filters_ref as ofr  # noqa: E402
from affine_ref import read_pfm, write_pfm  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import core, stereo, synth  # noqa: E402

pytestmark = pytest.mark.gpu
TYPES = [np.int32, np.float32]
MAX_HALF = 15       # the documented maximum of half_h, half_v
MAX_STD_DEV = 31    # ... and of std_dev_image's kernel sizes
METHODS = {"mean": 0, "stddev": 1, "plane": 2}
PLAIN = {"mean": stereo.rm_outliers_using_mean, "stddev": stereo.rm_outliers_using_stddev, "plane": stereo.rm_outliers_using_plane}
CLEAN = {"mean": stereo.disparity_cleanup_using_mean, "stddev": stereo.disparity_cleanup_using_stddev,
         "plane": stereo.disparity_clean_using_plane}
ARGS = {"mean": (1.0,), "stddev": (1.5, 0.3), "plane": (1.5, 0.2)}
HALVES = [(1, 1), (2, 1), (1, 3), (5, 5)]


def _equal(got, want, what=""):
    """values (==) at valid pixels, validity everywhere; stored values of invalid pixels are copies of the input's"""
    assert got.shape == want.shape and got.dtype == want.dtype
    vg, vw = got[..., 2] != 0, want[..., 2] != 0
    bad = (vg != vw) | (vg & vw & ((got[..., 0] != want[..., 0]) | (got[..., 1] != want[..., 1])))
    diff = np.argwhere(bad)
    assert len(diff) == 0, "%s: %d pixels differ, first at %s: got %s want %s" % (
        what, len(diff), diff[0], got[tuple(diff[0])], want[tuple(diff[0])])
    assert np.array_equal(got[~vg].view(np.uint32), want[~vw].view(np.uint32)), what + ": invalid pixels are not copies"


def _scene(dtype, w, h, seed):
    return ofr.float_scene(w, h, seed) if dtype == np.float32 else ofr.int_scene(w, h, seed)


def _check(method, d, half, cleanup, sem="reference", args=None):
    args = ARGS[method] if args is None else args
    kw = {"semantics": sem} if method == "mean" else {}
    sw, sg = [], []
    want = ofr.rm_outliers(method, d, half[0], half[1], *args, cleanup=cleanup, semantics=sem, stats=sw)
    got = (CLEAN if cleanup else PLAIN)[method](d, half[0], half[1], *args, stats=sg, **kw)
    _equal(got, want, "%s %s half %s cleanup %d %s %dx%d" % (method, d.dtype, half, cleanup, sem, d.shape[1], d.shape[0]))
    assert sg == sw
    return got, sg


def _semantics(method):
    return ("reference", "skip") if method == "mean" else ("reference",)


# ---- every method, pixel type, window and tiling ------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("cleanup", [0, 1])
@pytest.mark.parametrize("method", list(METHODS))
def test_windows_and_tilings(method, cleanup, dtype):
    """37 x 29 and 70 x 45: partial tiles, more than one tile each way; the integer scene holds planted 1e6 outliers."""
    rejected = 0
    for (w, h), seed in (((37, 29), 3), ((70, 45), 4)):
        d = _scene(dtype, w, h, seed)
        for half in HALVES:
            for sem in _semantics(method):
                rejected += _check(method, d, half, cleanup, sem)[1][0]
    assert rejected > 0


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("method", list(METHODS))
def test_largest_window(method, dtype):
    d = _scene(dtype, 52, 40, 5)
    for sem in _semantics(method):
        _check(method, d, (MAX_HALF, MAX_HALF), 0, sem)
        _check(method, d, (MAX_HALF, 2), 1, sem)
        _check(method, d, (3, MAX_HALF), 1, sem)


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("method", list(METHODS))
def test_small_images_clamp_on_both_sides(method, dtype):
    for (w, h), half in (((5, 4), (3, 3)), ((1, 1), (1, 1)), ((1, 1), (5, 5)), ((2, 9), (4, 1)), ((17, 1), (2, 2))):
        d = _scene(dtype, w, h, 6 + w)
        d[0, 0, 2] = 1
        for cleanup in (0, 1):
            for sem in _semantics(method):
                _check(method, d, half, cleanup, sem, args=(0.4,) if method == "mean" else (1.0, 0.05))


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("method", list(METHODS))
def test_all_invalid_block_with_single_valid_pixels(method, dtype):
    """Windows that hold one valid pixel, a row or a column of them: zero pivots of the plane fit, sigma 0, and lone
    pixels that only the clean-up pass removes."""
    d = ofr.sparse_scene(48, 40, dtype, seed=7)
    second = 0
    for half in ((1, 1), (2, 3), (5, 5)):
        for sem in _semantics(method):
            _check(method, d, half, 0, sem)
            second += _check(method, d, half, 1, sem)[1][1]
    assert second > 0


@pytest.mark.parametrize("method", list(METHODS))
def test_mean_semantics_differ_and_other_methods_ignore_them(method):
    d = ofr.int_scene(70, 45, 4)
    ctx = core.default_context(0)
    outs = []
    for sem in (0, 1):
        out = np.empty_like(d)
        assert ctx._lib.vwgpu_rm_outliers(ctx._h, METHODS[method], 0, d.ctypes.data, 70, 45, 0, 2, 2, 1.0, 0.3, 0, sem,
                                          out.ctypes.data, 0, None) == 0
        outs.append(out)
    assert np.array_equal(outs[0], outs[1]) == (method != "mean")


def test_nan_among_valid_disparities_leaves_the_mean_window_alone():
    d = ofr.float_scene(40, 30, 8, hole=False)
    d[10, 10] = (np.nan, 1.0, 1)
    for sem in ("reference", "skip"):
        got = stereo.rm_outliers_using_mean(d, 2, 2, 0.5, semantics=sem)
        want = ofr.rm_outliers("mean", d, 2, 2, 0.5, semantics=sem)
        near = d[8:13, 8:13, 2] != 0
        assert np.array_equal(got[8:13, 8:13][near].view(np.uint32), d[8:13, 8:13][near].view(np.uint32))
        assert np.isnan(got[10, 10, 0]) and np.isnan(want[10, 10, 0])
        got[10, 10, 0] = want[10, 10, 0] = 0
        _equal(got, want, "mean with a valid NaN")
    for method in ("stddev", "plane"):      # NaN flows through the dx arithmetic, whose comparisons are then false
        got = PLAIN[method](d, 2, 2, *ARGS[method])
        want = ofr.rm_outliers(method, d, 2, 2, *ARGS[method])
        assert np.array_equal(got[..., 2], want[..., 2])
        got[10, 10, 0] = want[10, 10, 0] = 0
        _equal(got, want, method + " with a valid NaN")


# ---- entries: strided, host and device, chain ---------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TYPES)
def test_strided_input_and_output_through_the_c_entry(dtype):
    import torch
    w, h, stride = 37, 29, 37 + 5
    d = _scene(dtype, w, h, 9)
    ctx = core.default_context(0)
    L, H = ctx._lib, ctx._h
    tcode = 0 if dtype == np.int32 else 1
    src = np.full((h, stride, 3), 7, dtype)
    src[:, :w] = d
    for method, code in METHODS.items():
        for cleanup in (0, 1):
            want = ofr.rm_outliers(method, d, 2, 3, *ARGS[method], cleanup=cleanup)
            p = ARGS[method] + (0.0,)
            dst = np.full((h, stride, 3), -5, dtype)
            st = (ctypes.c_longlong * 2)()
            assert L.vwgpu_rm_outliers(H, code, tcode, src.ctypes.data, w, h, stride, 2, 3, p[0], p[1], cleanup, 0, dst.ctypes.data,
                                       stride, st) == 0
            _equal(np.ascontiguousarray(dst[:, :w]), want, "%s strided host" % method)
            assert (dst[:, w:] == -5).all()
            ts = torch.from_numpy(src).cuda()
            td = torch.full((h, stride, 3), -5, dtype=ts.dtype, device="cuda")
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            st2 = (ctypes.c_longlong * 2)()
            assert L.vwgpu_rm_outliers_dev(H, code, tcode, ts.data_ptr(), w, h, stride, 2, 3, p[0], p[1], cleanup, 0, td.data_ptr(),
                                           stride, st2) == 0
            torch.cuda.synchronize()
            assert np.array_equal(td.cpu().numpy(), dst) and list(st2) == list(st)
    img = ofr.image_scene(w, h, 10)
    simg = np.full((h, stride), 3, np.float32)
    simg[:, :w] = img
    dst = np.full((h, stride), -5, np.float32)
    assert L.vwgpu_std_dev_image(H, simg.ctypes.data, w, h, stride, 5, 3, 1, dst.ctypes.data, stride) == 0
    assert np.array_equal(dst[:, :w], ofr.std_dev_image(img, 5, 3, "zero")) and (dst[:, w:] == -5).all()


@pytest.mark.parametrize("dtype", TYPES)
def test_device_entries_equal_host_entries(dtype):
    import torch
    d = _scene(dtype, 70, 45, 11)
    dt = torch.from_numpy(d).cuda()
    keep = dt.clone()
    for method in METHODS:
        for fn in (PLAIN[method], CLEAN[method]):
            sh, sd = [], []
            host = fn(d, 2, 2, *ARGS[method], stats=sh)
            dev = fn(dt, 2, 2, *ARGS[method], stats=sd)
            torch.cuda.synchronize()
            assert dev.is_cuda and dev.dtype == dt.dtype
            _equal(dev.cpu().numpy(), host, method)
            assert sh == sd
    assert torch.equal(dt, keep)                                  # the Python surface leaves its input alone
    img = ofr.image_scene(70, 45, 12)
    dev = stereo.std_dev_image(torch.from_numpy(img).cuda(), 7, 4, "constant")
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), stereo.std_dev_image(img, 7, 4, "constant"))
    with pytest.raises(core.ArgumentErr):
        stereo.rm_outliers_using_mean(dt.double(), 2, 2, 1.0)
    with pytest.raises(core.ArgumentErr):
        stereo.rm_outliers_using_mean(d.astype(np.float64), 2, 2, 1.0)


def test_device_resident_chain_subpixel_then_cleanup():
    """pyramid_subpixel -> disparity_cleanup_using_stddev on device tensors, no host copy in between, equals the chain
    through host arrays, whose second step equals the restatement."""
    import torch
    left, right, truth = synth.stereo_pair(128, 96, 9, 1, block=64)
    d = np.zeros((96, 128, 3), np.float32)
    d[..., 0] = truth
    d[..., 2] = 1
    d[::7, ::5, 0] += 1                                           # coarse errors for the refiner and the filter
    d[40:50, 30:60, 2] = 0

    def chain(disp, l, r):
        sub = stereo.pyramid_subpixel(disp, l, r, 2, 1.4, (7, 7), 1)
        st = []
        return sub, stereo.disparity_cleanup_using_stddev(sub, 3, 3, 1.5, 0.1, stats=st), st

    host_sub, host, sh = chain(d, left, right)
    dev_sub, dev, sd = chain(torch.from_numpy(d).cuda(), torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda())
    torch.cuda.synchronize()
    assert dev_sub.is_cuda and dev.is_cuda
    _equal(dev_sub.cpu().numpy(), host_sub, "sub-pixel step")
    _equal(dev.cpu().numpy(), host, "chain")
    sw = []
    _equal(host, ofr.rm_outliers("stddev", host_sub, 3, 3, 1.5, 0.1, cleanup=True, stats=sw), "second step")
    assert sh == sd == sw and (host_sub[..., 2] != 0).sum() > 1000 and sh[0] > 0


# ---- std_dev_image ------------------------------------------------------------------------------------------------

def _same_floats(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), what + ": NaN positions differ"
    ok = ~np.isnan(want)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    bad = [b for b in bad if ok[tuple(b)]]
    assert not bad, "%s: %d pixels differ, first at %s" % (what, len(bad), bad[0])


@pytest.mark.parametrize("edge", ["zero", "constant"])
def test_std_dev_image_sizes_and_edges(edge):
    for (w, h), seed in (((37, 29), 13), ((70, 45), 14), ((5, 4), 15), ((1, 1), 16)):
        img = ofr.image_scene(w, h, seed)
        for kw, kh in ((1, 1), (2, 2), (3, 3), (4, 4), (7, 7), (31, 31), (2, 7), (31, 1), (4, 3)):
            _same_floats(stereo.std_dev_image(img, kw, kh, edge), ofr.std_dev_image(img, kw, kh, edge),
                         "std_dev_image %dx%d %s on %dx%d" % (kw, kh, edge, w, h))
    assert np.isnan(stereo.std_dev_image(ofr.image_scene(20, 10, 17), 1, 1, edge)).all()


# ---- limits and errors through the raw C entry -----------------------------------------------------------------

def test_limits_and_argument_errors():
    d = ofr.float_scene(40, 30, seed=70)
    di = ofr.int_scene(40, 30, seed=71)
    img = ofr.image_scene(40, 30, seed=72)
    out, outf = np.full_like(d, 9), np.full_like(img, 9)
    ctx = core.default_context(0)
    L, H = ctx._lib, ctx._h
    nan = float("nan")

    def rm(method=0, tcode=1, src=d, w=40, h=30, istride=0, hh=2, hv=2, p0=1.0, p1=0.2, cleanup=0, sem=0, dst=out, ostride=0):
        return L.vwgpu_rm_outliers(H, method, tcode, None if src is None else src.ctypes.data, w, h, istride, hh, hv, p0, p1, cleanup,
                                   sem, None if dst is None else dst.ctypes.data, ostride, None)

    def sd(src=img, w=40, h=30, stride=0, kw=3, kh=3, edge=1, dst=outf, ostride=0):
        return L.vwgpu_std_dev_image(H, None if src is None else src.ctypes.data, w, h, stride, kw, kh, edge,
                                     None if dst is None else dst.ctypes.data, ostride)

    for m in (0, 1, 2):
        assert rm(method=m) == 0 and rm(method=m, hh=MAX_HALF, hv=MAX_HALF) == 0
        assert rm(method=m, hh=MAX_HALF + 1) == -2 and rm(method=m, hv=MAX_HALF + 1, cleanup=1) == -2       # NOIMPL
        for kw in ({"hh": 0}, {"hv": 0}, {"hh": -3}, {"p0": nan}, {"dst": d}, {"src": None}, {"dst": None}, {"w": 0}, {"h": -1},
                   {"istride": 39}, {"ostride": 39}, {"sem": 2}, {"sem": -1}, {"tcode": 2}):
            assert rm(method=m, **kw) == -1, (m, kw)
        assert (rm(method=m, p1=nan) == -1) == (m != 0)           # the mean filter takes one threshold
    assert rm(method=0, hh=0) == -1 and L.vwgpu_last_error(H) == b"RmOutliersUsingMeanFunc: half kernel sizes must be non-zero."
    assert rm(method=2, hv=0) == -1 and L.vwgpu_last_error(H) == b"RmOutliersFunc: half kernel sizes must be non-zero."
    assert rm(method=3) == -1 and rm(method=-1) == -1
    assert rm(tcode=0, src=di, dst=np.empty_like(di)) == 0
    assert (out == 9).sum() == 0                                  # the successful calls wrote every pixel ...
    out[:] = 9
    for kw in ({"hh": 0}, {"hh": MAX_HALF + 1}, {"p0": nan}, {"sem": 2}):
        rm(**kw)
    assert (out == 9).all()                                       # ... and a refused call none: reported before any launch
    assert sd() == 0 and sd(kw=MAX_STD_DEV, kh=MAX_STD_DEV) == 0 and sd(edge=0) == 0
    assert sd(kw=MAX_STD_DEV + 1) == -2 and sd(kh=MAX_STD_DEV + 1) == -2
    for kw in ({"kw": 0}, {"kh": 0}, {"kw": -5}, {"edge": 2}, {"dst": img}, {"src": None}, {"dst": None}, {"w": 0}, {"stride": 39},
               {"ostride": 39}):
        assert sd(**kw) == -1, kw
    assert sd(kw=0) == -1 and L.vwgpu_last_error(H) == b"StdDevImageFunc: kernel sizes must be non-zero."
    for fn in list(PLAIN.values()) + list(CLEAN.values()):
        with pytest.raises(core.ArgumentErr):
            fn(d, 0, 2, 1.0) if fn in (stereo.rm_outliers_using_mean, stereo.disparity_cleanup_using_mean) else fn(d, 0, 2, 1.0, 0.2)
        with pytest.raises(core.NoImplErr):
            fn(d, 2, MAX_HALF + 1, 1.0) if fn in (stereo.rm_outliers_using_mean, stereo.disparity_cleanup_using_mean) \
                else fn(d, 2, MAX_HALF + 1, 1.0, 0.2)
    with pytest.raises(core.ArgumentErr):
        stereo.rm_outliers_using_mean(d, 2, 2, 1.0, semantics="snapshot")
    with pytest.raises(core.ArgumentErr):
        stereo.rm_outliers_using_stddev(d, 2, 2, nan, 0.2)
    with pytest.raises(core.ArgumentErr):
        stereo.rm_outliers_using_plane(d[..., :2], 2, 2, 1.0, 0.2)
    with pytest.raises(core.ArgumentErr):
        stereo.std_dev_image(img, 0, 3)
    with pytest.raises(core.ArgumentErr):
        stereo.std_dev_image(img, 3, 3, edge="reflect")
    with pytest.raises(core.NoImplErr):
        stereo.std_dev_image(img, 3, MAX_STD_DEV + 1)


# ---- the C++ surface ---------------------------------------------------------------------------------------------

def test_cpp_surface(tmp_path):
    """vwlite's seven functions on both pixel types equal the Python calls."""
    exe = ofr.build_view_program()
    d = ofr.float_scene(70, 50, seed=80)
    di = ofr.int_scene(70, 50, seed=81, huge=5000)
    img = ofr.image_scene(70, 50, seed=82)
    p = {n: str(tmp_path / (n + ".pfm")) for n in ("d", "di", "img", "out")}
    write_pfm(p["d"], d)
    write_pfm(p["di"], di.astype(np.float32))
    write_pfm(p["img"], img)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout + r.stderr

    def same(got, want):
        v = want[..., 2] != 0
        return np.array_equal(got[..., 2] != 0, v) and np.array_equal(got[v][:, :2], want[v][:, :2].astype(np.float32))

    for method in METHODS:
        a = ARGS[method] + (0.0,)
        for cleanup in (0, 1):
            for is_int, src, key in ((0, d, "d"), (1, di, "di")):
                for ref_loop in ((1, 0) if (method, cleanup, is_int) == ("mean", 0, 1) else (1,)):
                    rc, msg = run(method, p[key], p["out"], 3, 2, a[0], a[1], cleanup, is_int, ref_loop)
                    assert rc == 0, msg
                    kw = {"semantics": "reference" if ref_loop else "skip"} if method == "mean" else {}
                    want = (CLEAN if cleanup else PLAIN)[method](src, 3, 2, *ARGS[method], **kw)
                    assert same(read_pfm(p["out"]), want), (method, cleanup, is_int, ref_loop)
    for zero in (1, 0):
        rc, msg = run("stddev_image", p["img"], p["out"], 5, 4, zero)
        assert rc == 0, msg
        assert np.array_equal(read_pfm(p["out"]), stereo.std_dev_image(img, 5, 4, "zero" if zero else "constant"))
    assert run("plane", p["d"], p["out"], MAX_HALF + 1, 2, 1.5, 0.2, 0, 0, 1)[0] == 3
    assert run("mean", p["d"], p["out"], 0, 2, 1.5, 0.0, 0, 0, 1)[0] == 1


# ---- 1024 x 768 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("method", list(METHODS))
def test_1024x768_at_11x11_in_full(method):
    d = ofr.float_scene(1024, 768, seed=90)
    got, st = _check(method, d, (5, 5), 1)
    assert st[0] > 0 and st[1] > 0
