"""GPU: get_disparity_range, disparity_range_mask, both transform_disparities overloads, disparity_subsample /
_upsample, transform(right, DisparityTransform(d)), missing_pixel_image and intersect_mask_and_data (libvwgpu.so,
disparity_map.hip) equal to the CPU restatement tests/refimpl/disparity_map_ref.cc at every pixel, values (==) and
validity, no tolerance: both pixel types, sizes with partial and several workgroups, reduction sizes across workgroup
and grid-stride boundaries, host and device entries, strided images, in-place calls, tiles and row strips through
x0 / y0, a device-resident chain, the C++ surface, argument errors, one 1024 x 768 run per operator."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import disparity_map_ref as ref  # noqa: E402
from affine_ref import read_pfm, write_pfm  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import core, stereo, synth  # noqa: E402

pytestmark = pytest.mark.gpu
TYPES = [np.int32, np.float32]
SIZES = [(37, 29), (70, 45), (1, 1), (2, 9), (17, 1)]
MATRICES = {"identity": np.eye(3), "translation": ref.inverse3(ref.TRANSLATION), "affine": ref.inverse3(ref.AFFINE),
            "projective": ref.PROJECTIVE}
ERR_ARGUMENT = -1


def same(got, want, what=""):
    """Exact equality of every word (values, mask words, stored values of invalid pixels); NaNs by position."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    eq = (got == want)
    if got.dtype.kind == "f":
        eq |= np.isnan(got) & np.isnan(want)
    bad = np.argwhere(~eq)
    assert len(bad) == 0, "%s: %d words differ, first at %s: got %s want %s" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def bounds(w, h):
    """min / max of the range mask for a scene of w x h at origin (5, 4): pixels on both sides of every bound."""
    return (3, 6), (w + 4, h + 3)


# ---- every operator, pixel type and size ----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TYPES, ids=["i32", "f32"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_operators_equal_restatement(dtype, size):
    w, h = size
    d = ref.scene(w, h, dtype, seed=21)
    what = "%s %dx%d" % (np.dtype(dtype).name, w, h)
    same(stereo.get_disparity_range(d), ref.get_disparity_range(d), "range " + what)
    mn, mx = bounds(w, h)
    for sem in ("reference", "fixed"):
        sg, sw = [], []
        same(stereo.disparity_range_mask(d, mn, mx, sem, 5, 4, stats=sg), ref.disparity_range_mask(d, mn, mx, sem, 5, 4, stats=sw),
             "mask %s %s" % (sem, what))
        assert sg == sw
    for name, m in MATRICES.items():
        same(stereo.transform_disparities(d, m, 3, 7), ref.transform_disparities(d, m, "functor", 3, 7), "transform %s %s" % (name, what))
        box = vwa.BBox2i(-6, 2, w, h)
        for do_round in (False, True):
            same(stereo.transform_disparities_subregion(do_round, box, m, d),
                 ref.transform_disparities(d, m, "subregion_round" if do_round else "subregion", -6, 2),
                 "subregion %s round %d %s" % (name, do_round, what))
    same(stereo.disparity_subsample(d), ref.disparity_subsample(d), "subsample " + what)
    same(stereo.disparity_upsample(d), ref.disparity_upsample(d), "upsample " + what)
    same(stereo.missing_pixel_image(d), ref.missing_pixel_image(d), "missing " + what)
    other = ref.scene(w, h, dtype, seed=22)
    same(stereo.intersect_mask_and_data(d, other), ref.intersect_mask_and_data(d, other), "intersect " + what)


@pytest.mark.parametrize("dtype", TYPES, ids=["i32", "f32"])
def test_range_mask_masks_and_keeps(dtype):
    """The scenes are chosen so that the mask removes pixels and keeps pixels, and the two semantics differ."""
    for w, h in ((37, 29), (70, 45)):
        d = ref.scene(w, h, dtype, seed=21)
        mn, mx = bounds(w, h)
        counts = {}
        for sem in ("reference", "fixed"):
            sw, sg = [], []
            want = ref.disparity_range_mask(d, mn, mx, sem, 5, 4, stats=sw)
            kept = int(((want[..., 2] != 0)).sum())
            assert sw[0] > 0 and kept > 0 and sw[0] + kept == int((d[..., 2] != 0).sum())
            same(stereo.disparity_range_mask(d, mn, mx, sem, 5, 4, stats=sg), want, sem)
            assert sg == sw
            counts[sem] = sw[0]
        assert counts["fixed"] > counts["reference"]      # min[1] = 6 > min[0] = 3 removes more rows of targets


def test_range_mask_semantics_differ_on_a_built_scene():
    d = np.array([[(1, 2, 1), (1, 7, 1)]], np.float32)          # lands on y = 2 and y = 7; min = (0, 5)
    same(stereo.disparity_range_mask(d, (0, 5), (100, 100), "reference"), d)
    got = stereo.disparity_range_mask(d, (0, 5), (100, 100), "fixed")
    assert got[0, 0].tolist() == [0, 0, 0] and got[0, 1].tolist() == [1, 7, 1]
    # max - 1 in the channel type: (float)2^24 - 1
    f = np.array([[(16777214, 0, 1), (16777214, 0, 1)]], np.float32)
    assert stereo.disparity_range_mask(f, (0, 0), (16777216, 10))[0, :, 2].tolist() == [1, 0]


def test_identity_leaves_float_disparities_unchanged():
    d = ref.float_scene(70, 45, seed=23)
    same(stereo.transform_disparities(d, np.eye(3)), d)
    same(stereo.transform_disparities(d, stereo.HomographyTransform(np.eye(3))), d)


def test_homography_helper_applies_the_inverse():
    d = ref.float_scene(37, 29, seed=24)
    h = stereo.HomographyTransform(ref.AFFINE)
    same(stereo.transform_disparities(d, h), ref.transform_disparities(d, h.inverse_matrix))
    same(stereo.transform_disparities(d, h), stereo.transform_disparities(d, h.inverse_matrix))


# ---- the reduction --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TYPES, ids=["i32", "f32"])
@pytest.mark.parametrize("size", [(1, 1), (257, 3), (1000, 7), (900, 700)], ids=lambda s: "%dx%d" % s)
def test_range_reduction_sizes(dtype, size):
    """1, just above 256 and 3 x 256 pixels, 7000 pixels (28 workgroups), 630000 (above the 2048 x 256 lanes of the
    largest grid: the stride loop runs twice for some lanes)."""
    w, h = size
    d = ref.scene(w, h, dtype, seed=31)
    same(stereo.get_disparity_range(d), ref.get_disparity_range(d))
    e = d.copy()
    e[..., 2] = 0                                                   # no valid pixel
    assert stereo.get_disparity_range(e).tolist() == [0, 0, 0, 0]
    e[-1, -1] = (-77, 55, 1)                                        # one valid pixel, in the last position
    assert stereo.get_disparity_range(e).tolist() == [-77, 55, -77, 55]
    if w * h > 1:
        e = d.copy()
        e[0, 0] = (1000, -1000, 1)                                  # the extrema in the first and the last pixel
        e[-1, -1] = (-1000, 1000, 1)
        assert stereo.get_disparity_range(e).tolist() == [-1000, -1000, 1000, 1000]


@pytest.mark.parametrize("size", [(1, 1), (257, 3), (1000, 7)], ids=lambda s: "%dx%d" % s)
def test_range_nan_in_first_valid_pixel(size):
    w, h = size
    d = ref.float_scene(w, h, seed=32)
    flat = d.reshape(-1, 3)
    first = int(np.argmax(flat[:, 2] != 0)) if (flat[:, 2] != 0).any() else 0
    e = d.copy()
    e.reshape(-1, 3)[first] = (np.nan, 2, 1)
    got, want = stereo.get_disparity_range(e), ref.get_disparity_range(e)
    assert np.isnan(want[0]) and np.isnan(want[2])
    same(got, want)
    if w * h > 1:
        e = d.copy()
        e[..., 2] = 1
        e.reshape(-1, 3)[w * h // 2] = (np.nan, np.nan, 1)          # later than the first: ignored
        got, want = stereo.get_disparity_range(e), ref.get_disparity_range(e)
        assert not np.isnan(want).any()
        same(got, want)
        e.reshape(-1, 3)[0] = (3, np.nan, 1)
        same(stereo.get_disparity_range(e), ref.get_disparity_range(e))


# ---- the warp -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [((37, 29), (37, 29)), ((37, 29), (20, 33)), ((24, 18), (70, 45)), ((1, 1), (3, 2)), ((17, 1), (2, 9))],
                         ids=["equal", "smaller", "larger", "one", "line"])
def test_warp(sizes):
    """Fractional offsets, integer offsets (the shortcut), offsets that lead outside, invalid offsets; a disparity map
    smaller than, equal to and larger than the right image."""
    (rw, rh), (dw, dh) = sizes
    right, d = ref.image_scene(rw, rh), ref.warp_scene(dw, dh)
    want = ref.disparity_transform_image(right, d)
    same(stereo.disparity_transform_image(right, d), want)
    if rw > 1 and rh > 1:
        assert (want != 0).any() and (want == 0).any()


def test_warp_hand_cases():
    right = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.float32)
    d = np.zeros((3, 3, 3), np.float32)
    d[..., 2] = 1
    d[1, 1] = (1, 0, 1)
    d[0, 0] = (-1, 0, 1)
    d[2, 2] = (0, 0, 0)
    d[1, 0] = (0.5, 0, 1)
    d[0, 1] = (np.nan, 0, 1)
    d[0, 2] = (3e9, 0, 1)
    got = stereo.disparity_transform_image(right, d)
    same(got, ref.disparity_transform_image(right, d))
    assert got[1, 1] == 6 and got[0, 0] == 0 and got[2, 2] == 0 and got[1, 0] == 4.5 and got[0, 1] == 0 and got[0, 2] == 0


# ---- round trips ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", TYPES, ids=["i32", "f32"])
def test_resampling_round_trip_and_edge_clamp(dtype):
    for w, h in ((37, 29), (70, 45), (5, 1), (1, 6)):
        d = ref.scene(w, h, dtype, seed=41)
        s = stereo.disparity_subsample(d)
        assert s.shape == (1 + (h - 1) // 2, 1 + (w - 1) // 2, 3)
        u = stereo.disparity_upsample(s)
        assert u.shape == (2 * s.shape[0], 2 * s.shape[1], 3)
        same(u, ref.disparity_upsample(ref.disparity_subsample(d)))
    # an odd size: the last output sits on the last pixel and its +1 taps clamp onto it
    d = np.zeros((1, 3, 3), dtype)
    d[0, 2] = (8, -6, 1)
    s = stereo.disparity_subsample(d)
    same(s, ref.disparity_subsample(d))
    assert s[0, 1, :2].tolist() == [4, -3] and s[0, 1, 2] != 0      # 8 * (10 + 5 + 5 + 5 + 2 + 2) / (2 * 29)
    assert s[0, 0].tolist() == [0, 0, 0]                            # its taps reach column 1 at most


# ---- entries and layout ---------------------------------------------------------------------------------------------

def _raw(ctx):
    return ctx._lib, ctx._h


@pytest.mark.parametrize("dtype", TYPES, ids=["i32", "f32"])
def test_strided_and_in_place_host_entries(dtype):
    """Row strides larger than the width on inputs and outputs; the padding of the output stays untouched; in == out
    where it is allowed."""
    w, h, si, so = 37, 29, 45, 41
    t = 0 if dtype == np.int32 else 1
    d = ref.scene(w, h, dtype, seed=51)
    other = ref.scene(w, h, dtype, seed=52)
    wide = np.full((h, si, 3), 7, dtype)
    wide[:, :w] = d
    wide_other = np.full((h, si, 3), 5, dtype)
    wide_other[:, :w] = other
    L, H = _raw(core.default_context(0))
    mn, mx = np.array(bounds(w, h)[0], np.float64), np.array(bounds(w, h)[1], np.float64)
    m = np.ascontiguousarray(MATRICES["projective"])

    def fresh(cols=so, rows=h, dt=dtype):
        return np.full((rows, cols, 3), 9, dt)

    def inner(out, cols):
        assert (out[:, cols:] == 9).all()
        return np.ascontiguousarray(out[:, :cols])

    r = np.zeros(4, np.float32)
    assert L.vwgpu_get_disparity_range(H, t, wide.ctypes.data, w, h, si, r.ctypes.data) == 0
    same(r, ref.get_disparity_range(d))
    out = fresh()
    st = (ctypes.c_longlong * 1)()
    assert L.vwgpu_disparity_range_mask(H, t, wide.ctypes.data, w, h, si, 5, 4, mn.ctypes.data, mx.ctypes.data, 0, out.ctypes.data, so, st) == 0
    sw = []
    same(inner(out, w), ref.disparity_range_mask(d, mn, mx, "reference", 5, 4, stats=sw))
    assert [st[0]] == sw
    out = fresh()
    assert L.vwgpu_transform_disparities(H, t, wide.ctypes.data, w, h, si, 3, 7, m.ctypes.data, 0, out.ctypes.data, so) == 0
    same(inner(out, w), ref.transform_disparities(d, m, "functor", 3, 7))
    out = fresh()
    assert L.vwgpu_intersect_mask_and_data(H, t, wide.ctypes.data, si, wide_other.ctypes.data, si, w, h, out.ctypes.data, so) == 0
    same(inner(out, w), ref.intersect_mask_and_data(d, other))
    ow, oh = 1 + (w - 1) // 2, 1 + (h - 1) // 2
    out = fresh(ow + 3, oh)
    assert L.vwgpu_disparity_subsample(H, t, wide.ctypes.data, w, h, si, out.ctypes.data, ow + 3) == 0
    same(inner(out, ow), ref.disparity_subsample(d))
    out = fresh(2 * w + 5, 2 * h)
    assert L.vwgpu_disparity_upsample(H, t, wide.ctypes.data, w, h, si, out.ctypes.data, 2 * w + 5) == 0
    same(inner(out, 2 * w), ref.disparity_upsample(d))
    out = fresh(so, h, np.uint8)
    assert L.vwgpu_missing_pixel_image(H, t, wide.ctypes.data, w, h, si, out.ctypes.data, so) == 0
    same(inner(out, w), ref.missing_pixel_image(d))
    # in place, strided
    buf = wide.copy()
    assert L.vwgpu_disparity_range_mask(H, t, buf.ctypes.data, w, h, si, 5, 4, mn.ctypes.data, mx.ctypes.data, 1, buf.ctypes.data, si, None) == 0
    same(np.ascontiguousarray(buf[:, :w]), ref.disparity_range_mask(d, mn, mx, "fixed", 5, 4))
    assert (buf[:, w:] == 7).all()
    buf = wide.copy()
    assert L.vwgpu_transform_disparities(H, t, buf.ctypes.data, w, h, si, -6, 2, m.ctypes.data, 2, buf.ctypes.data, si) == 0
    same(np.ascontiguousarray(buf[:, :w]), ref.transform_disparities(d, m, "subregion_round", -6, 2))
    buf = wide.copy()
    assert L.vwgpu_intersect_mask_and_data(H, t, buf.ctypes.data, si, wide_other.ctypes.data, si, w, h, buf.ctypes.data, si) == 0
    same(np.ascontiguousarray(buf[:, :w]), ref.intersect_mask_and_data(d, other))


def test_strided_warp_host_entry():
    rw, rh, dw, dh = 37, 29, 30, 33
    right, d = ref.image_scene(rw, rh), ref.warp_scene(dw, dh)
    wr = np.full((rh, rw + 6), 3, np.float32)
    wr[:, :rw] = right
    wd = np.full((dh, dw + 2, 3), 4, np.float32)
    wd[:, :dw] = d
    out = np.full((rh, rw + 4), 9, np.float32)
    L, H = _raw(core.default_context(0))
    assert L.vwgpu_disparity_warp(H, wr.ctypes.data, rw, rh, rw + 6, wd.ctypes.data, dw, dh, dw + 2, out.ctypes.data, rw + 4) == 0
    same(np.ascontiguousarray(out[:, :rw]), ref.disparity_transform_image(right, d))
    assert (out[:, rw:] == 9).all()


@pytest.mark.parametrize("dtype", TYPES, ids=["i32", "f32"])
def test_device_entries(dtype):
    """CUDA tensors in, CUDA tensors out, equal to the host entries; strided and in-place device images through the raw
    entry; the range without a host copy."""
    import torch
    w, h = 70, 45
    d = ref.scene(w, h, dtype, seed=61)
    other = ref.scene(w, h, dtype, seed=62)
    dt, ot = torch.from_numpy(d).cuda(), torch.from_numpy(other).cuda()
    keep = dt.clone()
    mn, mx = bounds(w, h)
    m = MATRICES["affine"]
    sg, sw = [], []
    pairs = [
        (stereo.disparity_range_mask(dt, mn, mx, "reference", 5, 4, stats=sg), ref.disparity_range_mask(d, mn, mx, "reference", 5, 4, stats=sw)),
        (stereo.transform_disparities(dt, m, 3, 7), ref.transform_disparities(d, m, "functor", 3, 7)),
        (stereo.transform_disparities_subregion(True, vwa.BBox2i(-6, 2, w, h), m, dt), ref.transform_disparities(d, m, "subregion_round", -6, 2)),
        (stereo.disparity_subsample(dt), ref.disparity_subsample(d)),
        (stereo.disparity_upsample(dt), ref.disparity_upsample(d)),
        (stereo.missing_pixel_image(dt), ref.missing_pixel_image(d)),
        (stereo.intersect_mask_and_data(dt, ot), ref.intersect_mask_and_data(d, other)),
    ]
    r_dev = stereo.get_disparity_range(dt, device_result=True)
    torch.cuda.synchronize()
    for got, want in pairs:
        assert got.is_cuda
        same(got.cpu().numpy(), want)
    assert sg == sw
    assert r_dev.is_cuda
    same(r_dev.cpu().numpy(), ref.get_disparity_range(d))
    same(stereo.get_disparity_range(dt), ref.get_disparity_range(d))
    assert torch.equal(dt, keep)                                  # the Python surface leaves its input alone
    if dtype == np.float32:
        right = ref.image_scene(50, 40)
        got = stereo.disparity_transform_image(torch.from_numpy(right).cuda(), dt)
        assert got.is_cuda
        same(got.cpu().numpy(), ref.disparity_transform_image(right, d))
    # raw device entry: a strided image, masked in place
    ctx = core.default_context(0)
    L, H = _raw(ctx)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    wide = np.full((h, w + 8, 3), 7, dtype)
    wide[:, :w] = d
    wt = torch.from_numpy(wide).cuda()
    lo, hi = np.array(mn, np.float64), np.array(mx, np.float64)
    t = 0 if dtype == np.int32 else 1
    assert L.vwgpu_disparity_range_mask_dev(H, t, wt.data_ptr(), w, h, w + 8, 5, 4, lo.ctypes.data, hi.ctypes.data, 0, wt.data_ptr(), w + 8, None) == 0
    r = torch.empty(4, dtype=torch.float32, device="cuda")
    assert L.vwgpu_get_disparity_range_dev(H, t, wt.data_ptr(), w, h, w + 8, r.data_ptr(), None) == 0
    torch.cuda.synchronize()
    back = wt.cpu().numpy()
    masked = ref.disparity_range_mask(d, mn, mx, "reference", 5, 4)
    same(np.ascontiguousarray(back[:, :w]), masked)
    assert (back[:, w:] == 7).all()
    same(r.cpu().numpy(), ref.get_disparity_range(masked))


@pytest.mark.parametrize("dtype", TYPES, ids=["i32", "f32"])
def test_tiles_and_strips_equal_the_whole_map(dtype):
    """Four tiles and three row strips handed in with their x0, y0 give the pixels of the whole-map call."""
    w, h = 70, 45
    d = ref.scene(w, h, dtype, seed=71)
    mn, mx = bounds(w, h)
    m = MATRICES["projective"]
    whole = {
        "mask": stereo.disparity_range_mask(d, mn, mx, "reference", 5, 4),
        "functor": stereo.transform_disparities(d, m, 5, 4),
        "subregion": stereo.transform_disparities_subregion(True, vwa.BBox2i(5, 4, w, h), m, d),
    }
    tiles = [(0, 0, 33, 20), (33, 0, w, 20), (0, 20, 33, h), (33, 20, w, h)]
    strips = [(0, 0, w, 13), (0, 13, w, 30), (0, 30, w, h)]
    for parts in (tiles, strips):
        got = {k: np.zeros_like(d) for k in whole}
        for x0, y0, x1, y1 in parts:
            piece = np.ascontiguousarray(d[y0:y1, x0:x1])
            got["mask"][y0:y1, x0:x1] = stereo.disparity_range_mask(piece, mn, mx, "reference", 5 + x0, 4 + y0)
            got["functor"][y0:y1, x0:x1] = stereo.transform_disparities(piece, m, 5 + x0, 4 + y0)
            got["subregion"][y0:y1, x0:x1] = stereo.transform_disparities_subregion(
                True, vwa.BBox2i(5 + x0, 4 + y0, x1 - x0, y1 - y0), m, piece)
        for k in whole:
            same(got[k], whole[k], k)


def test_device_resident_chain_from_pyramid_correlate():
    """pyramid_correlate tile -> transform_disparities -> disparity_range_mask -> get_disparity_range on torch tensors
    equals the same chain on host arrays, whose steps equal the restatement."""
    import torch
    left, right, _ = synth.stereo_pair(160, 96, 9, 1, block=64)
    box = vwa.BBox2i.from_corners((-10, -1), (10, 1))
    h = stereo.HomographyTransform(ref.AFFINE)

    def chain(l, r):
        d = stereo.pyramid_correlate(l, r, None, None, 0, 0.0, box, (7, 7), 0, consistency_threshold=2, filter_half_kernel=3,
                                     max_pyramid_levels=2)
        t = stereo.transform_disparities(d, h)
        st = []
        m = stereo.disparity_range_mask(t, (-200, -50), (60, 90), stats=st)
        return d, t, m, st

    hd, ht, hm, hs = chain(left, right)
    dd, dt, dm, ds = chain(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda())
    dr = stereo.get_disparity_range(dm, device_result=True)
    torch.cuda.synchronize()
    assert dd.is_cuda and dt.is_cuda and dm.is_cuda and dr.is_cuda
    same(dd.cpu().numpy(), hd, "correlation")
    same(dt.cpu().numpy(), ht, "transform")
    same(dm.cpu().numpy(), hm, "mask")
    same(dr.cpu().numpy(), stereo.get_disparity_range(hm), "range")
    sw = []
    same(ht, ref.transform_disparities(hd, h.inverse_matrix), "transform against the restatement")
    same(hm, ref.disparity_range_mask(ht, (-200, -50), (60, 90), stats=sw), "mask against the restatement")
    same(stereo.get_disparity_range(hm), ref.get_disparity_range(hm))
    assert hs == ds == sw and hs[0] > 0 and (hm[..., 2] != 0).sum() > 1000


# ---- the C++ surface ------------------------------------------------------------------------------------------------

def test_cpp_surface(tmp_path):
    """vwlite's functions on both pixel types equal the Python calls."""
    exe = ref.build_view_program()
    w, h = 70, 45
    d = ref.float_scene(w, h, seed=80)
    di = ref.int_scene(w, h, seed=81)
    other, otheri = ref.float_scene(w, h, seed=82), ref.int_scene(w, h, seed=83)
    right = ref.image_scene(60, 50)
    p = {n: str(tmp_path / (n + ".pfm")) for n in ("d", "di", "o", "oi", "right", "out")}
    write_pfm(p["d"], d)
    write_pfm(p["di"], di.astype(np.float32))
    write_pfm(p["o"], other)
    write_pfm(p["oi"], otheri.astype(np.float32))
    write_pfm(p["right"], right)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    def agree(want):
        """the PFM holds float values and a 0 / 1 mask"""
        got = read_pfm(p["out"])
        assert got.shape == want.shape
        v = want[..., 2] != 0
        assert np.array_equal(got[..., 2] != 0, v)
        a, b = got[..., :2], want[..., :2].astype(np.float32)
        assert np.all((a == b) | (np.isnan(a) & np.isnan(b)))

    mn, mx = bounds(w, h)
    for is_int, src, key, oth, okey in ((0, d, "d", other, "o"), (1, di, "di", otheri, "oi")):
        out = run("range", p[key], is_int)
        assert np.array_equal(np.array(out.split()[:4], np.float32), stereo.get_disparity_range(src))
        for ref_bounds in (1, 0):
            run("mask", p[key], p["out"], is_int, mn[0], mn[1], mx[0], mx[1], ref_bounds)
            agree(stereo.disparity_range_mask(src, mn, mx, "reference" if ref_bounds else "fixed"))
        for H in (ref.AFFINE, np.linalg.inv(ref.PROJECTIVE)):
            run("transform", p[key], p["out"], is_int, *[repr(float(v)) for v in H.reshape(9)])
            agree(stereo.transform_disparities(src, stereo.HomographyTransform(H)))
        for do_round in (0, 1):
            run("subregion", p[key], p["out"], is_int, do_round, -6, 2, *[repr(float(v)) for v in ref.PROJECTIVE.reshape(9)])
            agree(stereo.transform_disparities_subregion(bool(do_round), vwa.BBox2i(-6, 2, w, h), ref.PROJECTIVE, src))
        run("subsample", p[key], p["out"], is_int)
        agree(stereo.disparity_subsample(src))
        run("upsample", p[key], p["out"], is_int)
        agree(stereo.disparity_upsample(src))
        run("intersect", p[key], p[okey], p["out"], is_int)
        agree(stereo.intersect_mask_and_data(src, oth))
        run("missing", p[key], p["out"], is_int)
        rgb = stereo.missing_pixel_image(src).astype(np.float32)
        assert np.array_equal(read_pfm(p["out"]), rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2])
    run("warp", p["right"], p["d"], p["out"])
    assert np.array_equal(read_pfm(p["out"]), stereo.disparity_transform_image(right, d))


# ---- argument errors through the raw C entries ----------------------------------------------------------------------

def test_argument_errors_leave_the_output_untouched():
    w, h = 40, 30
    d, di = ref.float_scene(w, h, seed=90), ref.int_scene(w, h, seed=91)
    right = ref.image_scene(w, h)
    L, H = _raw(core.default_context(0))
    nan = float("nan")
    out = np.full((2 * h, 2 * w, 3), 9, np.float32)
    outf = np.full((h, w), 9, np.float32)
    out8 = np.full((h, w, 3), 9, np.uint8)
    rng = np.full(4, 9, np.float32)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def vec(*v):
        return np.array(v, np.float64)

    def rng_(t=1, src=d, w_=w, h_=h, s=0, dst=rng):
        return L.vwgpu_get_disparity_range(H, t, P(src), w_, h_, s, P(dst))

    def mask(t=1, src=d, w_=w, h_=h, s=0, mn=vec(0, 0), mx=vec(30, 30), sem=0, dst=out, os_=0):
        return L.vwgpu_disparity_range_mask(H, t, P(src), w_, h_, s, 0, 0, P(mn), P(mx), sem, P(dst), os_, None)

    def tr(t=1, src=d, w_=w, h_=h, s=0, m=np.eye(3), mode=0, dst=out, os_=0):
        return L.vwgpu_transform_disparities(H, t, P(src), w_, h_, s, 0, 0, P(np.ascontiguousarray(m)) if m is not None else None, mode,
                                             P(dst), os_)

    def resample(fn, t=1, src=d, w_=w, h_=h, s=0, dst=out, os_=0):
        return getattr(L, "vwgpu_" + fn)(H, t, P(src), w_, h_, s, P(dst), os_)

    def warp(r=right, rw=w, rh=h, rs=0, dd=d, dw=w, dh=h, ds=0, dst=outf, os_=0):
        return L.vwgpu_disparity_warp(H, P(r), rw, rh, rs, P(dd), dw, dh, ds, P(dst), os_)

    def inter(t=1, a=d, as_=0, b=d, bs=0, w_=w, h_=h, dst=out, os_=0):
        return L.vwgpu_intersect_mask_and_data(H, t, P(a), as_, P(b), bs, w_, h_, P(dst), os_)

    common = ({"t": 2}, {"t": -1}, {"src": None}, {"dst": None}, {"w_": 0}, {"h_": -1}, {"s": w - 1})
    for kw in common:
        assert rng_(**kw) == ERR_ARGUMENT, kw
        assert mask(**kw) == ERR_ARGUMENT and tr(**kw) == ERR_ARGUMENT, kw
        for fn in ("disparity_subsample", "disparity_upsample"):
            assert resample(fn, **kw) == ERR_ARGUMENT, (fn, kw)
        assert resample("missing_pixel_image", **dict(kw, dst=None if "dst" in kw else out8)) == ERR_ARGUMENT, kw
    bad_mx = np.nan_to_num(vec(30, 30))
    bad_mx[1] = nan
    for kw in ({"os_": w - 1}, {"mn": vec(nan, 0)}, {"mx": bad_mx}, {"mn": None}, {"mx": None}, {"sem": 2}, {"sem": -1}):
        assert mask(**kw) == ERR_ARGUMENT, kw
    assert mask(t=0, src=di, mx=vec(3e9, 5)) == ERR_ARGUMENT          # a bound that does not fit the int32 pixel
    bad_m = np.eye(3)
    bad_m[2, 1] = nan
    for kw in ({"os_": w - 1}, {"m": bad_m}, {"m": None}, {"mode": 3}, {"mode": -1}):
        assert tr(**kw) == ERR_ARGUMENT, kw
    for fn, ow in (("disparity_subsample", 1 + (w - 1) // 2), ("disparity_upsample", 2 * w)):
        assert resample(fn, os_=ow - 1) == ERR_ARGUMENT and resample(fn, dst=d) == ERR_ARGUMENT, fn   # no in-place
    assert resample("missing_pixel_image", dst=out8, os_=w - 1) == ERR_ARGUMENT
    for kw in ({"r": None}, {"dd": None}, {"dst": None}, {"rw": 0}, {"dh": 0}, {"rs": w - 1}, {"ds": w - 1}, {"os_": w - 1}, {"dst": right}):
        assert warp(**kw) == ERR_ARGUMENT, kw
    for kw in ({"t": 3}, {"a": None}, {"b": None}, {"dst": None}, {"w_": 0}, {"as_": w - 1}, {"bs": w - 1}, {"os_": w - 1}):
        assert inter(**kw) == ERR_ARGUMENT, kw
    assert L.vwgpu_get_disparity_range_dev(H, 1, 1, w, h, 0, None, None) == ERR_ARGUMENT   # neither result asked for
    assert b"get_disparity_range" in L.vwgpu_last_error(H)
    # every refused call reported before any device work: nothing was written
    assert (out == 9).all() and (outf == 9).all() and (out8 == 9).all() and (rng == 9).all()
    # ... and the same calls with good arguments write everything they own
    assert rng_() == 0 and mask() == 0 and tr() == 0 and warp() == 0 and inter() == 0
    assert resample("disparity_upsample") == 0 and resample("missing_pixel_image", dst=out8) == 0
    assert (out != 9).any() and (outf != 9).any() and (out8 != 9).all() and (rng != 9).all()
    for call, kw in ((stereo.disparity_range_mask, dict(min=(0, 0), max=(9, 9), semantics="snapshot")),):
        with pytest.raises(core.ArgumentErr):
            call(d, **kw)
    with pytest.raises(core.ArgumentErr):
        stereo.transform_disparities(d, np.eye(2))
    with pytest.raises(core.ArgumentErr):
        stereo.transform_disparities_subregion(False, vwa.BBox2i(0, 0, w + 1, h), np.eye(3), d)
    with pytest.raises(core.ArgumentErr):
        stereo.get_disparity_range(d.astype(np.float64))
    with pytest.raises(core.ArgumentErr):
        stereo.disparity_transform_image(right, di)
    with pytest.raises(core.ArgumentErr):
        stereo.intersect_mask_and_data(d, di)
    with pytest.raises(core.ArgumentErr):
        stereo.disparity_subsample(d[..., :2])


# ---- 1024 x 768 -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def large():
    """One 1024 x 768 scene per pixel type with the restatement's results, computed once."""
    w, h = 1024, 768
    out = {}
    for dtype in TYPES:
        d = ref.scene(w, h, dtype, seed=95)
        mn, mx = (40, 30), (w - 20, h - 10)
        sw = []
        out[dtype] = {
            "d": d, "mn": mn, "mx": mx,
            "range": ref.get_disparity_range(d),
            "mask": ref.disparity_range_mask(d, mn, mx, "reference", stats=sw), "stats": sw,
            "functor": ref.transform_disparities(d, MATRICES["projective"]),
            "subregion": ref.transform_disparities(d, MATRICES["affine"], "subregion_round", 100, 200),
            "subsample": ref.disparity_subsample(d), "upsample": ref.disparity_upsample(d),
            "missing": ref.missing_pixel_image(d),
            "other": ref.scene(w, h, dtype, seed=96),
        }
        out[dtype]["intersect"] = ref.intersect_mask_and_data(d, out[dtype]["other"])
    out["right"] = ref.image_scene(w, h)
    out["warp_d"] = ref.warp_scene(w, h)
    out["warp"] = ref.disparity_transform_image(out["right"], out["warp_d"])
    return out


@pytest.mark.parametrize("dtype", TYPES, ids=["i32", "f32"])
@pytest.mark.parametrize("op", ["range", "mask", "functor", "subregion", "subsample", "upsample", "missing", "intersect"])
def test_1024x768_in_full(large, op, dtype):
    s = large[dtype]
    d, w, h = s["d"], 1024, 768
    if op == "range":
        got = stereo.get_disparity_range(d)
    elif op == "mask":
        st = []
        got = stereo.disparity_range_mask(d, s["mn"], s["mx"], stats=st)
        assert st == s["stats"] and st[0] > 0
    elif op == "functor":
        got = stereo.transform_disparities(d, MATRICES["projective"])
    elif op == "subregion":
        got = stereo.transform_disparities_subregion(True, vwa.BBox2i(100, 200, w, h), MATRICES["affine"], d)
    elif op == "intersect":
        got = stereo.intersect_mask_and_data(d, s["other"])
    else:
        got = {"subsample": stereo.disparity_subsample, "upsample": stereo.disparity_upsample,
               "missing": stereo.missing_pixel_image}[op](d)
    same(got, s[op], op)


def test_1024x768_warp_in_full(large):
    same(stereo.disparity_transform_image(large["right"], large["warp_d"]), large["warp"])
