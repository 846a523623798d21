"""CAHVOR and CAHVORE cameras on the GPU against the CPU restatement (tests/refimpl/cahvor_ref.cc).

CAHVOR uses only + - * / sqrt fabs: every word equals the restatement's (same(), NaNs by position).  CAHVORE calls sin,
cos, tan, atan, atan2 and asin, which the device library and glibc both give to about an ulp but not to the same bits, so
its results are held to bounds that are derived, not measured:
  points   |q_gpu - q_ref| <= 1e-9 px for |q| <= 1e4: an ulp of a trig result moves theta by ~1e-16, a Newton exit taken a
           pass earlier or later leaves ~1e-16, scaled by |H|, |V| ~ 1e3 gives 1e-13 .. 1e-12 px.
  images   source <= 128 px wide, values in [0, 1]: |out_gpu - out_ref| <= 1e-4: float(q) may round one float ulp apart
           (2^-16 below 128), the weights move by that much, the result by at most twice that, plus the rounding of four
           products.
  masks, counts   equal, except (the mask only) where the restatement's q lies within 1e-6 of an integer in x or y and
           floor may pick the neighbouring taps; at most 1 % of an image may be excused (asserted on the restatement).
  triangulation   |dxyz| <= 64 * 2^-52 * range^2 / baseline with range the largest distance of the restatement's points
           from camera 1; the error (a length) gets the same bound; the convergence angle acos(dot) amplifies the angular
           budget 64 * 2^-52 of a ray by 1 / sin(angle) <= range / baseline.
The measured maxima are printed (pytest -s) and recorded in profiles/cahvor.md."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import cahvor_ref as ref  # noqa: E402
import epipolar_ref as epi  # noqa: E402
import triangulate_ref as tri  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import _lib, camera, stereo  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = ["cahvor", "cahvore"]
SIZES = [(1, 1), (2, 9), (17, 1), (65, 5), (70, 45)]
EDGES = {"zero": (0, False), "value_valid": (7.5, True), "value_invalid": (-3.25, False)}
POINT_TOL, IMAGE_TOL = 1e-9, 1e-4


def same(got, want, what=""):
    """Exact equality of every word; NaNs by position."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.dtype.kind != "f":
        bad = np.argwhere(got != want)
        assert bad.size == 0, "%s: %d words differ, first at %s: got %r, want %r" % (
            what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaNs in different places" % what
    g, w = got.copy(), want.copy()
    g[gn], w[wn] = 0, 0
    bits = {8: np.uint64, 4: np.uint32}[got.dtype.itemsize]
    bad = np.argwhere(g.view(bits) != w.view(bits))
    assert bad.size == 0, "%s: %d words differ, first at %s: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def close(got, want, tol, what):
    """|got - want| <= tol, NaNs by position; prints the measured maximum."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaNs in different places" % what
    worst = float(np.abs(got - want)[~gn].max()) if (~gn).any() else 0.0
    print("MEASURED %s: max difference %.3g (bound %.3g)" % (what, worst, tol))
    assert worst <= tol, "%s: max difference %.3g > %.3g" % (what, worst, tol)


def check_image(kind, got, want, masked, what, edge_value=0.0):
    """got: image or (image, mask); want: the restatement's dict."""
    img, mask = got if masked else (got, None)
    if kind == "cahvor":
        same(img, want["out"], what + " image")
        if masked:
            same(mask, want["mask"], what + " mask")
        return
    assert abs(edge_value) <= 8      # the edge value enters the taps: the bound is for values in [0, 1] and scales with the range
    close(img, want["out"], IMAGE_TOL * max(1.0, abs(edge_value)), what + " image")
    if masked:
        near = (np.abs(want["q"] - np.round(want["q"])) < 1e-6).any(axis=2) & (want["status"] == 0)
        assert near.mean() <= 0.01, what
        bad = (mask != want["mask"]) & ~near
        assert not bad.any(), "%s mask: %d pixels differ away from integer positions" % (what, bad.sum())


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def source():
    return ref.source_image()


@pytest.fixture(scope="module")
def linear():
    """kind -> (the small fixture camera, its own linearisation by the restatement)."""
    return {k: (ref.small(k), ref.linearize_model(ref.small(k), (ref.SW, ref.SH))) for k in KINDS}


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_sizes(ctx, source, linear, kind, size, masked):
    """Partial workgroups, a single row and column, more than one block in x, several bands."""
    img, mask = source
    src, dst = linear[kind]
    m = mask if masked else None
    want = ref.camera_transform(img, src, dst, size=size, mask=m)
    assert want["failed"] == 0
    check_image(kind, camera.camera_transform(img, src, dst, size=size, mask=m, ctx=ctx), want, masked, "%s %dx%d" % ((kind,) + size))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_both_roles(ctx, source, linear, kind, masked):
    """CAHV src -> CAHVOR / CAHVORE dst: re-distortion."""
    img, mask = source
    cam, lin = linear[kind]
    m = mask if masked else None
    want = ref.camera_transform(img, lin, cam, size=(37, 29), mask=m)
    assert want["failed"] == 0 and np.any(want["out"] != 0)
    check_image(kind, camera.camera_transform(img, lin, cam, size=(37, 29), mask=m, ctx=ctx), want, masked, kind + " as dst")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("edge", sorted(EDGES))
@pytest.mark.parametrize("kind", KINDS)
def test_edge_pixels(ctx, source, linear, kind, edge, masked):
    """A dst turned so that part of the output leaves the source."""
    img, mask = source
    src, lin = linear[kind]
    dst = ref.turned(lin, -8.0, -4.0)
    m = mask if masked else None
    want = ref.camera_transform(img, src, dst, size=(37, 29), mask=m, edge=EDGES[edge])
    outside = (want["q"][..., 0] < -1) | (want["q"][..., 1] < -1)
    assert 0.05 < outside.mean() < 0.95 and want["failed"] == 0
    got = camera.camera_transform(img, src, dst, size=(37, 29), mask=m, edge=EDGES[edge], ctx=ctx)
    check_image(kind, got, want, masked, "%s edge %s" % (kind, edge), edge_value=EDGES[edge][0])


@pytest.mark.parametrize("kind", KINDS)
def test_tiles_and_row_strips_equal_the_whole(ctx, source, linear, kind):
    """The device against itself: exact for both kinds."""
    img, mask = source
    src, dst = linear[kind]
    whole, whole_mask = camera.camera_transform(img, src, dst, size=(70, 45), mask=mask, ctx=ctx)
    for x0, y0, w, h in ((0, 0, 35, 22), (35, 0, 35, 22), (0, 22, 35, 23), (35, 22, 35, 23), (0, 17, 70, 5), (0, 0, 70, 1), (0, 44, 70, 1)):
        out, om = camera.camera_transform(img, src, dst, size=(w, h), mask=mask, x0=x0, y0=y0, ctx=ctx)
        same(out, whole[y0:y0 + h, x0:x0 + w], "tile image")
        same(om, whole_mask[y0:y0 + h, x0:x0 + w], "tile mask")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_host_and_device_entries_agree(ctx, source, linear, kind, masked):
    import torch
    img, mask = source
    src, dst = linear[kind]
    m = mask if masked else None
    host = camera.camera_transform(img, src, dst, size=(70, 45), mask=m, edge=(2.0, True), ctx=ctx)
    dev = camera.camera_transform(torch.from_numpy(img).cuda(), src, dst, size=(70, 45), mask=None if m is None else torch.from_numpy(m).cuda(),
                                  edge=(2.0, True), ctx=ctx)
    if masked:
        same(dev[0].cpu().numpy(), host[0], "image")
        same(dev[1].cpu().numpy(), host[1], "mask")
    else:
        same(dev.cpu().numpy(), host, "image")


def test_cahvor_loop_exits(ctx, source, linear):
    img, mask = source
    lin = linear["cahvor"][1]
    # deriv <= 0 on the first pass: the ray from the start value
    dst = ref.small("cahvor", R=(-1.5, 0, 0))
    want = ref.camera_transform(img, lin, dst, size=(37, 29), mask=mask)
    assert (want["passes"] == 0).all()
    check_image("cahvor", camera.camera_transform(img, lin, dst, size=(37, 29), mask=mask, ctx=ctx), want, True, "deriv <= 0")
    # pixels that leave the loop in pass 0 and pixels that leave it in pass 2 or later
    dst = ref.small("cahvor", R=ref.STRONG_R)
    want = ref.camera_transform(img, lin, dst, size=(37, 29), mask=mask)
    assert (want["passes"] == 0).any() and (want["passes"] >= 2).any()
    check_image("cahvor", camera.camera_transform(img, lin, dst, size=(37, 29), mask=mask, ctx=ctx), want, True, "strong R")
    # a start far from the root: many passes (none is a failure)
    dst = ref.small("cahvor", R=(0, 5, 50))
    want = ref.camera_transform(img, lin, dst, size=(37, 29), mask=mask)
    assert want["passes"].max() >= 10 and want["failed"] == 0
    check_image("cahvor", camera.camera_transform(img, lin, dst, size=(37, 29), mask=mask, ctx=ctx), want, True, "many passes")


def test_cahvore_dst_that_cannot_converge(ctx, source, linear):
    """1 + R0 = 0 as dst at (8, 8): every off-axis pixel is the edge pixel and is counted."""
    import torch
    img, mask = source
    lin = linear["cahvore"][1]
    dst = ref.small("cahvore", R=(-1, 0, 0))
    want = ref.camera_transform(img, lin, dst, size=(8, 8), mask=mask, edge=(0.25, True))
    assert want["failed"] == 64 and want["theta"] == 0 and (want["status"] == ref.ST_NOT_CONVERGED).all()
    with pytest.raises(vwa.LogicErr, match=r"CAHVOREModel: Did not converge\. \(64 pixels\)"):
        camera.camera_transform(img, lin, dst, size=(8, 8), mask=mask, edge=(0.25, True), ctx=ctx)
    failed = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    out, om = camera.camera_transform(torch.from_numpy(img).cuda(), lin, dst, size=(8, 8), mask=torch.from_numpy(mask).cuda(),
                                      edge=(0.25, True), ctx=ctx, failed=failed)
    assert int(failed.cpu()[0]) == 64
    same(out.cpu().numpy(), want["out"], "edge pixels")
    same(om.cpu().numpy(), want["mask"], "edge mask")
    # the C ABI's host entry: the images are complete, the count is returned, the status is the logic error
    o, k, cnt = np.empty((8, 8), np.float32), np.empty((8, 8), np.uint8), ctypes.c_longlong(-1)
    rc = ctx._lib.vwgpu_camera_transform(ctx._h, img.ctypes.data, ref.SW, ref.SH, 0, mask.ctypes.data, 0, ctypes.byref(lin.descriptor), None,
                                         ctypes.byref(dst.descriptor), None, 8, 8, 0, 0, 0.25, 1, 1, o.ctypes.data, 0, k.ctypes.data, 0,
                                         ctypes.addressof(cnt))
    assert rc == -5 and cnt.value == 64
    same(o, want["out"], "host entry image")
    same(k, want["mask"], "host entry mask")


def test_cahvore_theta_out_of_bounds(ctx, source):
    import torch
    img, mask = source
    src, dst = ref.theta_pair()
    want = ref.camera_transform(img, src, dst, size=(37, 29), mask=mask, edge=(0.5, False))
    share = want["theta"] / (37.0 * 29)
    assert 0.01 < share < 0.99 and want["failed"] == want["theta"]
    failed = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    out, om = camera.camera_transform(torch.from_numpy(img).cuda(), src, dst, size=(37, 29), mask=torch.from_numpy(mask).cuda(),
                                      edge=(0.5, False), ctx=ctx, failed=failed)
    assert int(failed.cpu()[0]) == want["failed"]
    check_image("cahvore", (out.cpu().numpy(), om.cpu().numpy()), want, True, "theta out of bounds", edge_value=0.5)
    with pytest.raises(vwa.LogicErr, match=r"CAHVOREModel: Theta out of bounds\. \(%d pixels\)" % want["failed"]):
        camera.camera_transform(img, src, dst, size=(37, 29), mask=mask, ctx=ctx)


@pytest.mark.parametrize("case", ["axis", "P0", "P037", "P1"])
def test_cahvore_branches(ctx, source, case):
    """chip < 1e-8 (a pixel on the optical axis), and the three linearity branches."""
    img, mask = source
    if case == "axis":
        cam = ref.small("cahvore", unit_O=True)
        lin = ref.linearize_model(cam, (ref.SW, ref.SH))
        axis = ref.axis_pixel(cam)
        pts = np.array([axis, axis + (0.5, 0.25), axis - (3, 2)])
        want, failed, _, rc = ref.transform_points(lin, cam, ref.REVERSE, pts)      # rays of cam (the dst), projected into lin
        assert (rc, failed) == (0, 0) and ref.pixel_to_vector(cam, axis)[2] == 0
        got = camera.CameraTransform(lin, cam, ctx=ctx).reverse(pts)
        close(got, want, POINT_TOL, "axis points")
        same(got[0], want[0], "the axis itself: O, no trigonometry")
        return
    cam = ref.small("cahvore", T={"P0": 2, "P037": 3, "P1": 1}[case])
    assert cam.P == {"P0": 0.0, "P037": 0.37, "P1": 1.0}[case]
    lin = ref.linearize_model(cam, (ref.SW, ref.SH))
    for src, dst in ((cam, lin), (lin, cam)):
        want = ref.camera_transform(img, src, dst, size=(37, 29), mask=mask)
        assert want["failed"] == 0
        check_image("cahvore", camera.camera_transform(img, src, dst, size=(37, 29), mask=mask, ctx=ctx), want, True, case)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("kind", KINDS)
def test_camera_transform_points(ctx, linear, kind, n):
    import torch
    cam, lin = linear[kind]
    rng = np.random.default_rng(n)
    pts = np.stack([rng.uniform(2, ref.SW - 3, n), rng.uniform(2, ref.SH - 3, n)], 1)
    pts[0] = (12.0, 7.0)
    for src, dst in ((cam, lin), (lin, cam)):
        t = camera.CameraTransform(src, dst, ctx=ctx)
        for direction, fn in ((ref.FORWARD, t.forward), (ref.REVERSE, t.reverse)):
            want, failed, _, rc = ref.transform_points(src, dst, direction, pts)
            assert (rc, failed) == (0, 0) and np.abs(want).max() <= 1e4
            what = "%s points %s %d" % (kind, "raw->cahv" if src is cam else "cahv->raw", direction)
            got = fn(pts)
            if kind == "cahvor":
                same(got, want, what)
            else:
                close(got, want, POINT_TOL, what)
            if n == 65:
                same(fn(torch.from_numpy(pts).cuda()).cpu().numpy(), got, what + " dev")
                inplace = torch.from_numpy(pts).cuda()
                rc = ctx._lib.vwgpu_camera_transform_points_dev(ctx._h, ctypes.byref(src.descriptor), None, ctypes.byref(dst.descriptor), None,
                                                                direction, 1, inplace.data_ptr(), n, inplace.data_ptr(), None)
                torch.cuda.synchronize()
                assert rc == 0
                same(inplace.cpu().numpy(), got, what + " in place")
    # failures: NaN pairs, counted; LogicErr from the host entry
    if kind == "cahvore":
        bad = ref.small("cahvore", R=(-1, 0, 0))
        grid = pts[:max(n, 2)]
        want, failed, theta, rc = ref.transform_points(lin, bad, ref.REVERSE, grid)
        assert failed == len(grid) and np.isnan(want).all()
        got = camera.CameraTransform(lin, bad, ctx=ctx).reverse(torch.from_numpy(grid).cuda()).cpu().numpy()
        same(got, want, "NaN pairs")
        with pytest.raises(vwa.LogicErr, match="Did not converge"):
            camera.CameraTransform(lin, bad, ctx=ctx).reverse(grid)


@pytest.fixture(scope="module")
def scenes():
    """kind -> (disparity, left, right, the restatement's VIEW and MODEL results)."""
    out = {}
    for kind in KINDS:
        d, left, right = ref.scene_disparity(kind)
        out[kind] = (d, left, right, ref.stereo_triangulate(d, left, right, ref.VIEW), ref.stereo_triangulate(d, left, right, ref.MODEL))
    return out


def _tri_bounds(want, left, right):
    valid = np.any(want["xyz"] != 0, axis=2)
    rng = float(np.sqrt(((want["xyz"] - left.C) ** 2).sum(axis=2))[valid].max())
    base = float(np.sqrt(((right.C - left.C) ** 2).sum()))
    return 64 * 2.0 ** -52 * rng * rng / base, 64 * 2.0 ** -52 * rng / base, int(valid.sum())


@pytest.mark.parametrize("kind", KINDS)
def test_triangulation(ctx, scenes, kind):
    import torch
    d, left, right, view, model = scenes[kind]
    xyz_tol, ang_tol, npoints = _tri_bounds(view, left, right)
    assert npoints >= 200 and d.shape == (21, 33, 3) and view["stats"][0] == int((d[..., 2] != 0).sum())

    def agree(got, want, tol, what):
        if kind == "cahvor":
            same(got, want, what)
        else:
            close(got, want, tol, what)
    for with_stats in (False, True):
        stats = [] if with_stats else None
        xyz, err, ev = stereo.stereo_triangulate(d, left, right, error=True, error_vector=True, stats=stats, ctx=ctx)
        agree(xyz, view["xyz"], xyz_tol, kind + " view xyz")
        agree(err, view["error"], xyz_tol, kind + " view error")
        agree(ev, view["errvec"], xyz_tol, kind + " view error vector")
        if with_stats:
            assert stats[0] == view["stats"][0]
            agree(np.array(stats[1]), np.array(view["stats"][1]), xyz_tol, kind + " max error")
            assert abs(stats[2] - view["stats"][2]) <= 1e-12 * view["stats"][2] + stats[0] * (0 if kind == "cahvor" else xyz_tol)
        mstats = [] if with_stats else None
        mxyz, merr = stereo.StereoModel(left, right)(d, stats=mstats, ctx=ctx)
        agree(mxyz, model["xyz"], xyz_tol, kind + " model xyz")
        agree(merr, model["error"], xyz_tol, kind + " model error")
        if with_stats:
            assert mstats[0] == model["stats"][0]
    assert np.isfinite(view["xyz"]).all() and (view["error"][np.any(view["xyz"] != 0, axis=2)] > 0).all()
    # the device entry
    txyz = stereo.stereo_triangulate(torch.from_numpy(d).cuda(), left, right, ctx=ctx)
    same(txyz.cpu().numpy(), stereo.stereo_triangulate(d, left, right, ctx=ctx), "device entry")
    # the convergence angle: acos is the device library's for both kinds
    ang = stereo.StereoModel(left, right).convergence_angle(d, semantics="view", ctx=ctx)
    close(ang, view["angle"], ang_tol, kind + " convergence angle")
    assert (ang[d[..., 2] != 0] > 0).all() and (ang[d[..., 2] == 0] == 0).all()


def test_cahvore_pair_that_cannot_converge_gives_zero_points(ctx, scenes):
    d = scenes["cahvore"][0]
    left, right = ref.stereo_pair("cahvore", R=(-1, 0, 0))
    want = ref.stereo_triangulate(d, left, right)
    assert not want["xyz"].any() and not want["errvec"].any()
    stats = []
    xyz, err, ev = stereo.stereo_triangulate(d, left, right, error=True, error_vector=True, stats=stats, ctx=ctx)
    same(xyz, want["xyz"], "zero points")
    same(err, want["error"], "zero error")
    same(ev, want["errvec"], "zero error vectors")
    assert stats[0] == want["stats"][0] and stats[1] == 0 and stats[2] == 0
    ang = stereo.StereoModel(left, right).convergence_angle(d, semantics="view", ctx=ctx)
    same(ang, want["angle"], "NaN angles at valid pixels, 0 at invalid ones")


def _copy_kind(cam, kind):
    d = _lib.Camera.from_buffer_copy(bytes(camera.descriptor_of(cam)))
    d.kind = kind
    return d


def test_refusals(ctx, source, linear):
    img, mask = source
    cahvor, lin = linear["cahvor"]
    cahvore = ref.small("cahvore", C=cahvor.C)
    pin = camera.PinholeModel(cahvor.C, np.eye(3), 60.0, 60.0, 30.0, 23.0)
    lin_e = camera.CAHVModel(cahvor.C, lin.A, lin.H, lin.V)
    noimpl = [(cahvor, pin), (pin, cahvor), (cahvore, pin), (pin, cahvore), (cahvor, cahvore), (cahvore, cahvor), (cahvor, cahvor),
              (cahvore, cahvore)]
    for src, dst in noimpl:
        with pytest.raises(vwa.NoImplErr, match="no kernel for the pair"):
            camera.camera_transform(img, src, dst, size=(8, 8), ctx=ctx)
        for fn in ("forward", "reverse"):
            with pytest.raises(vwa.NoImplErr, match="no kernel for the pair"):
                getattr(camera.CameraTransform(src, dst, ctx=ctx), fn)(np.zeros((3, 2)))
    d = np.zeros((4, 6, 3), np.float32)
    d[..., 2] = 1
    for c1, c2 in ((cahvor, lin_e), (lin_e, cahvor), (cahvore, lin_e), (lin_e, cahvore), (cahvor, pin), (pin, cahvore), (cahvor, cahvore),
                   (cahvore, cahvor)):
        with pytest.raises(vwa.NoImplErr, match="no kernel for the pair"):
            stereo.stereo_triangulate(d, c1, c2, ctx=ctx)
        with pytest.raises(vwa.NoImplErr, match="no kernel for the pair"):
            stereo.StereoModel(c1, c2).convergence_angle(d, ctx=ctx)
    # kind 2 stays unassigned and refused as an argument error, on either side and beside a new kind
    two = _copy_kind(lin, 2)
    for src, dst in ((two, lin), (lin, two), (cahvor, two), (two, cahvore)):
        with pytest.raises(vwa.ArgumentErr, match="unknown camera kind 2"):
            camera.camera_transform(img, src, dst, size=(8, 8), ctx=ctx)
    with pytest.raises(vwa.ArgumentErr, match="unknown camera kind 2"):
        stereo.stereo_triangulate(d, two, cahvor, ctx=ctx)
    with pytest.raises(vwa.ArgumentErr, match="unknown camera kind 5"):
        stereo.stereo_triangulate(d, _copy_kind(lin, 5), lin, ctx=ctx)
    # unequal centres are still the reference's assert
    moved = ref.linearize_model(ref.small("cahvor", C=(1, 2, 3)), (ref.SW, ref.SH))
    with pytest.raises(vwa.LogicErr, match="camera center"):
        camera.camera_transform(img, cahvor, moved, ctx=ctx)
    with pytest.raises(vwa.LogicErr, match="camera center"):
        camera.CameraTransform(moved, cahvore, ctx=ctx).forward(np.zeros((3, 2)))


# Which ordered pairs have a kernel, written from the rule of include/vwgpu.h (struct vwgpu_camera): every pair of pinholes
# (with any lens) and CAHV cameras has one; a CAHVOR or CAHVORE camera goes with a CAHV camera alone in a camera transform,
# in either role, and with one of its own kind alone in triangulation and the convergence angle.  Rows: the first camera
# (src, cam1); columns: the second (dst, cam2), in the order of PAIR_KINDS.
PAIR_KINDS = ["pinhole", "tsai", "fisheye", "brown_conrady", "cahv", "cahvor", "cahvore"]
PAIR_NAMES = {"pinhole": "Pinhole", "tsai": "Pinhole", "fisheye": "Pinhole", "brown_conrady": "Pinhole", "cahv": "CAHV", "cahvor": "CAHVOR",
              "cahvore": "CAHVORE"}
TRANSFORM_HAS_KERNEL = {
    "pinhole":       "YYYYYNN",
    "tsai":          "YYYYYNN",
    "fisheye":       "YYYYYNN",
    "brown_conrady": "YYYYYNN",
    "cahv":          "YYYYYYY",
    "cahvor":        "NNNNYNN",
    "cahvore":       "NNNNYNN",
}
TRIANGULATE_HAS_KERNEL = {
    "pinhole":       "YYYYYNN",
    "tsai":          "YYYYYNN",
    "fisheye":       "YYYYYNN",
    "brown_conrady": "YYYYYNN",
    "cahv":          "YYYYYNN",
    "cahvor":        "NNNNNYN",
    "cahvore":       "NNNNNNY",
}


def test_which_pairs_have_a_kernel(ctx, source):
    """Every ordered pair of seven descriptors through camera_transform, CameraTransform (both directions), stereo_triangulate
    and convergence_angle: a result of the right shape, or NoImplErr that names the pair.  The operands are tensors: such a
    call never synchronises, so a pixel that fails a check cannot turn an accepted pair into a LogicErr."""
    import torch
    import lens_ref
    C = ref.small("cahvor").C
    cams = {"pinhole": lens_ref.small(None, center=C), "tsai": lens_ref.small("TSAI", center=C), "fisheye": lens_ref.small("FISHEYE", center=C),
            "brown_conrady": lens_ref.small("BrownConrady", center=C), "cahv": lens_ref.cahv(center=C), "cahvor": ref.small("cahvor"),
            "cahvore": ref.small("cahvore", C=C)}
    assert sorted(cams) == sorted(PAIR_KINDS)
    img = torch.from_numpy(source[0]).cuda()
    pts = torch.from_numpy(np.stack([np.linspace(2, 50, 65), np.linspace(3, 40, 65)], 1)).cuda()
    d = np.zeros((29, 37, 3), np.float32)
    d[..., 0], d[..., 2] = -2.0, 1
    d = torch.from_numpy(d).cuda()

    def expect(has_kernel, shape, first, second, fn):
        if has_kernel:
            assert tuple(fn().shape) == shape, (first, second)
            return
        with pytest.raises(vwa.NoImplErr, match="no kernel for the pair") as e:
            fn()
        assert PAIR_NAMES[first] in str(e.value) and PAIR_NAMES[second] in str(e.value), str(e.value)
    for first in PAIR_KINDS:
        for k, second in enumerate(PAIR_KINDS):
            a, b = cams[first], cams[second]
            has = TRANSFORM_HAS_KERNEL[first][k] == "Y"
            expect(has, (29, 37), first, second, lambda: camera.camera_transform(img, a, b, size=(37, 29), ctx=ctx))
            expect(has, (65, 2), first, second, lambda: camera.CameraTransform(a, b, ctx=ctx).forward(pts))
            expect(has, (65, 2), first, second, lambda: camera.CameraTransform(a, b, ctx=ctx).reverse(pts))
            has = TRIANGULATE_HAS_KERNEL[first][k] == "Y"
            expect(has, (29, 37, 3), first, second, lambda: stereo.stereo_triangulate(d, a, b, ctx=ctx))
            expect(has, (29, 37), first, second, lambda: stereo.StereoModel(a, b).convergence_angle(d, ctx=ctx))
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", KINDS)
def test_epipolar_transformed_images_end_to_end(ctx, source, kind):
    """Two scaled models with a baseline: linearize_camera per frame, epipolar() on the two CAHV results and one
    camera_transform(frame, raw model, rectified CAHV) per image, against the same composition on the restatement."""
    img, mask = source
    right_img = np.ascontiguousarray(img[:-3, ::-1][:, :-5])      # another frame size: 91 x 77
    cam_l, cam_r = ref.stereo_pair(kind)
    rmask = np.full(right_img.shape, 255, np.uint8)
    lo, lom, ro, rom, epi_l, epi_r = stereo.epipolar_transformed_images(img, right_img, cam_l, cam_r, left_mask=mask, right_mask=rmask, ctx=ctx)
    lin_l = ref.linearize_model(cam_l, (img.shape[1], img.shape[0]))
    lin_r = ref.linearize_model(cam_r, (right_img.shape[1], right_img.shape[0]))
    d0, d1 = epi.epipolar_cahv(lin_l, lin_r)
    assert bytes(epi_l.descriptor) == bytes(d0) and bytes(epi_r.descriptor) == bytes(d1)
    want_l = ref.camera_transform(img, cam_l, epi_l, mask=mask)
    want_r = ref.camera_transform(right_img, cam_r, epi_r, mask=rmask)
    assert want_l["failed"] == 0 and want_r["failed"] == 0 and (want_l["mask"] == 255).mean() > 0.3
    check_image(kind, (lo, lom), want_l, True, kind + " left")
    check_image(kind, (ro, rom), want_r, True, kind + " right")
    assert lo.shape == img.shape and ro.shape == right_img.shape
    # without masks: four results
    plain = stereo.epipolar_transformed_images(img, right_img, cam_l, cam_r, ctx=ctx)
    assert len(plain) == 4
    same(plain[0], lo, "unmasked left")
    # the rectified cameras triangulate a constant-row disparity to finite points in front of both
    d = np.zeros((4, 6, 3), np.float32)
    d[..., 0], d[..., 2] = -3.0, 1
    xyz = stereo.stereo_triangulate(d, epi_l, epi_r, x0=40, y0=30, ctx=ctx)
    same(xyz, tri.stereo_triangulate(d, epi_l, epi_r, x0=40, y0=30)["xyz"], "triangulated")
    assert np.isfinite(xyz).all() and np.any(xyz != 0, axis=2).all()
    with pytest.raises(vwa.ArgumentErr):
        stereo.epipolar_transformed_images(img, right_img, cam_l, epi_r, ctx=ctx)


@pytest.mark.parametrize("kind", KINDS)
def test_linearize_camera_transform(ctx, source, linear, kind):
    img, mask = source
    src, lin = linear[kind]
    out, om, cahv = camera.linearize_camera_transform(img, src, mask=mask, ctx=ctx)
    assert bytes(cahv.descriptor) == bytes(lin.descriptor)
    want = camera.camera_transform(img, src, lin, mask=mask, ctx=ctx)
    same(out, want[0], "image")
    same(om, want[1], "mask")
    out2, cahv2 = camera.linearize_camera_transform(img, src, edge=(0.5, True), ctx=ctx)
    same(out2, camera.camera_transform(img, src, lin, edge=(0.5, True), ctx=ctx), "unmasked")


def _words(cam):
    e = getattr(cam, "E", np.zeros(3))
    p = getattr(cam, "P", 0.0)
    return np.concatenate([cam.C, cam.A, cam.H, cam.V, cam.O, cam.R, e, [3.0, p]])


@pytest.mark.parametrize("kind", KINDS)
def test_vwlite_program_equals_the_python_calls(ctx, source, scenes, kind, tmp_path):
    """cahvor_view.cc: linearize_camera, linearize_camera_transform (a masked view rasterised whole with a value edge),
    camera_transform back into the raw camera (a float view box by box), CameraTransform, the models' own host functions
    and stereo_triangulate give what the Python calls give."""
    exe = ref.build_view_program()
    img, mask = source
    d, left, right = scenes[kind][:3]
    np.concatenate([_words(left), _words(right)]).tofile(str(tmp_path / "cams.bin"))
    img.tofile(str(tmp_path / "img.bin"))
    mask.tofile(str(tmp_path / "mask.bin"))
    d.tofile(str(tmp_path / "disp.bin"))
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, kind, str(tmp_path / "cams.bin"), str(tmp_path / "img.bin"), str(tmp_path / "mask.bin"), str(ref.SW),
                          str(ref.SH), str(tmp_path / "disp.bin"), str(d.shape[1]), str(d.shape[0]), prefix], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    out, om, lin = camera.linearize_camera_transform(img, left, mask=mask, edge=(0.5, True), ctx=ctx)
    assert np.fromfile(prefix + ".lin", np.uint8).tobytes() == bytes(lin.descriptor)
    same(np.fromfile(prefix + ".out", np.float32).reshape(out.shape), out, "linearised image")
    same(np.fromfile(prefix + ".omask", np.uint8).reshape(om.shape), om, "linearised mask")
    same(np.fromfile(prefix + ".back", np.float32).reshape(img.shape), camera.camera_transform(img, lin, left, ctx=ctx), "re-distorted")
    same(np.fromfile(prefix + ".xyz", np.float64).reshape(d.shape), stereo.stereo_triangulate(d, left, right, ctx=ctx), "points")
    meta = np.fromfile(prefix + ".meta", np.float64)
    t = camera.CameraTransform(left, lin, ctx=ctx)
    fwd = t.forward(np.array([[ref.SW / 3.0, ref.SH / 4.0]]))
    same(meta[0:2], fwd[0], "forward")
    same(meta[2:4], t.reverse(fwd)[0], "reverse")
    ray, st, _ = ref.pixel_to_vector(left, (ref.SW / 3.0, ref.SH / 4.0))
    pix, st2 = ref.point_to_pixel(left, left.C + 7.0 * ray)
    assert st == 0 and st2 == 0
    same(meta[4:7], ray, "the C++ model's ray (host code, glibc: the restatement's bits)")
    same(meta[7:9], pix, "the C++ model's pixel")
