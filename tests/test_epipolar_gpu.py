"""camera_transform / CameraTransform / epipolar_transformed_images on the GPU against the CPU restatement
(tests/refimpl/epipolar_ref.cc): every output word with ==, NaNs by position.  The scenes and the conditions they meet are
checked without a GPU in test_epipolar_cpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import epipolar_ref as ref  # noqa: E402
import triangulate_ref as tri  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import _lib, camera, stereo, synth  # noqa: E402
from visionworkbench_amd.core import BBox2i  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (2, 9), (17, 1), (37, 29), (70, 45), (300, 200)]
EDGES = {"zero": (0, False), "value_valid": (7.5, True), "value_invalid": (-3.25, False)}


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
def main(source):
    """The main pair at 70 x 45, masked, with the restatement's result."""
    src, dst = ref.camera_pairs()["pinhole_pinhole"]
    return src, dst, ref.camera_transform(source[0], src, dst, size=(70, 45), mask=source[1])


def check(got, want, masked, what):
    if masked:
        same(got[0], want["out"], what + " image")
        same(got[1], want["mask"], what + " mask")
    else:
        same(got, want["out"], what + " image")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_sizes(ctx, source, size, masked):
    """Partial workgroups, a single row and column, and several workgroups in both directions."""
    img, mask = source
    src, dst = ref.camera_pairs()["pinhole_pinhole"]
    m = mask if masked else None
    want = ref.camera_transform(img, src, dst, size=size, mask=m)
    check(camera.camera_transform(img, src, dst, size=size, mask=m, ctx=ctx), want, masked, "%dx%d" % size)


@pytest.mark.parametrize("check_on", [True, False])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("pair", sorted(ref.camera_pairs()))
def test_camera_pairs(ctx, source, pair, masked, check_on):
    img, mask = source
    src, dst = ref.camera_pairs()[pair]
    m = mask if masked else None
    want = ref.camera_transform(img, src, dst, size=(37, 29), mask=m, check=check_on)
    assert want["failed"] == 0 and np.any(want["out"] != 0)
    check(camera.camera_transform(img, src, dst, size=(37, 29), mask=m, check=check_on, ctx=ctx), want, masked, pair)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("edge", sorted(EDGES))
def test_edge_pixels(ctx, source, edge, masked):
    img, mask = source
    src, dst = ref.camera_pairs()["pinhole_pinhole"]
    m = mask if masked else None
    want = ref.camera_transform(img, src, dst, size=(70, 45), mask=m, edge=EDGES[edge])
    check(camera.camera_transform(img, src, dst, size=(70, 45), mask=m, edge=EDGES[edge], ctx=ctx), want, masked, edge)


def test_tile_and_row_strip_equal_the_whole(ctx, source, main):
    img, mask = source
    src, dst, whole = main
    for x0, y0, w, h in ((13, 9, 20, 10), (0, 17, 70, 5), (64, 3, 6, 40)):
        out, om = camera.camera_transform(img, src, dst, size=(w, h), mask=mask, x0=x0, y0=y0, ctx=ctx)
        same(out, whole["out"][y0:y0 + h, x0:x0 + w], "tile image")
        same(om, whole["mask"][y0:y0 + h, x0:x0 + w], "tile mask")
    # and negative origins: the restatement again
    want = ref.camera_transform(img, src, dst, size=(33, 21), mask=mask, x0=-7, y0=-5)
    check(camera.camera_transform(img, src, dst, size=(33, 21), mask=mask, x0=-7, y0=-5, ctx=ctx), want, True, "negative origin")


def _raw_dev(ctx, img, mask, src, dst, w, h, pads=(0, 0, 0, 0), edge=(0, False), check_on=True, want_failed=False):
    """vwgpu_camera_transform_dev on tensors whose rows are pads[k] elements wider than the images: (out, mask, failed, rc)."""
    import torch
    dev = torch.device("cuda", 0)
    sh, sw = img.shape

    def padded(a, pad, fill):
        t = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.from_numpy(a[:1, :1].copy()).dtype, device=dev)
        t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t
    timg = padded(img, pads[0], 1e30)
    tmask = None if mask is None else padded(mask, pads[1], 255)
    tout = torch.full((h, w + pads[2]), -77.0, dtype=torch.float32, device=dev)
    tom = None if mask is None else torch.full((h, w + pads[3]), 99, dtype=torch.uint8, device=dev)
    tfail = torch.full((1,), -1, dtype=torch.int64, device=dev) if want_failed else None
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    ms, md = camera.matrix_of(src), camera.matrix_of(dst)
    rc = ctx._lib.vwgpu_camera_transform_dev(
        ctx._h, timg.data_ptr(), sw, sh, timg.stride(0), None if tmask is None else tmask.data_ptr(),
        0 if tmask is None else tmask.stride(0), ctypes.byref(camera.descriptor_of(src)), None if ms is None else ms.ctypes.data,
        ctypes.byref(camera.descriptor_of(dst)), None if md is None else md.ctypes.data, w, h, 0, 0, float(edge[0]), int(edge[1]),
        int(check_on), tout.data_ptr(), tout.stride(0), None if tom is None else tom.data_ptr(), 0 if tom is None else tom.stride(0),
        None if tfail is None else tfail.data_ptr())
    torch.cuda.synchronize()
    return (tout.cpu().numpy(), None if tom is None else tom.cpu().numpy(), None if tfail is None else int(tfail.cpu()[0]), rc)


def test_row_strides(ctx, source, main):
    img, mask = source
    src, dst, whole = main
    out, om, _, rc = _raw_dev(ctx, img, mask, src, dst, 70, 45, pads=(3, 5, 7, 2))
    assert rc == 0
    same(out[:, :70], whole["out"], "strided image")
    same(om[:, :70], whole["mask"], "strided mask")
    assert (out[:, 70:] == -77.0).all() and (om[:, 70:] == 99).all()      # the padding is not written
    # a strided host image: the packed copy the wrapper makes, and a strided tensor passed as a view
    import torch
    wide = np.full((ref.SH, ref.SW + 4), 1e30, np.float32)
    wide[:, :ref.SW] = img
    check(camera.camera_transform(wide[:, :ref.SW], src, dst, size=(70, 45), mask=mask, ctx=ctx), whole, True, "host view")
    t = torch.from_numpy(wide).cuda()
    got = camera.camera_transform(t[:, :ref.SW], src, dst, size=(70, 45), mask=torch.from_numpy(mask).cuda(), ctx=ctx)
    check((got[0].cpu().numpy(), got[1].cpu().numpy()), whole, True, "tensor view")


@pytest.mark.parametrize("masked", [False, True])
def test_host_and_device_entries_agree(ctx, source, masked):
    import torch
    img, mask = source
    src, dst = ref.camera_pairs()["tsai_cahv"]
    m = mask if masked else None
    host = camera.camera_transform(img, src, dst, size=(70, 45), mask=m, edge=(2.0, True), ctx=ctx)
    dev = camera.camera_transform(torch.from_numpy(img).cuda(), src, dst, size=(70, 45), mask=None if m is None else torch.from_numpy(m).cuda(),
                                  edge=(2.0, True), ctx=ctx)
    if masked:
        same(dev[0].cpu().numpy(), host[0], "image")
        same(dev[1].cpu().numpy(), host[1], "mask")
    else:
        same(dev.cpu().numpy(), host, "image")


def test_identity_pair_reproduces_the_source(ctx, source):
    img, mask = source
    src, dst = ref.identity_pair()
    want = ref.camera_transform(img, src, dst, size=(70, 45), mask=mask)
    out, om = camera.camera_transform(img, src, dst, size=(70, 45), mask=mask, ctx=ctx)
    same(out, want["out"], "image")
    same(om, want["mask"], "mask")
    hit = want["classes"] == ref.CL_INTEGER
    ys, xs = np.nonzero(hit)
    assert hit.sum() > 0
    assert np.array_equal(out[hit], img[ys, xs]) and np.array_equal(om[hit], mask[ys, xs])


@pytest.mark.parametrize("cahv", [False, True])
def test_right_angle_pair_nan_and_huge(ctx, source, cahv):
    img, mask = source
    src, dst = ref.right_angle_pair(cahv)
    want = ref.camera_transform(img, src, dst, size=(37, 29), mask=mask, check=False, edge=(4.0, True))
    assert (want["classes"] == ref.CL_NAN_HUGE).sum() > 0
    check(camera.camera_transform(img, src, dst, size=(37, 29), mask=mask, check=False, edge=(4.0, True), ctx=ctx), want, True, "right angle")


def test_strong_tsai_counts_and_writes_the_edge_pixel(ctx, source):
    img, mask = source
    src, dst = ref.strong_tsai_pair()
    want = ref.camera_transform(img, src, dst, size=(70, 45), mask=mask, edge=(7.5, True))
    bad = want["classes"] == ref.CL_CHECK_FAILED
    assert want["failed"] == bad.sum() > 0
    # the _dev entry: OK, the count in device memory, the images complete
    out, om, failed, rc = _raw_dev(ctx, img, mask, src, dst, 70, 45, edge=(7.5, True), want_failed=True)
    assert rc == 0 and failed == want["failed"]
    same(out, want["out"], "image")
    same(om, want["mask"], "mask")
    assert (out[bad] == np.float32(7.5)).all() and (om[bad] == 255).all()
    # the host entry: VWGPU_ERR_LOGIC with the reference's message and the count; the images are complete all the same
    h_out, h_mask, h_failed = np.empty((45, 70), np.float32), np.empty((45, 70), np.uint8), ctypes.c_longlong(-1)
    m8 = np.ascontiguousarray(mask != 0, np.uint8)
    rc = ctx._lib.vwgpu_camera_transform(
        ctx._h, img.ctypes.data, ref.SW, ref.SH, 0, m8.ctypes.data, 0, ctypes.byref(src.descriptor), src.matrix.ctypes.data,
        ctypes.byref(dst.descriptor), dst.matrix.ctypes.data, 70, 45, 0, 0, 7.5, 1, 1, h_out.ctypes.data, 0, h_mask.ctypes.data, 0,
        ctypes.addressof(h_failed))
    assert rc == -5 and h_failed.value == want["failed"]
    message = ctx._lib.vwgpu_last_error(ctx._h).decode()
    assert "PinholeModel: Projection into pinhole camera is inaccurate." in message and str(want["failed"]) in message
    same(h_out, want["out"], "host image")
    same(h_mask, want["mask"], "host mask")
    with pytest.raises(vwa.LogicErr, match="inaccurate"):
        camera.camera_transform(img, src, dst, size=(70, 45), mask=mask, ctx=ctx)
    # with the check off nothing fails, and a count that was asked for is 0
    off = ref.camera_transform(img, src, dst, size=(70, 45), mask=mask, check=False)
    out, om, failed, rc = _raw_dev(ctx, img, mask, src, dst, 70, 45, check_on=False, want_failed=True)
    assert rc == 0 and failed == 0
    same(out, off["out"], "unchecked image")
    same(om, off["mask"], "unchecked mask")
    # the mild lens: no failure
    src, dst = ref.mild_tsai_pair()
    want = ref.camera_transform(img, src, dst, size=(70, 45), mask=mask)
    out, om, failed, rc = _raw_dev(ctx, img, mask, src, dst, 70, 45, want_failed=True)
    assert rc == 0 and failed == 0 == want["failed"]
    same(out, want["out"], "mild image")


POINT_PAIRS = ["pinhole_pinhole", "turned_pitch", "tsai_src", "tsai_dst", "cahv_cahv", "cahv_cahv_flipped", "pinhole_cahv", "tsai_cahv"]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_camera_transform_points(ctx, n):
    """At n = 65 every pair of ref.camera_pairs() in both directions with the check on and off: every point kernel of the
    null / Tsai pinholes and CAHV (the rows of ct_pairs in camera_transform.hip) against the restatement."""
    import torch
    rng = np.random.default_rng(n)
    pts = np.stack([rng.uniform(-5, 66, n), rng.uniform(-5, 52, n)], 1)
    pts[0] = (12.0, 7.0)
    for pair in (sorted(ref.camera_pairs()) if n == 65 else POINT_PAIRS):
        src, dst = ref.camera_pairs()[pair]
        for check_on in ((True, False) if n == 65 else (True,)):
            t = camera.CameraTransform(src, dst, check=check_on, ctx=ctx)
            for direction, fn in ((ref.FORWARD, t.forward), (ref.REVERSE, t.reverse)):
                want, failed, rc = ref.transform_points(src, dst, direction, pts, check=check_on)
                assert (rc, failed) == (0, 0)
                same(fn(pts), want, "%s %d check %d" % (pair, direction, check_on))
                if n == 65:
                    same(fn(torch.from_numpy(pts).cuda()).cpu().numpy(), want, "%s %d check %d dev" % (pair, direction, check_on))
    # the strong lens: NaN pairs where the check fails; LogicErr from the host entry, the NaNs from the device entry
    src, dst = ref.strong_tsai_pair()
    grid = np.stack(np.meshgrid(np.arange(0.0, 70.0, 3.0), np.arange(0.0, 45.0, 4.0)), -1).reshape(-1, 2)[:max(n, 2)]
    want, failed, rc = ref.transform_points(src, dst, ref.REVERSE, grid)
    got = camera.CameraTransform(src, dst, ctx=ctx).reverse(torch.from_numpy(grid).cuda()).cpu().numpy()
    same(got, want, "strong lens")
    if failed:
        with pytest.raises(vwa.LogicErr, match="inaccurate"):
            camera.CameraTransform(src, dst, ctx=ctx).reverse(grid)


def test_resize_epipolar_cameras_to_fit(ctx):
    for lens in (None, ref.MILD_TSAI):
        a, b = ref.stereo_pair(lens)
        e0, e1 = camera.epipolar(a, b)
        roi1, roi2 = BBox2i(0, 0, ref.SW, ref.SH), BBox2i(0, 0, 57, 44)
        g0, g1, gs1, gs2 = camera.resize_epipolar_cameras_to_fit(a, b, e0, e1, roi1, roi2, ctx=ctx)
        w0, w1, ws1, ws2 = ref.resize_epipolar_cameras_to_fit(a, b, e0, e1, roi1, roi2)
        assert (gs1, gs2) == (ws1, ws2) and gs1[0] > 0 and gs1[1] > 0
        assert bytes(g0.descriptor) == bytes(w0.descriptor) and bytes(g1.descriptor) == bytes(w1.descriptor)
        assert e0.cu != g0.cu      # the input cameras are left as they were, the new ones are shifted


def test_epipolar_transformed_images_end_to_end(ctx):
    """A synthetic pair from synth through epipolar_transformed_images: the aligned images and masks equal the restatement's
    for the cameras and sizes the restatement derives, and the rectified cameras go straight into stereo_triangulate."""
    left, right = synth.stereo_pair(ref.SW, ref.SH, 9, block=16)[:2]      # the right frame is 8 columns wider
    left, right = np.ascontiguousarray(left, np.float32), np.ascontiguousarray(right, np.float32)
    lm = (np.random.default_rng(8).random(left.shape) >= 0.05).astype(np.uint8) * 255
    rm = np.full(right.shape, 255, np.uint8)
    a, b = ref.stereo_pair(ref.MILD_TSAI)
    lo, lom, ro, rom, epi_l, epi_r = stereo.epipolar_transformed_images(left, right, a, b, left_mask=lm, right_mask=rm, ctx=ctx)
    e0, e1 = ref.epipolar(a, b)
    w0, w1, s0, s1 = ref.resize_epipolar_cameras_to_fit(a, b, e0, e1, BBox2i(0, 0, left.shape[1], left.shape[0]),
                                                        BBox2i(0, 0, right.shape[1], right.shape[0]))
    assert bytes(epi_l.descriptor) == bytes(w0.descriptor) and bytes(epi_r.descriptor) == bytes(w1.descriptor)
    want_l = ref.camera_transform(left, a, w0, size=s0, mask=lm)
    want_r = ref.camera_transform(right, b, w1, size=s1, mask=rm)
    assert want_l["failed"] == 0 and want_r["failed"] == 0
    same(lo, want_l["out"], "left")
    same(lom, want_l["mask"], "left mask")
    same(ro, want_r["out"], "right")
    same(rom, want_r["mask"], "right mask")
    assert (lo.shape[1], lo.shape[0]) == s0 and (ro.shape[1], ro.shape[0]) == s1
    # the rectified cameras triangulate: a zero-row-offset disparity of the aligned pair gives points in front of both
    d = np.zeros((4, 6, 3), np.float32)
    d[..., 0], d[..., 2] = -6.0, 1
    xyz = stereo.stereo_triangulate(d, epi_l, epi_r, x0=30, y0=20, ctx=ctx)
    same(xyz, tri.stereo_triangulate(d, epi_l, epi_r, x0=30, y0=20)["xyz"], "triangulated")
    assert (xyz[..., 2] > 0).all()
    # CAHV cameras: the frames keep their sizes
    ca, cb = tri.cahv_of(ref.stereo_pair()[0]), tri.cahv_of(ref.stereo_pair()[1])
    lo, ro, epi_l, epi_r = stereo.epipolar_transformed_images(left, right, ca, cb, ctx=ctx)
    d0, d1 = ref.epipolar_cahv(ca, cb)
    assert bytes(epi_l.descriptor) == bytes(d0) and bytes(epi_r.descriptor) == bytes(d1)
    same(lo, ref.camera_transform(left, ca, epi_l)["out"], "cahv left")
    same(ro, ref.camera_transform(right, cb, epi_r)["out"], "cahv right")


def _pinhole_words(cam):
    lens = np.zeros(5) if cam.distortion is None else cam.distortion.params
    return np.concatenate([cam.center, cam.rotation.ravel(), [cam.fu, cam.fv, cam.cu, cam.cv, cam.pixel_pitch,
                                                               0.0 if cam.distortion is None else 1.0], lens])


def test_vwlite_program_equals_the_python_calls(ctx, tmp_path):
    """epipolar_view.cc: camera::epipolar, resize_epipolar_cameras_to_fit, camera_transform (a masked view rasterised whole
    with a value edge, a float view box by box with the zero edge) and CameraTransform give what the Python calls give."""
    exe = ref.build_view_program()
    left, right = synth.stereo_pair(ref.SW, ref.SH, 9, block=16)[:2]
    lm = (np.random.default_rng(8).random(left.shape) >= 0.05).astype(np.uint8) * 255
    a, b = ref.stereo_pair(ref.MILD_TSAI)
    np.concatenate([_pinhole_words(a), _pinhole_words(b)]).tofile(str(tmp_path / "cams.bin"))
    left.tofile(str(tmp_path / "left.bin"))
    lm.tofile(str(tmp_path / "lmask.bin"))
    right.tofile(str(tmp_path / "right.bin"))
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, "pair", str(tmp_path / "cams.bin"), str(tmp_path / "left.bin"), str(tmp_path / "lmask.bin"),
                          str(left.shape[1]), str(left.shape[0]), str(tmp_path / "right.bin"), str(right.shape[1]), str(right.shape[0]),
                          prefix], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    e0, e1 = camera.epipolar(a, b)
    e0, e1, s0, s1 = camera.resize_epipolar_cameras_to_fit(a, b, e0, e1, BBox2i(0, 0, left.shape[1], left.shape[0]),
                                                           BBox2i(0, 0, right.shape[1], right.shape[0]), ctx=ctx)
    meta = np.fromfile(prefix + ".meta", np.float64)
    assert (int(meta[0]), int(meta[1])) == s0 and (int(meta[2]), int(meta[3])) == s1
    assert np.fromfile(prefix + ".epi", np.uint8).tobytes() == bytes(e0.descriptor) + bytes(e1.descriptor)
    lo, lom = camera.camera_transform(left, a, e0, size=s0, mask=lm, edge=(7.5, True), ctx=ctx)
    ro = camera.camera_transform(right, b, e1, size=s1, ctx=ctx)
    same(np.fromfile(prefix + ".left", np.float32).reshape(lo.shape), lo, "left")
    same(np.fromfile(prefix + ".lmask", np.uint8).reshape(lom.shape), lom, "left mask")
    same(np.fromfile(prefix + ".right", np.float32).reshape(ro.shape), ro, "right")
    t = camera.CameraTransform(a, e0, ctx=ctx)
    fwd = t.forward(np.array([[left.shape[1] - 1.0, 3.0]]))
    same(meta[4:6], fwd[0], "forward")
    same(meta[6:8], t.reverse(fwd)[0], "reverse")
    # the CAHV overload
    ca, cb = tri.cahv_of(ref.stereo_pair()[0]), tri.cahv_of(ref.stereo_pair()[1])
    np.concatenate([ca.C, ca.A, ca.H, ca.V, cb.C, cb.A, cb.H, cb.V]).tofile(str(tmp_path / "cahv.bin"))
    run = subprocess.run([exe, "cahv", str(tmp_path / "cahv.bin"), prefix + "_cahv"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    g0, g1 = camera.epipolar(ca, cb)
    assert np.fromfile(prefix + "_cahv.epi", np.uint8).tobytes() == bytes(g0.descriptor) + bytes(g1.descriptor)


def test_errors(ctx, source):
    import torch
    img, mask = source
    src, dst = ref.camera_pairs()["pinhole_pinhole"]
    other = ref.stereo_pair()[1]
    with pytest.raises(vwa.LogicErr, match="camera center"):
        camera.camera_transform(img, src, other, ctx=ctx)
    with pytest.raises(vwa.LogicErr, match="camera center"):
        camera.CameraTransform(src, other, ctx=ctx).forward(np.zeros((3, 2)))
    with pytest.raises(vwa.ArgumentErr):
        camera.camera_transform(img, src, dst, size=(0, 5), ctx=ctx)
    with pytest.raises(vwa.ArgumentErr):
        camera.camera_transform(img, src, dst, edge=(float("nan"), True), ctx=ctx)
    with pytest.raises(vwa.ArgumentErr):
        camera.camera_transform(img, src, dst, mask=mask[:-1], ctx=ctx)
    with pytest.raises(vwa.ArgumentErr):
        camera.camera_transform(img, src, dst, mask=torch.from_numpy(mask).cuda(), ctx=ctx)      # mixed sides
    with pytest.raises(vwa.ArgumentErr):
        camera.CameraTransform(src, dst, ctx=ctx).forward(np.zeros((3, 3)))
    # a NaN edge value that is not valid is allowed (the unmasked ZeroEdgeExtension analogue with another value)
    camera.camera_transform(img, src, dst, size=(5, 4), edge=(float("nan"), False), ctx=ctx)

    # the C ABI: every refusal comes before any device work, so host pointers do for the device entry too
    lib, h = ctx._lib, ctx._h
    out = np.empty((ref.SH, ref.SW), np.float32)
    om = np.empty((ref.SH, ref.SW), np.uint8)
    m8 = np.ascontiguousarray(mask)
    bad_kind, bad_lens = _lib.Camera(), _lib.Camera()
    ctypes.memmove(ctypes.addressof(bad_kind), ctypes.addressof(src.descriptor), ctypes.sizeof(_lib.Camera))
    ctypes.memmove(ctypes.addressof(bad_lens), ctypes.addressof(src.descriptor), ctypes.sizeof(_lib.Camera))
    bad_kind.kind, bad_lens.distortion_kind = 2, 5
    base = dict(src=img.ctypes.data, sw=ref.SW, sh=ref.SH, ss=0, smask=m8.ctypes.data, ms=0, sc=ctypes.byref(src.descriptor),
                sm=src.matrix.ctypes.data, dc=ctypes.byref(dst.descriptor), dm=dst.matrix.ctypes.data, w=ref.SW, h=ref.SH, edge=0.0,
                ev=0, out=out.ctypes.data, os=0, om=om.ctypes.data, oms=0)

    def call(entry, **kw):
        a = dict(base, **kw)
        return entry(h, a["src"], a["sw"], a["sh"], a["ss"], a["smask"], a["ms"], a["sc"], a["sm"], a["dc"], a["dm"], a["w"], a["h"], 0, 0,
                     a["edge"], a["ev"], 1, a["out"], a["os"], a["om"], a["oms"], None)
    for entry in (lib.vwgpu_camera_transform, lib.vwgpu_camera_transform_dev):
        for kw in (dict(src=None), dict(out=None), dict(sc=None), dict(dc=None), dict(sw=0), dict(sh=-1), dict(w=0), dict(h=0),
                   dict(ss=ref.SW - 1), dict(ms=ref.SW - 1), dict(os=ref.SW - 1), dict(oms=ref.SW - 1), dict(sm=None), dict(dm=None),
                   dict(sc=ctypes.byref(bad_kind)), dict(dc=ctypes.byref(bad_lens)), dict(out=img.ctypes.data),
                   dict(om=m8.ctypes.data), dict(out=m8.ctypes.data), dict(om=img.ctypes.data), dict(edge=float("nan"), ev=1)):
            assert call(entry, **kw) == -1, (entry, sorted(kw))
            assert lib.vwgpu_last_error(h)
        assert call(entry, dc=ctypes.byref(other.descriptor), dm=other.matrix.ctypes.data) == -5
    assert call(lib.vwgpu_camera_transform) == 0      # and the unmodified call is accepted
    pts = np.zeros((4, 2))
    res = np.empty((4, 2))

    def points(entry, **kw):
        a = dict(dict(sc=base["sc"], sm=base["sm"], dc=base["dc"], dm=base["dm"], direction=0, p=pts.ctypes.data, n=4, out=res.ctypes.data), **kw)
        return entry(h, a["sc"], a["sm"], a["dc"], a["dm"], a["direction"], 1, a["p"], a["n"], a["out"], None)
    for entry in (lib.vwgpu_camera_transform_points, lib.vwgpu_camera_transform_points_dev):
        for kw in (dict(p=None), dict(out=None), dict(n=0), dict(n=-3), dict(direction=2), dict(direction=-1), dict(sc=None), dict(dm=None),
                   dict(sc=ctypes.byref(bad_kind))):
            assert points(entry, **kw) == -1, (entry, sorted(kw))
        assert points(entry, dc=ctypes.byref(other.descriptor), dm=other.matrix.ctypes.data) == -5
    assert points(lib.vwgpu_camera_transform_points) == 0
