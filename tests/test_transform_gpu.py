"""vw::transform on the GPU against the CPU restatement (tests/refimpl/transform_ref.cc): every output word with ==, NaNs
by position.  The scenes and the conditions they meet are checked without a GPU in test_transform_cpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import transform_ref as ref  # noqa: E402
from transform_ref import same  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import _lib, stereo  # noqa: E402
from visionworkbench_amd import transform as tf  # noqa: E402

pytestmark = pytest.mark.gpu
INTERP_TAGS = {ref.NEAREST: tf.NearestPixelInterpolation, ref.BILINEAR: tf.BilinearInterpolation, ref.BICUBIC: tf.BicubicInterpolation}
EDGE_TAGS = {ref.ZERO: tf.ZeroEdgeExtension, ref.CONSTANT: tf.ConstantEdgeExtension, ref.PERIODIC: tf.PeriodicEdgeExtension,
             ref.CYLINDRICAL: tf.CylindricalEdgeExtension, ref.REFLECT: tf.ReflectEdgeExtension, ref.LINEAR: tf.LinearEdgeExtension}
EDGE_VALUE = (7.5, True)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


def edge_tag(edge, value=EDGE_VALUE):
    return tf.ValueEdgeExtension(*value) if edge == ref.VALUE else EDGE_TAGS[edge]


def gpu(ctx, img, steps, size, x0, y0, interp, edge, mask=None, nodata=None, value=EDGE_VALUE):
    """The wrapper's call of one restatement call: out, or (out, mask)."""
    if nodata is None:
        return tf.transform(img, list(steps), size=size, x0=x0, y0=y0, edge=edge_tag(edge, value), interp=INTERP_TAGS[interp], mask=mask, ctx=ctx)
    return tf.transform_nodata(img, list(steps), size, edge_tag(edge, value), INTERP_TAGS[interp], nodata[0], nodata[1], mask=mask, x0=x0, y0=y0,
                               ctx=ctx)


def want(img, steps, size, x0, y0, interp, edge, mask=None, nodata=None, value=EDGE_VALUE):
    r = ref.image(img, steps, size, x0, y0, interp=interp, edge=edge, edge_value=value[0], edge_valid=value[1], mask=mask, nodata=nodata)
    assert r["rc"] == 0
    return r


def check(got, w, masked, what):
    if masked:
        same(got[0], w["out"], what + " image")
        same(got[1], w["mask"], what + " mask")
    else:
        same(got, w["out"], what + " image")


@pytest.mark.parametrize("interp", sorted(ref.INTERPS))
@pytest.mark.parametrize("name", sorted(ref.scenes()))
def test_maps(ctx, name, interp):
    """Every map, unmasked over ZeroEdgeExtension and masked over a valid ValueEdgeExtension pixel."""
    s, it = ref.scenes()[name], ref.INTERPS[interp]
    img, mask = ref.source_image(s["src"])
    for masked, edge in ((False, ref.ZERO), (True, ref.VALUE), (True, ref.ZERO)):
        m = mask if masked else None
        w = want(img, s["steps"], s["size"], s["x0"], s["y0"], it, edge, m)
        check(gpu(ctx, img, s["steps"], s["size"], s["x0"], s["y0"], it, edge, m), w, masked, "%s %s" % (name, interp))


@pytest.mark.parametrize("edge", sorted(ref.EDGES))
@pytest.mark.parametrize("interp", sorted(ref.INTERPS))
def test_every_interpolation_and_edge(ctx, interp, edge):
    """interpolation x edge kind on the rotated scene, unmasked and masked (Linear masked is refused), nodata on and off."""
    s, it, e = ref.scenes()["rotate"], ref.INTERPS[interp], ref.EDGES[edge]
    img, mask = ref.source_image(s["src"])
    for masked in (False, True):
        for nodata in (None, (-32768.0, False), (3.0, True)):
            m = mask if masked else None
            if masked and e == ref.LINEAR:
                with pytest.raises(vwa.NoImplErr):
                    gpu(ctx, img, s["steps"], s["size"], s["x0"], s["y0"], it, e, m, nodata)
                continue
            w = want(img, s["steps"], s["size"], s["x0"], s["y0"], it, e, m, nodata)
            check(gpu(ctx, img, s["steps"], s["size"], s["x0"], s["y0"], it, e, m, nodata), w, masked, "%s %s nodata %r" % (interp, edge, nodata))


@pytest.mark.parametrize("interp", sorted(ref.INTERPS))
@pytest.mark.parametrize("src", ref.SOURCE_SIZES)
def test_source_and_output_sizes(ctx, src, interp):
    """A single pixel, a single row, tiny and odd sources, over outputs that are no multiple of 64 x 4; every edge kind the
    source's size allows (Reflect and Linear need two pixels a side)."""
    it = ref.INTERPS[interp]
    img, mask = ref.source_image(src)
    steps = [ref.made(ref.TRANSLATE, (0.375, -1.25)), ref.rotate(0.1, src[0] / 2.0, src[1] / 2.0), ref.made(ref.RESAMPLE, (3.0, 0.75))]
    for size in ref.OUTPUT_SIZES:
        for e in sorted(ref.EDGES.values()):
            if e in (ref.REFLECT, ref.LINEAR) and min(src) < 2:
                continue
            for masked in ((False,) if e == ref.LINEAR else (False, True)):
                m = mask if masked else None
                w = want(img, steps, size, -5, -3, it, e, m)
                check(gpu(ctx, img, steps, size, -5, -3, it, e, m), w, masked, "%dx%d -> %dx%d edge %d" % (src + size + (e,)))


def test_inverse_and_chain_by_hand(ctx):
    """InverseTransform of a functor against the restatement's inverted descriptor; inverting twice gives the map back;
    compose of three functors against the restatement's chain, and against the three reverses applied by hand."""
    img, mask = ref.source_image((70, 45))
    shear = tf.AffineTransform([[1.1, 0.2], [-0.1, 0.9]], (3.5, -2.25))
    s = ref.scenes()["inverse"]
    w = want(img, s["steps"], s["size"], s["x0"], s["y0"], ref.BICUBIC, ref.REFLECT, mask)
    got = tf.transform(img, tf.InverseTransform(shear), size=s["size"], x0=s["x0"], y0=s["y0"], edge=tf.ReflectEdgeExtension,
                       interp=tf.BicubicInterpolation, mask=mask, ctx=ctx)
    check(got, w, True, "InverseTransform")
    # twice inverted is the map itself
    w = want(img, ref.scenes()["shear"]["steps"], (70, 9), 0, 0, ref.BILINEAR, ref.ZERO)
    same(tf.transform(img, tf.InverseTransform(tf.InverseTransform(shear)), size=(70, 9), ctx=ctx), w["out"], "inverted twice")
    s = ref.scenes()["chain3"]
    t, r, k = tf.TranslateTransform(2.5, -1.0), tf.RotateTransform(0.2, (30.0, 20.0)), tf.ResampleTransform(1.25, 0.8)
    w = want(img, s["steps"], s["size"], s["x0"], s["y0"], ref.BILINEAR, ref.PERIODIC, mask)
    got = tf.transform(img, tf.compose(t, r, k), size=s["size"], x0=s["x0"], y0=s["y0"], edge=tf.PeriodicEdgeExtension, mask=mask, ctx=ctx)
    check(got, w, True, "compose")
    # by hand: the positions of the three reverses in turn, sampled by the restatement through a translation per pixel
    ys, xs = np.mgrid[0:3, 0:5]
    p = np.stack([xs.ravel() + s["x0"] + 40.0, ys.ravel() + s["y0"] + 4.0], 1)
    q = ref.points([s["steps"][2]], ref.REVERSE, ref.points([s["steps"][1]], ref.REVERSE, ref.points([s["steps"][0]], ref.REVERSE, p)[1])[1])[1]
    tile = tf.transform(img, tf.compose(t, r, k), size=(5, 3), x0=s["x0"] + 40, y0=s["y0"] + 4, edge=tf.PeriodicEdgeExtension, ctx=ctx)
    by_hand = np.array([ref.at(img, qx, qy, ref.BILINEAR, ref.PERIODIC) for qx, qy in q], np.float32).reshape(3, 5)
    same(tile, by_hand, "three steps by hand")


def test_tiles_equal_the_whole(ctx):
    """The whole call equals the call assembled from 32 x 8 tiles through x0, y0."""
    for name, it, e in (("homography", ref.BICUBIC, ref.CYLINDRICAL), ("w_zero", ref.BILINEAR, ref.VALUE), ("rotate", ref.NEAREST, ref.ZERO)):
        s = ref.scenes()[name]
        img, mask = ref.source_image(s["src"])
        w, h = s["size"]
        whole = gpu(ctx, img, s["steps"], s["size"], s["x0"], s["y0"], it, e, mask)
        out, om = np.empty((h, w), np.float32), np.empty((h, w), np.uint8)
        for ty in range(0, h, 8):
            for tx in range(0, w, 32):
                tw, th = min(32, w - tx), min(8, h - ty)
                o, k = gpu(ctx, img, s["steps"], (tw, th), s["x0"] + tx, s["y0"] + ty, it, e, mask)
                out[ty:ty + th, tx:tx + tw], om[ty:ty + th, tx:tx + tw] = o, k
        same(out, whole[0], name + " tiles image")
        same(om, whole[1], name + " tiles mask")


def _raw_dev(ctx, img, mask, steps, params, w, h, x0, y0, pads=(0, 0, 0, 0)):
    """vwgpu_transform_image_dev on tensors whose rows are pads[k] elements wider than the images, the padding NaN (255 for
    the masks): (out, mask, rc) with the padding."""
    import torch
    dev = torch.device("cuda", 0)
    sh, sw = img.shape

    def padded(a, pad, fill):
        t = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.from_numpy(a[:1, :1].copy()).dtype, device=dev)
        t[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t
    timg = padded(img, pads[0], float("nan"))
    tmask = None if mask is None else padded(mask, pads[1], 255)
    tout = torch.full((h, w + pads[2]), float("nan"), dtype=torch.float32, device=dev)
    tom = None if mask is None else torch.full((h, w + pads[3]), 99, dtype=torch.uint8, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    arr = (_lib.Transform * len(steps))(*steps)
    rc = ctx._lib.vwgpu_transform_image_dev(
        ctx._h, timg.data_ptr(), sw, sh, timg.stride(0), None if tmask is None else tmask.data_ptr(), 0 if tmask is None else tmask.stride(0),
        arr, len(steps), ctypes.byref(params), w, h, x0, y0, tout.data_ptr(), tout.stride(0), None if tom is None else tom.data_ptr(),
        0 if tom is None else tom.stride(0))
    torch.cuda.synchronize()
    return tout.cpu().numpy(), None if tom is None else tom.cpu().numpy(), rc


@pytest.mark.parametrize("interp", sorted(ref.INTERPS))
def test_row_strides(ctx, interp):
    """Strided source, masks and output, the padding filled with NaN: no tap reads it and no store writes it."""
    it = ref.INTERPS[interp]
    s = ref.scenes()["shear"]
    img, mask = ref.source_image(s["src"])
    (w, h) = s["size"]
    for masked in (False, True):
        m = mask if masked else None
        r = want(img, s["steps"], s["size"], s["x0"], s["y0"], it, ref.CONSTANT, m)
        params = _lib.TransformParams(it, ref.CONSTANT, 0.0, 0, 0, 0.0, 0)
        out, om, rc = _raw_dev(ctx, img, m, s["steps"], params, w, h, s["x0"], s["y0"], pads=(3, 5, 7, 2))
        assert rc == 0
        same(out[:, :w], r["out"], "strided image")
        assert np.isnan(out[:, w:]).all()
        if masked:
            same(om[:, :w], r["mask"], "strided mask")
            assert (om[:, w:] == 99).all()
    # a strided tensor passed as a view through the wrapper
    import torch
    wide = np.full((img.shape[0], img.shape[1] + 4), np.nan, np.float32)
    wide[:, :img.shape[1]] = img
    t = torch.from_numpy(wide).cuda()
    got = tf.transform(t[:, :img.shape[1]], s["steps"], size=s["size"], x0=s["x0"], y0=s["y0"], edge=tf.ConstantEdgeExtension,
                       interp=INTERP_TAGS[it], mask=torch.from_numpy(mask).cuda(), ctx=ctx)
    same(got[0].cpu().numpy(), r["out"], "tensor view image")
    same(got[1].cpu().numpy(), r["mask"], "tensor view mask")


@pytest.mark.parametrize("masked", [False, True])
def test_host_and_device_entries_agree(ctx, masked):
    import torch
    s = ref.scenes()["homography"]
    img, mask = ref.source_image(s["src"])
    for it in (ref.NEAREST, ref.BILINEAR, ref.BICUBIC):
        m = mask if masked else None
        host = gpu(ctx, img, s["steps"], s["size"], s["x0"], s["y0"], it, ref.VALUE, m, (2.0, True))
        dev = gpu(ctx, torch.from_numpy(img).cuda(), s["steps"], s["size"], s["x0"], s["y0"], it, ref.VALUE,
                  None if m is None else torch.from_numpy(m).cuda(), (2.0, True))
        if masked:
            same(dev[0].cpu().numpy(), host[0], "image")
            same(dev[1].cpu().numpy(), host[1], "mask")
        else:
            same(dev.cpu().numpy(), host, "image")


def test_free_functions(ctx):
    """resample, resize, translate (both forms) and rotate with the reference's defaults, and the known answers of the
    reference's unit tests on the 2 x 3 image."""
    img, mask = ref.source_image((37, 23))
    w = want(img, [ref.made(ref.RESAMPLE, (2.0, 2.0))], (74, 46), 0, 0, ref.BILINEAR, ref.CONSTANT)
    same(tf.resample(img, 2, ctx=ctx), w["out"], "resample 2")
    w = want(img, [ref.made(ref.RESAMPLE, (0.5, 0.5))], (19, 12), 0, 0, ref.BILINEAR, ref.CONSTANT)
    same(tf.resample(img, 0.5, ctx=ctx), w["out"], "resample 0.5")
    for size in ((51, 9), (13, 31)):
        steps = [ref.made(ref.RESAMPLE, (size[0] / 37.0, size[1] / 23.0))]
        for it in (ref.BILINEAR, ref.BICUBIC):
            w = want(img, steps, size, 0, 0, it, ref.CONSTANT, mask)
            check(tf.resize(img, size[0], size[1], interp=INTERP_TAGS[it], mask=mask, ctx=ctx), w, True, "resize %dx%d" % size)
    for offset in ((3, -2), (3.0, -2.0), (0.375, -1.25)):
        w = want(img, [ref.made(ref.TRANSLATE, [float(v) for v in offset])], (37, 23), 0, 0, ref.BILINEAR, ref.ZERO)
        same(tf.translate(img, offset[0], offset[1], ctx=ctx), w["out"], "translate %r" % (offset,))
    w = want(img, [ref.rotate(0.3, 18.0, 11.0)], (37, 23), 0, 0, ref.BILINEAR, ref.ZERO)
    same(tf.rotate(img, 0.3, (18.0, 11.0), ctx=ctx), w["out"], "rotate")
    im = ref.sample_image()
    assert tf.resample(im, 2, 2, ctx=ctx).shape == (6, 4)
    got = tf.resample(im, 2, 2, ctx=ctx)
    assert (got[0, 0], got[2, 2], got[1, 1]) == (1, 4, 2.5)
    assert np.array_equal(tf.translate(im, 1, 1, ctx=ctx), [[0, 0], [0, 1], [0, 3]])
    assert np.array_equal(tf.transform(im, tf.IdentityTransform(), ctx=ctx), im)
    sq = np.array([[127, 255], [0, 64]], np.float32)
    assert np.abs(tf.rotate(sq, 2 * np.pi, (0.5, 0.5), ctx=ctx) - sq).max() < 1e-3


def test_translate_equals_disparity_warp(ctx):
    """translate(-dx, -dy), bilinear over ZeroEdgeExtension, is vwgpu_disparity_warp on a constant valid disparity (dx, dy)
    with dyadic dx, dy, bit for bit: two kernels of the library that were written apart."""
    img, _ = ref.source_image((70, 45))
    for dx, dy in ((0.375, -1.25), (3.0, -2.0), (-7.5, 0.0625)):
        d = np.zeros((45, 70, 3), np.float32)
        d[..., 0], d[..., 1], d[..., 2] = dx, dy, 1
        same(tf.translate(img, -dx, -dy, ctx=ctx), stereo.disparity_transform_image(img, d, ctx=ctx), "dx %r dy %r" % (dx, dy))


def test_refusals_write_nothing(ctx):
    lib, h = ctx._lib, ctx._h
    img, mask = ref.source_image((37, 23))
    sw, sh = 37, 23
    m8 = np.ascontiguousarray(mask)
    out = np.full((sh, sw), -77.0, np.float32)
    om = np.full((sh, sw), 99, np.uint8)
    ok = ref.made(ref.TRANSLATE, (0.375, -1.25))
    bad_kind, bad_word = ref.by_hand(5), ref.by_hand(ref.TRANSLATE)
    bad_word.reserved = 2
    one = (_lib.Transform * 1)(ok)
    five = (_lib.Transform * 5)(ok, ok, ok, ok, ok)
    tiny = np.ones((1, 5), np.float32)

    def P(interp=1, edge=0, edge_value=0.0, edge_valid=0, nodata=0, nodata_value=0.0, nodata_valid=0):
        return _lib.TransformParams(interp, edge, edge_value, edge_valid, nodata, nodata_value, nodata_valid)
    base = dict(src=img.ctypes.data, sw=sw, sh=sh, ss=0, smask=m8.ctypes.data, ms=0, steps=one, n=1, params=P(), w=sw, h=sh,
                out=out.ctypes.data, os=0, om=om.ctypes.data, oms=0)

    def call(entry, **kw):
        a = dict(base, **kw)
        p = a["params"]
        return entry(h, a["src"], a["sw"], a["sh"], a["ss"], a["smask"], a["ms"], a["steps"], a["n"], None if p is None else ctypes.byref(p),
                     a["w"], a["h"], 0, 0, a["out"], a["os"], a["om"], a["oms"])
    nan = float("nan")
    refused = [dict(src=None), dict(out=None), dict(steps=None), dict(params=None), dict(sw=0), dict(sh=-1), dict(w=0), dict(h=-2),
               dict(ss=sw - 1), dict(ms=sw - 1), dict(os=sw - 1), dict(oms=sw - 1), dict(n=0), dict(n=5, steps=five), dict(n=-1),
               dict(steps=(_lib.Transform * 1)(bad_kind)), dict(steps=(_lib.Transform * 1)(bad_word)),
               dict(params=P(interp=3)), dict(params=P(interp=-1)), dict(params=P(edge=7)), dict(params=P(edge=-1)),
               dict(smask=None), dict(om=None),      # one mask without the other
               dict(out=img.ctypes.data), dict(om=m8.ctypes.data), dict(out=m8.ctypes.data), dict(om=img.ctypes.data), dict(om=out.ctypes.data),
               dict(params=P(edge=1, edge_value=nan, edge_valid=1)), dict(params=P(nodata=1, nodata_value=nan, nodata_valid=1)),
               dict(params=P(edge=5), src=tiny.ctypes.data, sw=1, sh=5, smask=None, om=None),      # Reflect on a side of 1: % 0
               dict(params=P(edge=5), src=tiny.ctypes.data, sw=5, sh=1, smask=None, om=None),
               dict(params=P(edge=6), src=tiny.ctypes.data, sw=5, sh=1, smask=None, om=None),      # Linear on a side below 2
               dict(params=P(edge=6), src=tiny.ctypes.data, sw=1, sh=5, smask=None, om=None)]
    for entry in (lib.vwgpu_transform_image, lib.vwgpu_transform_image_dev):
        for kw in refused:
            assert call(entry, **kw) == -1, (entry, sorted(kw))
            assert lib.vwgpu_last_error(h)
        assert call(entry, params=P(edge=6)) == -2      # Linear with a mask: VWGPU_ERR_NOIMPL
        assert "Linear" in lib.vwgpu_last_error(h).decode()
    assert (out == -77.0).all() and (om == 99).all(), "a refused call wrote something"
    # what is allowed: a NaN edge or nodata value that is not valid, and one that no kind uses
    for kw in (dict(), dict(params=P(edge=1, edge_value=nan)), dict(params=P(nodata=1, nodata_value=nan)), dict(params=P(edge=0, edge_value=nan, edge_valid=1)),
               dict(params=P(edge=6), smask=None, om=None)):
        assert call(lib.vwgpu_transform_image, **kw) == 0, sorted(kw)
    # the wrapper's errors
    import torch
    with pytest.raises(vwa.ArgumentErr):
        tf.transform(img, ok, mask=torch.from_numpy(mask).cuda(), ctx=ctx)      # mixed sides
    with pytest.raises(vwa.ArgumentErr):
        tf.transform(img, ok, edge=tf.ValueEdgeExtension(nan, True), mask=mask, ctx=ctx)


def test_vwlite_program_equals_the_restatement(ctx, tmp_path):
    """transform_view.cc: the functors, transform over a box rasterised tile by tile, transform_nodata, resample, resize,
    translate and rotate of vw/Transform.h, as a reference user would call them."""
    exe = ref.build_view_program()
    img, mask = ref.source_image((70, 45))
    img.tofile(str(tmp_path / "src.bin"))
    mask.tofile(str(tmp_path / "mask.bin"))
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, str(tmp_path / "src.bin"), str(tmp_path / "mask.bin"), "70", "45", prefix], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout

    def read(name, size, masked=False):
        out = np.fromfile("%s.%s" % (prefix, name), np.float32).reshape(size[1], size[0])
        return (out, np.fromfile("%s.%s_mask" % (prefix, name), np.uint8).reshape(size[1], size[0])) if masked else out
    shear = ref.made(ref.AFFINE, (1.1, 0.2, -0.1, 0.9, 3.5, -2.25))
    same(read("affine", (70, 9)), want(img, [shear], (70, 9), 0, 0, ref.BICUBIC, ref.REFLECT)["out"], "affine")
    s = ref.scenes()["chain3"]
    check(read("chain", s["size"], True), want(img, s["steps"], s["size"], s["x0"], s["y0"], ref.BILINEAR, ref.VALUE, mask), True, "chain")
    same(read("resample", (35, 23)), want(img, [ref.made(ref.RESAMPLE, (0.5, 0.5))], (35, 23), 0, 0, ref.BILINEAR, ref.CONSTANT)["out"], "resample")
    same(read("resize", (51, 9)), want(img, [ref.made(ref.RESAMPLE, (51 / 70.0, 9 / 45.0))], (51, 9), 0, 0, ref.BILINEAR, ref.CONSTANT)["out"], "resize")
    same(read("translate", (70, 45)), want(img, [ref.made(ref.TRANSLATE, (3.0, -2.0))], (70, 45), 0, 0, ref.BILINEAR, ref.ZERO)["out"], "translate")
    same(read("rotate", (70, 45)), want(img, [ref.rotate(0.3, 34.5, 22.0)], (70, 45), 0, 0, ref.BILINEAR, ref.ZERO)["out"], "rotate")
    check(read("nodata", (70, 9), True), want(img, [ref.invert(shear)], (70, 9), 0, 0, ref.BICUBIC, ref.CONSTANT, mask, (-1.0, False)), True, "nodata")
    same(read("periodic", (70, 9)), want(img, [ref.made(ref.HOMOGRAPHY, (1.01, 0.02, -1.5, -0.01, 0.99, 2.0, 1e-4, -2e-4, 1.0))], (70, 9), 0, 0,
                                         ref.NEAREST, ref.PERIODIC)["out"], "homography")
    meta = np.fromfile(prefix + ".meta", np.float64)
    rot = ref.rotate(np.pi / 2, 1.0, 1.0)
    same(meta[0:2], ref.points([rot], ref.FORWARD, [[3.0, 1.0]])[1][0], "forward")
    same(meta[2:4], ref.points([rot], ref.REVERSE, [[3.0, 1.0]])[1][0], "reverse")
    same(meta[4:6], ref.points(s["steps"], ref.FORWARD, [[12.0, 7.0]])[1][0], "compose forward")
    same(meta[6:8], ref.points([ref.invert(shear)], ref.FORWARD, [[12.0, 7.0]])[1][0], "inverse forward")
