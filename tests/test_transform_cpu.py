"""vw::transform without a GPU: the CPU restatement (tests/refimpl/transform_ref.cc) against the reference's own known
answers, the pure-host entries of the library against the restatement word for word, their refusals, the ABI, what the
wrappers of transform.py hand to the library, and the conditions the scenes of test_transform_gpu.py have to meet."""
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import transform_ref as ref  # noqa: E402

from visionworkbench_amd import _lib, stereo  # noqa: E402
from visionworkbench_amd import transform as tf  # noqa: E402
from visionworkbench_amd.core import ArgumentErr, BBox2i  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "transform_known.json")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def known():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _image_of(known):
    g = known["image"]
    return np.array(g["pixels"], np.float32).reshape(g["rows"], g["cols"])


# ---- the restatement against the reference's unit tests --------------------------------------------------------------------

def test_restatement_interpolation_known_answers(known):
    im = _image_of(known)
    assert np.array_equal(im, ref.sample_image())
    for case in known["interpolation"]:
        got = ref.at(im, case["at"][0], case["at"][1], ref.INTERPS[case["interp"]], ref.EDGES[case["edge"]])
        assert abs(got - case["value"]) <= case["tol"], case


def test_restatement_edge_extension_tables(known):
    """Every index of TestEdgeExtension.cxx, through each interpolation: an integer position is one tap."""
    im = _image_of(known)
    for edge, table in known["edge_extension"].items():
        assert len(table) == 18
        for i, j, value in table:
            for interp in (ref.NEAREST, ref.BILINEAR, ref.BICUBIC):
                r = ref.image(im, [ref.made(ref.IDENTITY)], (1, 1), x0=i, y0=j, interp=interp, edge=ref.EDGES[edge])
                assert r["rc"] == 0 and r["out"][0, 0] == value, (edge, i, j, interp)


def test_restatement_transform_known_answers(known):
    im = _image_of(known)
    g = known["translate"]
    for x, y, value in g["pixels"]:
        r = ref.image(im, [ref.made(ref.TRANSLATE, g["offset"])], (1, 1), x0=x, y0=y, interp=ref.INTERPS[g["interp"]], edge=ref.EDGES[g["edge"]])
        assert r["out"][0, 0] == value, (x, y)
    g = known["resample"]
    assert [int(.5 + im.shape[1] * g["factor"][0]), int(.5 + im.shape[0] * g["factor"][1])] == g["size"]
    for x, y, value in g["pixels"]:
        r = ref.image(im, [ref.made(ref.RESAMPLE, g["factor"])], (1, 1), x0=x, y0=y, interp=ref.INTERPS[g["interp"]], edge=ref.EDGES[g["edge"]])
        assert r["out"][0, 0] == value, (x, y)
    g = known["rotate_full_turn"]
    sq = np.array([[127, 255], [0, 64]], np.float32)
    r = ref.image(sq, [ref.rotate(g["turns_of_pi"] * math.pi, 0.5, 0.5)], (2, 2))
    assert np.abs(r["out"] - sq).max() < 1e-3       # EXPECT_MATRIX_EQ on uint8 pixels: equal after rounding
    g = known["rotate_points"]
    rot = ref.rotate(g["turns_of_pi"] * math.pi, g["about"][0], g["about"][1])
    assert np.abs(ref.points([rot], ref.FORWARD, [g["point"]])[1][0] - g["forward"]).max() < g["tol"]
    assert np.abs(ref.points([rot], ref.REVERSE, [g["point"]])[1][0] - g["reverse"]).max() < g["tol"]


# ---- the pure-host entries against the restatement ---------------------------------------------------------------------------

MAKES = [(ref.IDENTITY, ()), (ref.TRANSLATE, (0.375, -1.25)), (ref.TRANSLATE, (-0.0, 1e300)), (ref.RESAMPLE, (2.0, 0.5)),
         (ref.RESAMPLE, (-3.0, 1e-310)), (ref.AFFINE, (1.1, 0.2, -0.1, 0.9, 3.5, -2.25)), (ref.AFFINE, (0.0, 1.0, 1.0, 0.0, 0.0, 0.0)),
         (ref.AFFINE, (1e200, 0.0, 0.0, 1e-200, 1.0, 2.0)), (ref.HOMOGRAPHY, (1.01, 0.02, -1.5, -0.01, 0.99, 2.0, 1e-4, -2e-4, 1.0)),
         (ref.HOMOGRAPHY, (0.0, 2.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, -3.0))]
REFUSED = [(ref.IDENTITY, (1.0,)), (ref.TRANSLATE, (1.0,)), (ref.TRANSLATE, (1.0, 2.0, 3.0)), (ref.TRANSLATE, (NAN, 0.0)),
           (ref.RESAMPLE, (0.0, 1.0)), (ref.RESAMPLE, (1.0, -0.0)), (ref.RESAMPLE, (INF, 1.0)), (ref.AFFINE, (1.0, 2.0, 2.0, 4.0, 0.0, 0.0)),
           (ref.AFFINE, (1.0, 0.0, 0.0, 1.0, NAN, 0.0)), (ref.AFFINE, (1.0, 0.0, 0.0, 1.0, 0.0)),
           (ref.HOMOGRAPHY, (1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.0, 0.0, 1.0)), (ref.HOMOGRAPHY, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)),
           (ref.HOMOGRAPHY, (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -INF)), (5, ()), (-1, ()), (ref.AFFINE, ())]


def _lib_make(lib, kind, params):
    d = _lib.Transform()
    ctypes.memset(ctypes.addressof(d), 0xff, ctypes.sizeof(d))
    p = np.ascontiguousarray(params, np.float64).reshape(-1)
    return lib.vwgpu_transform_make(kind, p.ctypes.data if p.size else None, int(p.size), ctypes.byref(d)), d


def test_make_rotate_invert_equal_the_restatement(lib):
    for kind, params in MAKES:
        rc, got = _lib_make(lib, kind, params)
        wrc, want = ref.make(kind, params)
        assert rc == wrc == 0 and bytes(got) == bytes(want), (kind, params)
        inv, winv = _lib.Transform(), ref.invert(want)
        assert lib.vwgpu_transform_invert(ctypes.byref(got), ctypes.byref(inv)) == 0 and bytes(inv) == bytes(winv)
        assert lib.vwgpu_transform_invert(ctypes.byref(inv), ctypes.byref(inv)) == 0 and bytes(inv) == bytes(want)      # in place, and back
    for theta, cx, cy in ((0.3, 34.5, 22.0), (math.pi / 2, 1.0, 1.0), (2 * math.pi, 0.5, 1.0), (-1e3, -7.25, 1e6), (0.0, 0.0, 0.0)):
        got = _lib.Transform()
        assert lib.vwgpu_transform_rotate(theta, cx, cy, ctypes.byref(got)) == 0
        assert bytes(got) == bytes(ref.rotate(theta, cx, cy)), theta


POINTS = np.array([[0.0, 0.0], [12.0, 7.0], [-3.5, 2.25], [-0.0, -1e-300], [1e300, -1e300], [1.5e9, 3.0], [NAN, 1.0], [2.0, NAN], [INF, -INF],
                   [16.0, 0.0], [16.0, 5.0], [15.999999999999998, 1.0], [-1e-320, 4.0]])


def test_points_equal_the_restatement(lib):
    """Every kind, inverted too, in both directions, and chains of 2, 3 and 4; the w = 0 homography divides by zero in
    column 16 (infinities and a NaN), and the NaN, infinite and huge points go through as IEEE arithmetic takes them."""
    singles = [ref.made(k, p) for k, p in MAKES] + [ref.rotate(0.3, 34.5, 22.0), ref.by_hand(ref.HOMOGRAPHY, fwd=ref.W0_REV, rev=ref.W0_REV)]
    chains = [[s] for s in singles] + [[ref.invert(s)] for s in singles]
    chains += [singles[1:3], [singles[5], ref.invert(singles[8]), singles[3]], [singles[1], singles[10], singles[3], singles[8]],
               ref.scenes()["chain3"]["steps"]]
    for chain in chains:
        arr = (_lib.Transform * len(chain))(*chain)
        for direction in (ref.FORWARD, ref.REVERSE):
            wrc, want = ref.points(chain, direction, POINTS)
            got = np.empty_like(POINTS)
            assert lib.vwgpu_transform_points(arr, len(chain), direction, POINTS.ctypes.data, len(POINTS), got.ctypes.data) == wrc == 0
            ref.same(got, want, "chain of %d, direction %d" % (len(chain), direction))
            inplace = POINTS.copy()      # out == points
            assert lib.vwgpu_transform_points(arr, len(chain), direction, inplace.ctypes.data, len(POINTS), inplace.ctypes.data) == 0
            ref.same(inplace, want, "in place")
    w0 = ref.points([ref.by_hand(ref.HOMOGRAPHY, rev=ref.W0_REV)], ref.REVERSE, [[16.0, 0.0], [16.0, 5.0]])[1]
    assert np.isinf(w0[0, 0]) and np.isnan(w0[0, 1]) and np.isinf(w0[1]).all()      # 8 / 0, 0 / 0; 8 / 0, 1.25 / 0
    # a chain of three is the three applied by hand
    a, b, c = ref.scenes()["chain3"]["steps"]
    by_hand = ref.points([c], ref.REVERSE, ref.points([b], ref.REVERSE, ref.points([a], ref.REVERSE, POINTS)[1])[1])[1]
    ref.same(ref.points([a, b, c], ref.REVERSE, POINTS)[1], by_hand, "reverse by hand")
    by_hand = ref.points([a], ref.FORWARD, ref.points([b], ref.FORWARD, ref.points([c], ref.FORWARD, POINTS)[1])[1])[1]
    ref.same(ref.points([a, b, c], ref.FORWARD, POINTS)[1], by_hand, "forward by hand")


def test_refusals_of_the_host_entries(lib):
    for kind, params in REFUSED:
        rc, got = _lib_make(lib, kind, params)
        wrc, want = ref.make(kind, params)
        assert rc == -1 and wrc == -1, (kind, params)
        assert bytes(got) == b"\xff" * ctypes.sizeof(got) == bytes(want), "out must be unchanged"
    ok = ref.made(ref.TRANSLATE, (1.0, 2.0))
    two = np.array([1.0, 2.0])
    assert lib.vwgpu_transform_make(ref.TRANSLATE, two.ctypes.data, 2, None) == -1
    assert lib.vwgpu_transform_make(ref.TRANSLATE, None, 2, ctypes.byref(_lib.Transform())) == -1
    out = _lib.Transform()
    assert lib.vwgpu_transform_rotate(0.1, 0.0, 0.0, None) == -1
    for bad in ((NAN, 0.0, 0.0), (0.1, INF, 0.0), (0.1, 0.0, NAN)):
        assert lib.vwgpu_transform_rotate(bad[0], bad[1], bad[2], ctypes.byref(out)) == -1
    assert lib.vwgpu_transform_invert(None, ctypes.byref(out)) == -1 and lib.vwgpu_transform_invert(ctypes.byref(ok), None) == -1
    bad_kind, bad_word = ref.by_hand(5), ref.by_hand(ref.TRANSLATE)
    bad_word.reserved = 2
    assert lib.vwgpu_transform_invert(ctypes.byref(bad_kind), ctypes.byref(out)) == -1
    assert lib.vwgpu_transform_invert(ctypes.byref(bad_word), ctypes.byref(out)) == -1
    pts, res = np.zeros((3, 2)), np.full((3, 2), 7.0)
    one = (_lib.Transform * 1)(ok)
    five = (_lib.Transform * 5)(ok, ok, ok, ok, ok)

    def points(steps=one, n=1, direction=0, p=pts.ctypes.data, count=3, out=res.ctypes.data):
        return lib.vwgpu_transform_points(steps, n, direction, p, count, out)
    assert points() == 0
    for kw in (dict(steps=None), dict(n=0), dict(n=5, steps=five), dict(direction=2), dict(direction=-1), dict(p=None), dict(out=None),
               dict(count=-1), dict(steps=(_lib.Transform * 1)(bad_kind)), dict(steps=(_lib.Transform * 1)(bad_word))):
        res[:] = 7.0
        assert points(**kw) == -1, sorted(kw)
        assert (res == 7.0).all()
    assert points(count=0) == 0 and points(count=0, p=None, out=None) == 0
    assert ref.points([ok] * 5, 0, pts)[0] == -1 and ref.points([bad_kind], 0, pts)[0] == -1 and ref.points([ok], 2, pts)[0] == -1


# ---- the ABI -----------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ["vwgpu_transform_make", "vwgpu_transform_rotate", "vwgpu_transform_invert", "vwgpu_transform_points",
               "vwgpu_transform_image_dev", "vwgpu_transform_image"]


def test_abi(lib):
    with open(os.path.join(ROOT, "include", "vwgpu.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SYMBOLS and getattr(lib, name)
    assert lib.vwgpu_abi_version() == 3
    assert re.search(r"VWGPU_EDGE_CONSTANT = 0, VWGPU_EDGE_ZERO = 1 }", header)      # vwgpu_edge keeps its two values
    for enum, names in (("vwgpu_transform_kind", ["IDENTITY", "TRANSLATE", "RESAMPLE", "AFFINE", "HOMOGRAPHY"]),
                        ("vwgpu_transform_interp", ["INTERP_NEAREST", "INTERP_BILINEAR", "INTERP_BICUBIC"]),
                        ("vwgpu_transform_edge", ["EDGE_ZERO", "EDGE_VALUE", "EDGE_CONSTANT", "EDGE_PERIODIC", "EDGE_CYLINDRICAL",
                                                  "EDGE_REFLECT", "EDGE_LINEAR"])):
        body = re.search(r"typedef enum %s \{(.*?)\}" % enum, header, re.S).group(1)
        assert [(n, int(v)) for n, v in re.findall(r"VWGPU_TRANSFORM_(\w+) = (\d+)", body)] == [(n, k) for k, n in enumerate(names)]
    assert ctypes.sizeof(_lib.Transform) == 8 + 18 * 8 and ctypes.sizeof(_lib.TransformParams) == 28
    assert (tf.IDENTITY, tf.TRANSLATE, tf.RESAMPLE, tf.AFFINE, tf.HOMOGRAPHY) == (0, 1, 2, 3, 4)
    assert [e.code for e in (tf.ZeroEdgeExtension, tf.ValueEdgeExtension, tf.ConstantEdgeExtension, tf.PeriodicEdgeExtension,
                             tf.CylindricalEdgeExtension, tf.ReflectEdgeExtension, tf.LinearEdgeExtension)] == list(range(7))
    assert [(i.code, i.pixel_buffer) for i in (tf.NearestPixelInterpolation, tf.BilinearInterpolation, tf.BicubicInterpolation)] == [
        (0, 1), (1, 1), (2, 2)]


# ---- the wrappers ------------------------------------------------------------------------------------------------------------

class Recorder(object):
    """Stands for ctx._lib: records (entry, arguments) and answers 0; ctypes arguments are read at call time."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, [_snapshot(a) for a in args]))
            return 0
        return entry


def _snapshot(a):
    if isinstance(a, ctypes.Array):
        return [bytes(x) for x in a]
    if hasattr(a, "_obj"):      # ctypes.byref(x)
        return {f[0]: getattr(a._obj, f[0]) for f in a._obj._fields_}
    return a


class FakeContext(object):
    _h = "ctx"

    def __init__(self):
        self._lib = Recorder()

    def check(self, rc):
        assert rc == 0

    def set_stream(self, stream):
        pytest.fail("a numpy call must not touch the stream")


def _one_call(fn, *args, **kw):
    ctx = FakeContext()
    res = fn(*args, ctx=ctx, **kw)
    assert len(ctx._lib.calls) == 1
    name, a = ctx._lib.calls[0]
    assert name == "vwgpu_transform_image" and a[0] == "ctx" and len(a) == 18
    keys = ["ctx", "src", "sw", "sh", "sstride", "mask", "mstride", "steps", "n", "params", "w", "h", "x0", "y0", "out", "ostride", "omask", "omstride"]
    return res, dict(zip(keys, a))


def _params(interp, edge, edge_value=0.0, edge_valid=0, nodata=0, nodata_value=0.0, nodata_valid=0):
    return dict(interp=interp, edge=edge, edge_value=edge_value, edge_valid=edge_valid, nodata=nodata, nodata_value=nodata_value,
                nodata_valid=nodata_valid)


def test_wrappers_hand_the_library_what_the_reference_defaults_say():
    img = np.arange(35, dtype=np.float32).reshape(5, 7)
    mask = np.ones((5, 7), np.uint8)
    shear = tf.AffineTransform([[1.1, 0.2], [-0.1, 0.9]], (3.5, -2.25))
    want_shear = bytes(ref.made(ref.AFFINE, (1.1, 0.2, -0.1, 0.9, 3.5, -2.25)))

    # transform: ZeroEdgeExtension and bilinear; the image's own size; the input passed as it is, the result the output
    res, a = _one_call(tf.transform, img, shear)
    assert a["src"] == img.ctypes.data and (a["sw"], a["sh"], a["sstride"]) == (7, 5, 7) and a["mask"] is None and a["omask"] is None
    assert a["steps"] == [want_shear] and a["n"] == 1 and a["params"] == _params(1, 0)
    assert (a["w"], a["h"], a["x0"], a["y0"]) == (7, 5, 0, 0) and a["out"] == res.ctypes.data and res.shape == (5, 7) and res.dtype == np.float32
    # ... with a size, an origin, tags as instances, a mask: two results
    res, a = _one_call(tf.transform, img, shear, size=(9, 4), x0=-3, y0=2, edge=tf.ValueEdgeExtension(7.5, True), interp=tf.BicubicInterpolation(),
                       mask=mask * 255)
    assert (a["w"], a["h"], a["x0"], a["y0"]) == (9, 4, -3, 2) and a["params"] == _params(2, 1, 7.5, 1)
    assert a["mask"] is not None and res[0].shape == (4, 9) and res[1].dtype == np.uint8 and a["omask"] == res[1].ctypes.data
    # ... with a box of the transformed space
    res, a = _one_call(tf.transform, img, shear, bbox=BBox2i(-2, 1, 6, 3), edge=tf.ReflectEdgeExtension, interp=tf.NearestPixelInterpolation)
    assert (a["w"], a["h"], a["x0"], a["y0"]) == (6, 3, -2, 1) and a["params"] == _params(0, 5)
    # transform_nodata
    res, a = _one_call(tf.transform_nodata, img, shear, (8, 6), tf.ConstantEdgeExtension, tf.BicubicInterpolation, -32768.0)
    assert a["params"] == _params(2, 2, nodata=1, nodata_value=-32768.0) and (a["w"], a["h"]) == (8, 6)
    # resample: Constant, bilinear, int(.5 + cols * f)
    res, a = _one_call(tf.resample, img, 1.5, 0.5)
    assert a["steps"] == [bytes(ref.made(ref.RESAMPLE, (1.5, 0.5)))] and (a["w"], a["h"]) == (11, 3) and a["params"] == _params(1, 2)
    res, a = _one_call(tf.resample, img, 2)
    assert a["steps"] == [bytes(ref.made(ref.RESAMPLE, (2.0, 2.0)))] and (a["w"], a["h"]) == (14, 10)
    res, a = _one_call(tf.resample, img, 0.75, size=(4, 2), edge=tf.PeriodicEdgeExtension)
    assert a["steps"] == [bytes(ref.made(ref.RESAMPLE, (0.75, 0.75)))] and (a["w"], a["h"]) == (4, 2) and a["params"] == _params(1, 3)
    # resize: the factors are out / (double) cols
    res, a = _one_call(tf.resize, img, 11, 3)
    assert a["steps"] == [bytes(ref.made(ref.RESAMPLE, (11 / 7.0, 3 / 5.0)))] and (a["w"], a["h"]) == (11, 3) and a["params"] == _params(1, 2)
    # translate, the double and the int form: Zero, bilinear, the image's size
    for offset in ((1.5, -2.0), (1, -2)):
        res, a = _one_call(tf.translate, img, offset[0], offset[1])
        assert a["steps"] == [bytes(ref.made(ref.TRANSLATE, [float(v) for v in offset]))] and (a["w"], a["h"]) == (7, 5) and a["params"] == _params(1, 0)
    # rotate: about `translate`, the image's size
    res, a = _one_call(tf.rotate, img, 0.3, (3.0, 2.0), edge=tf.CylindricalEdgeExtension)
    assert a["steps"] == [bytes(ref.rotate(0.3, 3.0, 2.0))] and (a["w"], a["h"]) == (7, 5) and a["params"] == _params(1, 4)
    # chains: compose in reverse's order, InverseTransform the other way round with every step inverted
    t, r, s = tf.TranslateTransform(2.5, -1.0), tf.RotateTransform(0.2, (30.0, 20.0)), tf.ResampleTransform(1.25, 0.8)
    res, a = _one_call(tf.transform, img, tf.compose(t, r, s))
    want = ref.scenes()["chain3"]["steps"]
    assert a["n"] == 3 and a["steps"] == [bytes(d) for d in want]
    res, a = _one_call(tf.transform, img, tf.InverseTransform(tf.compose(t, r)))
    assert a["steps"] == [bytes(ref.invert(want[1])), bytes(ref.invert(want[0]))]
    # stereo.HomographyTransform as it is, through its matrix and inverse_matrix
    h = stereo.HomographyTransform([[1.01, 0.02, -1.5], [-0.01, 0.99, 2.0], [1e-4, -2e-4, 1.0]])
    res, a = _one_call(tf.transform, img, h)
    assert a["steps"] == [bytes(ref.by_hand(ref.HOMOGRAPHY, fwd=h.matrix.ravel(), rev=h.inverse_matrix.ravel()))]
    assert a["steps"] == [bytes(ref.made(ref.HOMOGRAPHY, h.matrix.ravel()))]      # the same adjugate on all three sides
    # a strided view of a wider array is copied packed on the host side
    wide = np.zeros((5, 9), np.float32)
    res, a = _one_call(tf.transform, wide[:, :7], shear)
    assert a["src"] != wide.ctypes.data and (a["sw"], a["sstride"]) == (7, 7)


def test_wrapper_refusals_and_points():
    img = np.zeros((5, 7), np.float32)
    t = tf.TranslateTransform(1.0, 2.0)
    for bad in (lambda: tf.transform(img[0], t, ctx=FakeContext()), lambda: tf.transform(img, t, size=(0, 3), ctx=FakeContext()),
                lambda: tf.transform(img, t, mask=np.ones((4, 7), np.uint8), ctx=FakeContext()),
                lambda: tf.transform(img, t, size=(3, 3), bbox=BBox2i(0, 0, 3, 3), ctx=FakeContext()),
                lambda: tf.transform(img, "shift", ctx=FakeContext()), lambda: tf.transform(img, t, edge=7, ctx=FakeContext()),
                lambda: tf.transform(img, tf.compose(t, t, t, tf.compose(t, t)), ctx=FakeContext()),
                lambda: tf.ResampleTransform(0.0, 1.0), lambda: tf.LinearTransform([[1.0, 2.0], [2.0, 4.0]]),
                lambda: tf.AffineTransform(np.eye(3), (0, 0)), lambda: tf.RotateTransform(NAN), lambda: t.forward(np.zeros((3, 3)))):
        with pytest.raises(ArgumentErr):
            bad()
    # the functors' points are the restatement's
    shear = tf.AffineTransform([[1.1, 0.2], [-0.1, 0.9]], (3.5, -2.25))
    want = ref.made(ref.AFFINE, (1.1, 0.2, -0.1, 0.9, 3.5, -2.25))
    ref.same(shear.forward(POINTS), ref.points([want], ref.FORWARD, POINTS)[1], "forward")
    ref.same(tf.reverse(shear, POINTS), ref.points([want], ref.REVERSE, POINTS)[1], "reverse")
    ref.same(tf.InverseTransform(shear).forward(POINTS), ref.points([want], ref.REVERSE, POINTS)[1], "inverse forward")
    ref.same(tf.LinearTransform([[1.1, 0.2], [-0.1, 0.9]]).reverse(POINTS),
             ref.points([ref.made(ref.AFFINE, (1.1, 0.2, -0.1, 0.9, 0.0, 0.0))], ref.REVERSE, POINTS)[1], "linear")
    ref.same(tf.IdentityTransform().forward(POINTS.reshape(1, -1, 2)), POINTS.reshape(1, -1, 2), "identity keeps the shape")
    # compute_transformed_bbox_fast: the perimeter forward, the box in float
    lo, hi = tf.compute_transformed_bbox_fast(BBox2i(0, 0, 7, 5), tf.ResampleTransform(2.0, 0.5))
    assert lo.dtype == np.float32 and tuple(lo) == (0.0, 0.0) and tuple(hi) == (12.0, 2.0)
    lo, hi = tf.compute_transformed_bbox_fast(BBox2i(1, 2, 3, 2), tf.TranslateTransform(0.1, -0.5))
    assert tuple(lo) == (np.float32(1.1), np.float32(1.5)) and tuple(hi) == (np.float32(3.1), np.float32(2.5))


# ---- the scenes of the GPU test ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("interp", sorted(ref.INTERPS))
@pytest.mark.parametrize("name", sorted(ref.scenes()))
def test_scene_conditions(name, interp):
    it = ref.INTERPS[interp]
    r = ref.scene_result(name, it, True)
    assert r["rc"] == 0
    c, n = r["classes"], r["classes"].size
    assert ((c & ref.C_ALL_INSIDE) != 0).sum() >= 0.1 * n, "too few pixels with every tap inside the source"
    assert ((c & ref.C_SOME_OUTSIDE) != 0).sum() >= 0.1 * n, "too few pixels with a tap outside the source"
    assert (r["mask"] != 0).any() and (r["mask"] == 0).any(), "a masked scene needs valid and invalid outputs"
    if name in ("int_translate", "resample_2") and it != ref.NEAREST:
        assert ((c & ref.C_INTEGER) != 0).any(), "no pixel at an exact integer position"
    if name == "w_zero":
        assert ((c & ref.C_NAN_HUGE) != 0).any(), "no NaN or out-of-range coordinate"
        assert ((c[:, 16] & ref.C_NAN_HUGE) != 0).all()      # w is exactly 0 in column 16
    if it != ref.NEAREST and name not in ref.INTEGER_ONLY:
        # (a scene whose every position is an integer uses one tap per pixel: there is no other tap to be invalid)
        assert ((c & ref.C_OTHER_TAP) != 0).any(), "no pixel that is invalid only because of a tap other than the nearest"
    if name in ref.INTEGER_ONLY and it != ref.NEAREST:
        assert ((c & ref.C_INTEGER) != 0).sum() == n


def test_nodata_scene_conditions():
    for it in (ref.NEAREST, ref.BILINEAR, ref.BICUBIC):
        r = ref.scene_result("rotate", it, True, nodata=(-1.0, False))
        c = r["classes"]
        assert ((c & ref.C_NODATA) != 0).sum() >= 0.1 * c.size and ((c & ref.C_ALL_INSIDE) != 0).sum() >= 0.1 * c.size
        # the nodata test leaves no tap outside the source: what is not nodata has every tap inside
        assert not ((c & ref.C_SOME_OUTSIDE) != 0).any()
        assert (r["out"][(c & ref.C_NODATA) != 0] == np.float32(-1.0)).all() and (r["mask"][(c & ref.C_NODATA) != 0] == 0).all()
