"""The CPU restatement of epipolar rectification (tests/refimpl/epipolar_ref.cc) and the library's host arithmetic
(vwgpu_epipolar_pinhole, vwgpu_epipolar_cahv, vwgpu_pinhole_camera_matrix) against the reference's own known answer
(src/vw/Camera/tests/TestCAHVModel.cxx), the properties of a rectified pair, each other, and the conditions the scenes of
the GPU tests must meet.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import epipolar_ref as ref  # noqa: E402
import triangulate_ref as tri  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import _lib, camera  # noqa: E402

# The largest row disagreement of the restatement over scene_points() (profiles/epipolar.md); the tests allow 16 x that for
# other point sets.  The pinhole pair is rectified to rounding; epipolar(CAHVModel) keeps the image plane perpendicular to
# the mean of the two A vectors (CAHVModel.cc:313-326), not parallel to the baseline, so its rows agree only as far as the
# mean look direction is perpendicular to the baseline.
ROW_MAX = {"pinhole": 8.8817841970012523e-16, "cahv": 0.026678462808689574, "cahv_flipped": 0.026678462808689574}


def _unit(v):
    v = np.array(v, np.float64)
    return v / np.sqrt(v @ v)


# ---- 1. the reference's known answer -------------------------------------------------------------------------------------

def test_fake_epipolar_conversion_known_answer():
    """TEST(CAHVModel, FakeEpipolarConversion) (TestCAHVModel.cxx:99-154): two CAHV cameras at (+-30, 0, 30) looking down at
    45 degrees on points with z = 0 in [-15, 15]^2; after epipolar() and CameraTransform::forward the two images differ by
    (-40, 0) within 0.1."""
    def cahv(f, pixel, hc, vc, c, a, hvec, vvec):      # CAHVModel(f, pixel_size, Hc, Vc, C, A, Hvec, Vvec) (CAHVModel.cc:153-165)
        a, hvec, vvec = (np.array(x, np.float64) for x in (a, hvec, vvec))
        return camera.CAHVModel(c, a, f / pixel[0] * hvec + hc * a, f / pixel[1] * vvec + vc * a)
    aa, ab = _unit((-1, 0, -1)), _unit((1, 0, -1))
    model_a = cahv(2, (.1, .1), 0, 0, (30, 0, 30), aa, (0, 1, 0), np.cross(aa, (0, 1, 0)))
    model_b = cahv(2, (.1, .1), 0, 0, (-30, 0, 30), ab, (0, -1, 0), np.cross(ab, (0, -1, 0)))
    rng = np.random.default_rng(1)
    points = np.concatenate([rng.uniform(-15, 15, (100, 2)), np.zeros((100, 1))], 1)
    image_a = np.array([ref.project(model_a, p) for p in points])
    image_b = np.array([ref.project(model_b, p) for p in points])
    for epi in (ref.epipolar, camera.epipolar):
        epi_a, epi_b = epi(model_a, model_b)
        new_a, failed_a, rc_a = ref.transform_points(model_a, epi_a, ref.FORWARD, image_a)
        new_b, failed_b, rc_b = ref.transform_points(model_b, epi_b, ref.FORWARD, image_b)
        assert (rc_a, rc_b, failed_a, failed_b) == (0, 0, 0, 0)
        temp = new_a - new_b
        assert np.abs(temp[:, 0] + 40).max() < 0.1 and np.abs(temp[:, 1]).max() < 0.1, temp


# ---- 2. rectification properties -----------------------------------------------------------------------------------------

def _pairs():
    a, b = ref.stereo_pair()
    return {"pinhole": (a, b), "cahv": (tri.cahv_of(a), tri.cahv_of(b)), "cahv_flipped": (tri.cahv_of(a, True), tri.cahv_of(b, True))}


@pytest.mark.parametrize("kind", ["pinhole", "cahv", "cahv_flipped"])
@pytest.mark.parametrize("which", ["restatement", "library"])
def test_rectified_pair_properties(kind, which):
    c0, c1 = _pairs()[kind]
    e0, e1 = (ref.epipolar if which == "restatement" else camera.epipolar)(c0, c1)
    if kind == "pinhole":
        assert np.array_equal(e0.rotation, e1.rotation)
        assert (e0.fu, e0.fv, e0.cu, e0.cv, e0.pixel_pitch) == (e1.fu, e1.fv, e1.cu, e1.cv, e1.pixel_pitch)
        assert e0.distortion is None and e1.distortion is None
        assert np.array_equal(e0.center, c0.center) and np.array_equal(e1.center, c1.center)
        assert np.abs(e0.rotation @ e0.rotation.T - np.eye(3)).max() < 1e-14
        # the new x axis is the baseline
        assert np.abs(e0.rotation[:, 0] - _unit(c1.center - c0.center)).max() < 1e-15
    else:
        assert all(np.array_equal(getattr(e0, k), getattr(e1, k)) for k in "AHV")
        assert np.array_equal(e0.C, c0.C) and np.array_equal(e1.C, c1.C)
        assert abs(np.sqrt(e0.A @ e0.A) - 1) < 1e-15
    rows = np.array([[ref.project(e, p)[1] for e in (e0, e1)] for p in ref.scene_points()])
    worst = np.abs(rows[:, 0] - rows[:, 1]).max()
    print("%s %s: max row disagreement %.17g" % (kind, which, worst))
    assert worst <= 16 * ROW_MAX[kind]
    cols = np.array([[ref.project(e, p)[0] for e in (e0, e1)] for p in ref.scene_points()])
    assert (cols[:, 0] > cols[:, 1]).all()      # a positive disparity everywhere: the cameras look the same way


# ---- 3. host functions against the restatement ---------------------------------------------------------------------------

def test_epipolar_pinhole_matches_restatement():
    for a, b in (ref.stereo_pair(), ref.stereo_pair(ref.MILD_TSAI), (ref.src_pinhole(), ref.stereo_pair()[1]),
                 (ref.turned_pinhole(), ref.stereo_pair()[0])):
        got, want = camera.epipolar(a, b), ref.epipolar(a, b)
        rot, focal, offset, pitch = ref.epipolar_pinhole(a, b)
        for g, w in zip(got, want):
            assert g.rotation.tobytes() == rot.tobytes()
            assert (g.fu, g.fv, g.cu, g.cv, g.pixel_pitch) == (focal[0], focal[1], offset[0], offset[1], pitch)
            assert bytes(g.descriptor) == bytes(w.descriptor)


def test_pose_round_trip_takes_every_branch():
    """Quaternion(matrix) (Quaternion.h:226-250) has four branches, chosen by the largest of ww, xx, yy, zz: rotations by 0,
    and by 170 degrees about x, y and z, take one each; library and restatement agree on all of them."""
    half_turns = [np.eye(3), ref.rot_x(170.0), tri.rot_y(170.0),
                  np.array([[np.cos(3.0), -np.sin(3.0), 0], [np.sin(3.0), np.cos(3.0), 0], [0, 0, 1]])]
    seen = set()
    for r in half_turns:
        d = np.diag(r)
        seen.add(int(np.argmax([1 + d[0] + d[1] + d[2], 1 + d[0] - d[1] - d[2], 1 - d[0] + d[1] - d[2], 1 - d[0] - d[1] + d[2]])))
        a = camera.PinholeModel((0, 0, 0), r, 50, 50, 10, 10)
        b = camera.PinholeModel((1, 0.5, 0.25), r, 50, 50, 10, 10)
        assert camera.epipolar(a, b)[0].rotation.tobytes() == ref.epipolar_pinhole(a, b)[0].tobytes()
    assert seen == {0, 1, 2, 3}


def test_epipolar_cahv_matches_restatement():
    for kind in ("cahv", "cahv_flipped"):
        c0, c1 = _pairs()[kind]
        got, want = camera.epipolar(c0, c1), ref.epipolar_cahv(c0, c1)
        for g, w in zip(got, want):
            assert bytes(g.descriptor) == bytes(w)
    # the branch dot(f, H0) <= 0: the cameras handed over in the other order
    c0, c1 = _pairs()["cahv"]
    for g, w in zip(camera.epipolar(c1, c0), ref.epipolar_cahv(c1, c0)):
        assert bytes(g.descriptor) == bytes(w)


def test_camera_matrix_matches_restatement():
    cams = [ref.src_pinhole(), ref.dst_pinhole(ref.MILD_TSAI), ref.turned_pinhole(), ref.stereo_pair()[1], ref.right_angle_pair()[1]]
    for cam in cams:
        assert cam.camera_matrix().tobytes() == ref.camera_matrix(cam).tobytes()
        assert np.array_equal(camera.matrix_of(cam), cam.camera_matrix())
    # and it is the matrix of rebuild_camera_matrix: K [uvw R^T | -uvw R^T C] to rounding
    cam = ref.turned_pinhole()
    uvw = np.stack([cam.u, cam.v, cam.w])
    k = np.array([[cam.fu, 0, cam.cu], [0, cam.fv, cam.cv], [0, 0, 1.0]])
    want = k @ np.concatenate([uvw @ cam.rotation.T, (-uvw @ cam.rotation.T @ cam.center)[:, None]], 1)
    assert np.abs(cam.camera_matrix() - want).max() < 1e-13
    assert camera.matrix_of(tri.cahv_of(cams[0])) is None


def test_set_point_offset_rebuilds():
    cam = ref.src_pinhole(ref.MILD_TSAI)
    cam.set_point_offset((12.5, -3.0))
    fresh = camera.PinholeModel(cam.center, cam.rotation, cam.fu, cam.fv, 12.5, -3.0, distortion=cam.distortion)
    assert np.array_equal(cam.point_offset(), [12.5, -3.0])
    assert bytes(cam.descriptor) == bytes(fresh.descriptor) and cam.camera_matrix().tobytes() == fresh.camera_matrix().tobytes()


# ---- 4. scene conditions, on the restatement alone -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def source():
    return ref.source_image()


def _classes(r):
    return np.bincount(r["classes"].ravel(), minlength=6)


def test_every_class_occurs(source):
    img, mask = source
    total = np.zeros(6, np.int64)
    main = ref.camera_pairs()["pinhole_pinhole"]
    for size in ((1, 1), (2, 9), (17, 1), (37, 29), (70, 45), (300, 200)):
        total += _classes(ref.camera_transform(img, main[0], main[1], size=size, mask=mask))
    for src, dst in ref.camera_pairs().values():
        total += _classes(ref.camera_transform(img, src, dst, size=(37, 29), mask=mask))
    ident = ref.camera_transform(img, *ref.identity_pair(), size=(70, 45))
    assert _classes(ident)[ref.CL_INTEGER] > 0
    hit = ident["classes"] == ref.CL_INTEGER
    ys, xs = np.nonzero(hit)
    assert np.array_equal(ident["out"][hit], img[ys, xs])      # an integer hit of the identity pair is the source pixel itself
    total += _classes(ident)
    for cahv in (False, True):
        r = ref.camera_transform(img, *ref.right_angle_pair(cahv), size=(37, 29), check=False)
        assert _classes(r)[ref.CL_NAN_HUGE] > 0 and r["failed"] == 0
        assert (r["out"][r["classes"] == ref.CL_NAN_HUGE] == 0).all() and (r["mask"][r["classes"] == ref.CL_NAN_HUGE] == 0).all()
        total += _classes(r)
    total += _classes(ref.camera_transform(img, *ref.strong_tsai_pair(), size=(70, 45)))
    print(dict(zip(ref.CLASS_NAMES, total)))
    assert (total > 0).all()


def test_tsai_scenes(source):
    img, mask = source
    mild = ref.camera_transform(img, *ref.mild_tsai_pair(), size=(70, 45), mask=mask, edge=(7.5, True))
    assert mild["failed"] == 0 and _classes(mild)[ref.CL_CHECK_FAILED] == 0
    strong = ref.camera_transform(img, *ref.strong_tsai_pair(), size=(70, 45), mask=mask, edge=(7.5, True))
    bad = strong["classes"] == ref.CL_CHECK_FAILED
    assert strong["failed"] == bad.sum() >= 1
    assert (strong["out"][bad] == np.float32(7.5)).all() and (strong["mask"][bad] == 255).all()
    off = ref.camera_transform(img, *ref.strong_tsai_pair(), size=(70, 45), check=False)
    assert off["failed"] == 0
    for name in ("tsai_src", "tsai_dst", "tsai_cahv"):
        src, dst = ref.camera_pairs()[name]
        assert ref.camera_transform(img, src, dst, size=(37, 29))["failed"] == 0


def test_main_scene_is_mostly_inside(source):
    img, mask = source
    src, dst = ref.camera_pairs()["pinhole_pinhole"]
    r = ref.camera_transform(img, src, dst, size=(70, 45), mask=mask)
    c = _classes(r)
    assert 2 * c[ref.CL_INSIDE] >= 70 * 45 and c[ref.CL_STRADDLE] > 0 and c[ref.CL_OUTSIDE] > 0
    # the mask matters: some valid and some invalid results among the pixels with all taps inside
    inside = r["classes"] == ref.CL_INSIDE
    assert (r["mask"][inside] == 255).any() and (r["mask"][inside] == 0).any()
    # a tile equals that region of the whole call
    tile = ref.camera_transform(img, src, dst, size=(20, 10), mask=mask, x0=13, y0=9)
    assert np.array_equal(tile["out"], r["out"][9:19, 13:33]) and np.array_equal(tile["mask"], r["mask"][9:19, 13:33])


def test_restatement_points_agree_with_the_image_path(source):
    """CameraTransform::reverse through the points entry of the restatement reproduces the positions the image path taps:
    an integer-position class exactly where both coordinates are integers."""
    src, dst = ref.identity_pair()
    ys, xs = np.mgrid[0:45, 0:70].astype(np.float64)
    q, failed, rc = ref.transform_points(src, dst, ref.REVERSE, np.stack([xs.ravel(), ys.ravel()], 1))
    assert (rc, failed) == (0, 0)
    integer = ((q == np.floor(q)).all(axis=1)).reshape(45, 70)
    r = ref.camera_transform(source[0], src, dst, size=(70, 45))
    inside = (q[:, 0] >= 0) & (q[:, 0] < ref.SW) & (q[:, 1] >= 0) & (q[:, 1] < ref.SH)
    assert np.array_equal(integer & inside.reshape(45, 70), r["classes"] == ref.CL_INTEGER)
    rc = ref.transform_points(src, ref.stereo_pair()[1], ref.FORWARD, [[1.0, 2.0]])[2]
    assert rc == ref.RC_LOGIC      # unequal centres


# ---- 5. argument errors of the host functions; the header ----------------------------------------------------------------

def test_host_function_errors():
    lib = _lib.load()
    a, b = ref.stereo_pair()
    with pytest.raises(vwa.ArgumentErr):
        camera.epipolar(a, camera.PinholeModel(a.center, b.rotation, 1, 1, 0, 0))      # no baseline
    ca, cb = tri.cahv_of(a), tri.cahv_of(b)
    with pytest.raises(vwa.ArgumentErr):
        camera.epipolar(ca, tri.cahv_of(camera.PinholeModel(a.center, b.rotation, 60, 60, 30, 23)))
    with pytest.raises(vwa.ArgumentErr):
        camera.epipolar(a, cb)      # mixed kinds
    d0, d1 = _lib.Camera(), _lib.Camera()
    byref = ctypes.byref
    assert lib.vwgpu_epipolar_cahv(byref(a.descriptor), byref(cb.descriptor), byref(d0), byref(d1)) == -1      # a pinhole
    assert lib.vwgpu_epipolar_cahv(None, byref(cb.descriptor), byref(d0), byref(d1)) == -1
    assert lib.vwgpu_epipolar_cahv(byref(ca.descriptor), byref(cb.descriptor), byref(d0), None) == -1
    assert lib.vwgpu_epipolar_cahv(byref(ca.descriptor), byref(cb.descriptor), byref(d0), byref(d1)) == 0
    v = [np.zeros(3), np.eye(3), np.array([1.0, 1.0]), np.array([0.0, 0.0])]
    out = [np.empty(9), np.empty(2), np.empty(2), ctypes.c_double()]
    c1 = np.array([1.0, 0, 0])

    def call(center0=v[0].ctypes.data, rot=v[1].ctypes.data, center1=c1.ctypes.data, rot_out=out[0].ctypes.data):
        return lib.vwgpu_epipolar_pinhole(center0, rot, v[2].ctypes.data, v[3].ctypes.data, 1.0, center1, v[1].ctypes.data,
                                          v[2].ctypes.data, v[3].ctypes.data, 1.0, rot_out, out[1].ctypes.data, out[2].ctypes.data,
                                          ctypes.addressof(out[3]))
    assert call() == 0
    assert call(center0=None) == -1 and call(rot=None) == -1 and call(rot_out=None) == -1
    assert call(center1=v[0].ctypes.data) == -1      # equal centres
    m = np.empty(12)
    u, vv, w = (np.array(x, np.float64) for x in ((1, 0, 0), (0, 1, 0), (0, 0, 1)))

    def matrix(u=u, out=m.ctypes.data, kind=0):
        return lib.vwgpu_pinhole_camera_matrix(v[0].ctypes.data, v[1].ctypes.data, 1.0, 1.0, 0.0, 0.0, u.ctypes.data, vv.ctypes.data,
                                               w.ctypes.data, 1.0, kind, None, out)
    assert matrix() == 0
    assert matrix(out=None) == -1 and matrix(kind=7) == -1 and matrix(u=np.array([1.0, 0.01, 0])) == -1


def test_header_declares_every_new_symbol():
    text = open(os.path.join(ROOT, "include", "vwgpu.h")).read()
    new = ["vwgpu_pinhole_camera_matrix", "vwgpu_epipolar_pinhole", "vwgpu_epipolar_cahv", "vwgpu_camera_transform_dev",
           "vwgpu_camera_transform", "vwgpu_camera_transform_points_dev", "vwgpu_camera_transform_points"]
    lib = _lib.load()
    for name in new:
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS and getattr(lib, name)
    assert lib.vwgpu_abi_version() == 3 and "#define VWGPU_ABI_VERSION 3" in text
    assert ctypes.sizeof(_lib.Camera) == ref.lib().trr_camera_size()      # the descriptor did not grow
