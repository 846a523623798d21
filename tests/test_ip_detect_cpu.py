"""CPU-only: the restatement of the OBALoG detectors against the reference's known answers, what makes the GPU tests able to
catch a wrong kernel (the serial order of the integral image, OBALoG's shifted points, the shared atan2f), the host logic of
the tile loops and the cull, the ABI and the wrapper's calls.  No GPU.

The shared atan2f form against libm on this host, and what switching the restatement to libm's atan2f changes, are printed
and recorded in profiles/ip_detect.md."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ip_detect_ref as ref  # noqa: E402
import ip_detect_scenes as sc  # noqa: E402

from visionworkbench_amd import _lib  # noqa: E402
from visionworkbench_amd import interest_point as ipm  # noqa: E402
from visionworkbench_amd.core import ArgumentErr, NoImplErr  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "ip_detect_known.json")))
NEW_SYMBOLS = ["vwgpu_integral_image_dev", "vwgpu_integral_image", "vwgpu_ip_detect_dev", "vwgpu_ip_detect", "vwgpu_ip_orientation_dev",
               "vwgpu_ip_orientation", "vwgpu_ip_describe_dev", "vwgpu_ip_describe", "vwgpu_ip_cull_order"]


@pytest.fixture(scope="module")
def scenes():
    return sc.scenes()


# ---- the restatement against TestBoxFilter.cxx and TestIntegral.cxx ------------------------------------------------------------------

def test_restatement_reproduces_the_box_filter_answers():
    g = GOLDEN["box_filter"]
    one = g["apply_at_point"]
    integ = ref.integral(np.array(one["image"], np.float32))
    assert list(integ.shape[::-1]) == one["integral_size"]
    assert abs(ref.box_at(integ, one["at"][0], one["at"][1], g["boxes"], g["weights"]) - one["response"]) <= g["tolerance"]
    view = g["filter_view"]
    integ = ref.integral(np.array(view["image"], np.float32))
    assert list(integ.shape[::-1]) == view["integral_size"]
    applied = ref.box_filter(integ, g["boxes"], g["weights"])
    assert list(applied.shape[::-1]) == view["applied_size"]
    for r in view["responses"]:
        assert abs(applied[r["at"][1], r["at"][0]] - r["value"]) <= g["tolerance"], r


def test_restatement_reproduces_the_interpolation_identity():
    g = GOLDEN["interpolation_proof"]
    integ = ref.integral(np.array(g["image"], np.float32))
    left, right = (ref.haar(integ, p[0], p[1], g["size"]) for p in (g["left"], g["right"]))
    assert left != right
    assert abs((left + right) / 2 - ref.haar(integ, g["between"][0], g["between"][1], g["size"])) <= g["tolerance"]


def test_integral_shows_the_serial_order(scenes):
    """On the 96 x 80 scene the words of the reference's recurrence differ from a double cumulative sum rounded to float, so a
    kernel that scans instead is caught by the GPU test."""
    integ = ref.integral(scenes[0])
    assert integ.shape == (81, 97) and not integ[0].any() and not integ[:, 0].any()
    scan = np.cumsum(np.cumsum(scenes[0].astype(np.float64), 0), 1).astype(np.float32)
    assert (integ[1:, 1:] != scan).sum() > 0
    # the recurrence itself, in numpy float32
    h, w = scenes[0].shape
    I = np.zeros((h + 1, w + 1), np.float32)
    for y in range(h):
        for x in range(w):
            I[y + 1, x + 1] = np.float32(np.float32(np.float32(scenes[0][y, x] + I[y + 1, x]) + I[y, x + 1]) - I[y, x])
    ref.same(integ, I, "recurrence")


# ---- OBALoG's off-by-one, by hand ------------------------------------------------------------------------------------------------------

def _extrema_by_hand(img):
    """{(scale index, x, y): interest} of the pixels of a middle plane strictly above their 26 neighbours, with numpy."""
    integ = ref.integral(img)
    planes = np.stack([ref.plane(integ, s) for s in range(8)])
    extrema = {}
    for m in range(1, 7):
        for y in range(1, img.shape[0] - 1):
            for x in range(1, img.shape[1] - 1):
                v = planes[m, y, x]
                if (planes[m - 1:m + 2, y - 1:y + 2, x - 1:x + 2] < v).sum() == 26:
                    extrema[(m, x, y)] = v
    return extrema


def test_obalog_points_sit_one_pixel_right_and_down_of_the_extremum():
    """A bright square on a dark 64 x 64 image.  The extrema are found here from the interest planes with numpy, not by the
    restatement's detector loop: IAGD puts its points on them, OBALoG at (+1, +1) with the same interest.
    A 3 x 3 square answers most strongly at scale 0 (0.5 against 0.482 at scale 1 in its centre), which is no middle scale: it
    has no extremum and gives no point with either detector.  A 5 x 5 square peaks at scale 2 and carries the assertion."""
    img = np.zeros((64, 64), np.float32)
    img[30:33, 28:31] = 1.0
    assert _extrema_by_hand(img) == {}
    assert ref.detect(img, ref.IAGD)[1] == [0, 0, 0] and ref.detect(img, ref.OBALOG, threshold=1e-6)[1] == [0, 0, 0]
    img = np.zeros((64, 64), np.float32)
    img[30:35, 28:33] = 1.0
    extrema = _extrema_by_hand(img)
    assert (2, 30, 32) in extrema      # the square's centre, at the scale of sigma 1.875
    sigma = [1.2, 1.5, 1.875, 2.34375, 2.9296875, 3.662109, 4.577636, 5.722046]
    iagd, istats = ref.detect(img, ref.IAGD)
    obalog, ostats = ref.detect(img, ref.OBALOG, threshold=1e-6)
    assert istats[0] == ostats[0] == len(extrema) and istats[2] > 0 and ostats[2] > 0
    at = {(float(np.float32(sigma[m])), x, y): v for (m, x, y), v in extrema.items()}
    for f, shift in ((iagd, 0), (obalog, 1)):
        for k in range(f["x"].size):
            key = (float(f["scale"][k]), int(f["ix"][k]) - shift, int(f["iy"][k]) - shift)
            assert key in at and at[key] == f["interest"][k], (shift, key)
            assert f["x"][k] == f["ix"][k] and f["y"][k] == f["iy"][k]
    # the strongest point: the square's centre with IAGD, one pixel right and down of it with OBALoG, the same interest
    i, o = int(np.argmax(iagd["interest"])), int(np.argmax(obalog["interest"]))
    assert (iagd["ix"][i], iagd["iy"][i]) == (30, 32) and (obalog["ix"][o], obalog["iy"][o]) == (31, 33)
    assert obalog["interest"][o] == iagd["interest"][i] == extrema[(2, 30, 32)]


def test_harris_reads_stay_inside_and_nine_scales_are_refused(scenes):
    for img in scenes:
        for kind, thr in ((ref.IAGD, 0.0), (ref.OBALOG, 0.05), (ref.OBALOG, 0.01)):
            assert ref.detect(img, kind, threshold=thr)[1][2] > 0
    assert ref.harris_outside() == 0
    with pytest.raises(NoImplErr):
        ipm.IntegralAutoGainDetector(scales=9).process_image(scenes[0])
    with pytest.raises(ArgumentErr):
        ipm.IntegralAutoGainDetector(scales=0).process_image(scenes[0])


# ---- the shared atan2f form ----------------------------------------------------------------------------------------------------------

def _ulps(a, b):
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    ia, ib = (v if v >= 0 else -(v & 0x7fffffff) for v in (ia, ib))
    return abs(ia - ib)


def test_shared_atan2f_against_libm_and_float64(scenes):
    values = [0.0, -0.0, 1e-45, -1e-45, 3e-41, -1e-39, 1.17549435e-38, 1.0, -1.0, 0.5, 3.0, -7.25, 1e30, -1e30, 1e-30, 2.5e-3, 123.456,
              float("inf"), -float("inf")]
    rng = np.random.RandomState(1)
    values += [float(v) for v in (rng.standard_normal(120) * 10 ** rng.uniform(-6, 6, 120)).astype(np.float32)]
    worst_libm = worst_f64 = 0
    for y in values:
        for x in values:
            a = ref.atan2f(y, x)
            worst_libm = max(worst_libm, _ulps(a, ref.atan2f(y, x, True)))
            worst_f64 = max(worst_f64, _ulps(a, np.float32(np.arctan2(np.float64(np.float32(y)), np.float64(np.float32(x))))))
            assert np.signbit(a) == np.signbit(np.float32(y))
    assert np.isnan(ref.atan2f(float("nan"), 1.0)) and np.isnan(ref.atan2f(1.0, float("nan")))
    # the share of OBALoG points whose orientation moves by more than 1e-5 rad when the restatement uses libm's atan2f
    moved = total = 0
    for img in scenes:
        for thr in (0.05, 0.01):
            a = ref.detect(img, ref.OBALOG, threshold=thr)[0]["orientation"]
            b = ref.detect(img, ref.OBALOG, threshold=thr, libm=True)[0]["orientation"]
            moved += int((np.abs(a - b) > 1e-5).sum())
            total += a.size
    print("shared atan2f: at most %d ulp from libm's atan2f, %d ulp from the rounded float64 arctan2; %d of %d orientations differ"
          % (worst_libm, worst_f64, moved, total))
    assert worst_f64 <= 1 and worst_libm <= 2
    assert total > 300 and moved <= 0.01 * total


# ---- host logic ------------------------------------------------------------------------------------------------------------------------

def test_detection_tiles_and_counts():
    assert ipm.detection_tiles(1024, 1024, 250) == ([(0, 0, 1024, 1024)], [250])
    assert ipm.detection_tiles(1024, 1024) == ([(0, 0, 1024, 1024)], [0])
    rects, counts = ipm.detection_tiles(1500, 1100, 250)
    assert rects == [(0, 0, 1024, 1024), (1024, 0, 476, 1024), (0, 1024, 1024, 76), (1024, 1024, 476, 76)]
    assert counts == [250, 117, 19, 9]      # ceil(area / 1024^2 * 250)
    rects, counts = ipm.detection_tiles(2049, 1, 100)
    assert rects == [(0, 0, 1024, 1), (1024, 0, 1024, 1), (2048, 0, 1, 1)] and counts == [1, 1, 1]


def test_description_crop_leaves_the_image_at_a_corner():
    """Scale 1, orientation 0: the map is a translation by (x - 20.5, y - 20.5), the support's corners 0 and 41 go to x - 20.5 and
    x + 20.5, the box to floor .. floor + 1, one pixel more on every side."""
    ip = ipm.InterestPoints([3.0], [2.0], np.zeros((1, 0), np.float32))
    assert ipm.description_crop(ip, 42) == (-19, -20, 44, 44)      # x: floor(-17.5) - 1 = -19 .. floor(23.5) + 1 + 1 = 25
    two = ipm.InterestPoints([3.0, 100.0], [2.0, 50.0], np.zeros((2, 0), np.float32), scale=[1.0, 2.0])
    x, y, w, h = ipm.description_crop(two, 42)
    assert (x, y) == (-19, -20) and x + w == 100 + 41 + 2 and y + h == 50 + 41 + 2
    assert ipm.description_crop(ipm.InterestPoints([3.0], [2.0], np.zeros((1, 0), np.float32)), 41) == (-18, -19, 43, 43)


def test_cull_order_with_ties():
    interest = [0.5, 0.9, 0.5, 0.9, 0.1, 0.7]      # natural order: scale, row, column
    by_interest = [1, 3, 5, 0, 2, 4]               # descending, ties in natural order
    for limit, want in ((0, [0, 1, 2, 3, 4, 5]), (-1, [0, 1, 2, 3, 4, 5]), (3, by_interest[:3]), (6, by_interest), (9, by_interest)):
        assert list(ipm.cull_order("obalog", interest, limit)) == want, limit
    for limit, want in ((0, [0, 1, 2, 3, 4, 5]), (3, by_interest[:3]), (6, [0, 1, 2, 3, 4, 5]), (9, [0, 1, 2, 3, 4, 5]), (5, by_interest[:5])):
        assert list(ipm.cull_order("iagd", interest, limit)) == want, limit
    assert list(ipm.cull_order("iagd", [], 3)) == []


# ---- ABI and wrapper ---------------------------------------------------------------------------------------------------------------------

def test_new_symbols_and_abi_version():
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert lib.vwgpu_abi_version() == 3
    assert ctypes.sizeof(_lib.IpDetectParams) == 24 and ctypes.sizeof(_lib.IpPoints) == 7 * ctypes.sizeof(ctypes.c_void_p)
    assert lib.vwgpu_strerror(-6) == b"an output segment is too small"
    for name in ("integral_image", "OBALoGInterestOperator", "IntegralInterestPointDetector", "IntegralAutoGainDetector",
                 "detect_interest_points", "SGradDescriptorGenerator", "SGrad2DescriptorGenerator", "describe_interest_points", "ipfind"):
        assert name in ipm.__all__


class Recorder(object):
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


class FakeContext(object):
    _h = "ctx"

    def __init__(self):
        self._lib = Recorder()

    def check(self, rc):
        assert rc == 0

    def set_stream(self, stream):
        pytest.fail("a numpy call must not touch the stream")


def test_wrapper_calls():
    img = np.zeros((30, 50), np.float32)
    ctx = FakeContext()
    out = ipm.integral_image(img, ctx=ctx)
    (name, a), = ctx._lib.calls
    assert name == "vwgpu_integral_image" and a[0] == "ctx" and a[2:5] == (50, 30, 50) and a[5] == out.ctypes.data and a[6] == 51
    assert out.shape == (31, 51) and out.dtype == np.float32
    ctx = FakeContext()
    wide = np.zeros((31, 60), np.float32)
    ori = ipm.assign_orientation(wide[:, :51], [5, 6], [7, 8], [1.5, 1.2], ctx=ctx)      # a view is made dense on the host side
    (name, a), = ctx._lib.calls
    assert name == "vwgpu_ip_orientation" and a[2:6] == (51, 31, 51, 2) and a[9] == ori.ctypes.data and ori.shape == (2,)
    assert len({a[6], a[7], a[8]}) == 3
    assert ipm.assign_orientation(wide, [], [], [], ctx=FakeContext()).shape == (0,)
    # IntegralAutoGainDetector(max_points = 200, scales = 8); IntegralInterestPointDetector(threshold 0.05, 8 scales, 1000 points)
    for det, want in ((ipm.IntegralAutoGainDetector(), (0, 8, 0.0, 200)), (ipm.IntegralInterestPointDetector(), (1, 8, 0.05, 1000)),
                      (ipm.IntegralInterestPointDetector(ipm.OBALoGInterestOperator(0.02), 5, 7), (1, 5, 0.02, 7))):
        ctx = FakeContext()
        got = det.process_image(img, 12, ctx=ctx)
        (name, a), = ctx._lib.calls
        assert name == "vwgpu_ip_detect" and a[2:5] == (50, 30, 50) and a[6] == 1 and len(got) == 0
        P = a[7]._obj
        assert (P.detector, P.scales, P.threshold, P.max_points, P.reserved) == want + (0,)
        assert list(np.ctypeslib.as_array((ctypes.c_int * 4).from_address(a[5]))) == [0, 0, 50, 30]
        assert (ctypes.c_int * 1).from_address(a[8])[0] == 12 and a[9] == 12      # the capacity is the limit
    ip = ipm.InterestPoints([10.0, 20.0], [11.0, 12.0], np.zeros((2, 0), np.float32), scale=[1.5, 1.2])
    for gen, k in ((ipm.SGradDescriptorGenerator(), 180), (ipm.SGrad2DescriptorGenerator(), 128)):
        ctx = FakeContext()
        got = gen(img, ip, crop=(-3, -4, 60, 40), ctx=ctx)
        (name, a), = ctx._lib.calls
        assert name == "vwgpu_ip_describe" and a[2:5] == (50, 30, 50) and a[6] == 2 and a[11] == gen.kind and a[13] == k
        assert list((ctypes.c_int * 4).from_address(a[5])) == [-3, -4, 60, 40]
        assert got.descriptor.shape == (2, k) and a[12] == got.descriptor.ctypes.data
    ctx = FakeContext()
    assert len(ipm.describe_interest_points(img, ipm.SGradDescriptorGenerator(), ip.take(np.zeros(0, np.int64)), ctx=ctx)) == 0 and not ctx._lib.calls
    with pytest.raises(ArgumentErr):
        ipm.describe_interest_points(img, ipm.SGradDescriptorGenerator(), ipm.InterestPoints([60.0], [1.0], np.zeros((1, 0), np.float32)))


def test_vwip_round_trip_of_a_described_list(tmp_path, scenes):
    """A detected and described list (from the restatement, no GPU here) through write_binary_ip_file / read_binary_ip_file."""
    f, _ = ref.detect(scenes[0], ref.OBALOG, threshold=0.01, max_points=20)
    ip = ipm.InterestPoints(f["x"], f["y"], np.zeros((f["x"].size, 0), np.float32), **{k: f[k] for k in ("ix", "iy", "orientation", "scale", "interest")})
    desc = ref.describe(scenes[0], ipm.description_crop(ip, 42), ip.x, ip.y, ip.scale, ip.orientation, ref.SGRAD)
    ip = ipm.InterestPoints(ip.x, ip.y, desc, **{k: f[k] for k in ("ix", "iy", "orientation", "scale", "interest")})
    path = str(tmp_path / "scene.vwip")
    ipm.write_binary_ip_file(path, ip)
    back = ipm.read_binary_ip_file(path)
    assert len(back) == 20
    for name in ("x", "y", "ix", "iy", "orientation", "scale", "interest", "polarity", "octave", "scale_lvl", "descriptor"):
        ref.same(getattr(back, name), getattr(ip, name), name)
