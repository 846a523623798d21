"""CPU-only: the restatement of the interest-point matchers against the reference's known answers, the host entries
(remove_duplicates, the fits, RANSAC), the binary files, the ABI and the wrapper's calls.  No GPU."""
import ctypes
import json
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import ip_match_ref as ref  # noqa: E402

from visionworkbench_amd import _lib  # noqa: E402
from visionworkbench_amd import interest_point as ipm  # noqa: E402
from visionworkbench_amd import transform as tf  # noqa: E402
from visionworkbench_amd.core import ArgumentErr, IOErr, LogicErr  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "ip_known.json")))
KIND = {"none": ref.NONE, "scale_orientation": ref.SCALE_ORIENTATION, "position": ref.POSITION}


# ---- the restatement against TestMatcher.cxx -----------------------------------------------------------------------------------

def test_restatement_reproduces_the_known_distances():
    for case in GOLDEN["distance_metric"]:
        fn = ref.l2 if case["metric"] == "L2" else ref.hamming
        assert fn(case["a"], case["b"]) == case["distance"], case


def test_restatement_reproduces_the_constraint_truth_table():
    c = GOLDEN["constraints"]
    for case in c["cases"]:
        assert ref.constraint(KIND[case["kind"]], case["bounds"], c["ip1"], c["ip2"]) == case["result"], case["name"]


def _golden_matcher():
    m = GOLDEN["matcher"]
    d1 = np.array([m["ip1"]["descriptor"]], np.float32)
    d2 = np.array([p["descriptor"] for p in m["ip2"]], np.float32)
    return m, d1, d2


def test_restatement_reproduces_the_matcher_case():
    m, d1, d2 = _golden_matcher()
    for mode in (ref.SIMPLE, ref.KNN):
        index, dist, stats = ref.match(d1, d2, m["threshold"], mode=mode)
        assert list(index) == m["matched_indexes"] and stats == [1, 1]
        assert list(d2[index[0]]) == m["matched_ip2_descriptor"]


def test_uniform_scene_shows_the_serial_order():
    """The scene of the GPU test: at K = 128 the float sum in the order k = 0 .. K-1 differs from the double sum on at least
    one pair, so a kernel that reorders or widens the sum is caught."""
    d1, d2 = ref.uniform_scene(65, 2 * ipm_chunk() + 7, 128)
    differ = sum(ref.l2(d1[i], d2[j]) != np.float32(ref.l2_double(d1[i], d2[j])) for i in range(8) for j in range(64))
    assert differ > 0


def ipm_chunk():
    return ipm.chunk_size(1)


def test_modes_differ_where_the_reference_says():
    d2 = np.array([[0, 4, 0], [0, 4, 0], [3, 0, 0]], np.float32)
    d1 = np.array([[0, 4, 0]], np.float32)
    # an exact zero distance with a duplicate: SIMPLE accepts the first index (0 > t * 0 is false), KNN rejects (0 < 0 is false)
    assert list(ref.match(d1, d2, 0.5, mode=ref.SIMPLE)[0]) == [0] and list(ref.match(d1, d2, 0.5, mode=ref.KNN)[0]) == [-1]
    # first == threshold * second exactly: 4 against 16 at 0.25
    e1, e2 = np.array([[0, 0]], np.float32), np.array([[2, 0], [0, 4]], np.float32)
    i, d, _ = ref.match(e1, e2, 0.25, mode=ref.SIMPLE)
    assert list(d[0]) == [4, 16] and list(i) == [0] and list(ref.match(e1, e2, 0.25, mode=ref.KNN)[0]) == [-1]
    # one candidate: SIMPLE matches (the second pick is 1e100), KNN does not
    assert list(ref.match(e1, e2[:1], 0.5, mode=ref.SIMPLE)[0]) == [0] and list(ref.match(e1, e2[:1], 0.5, mode=ref.KNN)[0]) == [-1]


# ---- remove_duplicates -------------------------------------------------------------------------------------------------------

def test_remove_duplicates_against_the_restatement():
    rng = np.random.RandomState(4)
    xy1, xy2 = rng.randint(0, 12, (200, 2)).astype(np.float32), rng.randint(0, 12, (200, 2)).astype(np.float32)
    keep = ipm.remove_duplicates_mask(xy1, xy2)
    assert np.array_equal(keep, ref.remove_duplicates(xy1, xy2)) and 0 < keep.sum() < 200
    assert len({tuple(p) for p in xy1[keep]}) == keep.sum() and len({tuple(p) for p in xy2[keep]}) == keep.sum()
    assert ipm.remove_duplicates_mask(np.zeros((0, 2)), np.zeros((0, 2))).shape == (0,)


def test_remove_duplicates_a_skipped_pair_blocks_nothing():
    """Pairs 0, 1, 2 from the back: 2 is kept; 1 shares its list-2 point with 2 and is skipped; 0 shares its list-1 point with
    the skipped pair 1 only and must be kept."""
    xy1 = np.array([[5, 5], [5, 5], [9, 9]], np.float32)
    xy2 = np.array([[1, 1], [7, 7], [7, 7]], np.float32)
    assert list(ipm.remove_duplicates_mask(xy1, xy2)) == [True, False, True]
    # the last repeated one is kept, and the order of the survivors is the input order
    x = np.array([3, 1, 3, 2], np.float32)
    ip1 = ipm.InterestPoints(x, x, np.arange(8, dtype=np.float32).reshape(4, 2))
    ip2 = ipm.InterestPoints(np.arange(4), np.arange(4), np.zeros((4, 2), np.float32))
    a, b = ipm.remove_duplicates(ip1, ip2)
    assert list(a.x) == [1, 3, 2] and list(b.x) == [1, 2, 3] and a.descriptor.tolist() == [[2, 3], [4, 5], [6, 7]]
    with pytest.raises(ArgumentErr):
        ipm.remove_duplicates(ip1, ip2.take([0, 1]))


# ---- fits and RANSAC ---------------------------------------------------------------------------------------------------------

def _sse(H, p1, p2):
    return float((np.linalg.norm(ref.apply(H, p1) - p2, axis=1) ** 2).sum())


@pytest.mark.parametrize("kind", [ref.SIMILARITY, ref.AFFINE, ref.HOMOGRAPHY])
def test_ransac_planted_model_exact_inliers(kind):
    """40 pairs in 0 .. 4096 mapped by a known model and 20 outliers displaced by at least 200 px; 100 iterations, threshold 30,
    min_inliers 20, a fixed table: the inlier flags are the planted ones and every planted inlier is mapped within 1e-6 px."""
    p1, p2, flags = ref.planted(kind)
    table = ref.sample_table(len(p1), 4 if kind == ref.HOMOGRAPHY else 3, 100)
    H, inl = ipm.ransac(kind, p1, p2, 100, 30, 20, samples=table)
    assert np.array_equal(inl, flags)
    worst = np.linalg.norm(ref.apply(H, p1[flags]) - p2[flags], axis=1).max()
    print("kind %d: worst planted inlier %.3g px" % (kind, worst))
    assert worst <= 1e-6
    # the restatement of the loop picks the same model
    Hr, inlr = ref.ransac(kind, p1, p2, table, 30, 20)
    assert np.array_equal(inlr, flags) and np.abs(ref.apply(H, p1) - ref.apply(Hr, p1))[flags].max() <= 2e-6      # each within 1e-6 of the truth


@pytest.mark.parametrize("kind", [ref.SIMILARITY, ref.AFFINE, ref.HOMOGRAPHY])
def test_ransac_planted_model_noisy_inliers(kind):
    """Inliers with Gaussian noise of 0.5 px: the inlier flags are the planted ones (outliers are >= 200 px off, the threshold
    is 30).  The returned model is the refit with the lowest MEAN inlier error, which may have been made on a subset of the
    planted inliers (a three- or four-point fit of noisy points can miss some of them by more than 30 px), so the optimum
    conditions are asserted on the functor and the same pairs in test_fit_is_no_worse_than_the_planted_model."""
    p1, p2, flags = ref.planted(kind, sigma=0.5)
    table = ref.sample_table(len(p1), 4 if kind == ref.HOMOGRAPHY else 3, 100)
    H, inl = ipm.ransac(kind, p1, p2, 100, 30, 20, samples=table)
    assert np.array_equal(inl, flags)
    Hr, inlr = ref.ransac(kind, p1, p2, table, 30, 20)
    assert np.array_equal(inlr, flags)
    diff = np.abs(ref.apply(H, p1) - ref.apply(Hr, p1))[flags].max()
    print("kind %d: library against the restatement of the loop %.3g px" % (kind, diff))
    # the two closed-form fits agree with numpy's to rounding (about 1e-11 px here); the two iterative homography
    # minimisers stop where they like, so theirs is printed and the optimum is judged in the test named above
    assert kind == ref.HOMOGRAPHY or diff <= 1e-8


@pytest.mark.parametrize("kind,fit", [(ref.AFFINE, ipm.fit_affine), (ref.HOMOGRAPHY, ipm.fit_homography)])
def test_fit_is_no_worse_than_the_planted_model(kind, fit):
    """Affine and homography minimise the squared metric: on the noisy planted inliers their sum of squared errors is at most
    that of the planted model on the same pairs x (1 + 1e-9), and at most the restatement's optimum likewise."""
    p1, p2, flags = ref.planted(kind, sigma=0.5)
    a, b = p1[flags], p2[flags]
    H = fit(a, b)
    got, truth, other = _sse(H, a, b), _sse(ref.PLANTED[kind], a, b), _sse(ref.FITS[kind](a, b), a, b)
    print("kind %d: sse %.12g, planted %.12g, restatement %.12g" % (kind, got, truth, other))
    assert got <= truth * (1 + 1e-9) and got <= other * (1 + 1e-9)
    assert H[2, 2] == 1 and (kind == ref.HOMOGRAPHY or list(H[2]) == [0, 0, 1])


def test_fit_similarity_follows_the_reference_formula():
    """The similarity is no least-squares optimum (its scale is a ratio of mean distances): compared with the numpy
    restatement of the same formula, mapped points within 1e-8 px, on noisy planted inliers and on a set whose
    cross-covariance has a negative determinant (a reflection comes out, as from the reference's SVD)."""
    p1, p2, flags = ref.planted(ref.SIMILARITY, sigma=0.5)
    rng = np.random.RandomState(3)
    a = rng.uniform(0, 4096, (30, 2))
    mirror = np.array([[1.1 * np.cos(.4), 1.1 * np.sin(.4), 10], [1.1 * np.sin(.4), -1.1 * np.cos(.4), 2000], [0, 0, 1]])
    b = ref.apply(mirror, a) + 0.5 * rng.standard_normal((30, 2))
    for x, y, sign in ((p1[flags], p2[flags], 1), (a, b, -1)):
        H, Hr = ipm.fit_similarity(x, y), ref.fit_similarity(x, y)
        assert np.sign(np.linalg.det(H[:2, :2])) == sign and np.sign(np.linalg.det(Hr[:2, :2])) == sign
        assert np.abs(ref.apply(H, x) - ref.apply(Hr, x)).max() <= 1e-8


def test_fit_homography_four_pairs_and_seed():
    p1, p2, flags = ref.planted(ref.HOMOGRAPHY)
    a, b = p1[flags], p2[flags]
    H4, H4r = ipm.fit_homography(a[:4], b[:4]), ref.fit_homography(a[:4], b[:4])
    assert H4[2, 2] == 1 and np.abs(ref.apply(H4, a) - ref.apply(H4r, a)).max() <= 1e-6
    # homogeneous (N, 3) points and InterestPoints are taken as the reference's Vector3 lists are
    ones = np.ones((len(a), 1))
    assert np.array_equal(ipm.fit_homography(np.c_[a, ones], np.c_[b, ones]), ipm.fit_homography(a, b))
    assert np.abs(ref.apply(ipm.fit_homography(a, b, seed=ref.PLANTED[ref.HOMOGRAPHY]), a) - b).max() <= 1e-6


def test_ransac_failure_reduce_and_refusals():
    p1, p2, flags = ref.planted(ref.AFFINE)
    table = ref.sample_table(len(p1), 3, 100)
    with pytest.raises(LogicErr, match="RANSAC was unable to find a fit that matched the supplied data."):
        ipm.ransac("affine", p1, p2, 100, 30, 50, samples=table)             # 40 inliers, 50 asked for
    assert _lib.load().vwgpu_host_last_error() == b"RANSAC was unable to find a fit that matched the supplied data."
    assert _lib.load().vwgpu_last_error(None) == b""          # the context entry keeps its answer for no context
    H, inl = ipm.ransac("affine", p1, p2, 100, 30, 50, reduce=True, samples=table)      # 50 -> 33
    assert np.array_equal(inl, flags) and _lib.load().vwgpu_host_last_error() == b""      # cleared by a success
    assert ref.ransac(ref.AFFINE, p1, p2, table, 30, 50) is None and ref.ransac(ref.AFFINE, p1, p2, table, 30, 33) is not None
    for bad in (table[:, :2], np.where(table == table[3, 0], len(p1), table), np.repeat(table[:, :1], 3, axis=1)):
        with pytest.raises(ArgumentErr):
            ipm.ransac("affine", p1, p2, 100, 30, 20, samples=bad)
    for call in (lambda: ipm.ransac("affine", p1, p2, 100, 30, 2, samples=table), lambda: ipm.ransac("affine", p1, p2[:-1], 100, 30, 20),
                 lambda: ipm.ransac("affine", p1, p2, 100, float("nan"), 20, samples=table), lambda: ipm.ransac("rigid", p1, p2, 100, 30, 20),
                 lambda: ipm.ransac("homography", p1[:3], p2[:3], 5, 30, 4), lambda: ipm.fit_affine(p1[:2], p2[:2]),
                 lambda: ipm.fit_homography(p1[:3], p2[:3]), lambda: ipm.fit_similarity(p1, np.full_like(p2, np.inf)),
                 lambda: ipm.fit_affine(np.c_[p1, 2 * np.ones(len(p1))], p2)):
        with pytest.raises(ArgumentErr):
            call()
    with pytest.raises(LogicErr):
        ipm.fit_affine(np.ones((5, 2)), p2[:5])          # all points equal
    lib = _lib.load()
    H = np.zeros(9)
    assert lib.vwgpu_fit_transform(1, None, p2.ctypes.data, 5, None, H.ctypes.data) == -1
    assert lib.vwgpu_ransac(1, p1.ctypes.data, p2.ctypes.data, len(p1), None, 100, 30.0, 20, 0, H.ctypes.data, None, None) == -1
    assert lib.vwgpu_ip_remove_duplicates(None, None, 3, None, None) == -1 and lib.vwgpu_ip_remove_duplicates(None, None, -1, None, None) == -1


def test_ransac_samples():
    t = ipm.ransac_samples(60, 4, 100, seed=3)
    assert t.shape == (100, 4) and t.dtype == np.int32 and t.min() >= 0 and t.max() < 60
    assert all(len(set(row)) == 4 for row in t.tolist()) and np.array_equal(t, ipm.ransac_samples(60, 4, 100, seed=3))
    assert not np.array_equal(t, ipm.ransac_samples(60, 4, 100, seed=4))
    assert ipm.ransac_samples(5000, 3, 7).shape == (7, 3)
    with pytest.raises(ArgumentErr):
        ipm.ransac_samples(3, 4, 10)


# ---- files -------------------------------------------------------------------------------------------------------------------

def _points(n, k, seed):
    rng = np.random.RandomState(seed)
    return ipm.InterestPoints(rng.uniform(0, 500, n), rng.uniform(0, 500, n), rng.random_sample((n, k)).astype(np.float32),
                              orientation=rng.uniform(-3, 3, n), scale=rng.uniform(1, 4, n), interest=rng.random_sample(n),
                              polarity=rng.randint(0, 2, n), octave=rng.randint(0, 5, n), scale_lvl=rng.randint(0, 3, n))


def _same_points(a, b):
    for name in ("x", "y", "ix", "iy", "orientation", "scale", "interest", "polarity", "octave", "scale_lvl", "descriptor"):
        ref.same(getattr(a, name), getattr(b, name), name)


def test_file_round_trip_and_layout(tmp_path):
    ip1, ip2 = _points(7, 5, 1), _points(7, 5, 2)
    vwip, match = str(tmp_path / "a.vwip"), str(tmp_path / "a__b.match")
    ipm.write_binary_ip_file(vwip, ip1)
    _same_points(ipm.read_binary_ip_file(vwip), ip1)
    ipm.write_binary_match_file(match, ip1, ip2)
    r1, r2 = ipm.read_binary_match_file(match)
    _same_points(r1, ip1)
    _same_points(r2, ip2)
    # the byte layout of MatcherIO.cc:248-263: one record by hand
    one = ipm.InterestPoints([1.5], [2.25], np.array([[0.5, -1.0, 3.0]], np.float32), ix=[1], iy=[2], orientation=[0.75], scale=[2.0],
                             interest=[9.5], polarity=[1], octave=[3], scale_lvl=[4])
    ipm.write_binary_ip_file(vwip, one)
    record = (struct.pack("<ff", 1.5, 2.25) + struct.pack("<ii", 1, 2) + struct.pack("<fff", 0.75, 2.0, 9.5) + struct.pack("<B", 1) +
              struct.pack("<II", 3, 4) + struct.pack("<Q", 3) + struct.pack("<fff", 0.5, -1.0, 3.0))
    assert len(record) == 57 and open(vwip, "rb").read() == struct.pack("<Q", 1) + record
    ipm.write_binary_match_file(match, one, one)
    assert open(match, "rb").read() == struct.pack("<QQ", 1, 1) + record + record
    # the defaults of the reference's constructor
    d = ipm.InterestPoints([3.7], [-1.2], np.zeros((1, 2), np.float32))
    assert (d.ix[0], d.iy[0], d.scale[0], d.orientation[0], d.polarity[0]) == (3, -1, 1.0, 0.0, 0)
    # refusals: lists of different length, a truncated file; a match file that does not exist is two empty lists
    with pytest.raises(IOErr):
        ipm.write_binary_match_file(match, ip1, ip2.take([0, 1]))
    open(vwip, "wb").write((struct.pack("<Q", 2) + record)[:-3])
    with pytest.raises(IOErr):
        ipm.read_binary_ip_file(vwip)
    with pytest.raises(IOErr):
        ipm.read_binary_ip_file(str(tmp_path / "none.vwip"))
    e1, e2 = ipm.read_binary_match_file(str(tmp_path / "none.match"))
    assert len(e1) == 0 and len(e2) == 0
    assert ipm.iplist_to_vectorlist(one).tolist() == [[1.5, 2.25, 1.0]]


def test_align_homography_from_a_match_file(tmp_path):
    p1, p2, flags = ref.planted(ref.HOMOGRAPHY)
    n = len(p1)
    # correlate.cc:159 maps list 2 onto list 1: alignment = ransac(ransac_ip2, ransac_ip1)
    left = ipm.InterestPoints(p2[:, 0], p2[:, 1], np.zeros((n, 1), np.float32))
    right = ipm.InterestPoints(p1[:, 0], p1[:, 1], np.zeros((n, 1), np.float32))
    name = str(tmp_path / "l__r.match")
    ipm.write_binary_match_file(name, left, right)
    table = ref.sample_table(n, 4, 100)
    tx = ipm.align_homography(name, samples=table)
    assert isinstance(tx, tf.HomographyTransform) and len(tf.descriptors_of(tx)) == 1
    a, b = p1.astype(np.float32).astype(np.float64), p2.astype(np.float32).astype(np.float64)     # what the file holds
    assert np.abs(tf.forward(tx, a[flags]) - b[flags]).max() <= 1e-2      # the file's float32 coordinates round by 2^-13 px at 4096
    want, _ = ipm.ransac("homography", a, b, 100, 30, n // 2, reduce=True, samples=table)
    assert np.array_equal(tx.matrix, want)
    assert np.array_equal(ipm.align_homography((left, right), samples=table).matrix, want)


# ---- the ABI and the wrapper ---------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ["vwgpu_host_last_error", "vwgpu_ip_match_chunk", "vwgpu_ip_match_dev", "vwgpu_ip_match", "vwgpu_ip_remove_duplicates", "vwgpu_fit_transform",
               "vwgpu_ransac"]


def test_new_symbols_and_abi_version():
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert lib.vwgpu_abi_version() == 3
    assert ctypes.sizeof(_lib.IpMatchParams) == 56
    c = ipm.chunk_size(1)
    assert c >= 32 and ipm.chunk_size(3 * c + 7) == c and ipm.chunk_size(2 ** 31 - 1) >= c


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


KEYS = ["ctx", "desc1", "n1", "stride1", "desc2", "n2", "stride2", "k", "pol1", "pol2", "attr1", "attr2", "params", "index", "dist", "stats"]


def _one_call(*args, **kw):
    ctx = FakeContext()
    res = ipm.match(*args, ctx=ctx, **kw)
    assert len(ctx._lib.calls) == 1
    name, a = ctx._lib.calls[0]
    assert name == "vwgpu_ip_match" and len(a) == len(KEYS)
    a = dict(zip(KEYS, a))
    P = a["params"]._obj
    a["params"] = dict(metric=P.metric, mode=P.mode, threshold=P.threshold, constraint=P.constraint, bidirectional=P.bidirectional,
                       bounds=list(P.bounds))
    return res, a


def test_wrapper_hands_the_library_the_reference_defaults():
    ip1, ip2 = _points(6, 5, 1), _points(9, 5, 2)
    # InterestPointMatcherSimple(threshold = 0.5), L2, the polarities, no attributes, no distances, no stats
    res, a = _one_call(ip1, ip2)
    assert a["ctx"] == "ctx" and a["desc1"] == ip1.descriptor.ctypes.data and a["desc2"] == ip2.descriptor.ctypes.data
    assert (a["n1"], a["stride1"], a["n2"], a["stride2"], a["k"]) == (6, 5, 9, 5, 5)
    assert a["pol1"] == ip1.polarity.ctypes.data and a["pol2"] == ip2.polarity.ctypes.data and a["attr1"] is None and a["attr2"] is None
    assert a["params"] == dict(metric=0, mode=0, threshold=0.5, constraint=0, bidirectional=0, bounds=[0, 0, 0, 0])
    assert a["index"] == res.ctypes.data and res.shape == (6,) and res.dtype == np.int32 and a["dist"] is None and a["stats"] is None
    # the kd-tree matcher's call: no polarity; the constraint's defaults and the attributes {x, y, scale, orientation}
    (res, dist), a = _one_call(ip1, ip2, 0.8, mode="knn", constraint=ipm.ScaleOrientationConstraint, bidirectional=True, return_distances=True)
    assert a["pol1"] is None and a["pol2"] is None and a["attr1"] is not None and a["attr2"] is not None
    assert a["params"] == dict(metric=0, mode=1, threshold=0.8, constraint=1, bidirectional=1, bounds=[0.9, 1.1, -0.1, 0.1])
    assert a["dist"] == dist.ctypes.data and dist.shape == (6, 2) and dist.dtype == np.float32
    res, a = _one_call(ip1, ip2, mode="knn", constraint=ipm.PositionConstraint())
    assert a["params"]["constraint"] == 2 and a["params"]["bounds"] == [-10, 10, -10, 10]
    assert ip1.attributes().tolist() == np.stack([ip1.x, ip1.y, ip1.scale, ip1.orientation], 1).tolist()
    res, a = _one_call(ip1, ip2, mode="knn")
    assert a["attr1"] is None and a["params"]["constraint"] == 0
    # Hamming: float descriptors become bytes
    b1 = ipm.InterestPoints(ip1.x, ip1.y, np.arange(30, dtype=np.float32).reshape(6, 5))
    b2 = ipm.InterestPoints(ip2.x, ip2.y, np.arange(45, dtype=np.uint8).reshape(9, 5))
    res, a = _one_call(b1, b2, metric="hamming")
    assert a["params"]["metric"] == 1 and a["desc2"] == b2.descriptor.ctypes.data and a["desc1"] != b1.descriptor.ctypes.data
    for bad in (255.5, -1.0, 256.0, float("nan")):
        d = b1.descriptor.copy()
        d[2, 3] = bad
        with pytest.raises(ArgumentErr):
            ipm.match(ipm.InterestPoints(ip1.x, ip1.y, d), b2, metric="HAMMING", ctx=FakeContext())
    # a column slice of a wider matrix is copied packed on the host side; stats are handed over
    wide = np.zeros((6, 8), np.float32)
    stats = (ctypes.c_longlong * 2)()
    res, a = _one_call(ipm.InterestPoints(ip1.x, ip1.y, wide[:, 1:6]), ip2, stats=stats)
    assert a["desc1"] != wide.ctypes.data and a["stride1"] == 5 and a["stats"] is not None
    for call in (lambda: ipm.match(ip1, _points(4, 6, 3), ctx=FakeContext()), lambda: ipm.match(ip1, ip2, metric="entropy", ctx=FakeContext()),
                 lambda: ipm.match(ip1, ip2, mode="flann", ctx=FakeContext()), lambda: ipm.match(ip1, ip2, constraint=3, ctx=FakeContext())):
        with pytest.raises(ArgumentErr):
            call()


def test_matched_pairs():
    ip1, ip2 = _points(4, 3, 1), _points(5, 3, 2)
    a, b = ipm.matched_pairs(ip1, ip2, np.array([2, -1, 4, 0], np.int32))
    assert list(a.x) == list(ip1.x[[0, 2, 3]]) and list(b.x) == list(ip2.x[[2, 4, 0]]) and b.descriptor.tolist() == ip2.descriptor[[2, 4, 0]].tolist()
    with pytest.raises(ArgumentErr):
        ipm.matched_pairs(ip1, ip2, np.array([0, 1], np.int32))
