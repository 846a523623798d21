"""Interest-point matching on the GPU against the CPU restatement (tests/refimpl/ip_match_ref.cc): index, dist[0], dist[1]
and the stats with ==, NaNs by position, through the device entry (torch tensors) and the host entry (numpy).  The shapes
sit at the kernel's boundaries: partial waves, one chunk of list 2 less one, exactly, plus one, several chunks."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import ip_match_ref as ref  # noqa: E402
from ip_match_ref import same  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import _lib  # noqa: E402
from visionworkbench_amd import interest_point as ipm  # noqa: E402
from visionworkbench_amd import transform as tf  # noqa: E402
from visionworkbench_amd._operands import new_stats  # noqa: E402

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)
CONSTRAINTS = {ref.NONE: lambda b: None, ref.SCALE_ORIENTATION: lambda b: ipm.ScaleOrientationConstraint(*b),
               ref.POSITION: lambda b: ipm.PositionConstraint(*b)}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def chunk():
    return ipm.chunk_size(1)


def points(desc, pol=None, attr=None):
    n = desc.shape[0]
    a = np.zeros((n, 4), np.float32) if attr is None else np.asarray(attr, np.float32)
    ip = ipm.InterestPoints(a[:, 0], a[:, 1], desc, scale=a[:, 2] if attr is not None else None, orientation=a[:, 3], polarity=pol)
    if pol is None:
        ip.polarity = None      # a null polarity pointer
    return ip


def check(ctx, d1, d2, threshold=0.5, metric=ref.L2, mode=ref.SIMPLE, pol1=None, pol2=None, attr1=None, attr2=None, ckind=ref.NONE,
          bounds=(0, 0, 0, 0), bidirectional=False, what="", sides=("device", "host")):
    """Both entries against the restatement; returns the restatement's (index, dist, stats)."""
    import torch
    want = ref.match(d1, d2, threshold, metric, mode, pol1, pol2, attr1, attr2, ckind, bounds, bidirectional)
    kw = dict(threshold=threshold, metric="L2" if metric == ref.L2 else "HAMMING", mode="simple" if mode == ref.SIMPLE else "knn",
              constraint=CONSTRAINTS[ckind](bounds), bidirectional=bidirectional, return_distances=True, ctx=ctx)
    for side in sides:
        a, b = (torch.from_numpy(np.ascontiguousarray(d)).cuda() for d in (d1, d2)) if side == "device" else (d1, d2)
        stats = new_stats(2)
        index, dist = ipm.match(points(a, pol1, attr1), points(b, pol2, attr2), stats=stats, **kw)
        if side == "device":
            assert index.is_cuda and dist.is_cuda
            index, dist = index.cpu().numpy(), dist.cpu().numpy()
        same(index, want[0], "%s %s index" % (what, side))
        same(dist, want[1], "%s %s dist" % (what, side))
        assert list(stats) == want[2], "%s %s stats" % (what, side)
    return want


# ---- shapes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 3, 127, 128, 130, 512])
def test_descriptor_lengths(ctx, chunk, k):
    """Uniform floats, where the serial order of the sum shows, and integer values with their ties; two chunks and a tail."""
    d1, d2 = ref.uniform_scene(65, 2 * chunk + 7, k)
    for mode in (ref.SIMPLE, ref.KNN):
        check(ctx, d1, d2, 0.9, mode=mode, what="uniform k %d mode %d" % (k, mode))
    e1, e2 = ref.integer_scene(65, 2 * chunk + 7, k, top=3)
    check(ctx, e1, e2, 0.9, what="integer k %d" % k)


def test_longer_descriptors_are_not_implemented(ctx):
    d1, d2 = ref.uniform_scene(2, 3, 513)
    with pytest.raises(vwa.NoImplErr):
        ipm.match(points(d1), points(d2), ctx=ctx)
    b = np.zeros((2, 513), np.uint8)
    with pytest.raises(vwa.NoImplErr):
        ipm.match(points(b), points(b), metric="HAMMING", ctx=ctx)


@pytest.mark.parametrize("n1", [1, 63, 64, 65, 200])
def test_query_counts(ctx, chunk, n1):
    d1, d2 = ref.uniform_scene(n1, chunk + 1, 128, seed=n1)
    check(ctx, d1, d2, 0.95, what="n1 %d" % n1)
    check(ctx, d1, d2, 0.95, mode=ref.KNN, what="n1 %d knn" % n1, sides=("device",))


def test_candidate_counts(ctx, chunk):
    for n2 in (1, 2, chunk - 1, chunk, chunk + 1, 3 * chunk + 7):
        assert ipm.chunk_size(n2) == chunk
        d1, d2 = ref.uniform_scene(65, n2, 128, seed=n2)
        for mode in (ref.SIMPLE, ref.KNN):
            check(ctx, d1, d2, 0.95, mode=mode, what="n2 %d mode %d" % (n2, mode), sides=("device",) if mode == ref.KNN else ("device", "host"))


# ---- where the picks lie ------------------------------------------------------------------------------------------------------

def test_picks_in_different_chunks(ctx, chunk):
    k, n2 = 128, 3 * chunk + 7
    d1, d2 = ref.uniform_scene(65, n2, k, seed=9)
    near, nearer = d1 + np.float32(0.125), d1 + np.float32(0.0625)
    for lo, hi, what in ((3, n2 - 2, "minimum first, second last"), (n2 - 2, 3, "minimum last, second first")):
        e2 = d2.copy()
        e2[lo], e2[hi] = nearer[0], near[0]
        index, dist, _ = check(ctx, d1[:1], e2, 0.9, what=what)
        assert index[0] == lo and dist[0, 0] < dist[0, 1] < 3
        check(ctx, d1[:1], e2, 0.9, mode=ref.KNN, what=what + " knn")
    # the same descriptor at two indices of different chunks: the lowest index, and dist[0] == dist[1]
    e2 = d2.copy()
    e2[chunk + 5] = e2[5] = e2[2 * chunk + 1] = nearer[0]
    for mode in (ref.SIMPLE, ref.KNN):
        index, dist, _ = check(ctx, d1[:1], e2, 1.0, mode=mode, what="duplicate across chunks mode %d" % mode)
        assert dist[0, 0] == dist[0, 1] and index[0] == (5 if mode == ref.SIMPLE else -1)
    # every distance equal
    ones = np.ones((n2, k), np.float32)
    for mode, thr, hit in ((ref.SIMPLE, 1.0, 0), (ref.SIMPLE, 0.5, -1), (ref.KNN, 1.0, -1), (ref.KNN, 1.5, 0)):
        index, dist, stats = check(ctx, np.zeros((65, k), np.float32), ones, thr, mode=mode, what="all equal mode %d thr %g" % (mode, thr))
        assert (index == hit).all() and (dist == k).all() and stats == [65 if hit == 0 else 0, 65]


# ---- decisions -------------------------------------------------------------------------------------------------------------

def test_decisions(ctx):
    e1, e2 = np.array([[0, 0]], np.float32), np.array([[2, 0], [0, 4]], np.float32)
    # one candidate: SIMPLE matches (second pick 1e100), KNN does not
    for mode, hit in ((ref.SIMPLE, 0), (ref.KNN, -1)):
        index, dist, _ = check(ctx, e1, e2[:1], 0.5, mode=mode, what="one candidate")
        assert index[0] == hit and list(dist[0]) == [4, INF]
    # an exact zero distance with a duplicate
    z2 = np.array([[5, 5], [0, 0], [0, 0]], np.float32)
    for mode, hit in ((ref.SIMPLE, 1), (ref.KNN, -1)):
        index, dist, _ = check(ctx, e1, z2, 0.5, mode=mode, what="zero distance")
        assert index[0] == hit and list(dist[0]) == [0, 0]
    # first == threshold * second exactly: 4 and 16 at 0.25; > keeps the match, < drops it
    for mode, hit in ((ref.SIMPLE, 0), (ref.KNN, -1)):
        index, dist, _ = check(ctx, e1, e2, 0.25, mode=mode, what="equality")
        assert index[0] == hit and list(dist[0]) == [4, 16]
    # thresholds of 1 and more
    d1, d2 = ref.integer_scene(70, 90, 7, top=4)
    for thr in (1.0, 2.5, float("inf")):
        for mode in (ref.SIMPLE, ref.KNN):
            check(ctx, d1, d2, thr, mode=mode, what="threshold %g mode %d" % (thr, mode))


def test_polarity(ctx, chunk):
    d1, d2 = ref.integer_scene(65, chunk + 9, 16, top=5)
    n1, n2 = len(d1), len(d2)
    alt1, alt2 = (np.arange(n1) % 2).astype(np.uint8), (np.arange(n2) % 2).astype(np.uint8)
    equal = check(ctx, d1, d2, 0.8, pol1=np.ones(n1, np.uint8), pol2=np.ones(n2, np.uint8), what="all equal")
    null = check(ctx, d1, d2, 0.8, what="null polarity")
    assert np.array_equal(equal[0], null[0]) and np.array_equal(equal[1], null[1])
    alternating = check(ctx, d1, d2, 0.8, pol1=alt1, pol2=alt2, what="alternating")
    assert not np.array_equal(alternating[1], null[1])
    hit = alternating[0] >= 0
    assert (alt2[alternating[0][hit]] == alt1[hit]).all()
    none = check(ctx, d1, d2, 0.8, pol1=np.zeros(n1, np.uint8), pol2=np.ones(n2, np.uint8), what="none compatible")
    assert (none[0] == -1).all() and (none[1] == INF).all() and none[2] == [0, n1]
    # KNN ignores polarity
    import torch
    knn = ref.match(d1, d2, 0.8, mode=ref.KNN)
    for a, b in ((d1, d2), (torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda())):
        index = ipm.match(points(a, alt1), points(b, 1 - alt2), 0.8, mode="knn", ctx=ctx)
        same(index.cpu().numpy() if hasattr(index, "cpu") else index, knn[0], "knn ignores polarity")


def test_values_that_are_never_picked(ctx, chunk):
    k = 128
    d1, d2 = ref.uniform_scene(65, chunk + 3, k, seed=4)
    e2 = d2.copy()
    e2[7] = d1[0]
    e2[7, 100] = np.nan                      # the nearest but for one NaN element
    e2[chunk + 1] = d1[1]
    e2[chunk + 1, 5] = 3e38                  # the sum overflows to inf
    e2[9, :] = -3e38
    index, dist, _ = check(ctx, d1, e2, 0.95, what="nan and inf candidates")
    assert 7 not in index and chunk + 1 not in index and 9 not in index and np.isfinite(dist).all()
    check(ctx, d1, e2, 0.95, mode=ref.KNN, what="nan and inf candidates knn")
    # a NaN element in a query: no match, no picks
    e1 = d1.copy()
    e1[3, 0] = np.nan
    e1[64, k - 1] = np.nan
    for mode in (ref.SIMPLE, ref.KNN):
        index, dist, _ = check(ctx, e1, d2, 2.0, mode=mode, what="nan query mode %d" % mode)
        assert index[3] == -1 and index[64] == -1 and (dist[[3, 64]] == INF).all() and (index[:3] >= 0).all()
    # only unusable candidates
    index, dist, stats = check(ctx, d1[:2], e2[[7, 9]], 2.0, what="nothing comparable")
    assert list(index) == [-1, -1] and stats == [0, 2]


@pytest.mark.parametrize("k", [3, 15, 32, 64, 67])
def test_hamming(ctx, chunk, k):
    rng = np.random.RandomState(k)
    d1, d2 = rng.randint(0, 256, (65, k)).astype(np.uint8), rng.randint(0, 256, (chunk + 5, k)).astype(np.uint8)
    d2[chunk + 2] = d2[4] = d1[10]            # a zero distance twice
    for mode in (ref.SIMPLE, ref.KNN):
        index, dist, _ = check(ctx, d1, d2, 0.9, metric=ref.HAMMING, mode=mode, what="hamming k %d mode %d" % (k, mode))
        assert (dist == np.round(dist)).all() and dist[10, 0] == 0 and index[10] == (4 if mode == ref.SIMPLE else -1)
    # float input through the wrapper, on both sides
    import torch
    want = ref.match(d1, d2, 0.9, metric=ref.HAMMING)
    f1, f2 = d1.astype(np.float32), d2.astype(np.float32)
    for a, b in ((f1, f2), (torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda())):
        index, dist = ipm.match(points(a), points(b), 0.9, metric="HAMMING", return_distances=True, ctx=ctx)
        same(np.asarray(index.cpu() if hasattr(index, "cpu") else index), want[0], "hamming float input index")
        same(np.asarray(dist.cpu() if hasattr(dist, "cpu") else dist), want[1], "hamming float input dist")
    with pytest.raises(vwa.ArgumentErr):
        ipm.match(points(torch.from_numpy(f1 + 0.5).cuda()), points(torch.from_numpy(f2).cuda()), metric="HAMMING", ctx=ctx)


def test_hamming_long(ctx, chunk):
    rng = np.random.RandomState(2)
    d1, d2 = rng.randint(0, 256, (65, 512)).astype(np.uint8), rng.randint(0, 256, (chunk + 5, 512)).astype(np.uint8)
    check(ctx, d1, d2, 0.99, metric=ref.HAMMING, what="hamming k 512")
    check(ctx, d1[:, :130], d2[:, :130], 0.99, metric=ref.HAMMING, mode=ref.KNN, what="hamming k 130, a slice")


# ---- constraints ---------------------------------------------------------------------------------------------------------------

def test_constraints_in_knn(ctx):
    # query 0: the nearest (index 0) fails the position constraint, the second (index 1) would pass: -1
    d1 = np.array([[0, 0], [10, 10]], np.float32)
    d2 = np.array([[1, 0], [3, 0], [10, 11], [30, 30]], np.float32)
    attr1 = np.array([[100, 100, 1, 0], [50, 50, 1, 0]], np.float32)
    attr2 = np.array([[150, 100, 1, 0], [101, 101, 1, 0], [52, 47, 1, 0], [0, 0, 1, 0]], np.float32)
    # PositionConstraint(baseline = the candidate, test = the query): dx = query.x - candidate.x
    index, _, _ = check(ctx, d1, d2, 0.9, mode=ref.KNN, attr1=attr1, attr2=attr2, ckind=ref.POSITION, bounds=(-10, 10, -10, 10), what="position")
    assert list(index) == [-1, 2]
    assert list(check(ctx, d1, d2, 0.9, mode=ref.KNN, attr1=attr1, attr2=attr2, what="no constraint")[0]) == [0, 2]
    # asymmetric bounds: query 1 against candidate 2 has dx = -2, dy = 3; one way passes, the other way has dx = 2, dy = -3
    one_way = (-5, 0, 0, 5)
    assert list(check(ctx, d1, d2, 0.9, mode=ref.KNN, attr1=attr1, attr2=attr2, ckind=ref.POSITION, bounds=one_way, what="one way")[0]) == [-1, 2]
    assert list(check(ctx, d1, d2, 0.9, mode=ref.KNN, attr1=attr1, attr2=attr2, ckind=ref.POSITION, bounds=one_way, bidirectional=True,
                      what="both ways")[0]) == [-1, -1]
    both = (-5, 5, -5, 5)
    assert list(check(ctx, d1, d2, 0.9, mode=ref.KNN, attr1=attr1, attr2=attr2, ckind=ref.POSITION, bounds=both, bidirectional=True,
                      what="both ways, symmetric")[0]) == [-1, 2]
    # SIMPLE never consults its constraint
    assert list(check(ctx, d1, d2, 0.9, attr1=attr1, attr2=attr2, ckind=ref.POSITION, bounds=(-1, 1, -1, 1), what="simple")[0]) == [0, 2]


def test_orientation_wrap_and_scale(ctx):
    pi = np.float32(np.pi)
    d1 = np.array([[0, 0], [10, 10], [20, 20], [40, 40]], np.float32)
    d2 = np.array([[0, 1], [10, 11], [20, 21], [40, 41], [90, 90]], np.float32)
    # orientation differences query - candidate: 3.0 - (-3.1) = 6.1 -> wraps to -0.18; -3.1 - 3.0 = -6.1 -> 0.18; pi - (-pi) is
    # 2 * float(pi) in float and wraps once to about +1.7e-7, not to 0; the last query fails on the scale ratio 2
    attr1 = np.array([[0, 0, 1, 3.0], [0, 0, 1, -3.1], [0, 0, 1, pi], [0, 0, 2, 0]], np.float32)
    attr2 = np.array([[0, 0, 1, -3.1], [0, 0, 1, 3.0], [0, 0, 1, -pi], [0, 0, 1, 0], [0, 0, 1, 0]], np.float32)
    for bounds, want in (((0.9, 1.1, -0.2, 0.2), [0, 1, 2, -1]), ((0.9, 1.1, -0.2, 0.0), [0, -1, -1, -1]), ((0.9, 1.1, 0.0, 0.2), [-1, 1, 2, -1]),
                         ((0.9, 2.0, -0.1, 0.1), [-1, -1, 2, 3])):
        index, _, _ = check(ctx, d1, d2, 0.9, mode=ref.KNN, attr1=attr1, attr2=attr2, ckind=ref.SCALE_ORIENTATION, bounds=bounds,
                            what="scale orientation %s" % (bounds,))
        assert list(index) == want
    # both ways the scale ratio of the last query is 2 and 0.5
    index, _, _ = check(ctx, d1, d2, 0.9, mode=ref.KNN, attr1=attr1, attr2=attr2, ckind=ref.SCALE_ORIENTATION, bounds=(0.9, 2.0, -0.2, 0.2),
                        bidirectional=True, what="scale both ways")
    assert list(index) == [0, 1, 2, -1]
    # the golden truth table, with the query as test_ip
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "ip_known.json")))["constraints"]
    kinds = {"none": ref.NONE, "scale_orientation": ref.SCALE_ORIENTATION, "position": ref.POSITION}
    one = np.array([[0, 1, 0]], np.float32)
    two = np.array([[0, 1, 0], [9, 9, 9]], np.float32)
    for case in g["cases"]:
        index, _, _ = check(ctx, one, two, 0.5, mode=ref.KNN, attr1=np.array([g["ip2"]], np.float32), attr2=np.array([g["ip1"]] * 2, np.float32),
                            ckind=kinds[case["kind"]], bounds=case["bounds"], what=case["name"])
        assert (index[0] == 0) == case["result"]


# ---- layout ----------------------------------------------------------------------------------------------------------------

def test_strided_descriptors_and_sentinels(ctx, chunk):
    import torch
    lib = _lib.load()
    k, n1, n2 = 130, 70, chunk + 3
    rng = np.random.RandomState(8)
    wide1, wide2 = rng.random_sample((n1, k + 9)).astype(np.float32), rng.random_sample((n2, k + 20)).astype(np.float32)
    v1, v2 = wide1[:, 4:4 + k], wide2[:, 11:11 + k]
    want = ref.match(v1, v2, 0.95)
    t1, t2 = torch.from_numpy(wide1).cuda(), torch.from_numpy(wide2).cuda()
    s1, s2 = t1[:, 4:4 + k], t2[:, 11:11 + k]
    index, dist = ipm.match(points(s1), points(s2), 0.95, return_distances=True, ctx=ctx)
    same(index.cpu().numpy(), want[0], "strided index")
    same(dist.cpu().numpy(), want[1], "strided dist")
    same(ipm.match(points(v1), points(v2), 0.95, ctx=ctx), want[0], "strided host index")
    # outputs surrounded by sentinels: no word outside the payload changes, on either entry
    P = _lib.IpMatchParams(0, 0, 0.95, 0, 0, (ctypes.c_double * 4)(0, 0, 0, 0))
    pad = 64
    oi, od = torch.full((n1 + 2 * pad,), -77, dtype=torch.int32, device="cuda"), torch.full((2 * n1 + 2 * pad,), -77.0, device="cuda")
    stats = new_stats(2)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    rc = lib.vwgpu_ip_match_dev(ctx._h, s1.data_ptr(), n1, s1.stride(0), s2.data_ptr(), n2, s2.stride(0), k, None, None, None, None,
                                ctypes.byref(P), oi[pad:].data_ptr(), od[pad:].data_ptr(), stats)
    assert rc == 0 and list(stats) == want[2]
    oi, od = oi.cpu().numpy(), od.cpu().numpy()
    same(oi[pad:-pad], want[0], "sentinel index")
    same(od[pad:-pad].reshape(n1, 2), want[1], "sentinel dist")
    assert (oi[:pad] == -77).all() and (oi[-pad:] == -77).all() and (od[:pad] == -77).all() and (od[-pad:] == -77).all()
    hi, hd = np.full(n1 + 2 * pad, -77, np.int32), np.full(2 * n1 + 2 * pad, -77, np.float32)
    rc = lib.vwgpu_ip_match(ctx._h, v1.ctypes.data, n1, wide1.shape[1], v2.ctypes.data, n2, wide2.shape[1], k, None, None, None, None,
                            ctypes.byref(P), hi[pad:].ctypes.data, hd[pad:].ctypes.data, None)
    assert rc == 0
    same(hi[pad:-pad], want[0], "host sentinel index")
    same(hd[pad:-pad].reshape(n1, 2), want[1], "host sentinel dist")
    assert (hi[:pad] == -77).all() and (hi[-pad:] == -77).all() and (hd[:pad] == -77).all() and (hd[-pad:] == -77).all()


def test_argument_errors_come_before_device_work(ctx):
    lib, h = _lib.load(), ctx._h
    d = np.zeros((4, 8), np.float32)
    out, dist = np.full(4, -5, np.int32), np.zeros((4, 2), np.float32)
    pol = np.zeros(4, np.uint8)

    def call(d1=d.ctypes.data, n1=4, s1=8, d2=d.ctypes.data, n2=4, s2=8, k=8, p1=None, p2=None, a1=None, a2=None, params="default",
             index=out.ctypes.data, dd=None, metric=0, mode=0, thr=0.5, cons=0):
        P = _lib.IpMatchParams(metric, mode, thr, cons, 0, (ctypes.c_double * 4)(0, 0, 0, 0))
        return lib.vwgpu_ip_match(h, d1, n1, s1, d2, n2, s2, k, p1, p2, a1, a2, ctypes.byref(P) if params == "default" else None, index, dd, None)

    assert call() == 0
    bad = [dict(d1=None), dict(d2=None), dict(params=None), dict(index=None), dict(n1=0), dict(n2=0), dict(k=0), dict(s1=7), dict(s2=3),
           dict(metric=2), dict(metric=-1), dict(mode=2), dict(cons=3), dict(thr=float("nan")), dict(p1=pol.ctypes.data),
           dict(mode=1, cons=1), dict(index=d.ctypes.data), dict(dd=d.ctypes.data), dict(dd=out.ctypes.data)]
    out[:] = -5
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.vwgpu_last_error(h), kw
    assert (out == -5).all()
    assert call(k=513, s1=600, s2=600) == -2 and b"512" in lib.vwgpu_last_error(h)
    assert lib.vwgpu_ip_match(None, d.ctypes.data, 4, 8, d.ctypes.data, 4, 8, 8, None, None, None, None, None, out.ctypes.data, None, None) == -1


# ---- golden and end to end -----------------------------------------------------------------------------------------------------

def test_golden_matcher_case(ctx):
    m = json.load(open(os.path.join(ROOT, "tests", "golden", "ip_known.json")))["matcher"]
    d1 = np.array([m["ip1"]["descriptor"]], np.float32)
    d2 = np.array([p["descriptor"] for p in m["ip2"]], np.float32)
    for mode in (ref.SIMPLE, ref.KNN):
        index, _, _ = check(ctx, d1, d2, m["threshold"], mode=mode, what="golden")
        assert list(index) == m["matched_indexes"]
    ip1, ip2 = points(d1), points(d2)
    a, b = ipm.matched_pairs(ip1, ip2, ipm.match(ip1, ip2, mode="knn", ctx=ctx))
    assert len(a) == 1 and b.descriptor.tolist() == [m["matched_ip2_descriptor"]]


def test_end_to_end_alignment(ctx):
    """300 synthetic points with K = 128; list 2 holds the same descriptors permuted, with small noise, plus 100 distractors;
    its positions are the planted homography of list 1's.  match -> remove_duplicates -> ransac recovers the homography:
    every pair is an inlier, and, the positions being float32 (noise of about 1e-4 px), under the condition for noisy
    inliers: the sum of squared errors is at most that of the planted map on the same pairs x (1 + 1e-9).
    transform.transform with the result equals transform.transform with the same matrix passed directly."""
    import torch
    rng = np.random.RandomState(12)
    n, extra, k = 300, 100, 128
    desc1 = rng.random_sample((n, k)).astype(np.float32)
    perm = rng.permutation(n + extra)
    desc2 = np.concatenate([desc1 + 0.01 * rng.standard_normal((n, k)).astype(np.float32), rng.random_sample((extra, k)).astype(np.float32)])[perm]
    xy1 = rng.uniform(0, 4096, (n, 2))
    xy2 = np.concatenate([ref.apply(ref.PLANTED[ref.HOMOGRAPHY], xy1), rng.uniform(0, 4096, (extra, 2))])[perm]
    where = np.argsort(perm)[:n]            # the row of list 2 that holds point i of list 1
    ip1 = ipm.InterestPoints(xy1[:, 0], xy1[:, 1], torch.from_numpy(desc1).cuda())
    ip2 = ipm.InterestPoints(xy2[:, 0], xy2[:, 1], torch.from_numpy(desc2).cuda())
    index = ipm.match(ip1, ip2, 0.5, ctx=ctx)
    same(index.cpu().numpy(), ref.match(desc1, desc2, 0.5)[0], "end to end index")
    same(index.cpu().numpy(), where.astype(np.int32), "every point finds its partner")
    m1, m2 = ipm.remove_duplicates(*ipm.matched_pairs(ip1, ip2, index))
    assert len(m1) == n
    # as correlate.cc:159: the alignment maps list 2 onto list 1
    p1, p2 = ipm.iplist_to_vectorlist(m2), ipm.iplist_to_vectorlist(m1)
    H, inl = ipm.ransac("homography", p1, p2, 100, 30, n // 2, reduce=True, seed=1)
    assert inl.all()
    Hr, _ = ref.ransac(ref.HOMOGRAPHY, p1[:, :2], p2[:, :2], ipm.ransac_samples(n, 4, 100, seed=1), 30, n // 2)
    got, truth = ref.apply(H, p1[:, :2]), ref.apply(np.linalg.inv(ref.PLANTED[ref.HOMOGRAPHY]), xy2[where])
    sse = lambda M: float((np.linalg.norm(ref.apply(M, p1[:, :2]) - p2[:, :2], axis=1) ** 2).sum())      # noqa: E731
    print("worst against the planted map %.3g px; sse %.6g, restatement %.6g, planted %.6g" % (
        np.abs(got - truth).max(), sse(H), sse(Hr), sse(np.linalg.inv(ref.PLANTED[ref.HOMOGRAPHY]))))
    assert sse(H) <= sse(np.linalg.inv(ref.PLANTED[ref.HOMOGRAPHY])) * (1 + 1e-9)
    img = torch.from_numpy(np.random.RandomState(1).random_sample((96, 128)).astype(np.float32)).cuda()
    tx = ipm.align_homography((m1, m2), seed=1)
    assert np.array_equal(tx.matrix, H)
    a = tf.transform(img, tx, ctx=ctx)
    b = tf.transform(img, ipm.HomographyTransform(H.copy()), ctx=ctx)
    same(a.cpu().numpy(), b.cpu().numpy(), "aligned image")
    assert float(a.abs().sum()) > 0
