"""vw::ip matching and the RANSAC alignment of vw::math on the GPU: InterestPointMatcherSimple and InterestPointMatcher
(src/vw/InterestPoint/Matcher.h) as an exact search, remove_duplicates, the fitting functors of src/vw/Math/Geometry.h,
RandomSampleConsensus (src/vw/Math/RANSAC.h), the binary .vwip / .match files of src/vw/InterestPoint/MatcherIO.cc and the
alignment step of tools/correlate.cc:147-166; and what tools/ipfind.cc runs without OpenCV: IntegralImage, the OBALoG detectors
IntegralAutoGainDetector and IntegralInterestPointDetector (src/vw/InterestPoint/IntegralDetector.h) over the tiles of
detect_interest_points, and the SGrad / SGrad2 descriptors over the crops of describe_interest_points.

Descriptors are (N, K) arrays: numpy in -> numpy out, CUDA tensors in -> CUDA tensors out on the current torch stream.  The
fits, RANSAC and remove_duplicates run on the host; so do the tile loops, the cull rule and the crops of the detectors.
"""
import ctypes
import os
import struct

import numpy as np

from . import _lib
from ._operands import Operands, is_tensor, new_stats, put_stats
from .core import ArgumentErr, CapacityErr, IOErr, LogicErr, NoImplErr
from .stereo import HomographyTransform

METRICS = {"L2": 0, "HAMMING": 1}
MODES = {"simple": 0, "knn": 1}
SIMILARITY, AFFINE, HOMOGRAPHY = range(3)
KINDS = {"similarity": SIMILARITY, "affine": AFFINE, "homography": HOMOGRAPHY}
MAX_K = 512
_FIELDS = (("x", np.float32), ("y", np.float32), ("ix", np.int32), ("iy", np.int32), ("orientation", np.float32), ("scale", np.float32),
           ("interest", np.float32), ("polarity", np.uint8), ("octave", np.uint32), ("scale_lvl", np.uint32))
_HEAD = struct.Struct("<ffiifffBIIQ")      # one record up to and including the descriptor's size
_STATUS_EXC = {-1: ArgumentErr, -2: NoImplErr}


def chunk_size(n2=1):
    """The number of list-2 candidates one workgroup searches (vwgpu_ip_match_chunk)."""
    return int(_lib.load().vwgpu_ip_match_chunk(int(n2)))


class InterestPoints(object):
    """A list of vw::ip::InterestPoint (src/vw/InterestPoint/InterestPoint.h:43-124) as arrays: x, y, ix, iy, orientation, scale,
    interest, polarity, octave, scale_lvl of length N and descriptor (N, K).  Only x, y and descriptor must be given;
    ix, iy default to x, y converted to int as the reference's constructor does, scale to 1, the others to 0.  A list whose
    polarity attribute is set to None has no polarities: match() passes none (all equal), a file gets zeros."""

    def __init__(self, x, y, descriptor, ix=None, iy=None, orientation=None, scale=None, interest=None, polarity=None, octave=None,
                 scale_lvl=None):
        self.x, self.y = np.ascontiguousarray(x, np.float32).reshape(-1), np.ascontiguousarray(y, np.float32).reshape(-1)
        n = self.x.size
        self.descriptor = descriptor if is_tensor(descriptor) else np.asarray(descriptor)
        if self.descriptor.ndim != 2 or self.descriptor.shape[0] != n or self.y.size != n:
            raise ArgumentErr("InterestPoints: x, y of length N and a descriptor (N, K)")
        given = dict(ix=ix, iy=iy, orientation=orientation, scale=scale, interest=interest, polarity=polarity, octave=octave,
                     scale_lvl=scale_lvl)
        default = dict(ix=self.x.astype(np.int32), iy=self.y.astype(np.int32), scale=np.ones(n, np.float32))
        for name, dtype in _FIELDS[2:]:
            v = given[name]
            v = default.get(name, np.zeros(n, dtype)) if v is None else np.ascontiguousarray(v).reshape(-1)
            if v.size != n:
                raise ArgumentErr("InterestPoints: %s must have length %d" % (name, n))
            setattr(self, name, (v != 0).astype(np.uint8) if name == "polarity" else v.astype(dtype))

    def __len__(self):
        return int(self.x.size)

    def take(self, index):
        """The points at `index` (an index array or a boolean mask), in that order."""
        index = np.asarray(index)
        d = self.descriptor
        if is_tensor(d):
            import torch
            d = d[torch.as_tensor(index, device=d.device)]
        else:
            d = d[index]
        out = InterestPoints(self.x[index], self.y[index], d, **{name: getattr(self, name)[index] for name, _ in _FIELDS[2:]
                                                                 if getattr(self, name) is not None})
        if self.polarity is None:      # a list without polarities (match() then passes none) stays one
            out.polarity = None
        return out

    def attributes(self):
        """float32 (N, 4) = x, y, scale, orientation: what the constraints read."""
        return np.ascontiguousarray(np.stack([self.x, self.y, self.scale, self.orientation], axis=1), np.float32)


# ---- constraints ---------------------------------------------------------------------------------------------------------

class NullConstraint(object):
    code, bounds = 0, (0.0, 0.0, 0.0, 0.0)


class ScaleOrientationConstraint(object):
    """ScaleOrientationConstraint(srmin = 0.9, srmax = 1.1, odmin = -0.1, odmax = 0.1) (Matcher.h:113-130)."""
    code = 1

    def __init__(self, scale_ratio_min=0.9, scale_ratio_max=1.1, ori_diff_min=-0.1, ori_diff_max=0.1):
        self.bounds = (float(scale_ratio_min), float(scale_ratio_max), float(ori_diff_min), float(ori_diff_max))


class PositionConstraint(object):
    """PositionConstraint(min_x = -10, max_x = 10, min_y = -10, max_y = 10) (Matcher.h:133-149)."""
    code = 2

    def __init__(self, min_x=-10.0, max_x=10.0, min_y=-10.0, max_y=10.0):
        self.bounds = (float(min_x), float(max_x), float(min_y), float(max_y))


def _code(table, key, what):
    k = key.upper() if table is METRICS else str(key).lower()
    if k not in table:
        raise ArgumentErr("match: %s %r is not one of %s" % (what, key, ", ".join(sorted(table))))
    return table[k]


def _bytes(ops, d):
    """Descriptors for the Hamming metric as uint8; float values must be whole numbers of 0 .. 255 (the reference's
    static_cast<uint8> of anything else is undefined)."""
    if ops.dtype_of(d) == np.dtype(np.uint8):
        return d
    ok = (d >= 0) & (d <= 255)      # a NaN fails both
    if ops.tensor:
        import torch
        if d.is_floating_point():
            ok = ok & (d == torch.floor(d))
    elif d.dtype.kind == "f":
        ok = ok & (d == np.floor(d))
    if not bool(ok.all()):
        raise ArgumentErr("match: the Hamming metric needs descriptor values that are whole numbers of 0 .. 255")
    return d.to(torch.uint8) if ops.tensor else d.astype(np.uint8)


def _side(ops, a):
    """A small host array on the side of the call."""
    if a is None:
        return None
    if ops.tensor:
        import torch
        return torch.as_tensor(a, device=ops.device)
    return a


def match(ip1, ip2, threshold=0.5, metric="L2", mode="simple", constraint=None, bidirectional=False, return_distances=False, stats=None,
          ctx=None):
    """The matcher of ipmatch (tools/ipmatch.cc:356-373) as an exact search: for every point of ip1 the index of its match in
    ip2, or -1 (int32, length len(ip1)).
    mode "simple": InterestPointMatcherSimple<metric, constraint>(threshold) (Matcher.h:435-508): points of another polarity
    are skipped, no match when first_pick > threshold * second_pick; the constraint is not consulted, as in the reference.
    mode "knn": InterestPointMatcher<metric, constraint>(threshold, bidirectional) (Matcher.h:282-386) with an exact
    two-nearest search: a match when the constraint holds for the nearest candidate and dist0 < threshold * dist1.
    metric "L2" (float descriptors) or "HAMMING" (bytes; float descriptors are converted).
    return_distances: also float32 (N1, 2), the two smallest distances (+inf where there is none).
    stats: an optional _operands.new_stats(2) for {matched, queries}."""
    d1, d2 = ip1.descriptor, ip2.descriptor
    ops = Operands("match", d1, ctx)
    m, md = _code(METRICS, metric, "metric"), _code(MODES, mode, "mode")
    c = NullConstraint() if constraint is None else (constraint() if isinstance(constraint, type) else constraint)
    if not hasattr(c, "code") or not hasattr(c, "bounds"):
        raise ArgumentErr("match: %r is no constraint" % (constraint,))
    if d1.ndim != 2 or d2.ndim != 2 or d1.shape[1] != d2.shape[1]:
        raise ArgumentErr("match: the descriptors must be (N1, K) and (N2, K)")
    n1, n2, k = int(d1.shape[0]), int(d2.shape[0]), int(d1.shape[1])
    if n1 < 1 or n2 < 1 or k < 1:
        raise ArgumentErr("match: empty point list or descriptor")
    if m == METRICS["HAMMING"]:
        ops._side(d2)
        d1, d2 = _bytes(ops, d1), _bytes(ops, d2)
        dtype = np.uint8
    else:
        dtype = np.float32
    d1, d2 = ops.image(d1, dtype, rows=True), ops.image(d2, dtype, rows=True)
    simple = md == MODES["simple"]
    p1 = p2 = a1 = a2 = None
    if simple:
        p1, p2 = _side(ops, getattr(ip1, "polarity", None)), _side(ops, getattr(ip2, "polarity", None))      # None: all equal
    elif c.code != 0:
        a1, a2 = _side(ops, ip1.attributes()), _side(ops, ip2.attributes())
    params = _lib.IpMatchParams(m, md, float(threshold), c.code, int(bool(bidirectional)), (ctypes.c_double * 4)(*c.bounds))
    index = ops.empty((n1,), np.int32)
    dist = ops.empty((n1, 2), np.float32) if return_distances else None
    st = new_stats(2) if stats is not None else None
    ops.call("ip_match", ops.ptr(d1), n1, ops.row_stride(d1), ops.ptr(d2), n2, ops.row_stride(d2), k, ops.ptr(p1), ops.ptr(p2), ops.ptr(a1),
             ops.ptr(a2), ctypes.byref(params), ops.ptr(index), ops.ptr(dist), st)
    put_stats(stats, st if st is not None else ())
    return (index, dist) if return_distances else index


def matched_pairs(ip1, ip2, index):
    """(matched_ip1, matched_ip2): the points of ip1 that found a match and their partners, in ip1's order (Matcher.h:499-505)."""
    index = index.cpu().numpy() if is_tensor(index) else np.asarray(index)
    if index.shape != (len(ip1),):
        raise ArgumentErr("matched_pairs: one index per point of ip1")
    hit = np.flatnonzero((index >= 0) & (index < len(ip2)))
    return ip1.take(hit), ip2.take(index[hit])


def _host_check(rc):
    if rc != 0:
        lib = _lib.load()
        text = lib.vwgpu_host_last_error().decode()
        raise _STATUS_EXC.get(rc, LogicErr)(text or lib.vwgpu_strerror(rc).decode())


def remove_duplicates(ip1, ip2):
    """remove_duplicates(ip1, ip2) (Matcher.cc:152-195) of two matched lists: a pair is dropped when a later pair has the
    same (x, y) in list 1 or the same (x, y) in list 2.  Returns the two filtered lists."""
    if len(ip1) != len(ip2):
        raise ArgumentErr("Input vectors are not the same size.")
    keep = remove_duplicates_mask(np.stack([ip1.x, ip1.y], 1), np.stack([ip2.x, ip2.y], 1))
    return ip1.take(keep), ip2.take(keep)


def remove_duplicates_mask(xy1, xy2):
    """The boolean keep mask of remove_duplicates for two float32 (N, 2) arrays of positions."""
    a, b = np.ascontiguousarray(xy1, np.float32), np.ascontiguousarray(xy2, np.float32)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape != b.shape:
        raise ArgumentErr("Input vectors are not the same size.")
    keep = np.zeros(a.shape[0], np.uint8)
    kept = ctypes.c_longlong(0)
    _host_check(_lib.load().vwgpu_ip_remove_duplicates(a.ctypes.data, b.ctypes.data, a.shape[0], keep.ctypes.data, ctypes.byref(kept)))
    assert int(keep.sum()) == kept.value
    return keep != 0


def iplist_to_vectorlist(ip):
    """iplist_to_vectorlist (src/vw/InterestPoint/InterestPoint.cc:94-102): float64 (N, 3) = x, y, 1."""
    return np.stack([ip.x.astype(np.float64), ip.y.astype(np.float64), np.ones(len(ip))], axis=1)


def _xy(p, what):
    """Points given as InterestPoints, (N, 2) or homogeneous (N, 3) with a last column of ones."""
    if isinstance(p, InterestPoints):
        p = iplist_to_vectorlist(p)
    p = np.asarray(p.cpu() if is_tensor(p) else p, np.float64)
    if p.ndim != 2 or p.shape[1] not in (2, 3):
        raise ArgumentErr("%s: points are (N, 2) or homogeneous (N, 3)" % what)
    if p.shape[1] == 3 and not np.all(p[:, 2] == 1):
        raise ArgumentErr("%s: homogeneous points must end in 1" % what)
    return np.ascontiguousarray(p[:, :2])


def _kind(kind):
    if kind in (SIMILARITY, AFFINE, HOMOGRAPHY) and not isinstance(kind, str):
        return int(kind)
    if str(kind).lower() not in KINDS:
        raise ArgumentErr("%r is not one of similarity, affine, homography" % (kind,))
    return KINDS[str(kind).lower()]


def _fit(kind, p1, p2, seed=None):
    a, b = _xy(p1, "fit"), _xy(p2, "fit")
    if a.shape != b.shape:
        raise ArgumentErr("fit: p1 and p2 are not the same size.")
    s = None if seed is None else np.ascontiguousarray(seed, np.float64).reshape(9)
    H = np.empty((3, 3), np.float64)
    _host_check(_lib.load().vwgpu_fit_transform(kind, a.ctypes.data, b.ctypes.data, a.shape[0], None if s is None else s.ctypes.data,
                                                H.ctypes.data))
    return H


def fit_similarity(p1, p2):
    """SimilarityFittingFunctor()(p1, p2) (Geometry.h:294-348): the 3 x 3 matrix that takes p1 to p2."""
    return _fit(SIMILARITY, p1, p2)


def fit_affine(p1, p2):
    """AffineFittingFunctor()(p1, p2) (Geometry.h:210-271)."""
    return _fit(AFFINE, p1, p2)


def fit_homography(p1, p2, seed=None):
    """HomographyFittingFunctor()(p1, p2[, seed]) (Geometry.h:116-191)."""
    return _fit(HOMOGRAPHY, p1, p2, seed)


def ransac_samples(n, m, iterations, seed=0):
    """int32 (iterations, m): m distinct indices below n per row, drawn from numpy's RandomState(seed).  The reference
    draws with an unseeded rand() (RANSAC.h:139-155)."""
    n, m, iterations = int(n), int(m), int(iterations)
    if m < 1 or n < m or iterations < 1:
        raise ArgumentErr("Not enough samples (%d / %d)" % (m, n))
    rng = np.random.RandomState(seed)
    if n <= 4096:
        return np.ascontiguousarray(np.argsort(rng.random_sample((iterations, n)), axis=1)[:, :m], np.int32)
    out = np.empty((iterations, m), np.int32)
    for it in range(iterations):
        out[it] = rng.choice(n, m, replace=False)
    return out


def ransac(kind, p1, p2, iterations, inlier_threshold, min_inliers, reduce=False, samples=None, seed=0):
    """RandomSampleConsensus<kind's functor, InterestPointErrorMetric>(.., iterations, inlier_threshold, min_inliers,
    reduce)(p1, p2) (RANSAC.h:212-330).  Returns (H, inlier mask): the 3 x 3 matrix that takes p1 to p2 and
    inlier_indices(H, p1, p2) as a boolean array.  samples: the int32 (iterations, m) table of rows to fit
    (ransac_samples(n, m, iterations, seed) by default).  Raises LogicErr where the reference throws RANSACErr."""
    k = _kind(kind)
    a, b = _xy(p1, "ransac"), _xy(p2, "ransac")
    if a.shape != b.shape:
        raise ArgumentErr("RANSAC Error.  Data vectors are not the same size.")
    m = 4 if k == HOMOGRAPHY else 3
    if samples is None:
        samples = ransac_samples(a.shape[0], m, iterations, seed)
    s = np.ascontiguousarray(samples, np.int32)
    if s.shape != (int(iterations), m):
        raise ArgumentErr("ransac: the sample table must be (%d, %d)" % (int(iterations), m))
    H = np.empty((3, 3), np.float64)
    flags = np.zeros(a.shape[0], np.uint8)
    count = ctypes.c_longlong(0)
    _host_check(_lib.load().vwgpu_ransac(k, a.ctypes.data, b.ctypes.data, a.shape[0], s.ctypes.data, int(iterations), float(inlier_threshold),
                                         int(min_inliers), int(bool(reduce)), H.ctypes.data, flags.ctypes.data, ctypes.byref(count)))
    return H, flags != 0


# ---- files (src/vw/InterestPoint/MatcherIO.cc:248-345, :350-445) -------------------------------------------------------------

def _records(ip):
    d = ip.descriptor
    d = np.ascontiguousarray(d.cpu().numpy() if is_tensor(d) else d, "<f4")
    out = []
    polarity = np.zeros(len(ip), np.uint8) if ip.polarity is None else ip.polarity
    for i in range(len(ip)):
        out.append(_HEAD.pack(ip.x[i], ip.y[i], ip.ix[i], ip.iy[i], ip.orientation[i], ip.scale[i], ip.interest[i], polarity[i],
                              ip.octave[i], ip.scale_lvl[i], d.shape[1]))
        out.append(d[i].tobytes())
    return b"".join(out)


def _read_records(buf, pos, n, name):
    cols = [[] for _ in range(10)]
    desc = []
    for _ in range(n):
        if pos + _HEAD.size > len(buf):
            raise IOErr("Failed to read interest point from file %s." % name)
        head = _HEAD.unpack_from(buf, pos)
        pos += _HEAD.size
        size = head[10]
        if pos + 4 * size > len(buf):
            raise IOErr("Failed to read interest point from file %s." % name)
        desc.append(np.frombuffer(buf, "<f4", size, pos))
        pos += 4 * size
        for c, v in zip(cols, head):
            c.append(v)
    k = desc[0].size if desc else 0
    if any(d.size != k for d in desc):
        raise IOErr("%s: the descriptors differ in length" % name)
    d = np.stack(desc).astype(np.float32) if desc else np.zeros((0, 0), np.float32)
    fields = {f[0]: np.asarray(c, f[1]) for f, c in zip(_FIELDS[2:], cols[2:])}
    return InterestPoints(np.asarray(cols[0], np.float32), np.asarray(cols[1], np.float32), d, **fields), pos


def write_binary_ip_file(ip_file, ip):
    with open(ip_file, "wb") as f:
        f.write(struct.pack("<Q", len(ip)) + _records(ip))


def read_binary_ip_file(ip_file):
    if not os.path.exists(ip_file):
        raise IOErr('Failed to open "%s" as VWIP file.' % ip_file)
    buf = open(ip_file, "rb").read()
    n = struct.unpack_from("<Q", buf, 0)[0] if len(buf) >= 8 else 0
    return _read_records(buf, 8, n, ip_file)[0]


def write_binary_match_file(match_file, ip1, ip2):
    if len(ip1) != len(ip2):
        raise IOErr("The vectors of matching interest points must have the same size.")
    with open(match_file, "wb") as f:
        f.write(struct.pack("<QQ", len(ip1), len(ip2)) + _records(ip1) + _records(ip2))


def read_binary_match_file(match_file):
    """(ip1, ip2); two empty lists where the file does not exist, as the reference allows."""
    empty = InterestPoints([], [], np.zeros((0, 0), np.float32))
    if not os.path.exists(match_file):
        return empty, empty
    buf = open(match_file, "rb").read()
    if len(buf) < 16:
        return empty, empty
    n1, n2 = struct.unpack_from("<QQ", buf, 0)
    if n1 != n2:
        raise IOErr("The vectors of matching interest points must have the same size.")
    ip1, pos = _read_records(buf, 16, n1, match_file)
    ip2, pos = _read_records(buf, pos, n2, match_file)
    return ip1, ip2


def align_homography(matches, iterations=100, inlier_threshold=30, min_inliers=None, samples=None, seed=0):
    """The alignment step of tools/correlate.cc:147-166: `matches` is the name of a binary .match file or a pair
    (matched_ip1, matched_ip2); RANSAC with a homography, 100 iterations, threshold 30, at least half of the pairs as
    inliers, reducing that count when there is no fit, maps the points of list 2 onto those of list 1.  Returns the
    transform.HomographyTransform(alignment) with which transform.transform(right, ..) aligns the right image."""
    ip1, ip2 = read_binary_match_file(matches) if isinstance(matches, str) else matches
    p1, p2 = _xy(ip1, "align_homography"), _xy(ip2, "align_homography")
    if min_inliers is None:
        min_inliers = p1.shape[0] // 2
    H, _ = ransac(HOMOGRAPHY, p2, p1, iterations, inlier_threshold, min_inliers, reduce=True, samples=samples, seed=seed)
    return HomographyTransform(H)


# ---- detection and description (src/vw/InterestPoint/IntegralDetector.h, DetectorBase.h, Descriptor.h, tools/ipfind.cc) --------

DETECTORS = {"iagd": 0, "obalog": 1}
DESCRIPTORS = {"sgrad": 0, "sgrad2": 1}
IP_DEFAULT_SCALES = 8
MAX_SCALES = 8
TILE_SIZE = 1024
IDEAL_OBALOG_THRESHOLD = np.float32(.07)      # tools/ipfind.cc:71


def _image2d(ops, image, what):
    img = ops.image(image, np.float32, rows=True)
    if img.ndim != 2 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ArgumentErr("%s: a float32 image (rows, cols) with at least one pixel" % what)
    return img


def integral_image(image, ctx=None):
    """IntegralImage(image) (IntegralImage.h:43-91): float32 (rows + 1, cols + 1), row 0 and column 0 zero, every word
    ((src + left) + up) - upleft in float, in that order, which is not what a cumulative sum gives."""
    ops = Operands("integral_image", image, ctx)
    img = _image2d(ops, image, "integral_image")
    h, w = int(img.shape[0]), int(img.shape[1])
    out = ops.empty((h + 1, w + 1), np.float32)
    ops.call("integral_image", ops.ptr(img), w, h, ops.row_stride(img), ops.ptr(out), w + 1)
    return out


def assign_orientation(integral, ix, iy, scale, ctx=None):
    """AssignOrientation (IntegralDetector.cc:37-104) for points {ix, iy, scale} of an integral image (integral_image(image), or a
    view of a wider one): float32 orientations, on the side of `integral`."""
    ops = Operands("assign_orientation", integral, ctx)
    integ = ops.image(integral, np.float32, rows=True)
    if integ.ndim != 2 or integ.shape[0] < 2 or integ.shape[1] < 2:
        raise ArgumentErr("assign_orientation: an integral image of at least 2 x 2")
    px, py = np.ascontiguousarray(ix, np.int32).reshape(-1), np.ascontiguousarray(iy, np.int32).reshape(-1)
    ps = np.ascontiguousarray(scale, np.float32).reshape(-1)
    if not px.size == py.size == ps.size:
        raise ArgumentErr("assign_orientation: ix, iy and scale must have one length")
    out = ops.zeros((px.size,), np.float32)
    if px.size == 0:
        return out
    side = [_side(ops, v) for v in (px, py, ps)]      # kept alive over the call: a tensor freed at once hands its block to the next one
    ops.call("ip_orientation", ops.ptr(integ), int(integ.shape[1]), int(integ.shape[0]), ops.row_stride(integ), px.size, ops.ptr(side[0]),
             ops.ptr(side[1]), ops.ptr(side[2]), ops.ptr(out))
    return out


class OBALoGInterestOperator(object):
    """OBALoGInterestOperator(threshold = 0.05) (IntegralInterestOperator.h:67-159)."""

    def __init__(self, threshold=0.05):
        self.threshold = float(threshold)


def detection_tiles(width, height, desired_num_ip=0, tile_size=TILE_SIZE):
    """The tiles of detect_interest_points: subdivide_bbox of the image at tile_size (AlgorithmFunctions.cc:28-80) as rows
    (x, y, w, h), and the number of points asked of each (DetectorBase.h:276-290): 0 when desired_num_ip is not positive,
    else ceil(area / tile_size^2 * desired_num_ip) kept within [1, desired_num_ip]."""
    width, height, n = int(width), int(height), int(desired_num_ip)
    rects, counts = [], []
    for y in range(0, height, tile_size):
        for x in range(0, width, tile_size):
            w, h = min(tile_size, width - x), min(tile_size, height - y)
            rects.append((x, y, w, h))
            num = 0
            if n > 0:
                num = int(np.ceil(float(w * h) / float(tile_size * tile_size) * float(n)))
                num = min(max(num, 1), n)
            counts.append(num)
    return rects, counts


def cull_order(detector, interest, limit):
    """The indices that the detector's cull keeps of candidates given in natural order (scale, row, column), in output
    order (IntegralDetector.cc:227-237, :354-367): OBALoG sorts by interest descending whenever limit > 0, IAGD only when
    0 < limit < count; the sort is stable; then the list is cut at limit."""
    v = np.ascontiguousarray(interest, np.float32).reshape(-1)
    order = np.empty(v.size, np.int32)
    n = ctypes.c_int(0)
    _host_check(_lib.load().vwgpu_ip_cull_order(_code(DETECTORS, detector, "detector"), int(limit), v.size, v.ctypes.data, order.ctypes.data,
                                                ctypes.byref(n)))
    return order[:n.value].copy()


class _IntegralDetector(object):
    kind = None

    def _run(self, image, rects, desired, ctx=None, stats=None, capacity=None):
        """One vwgpu_ip_detect call over `rects`; the call is repeated with the capacity its counts ask for when a tile
        has more points than the first guess.  capacity: the segment size to use, without a second call: CapacityErr is
        raised when it is too small, with stats filled."""
        ops = Operands("detect", image, ctx)
        img = _image2d(ops, image, "detect")
        if not 1 <= self.scales <= MAX_SCALES:
            raise (NoImplErr if self.scales > MAX_SCALES else ArgumentErr)(
                "detect: %d scales; 1 .. %d are implemented (the reference's rows 8 and 9 are placeholders)" % (self.scales, MAX_SCALES))
        n = len(rects)
        tiles = np.ascontiguousarray(rects, np.int32).reshape(n, 4)
        want = np.ascontiguousarray(desired, np.int32).reshape(n)
        limits = np.where(want > 0, want, self.max_points)
        fixed = capacity is not None
        if not fixed:
            capacity = int(limits.max()) if int(limits.min()) > 0 else 4096
        params = _lib.IpDetectParams(self.kind, int(self.scales), float(self.threshold), int(self.max_points), 0)
        st = (ctypes.c_int * (3 * n))()
        while True:
            out = {name: ops.empty((n, capacity), dtype) for name, dtype in _FIELDS[:7]}
            pts = _lib.IpPoints(*[ops.ptr(out[name]) for name in ("x", "y", "ix", "iy", "orientation", "scale", "interest")])
            try:
                ops.call("ip_detect", ops.ptr(img), int(img.shape[1]), int(img.shape[0]), ops.row_stride(img), tiles.ctypes.data, n,
                         ctypes.byref(params), want.ctypes.data, capacity, ctypes.byref(pts), st)
                break
            except CapacityErr:
                if fixed:
                    if stats is not None:
                        stats[:] = np.asarray(st, np.int32).reshape(n, 3).tolist()
                    raise
                capacity = max(st[2::3])
        counts = np.asarray(st, np.int32).reshape(n, 3)
        if stats is not None:
            stats[:] = counts.tolist()
        fields = {}
        for name, _ in _FIELDS[:7]:
            a = out[name].cpu().numpy() if ops.tensor else out[name]
            fields[name] = np.concatenate([a[i, :counts[i, 2]] for i in range(n)]) if n else a.reshape(-1)
        total = int(counts[:, 2].sum())
        x, y = fields.pop("x"), fields.pop("y")
        return InterestPoints(x, y, ops.zeros((total, 0), np.float32), **fields)

    def process_image(self, image, desired_num_ip=0, ctx=None, stats=None, capacity=None):
        """process_image(image, desired_num_ip) (IntegralDetector.cc:150-245, :264-370): the image as one tile."""
        h, w = image.shape
        return self._run(image, [(0, 0, int(w), int(h))], [int(desired_num_ip)], ctx, stats, capacity)


class IntegralInterestPointDetector(_IntegralDetector):
    """IntegralInterestPointDetector (IntegralDetector.h:40-70), "obalog": OBALoG with a fixed threshold, the list sorted by
    interest whenever a limit is set, every point given the SURF-style orientation.  As in the reference a point lies one
    pixel right and down of its extremum."""
    kind = DETECTORS["obalog"]

    def __init__(self, interest=None, scales=IP_DEFAULT_SCALES, max_points=1000):
        self.interest = OBALoGInterestOperator() if interest is None else interest
        self.threshold, self.scales, self.max_points = self.interest.threshold, int(scales), int(max_points)


class IntegralAutoGainDetector(_IntegralDetector):
    """IntegralAutoGainDetector(max_points = 200, scales = 8) (IntegralDetector.h:76-97), "iagd": the threshold is 0.1 % of
    each interest plane's range; orientation stays 0."""
    kind = DETECTORS["iagd"]

    def __init__(self, max_points=200, scales=IP_DEFAULT_SCALES):
        self.threshold, self.scales, self.max_points = 0.0, int(scales), int(max_points)


def detect_interest_points(image, detector, desired_num_ip=0, ctx=None, stats=None):
    """detect_interest_points(view, detector, desired_num_ip) (DetectorBase.h:302-328): every 1024 x 1024 tile is an
    independent crop; the points are shifted by the tile's origin and appended in tile order.  All tiles go through one
    library call.  stats: an optional list that receives {extrema, passed, written} per tile."""
    h, w = image.shape
    rects, counts = detection_tiles(w, h, desired_num_ip)
    return detector._run(image, rects, counts, ctx, stats)


class SGradDescriptorGenerator(object):
    """SGradDescriptorGenerator (Descriptor.h:120-132): 180 floats from a 42 x 42 support."""
    kind, support_size, descriptor_size = DESCRIPTORS["sgrad"], 42, 180

    def __call__(self, image, ip, crop=None, ctx=None):
        """The generator run on `crop` = (x, y, w, h) of the image (the whole image by default), as operator()(image, points)
        does on the image it is given: returns ip with its descriptors set."""
        ops = Operands("describe", image, ctx)
        img = _image2d(ops, image, "describe")
        h, w = int(img.shape[0]), int(img.shape[1])
        rect = np.ascontiguousarray((0, 0, w, h) if crop is None else crop, np.int32).reshape(4)
        n = len(ip)
        desc = ops.zeros((n, self.descriptor_size), np.float32)
        side = [_side(ops, np.ascontiguousarray(v, np.float32)) for v in (ip.x, ip.y, ip.scale, ip.orientation)]
        if n:
            ops.call("ip_describe", ops.ptr(img), w, h, ops.row_stride(img), rect.ctypes.data, n, ops.ptr(side[0]), ops.ptr(side[1]),
                     ops.ptr(side[2]), ops.ptr(side[3]), self.kind, ops.ptr(desc), self.descriptor_size)
        return InterestPoints(ip.x, ip.y, desc, **{name: getattr(ip, name) for name, _ in _FIELDS[2:] if getattr(ip, name) is not None})


class SGrad2DescriptorGenerator(SGradDescriptorGenerator):
    """SGrad2DescriptorGenerator (IntegralDescriptor.h:76-179): 128 floats from the integral image of what it is given."""
    kind, support_size, descriptor_size = DESCRIPTORS["sgrad2"], 41, 128


def description_crop(ip, support_size):
    """The crop InterestPointDescriptionTask rasterises for the points of one tile (Descriptor.h:261-277): the union of
    reverse_bbox (Math/Transform.h:176-205) of every point's support square under its affine map, expanded by 1, as
    (x, y, w, h).  It may leave the image."""
    import math
    half = np.float32(support_size - 1) / np.float32(2.0)
    lo, hi = [None, None], [None, None]
    for x, y, scale, ori in zip(ip.x, ip.y, ip.scale, ip.orientation):
        scaling = np.float32(1.0) / np.float32(scale)
        c, s = math.cos(float(-np.float32(ori))), math.sin(float(-np.float32(ori)))
        sc, x, y = float(scaling), float(x), float(y)
        a, b, cc, d = sc * c, -sc * s, sc * s, sc * c
        mx, my = sc * (s * y - c * x) + float(half), -sc * (s * x + c * y) + float(half)
        det = a * d - b * cc
        ai, bi, ci, di = d / det, -b / det, -cc / det, a / det
        pts = []
        for px, py in ((0, 0), (support_size - 1, 0), (0, support_size - 1), (support_size - 1, support_size - 1)):
            qx, qy = px - mx, py - my
            pts.append((ai * qx + bi * qy, ci * qx + di * qy))
        bmin = [min(p[k] for p in pts) for k in (0, 1)]
        bmax = [max(p[k] for p in pts) for k in (0, 1)]
        for k in (0, 1):      # grow_bbox_to_int (BBox.tcc:368-389), then the union
            a0, a1 = int(math.floor(bmin[k])), int(math.floor(bmax[k])) + 1
            lo[k] = a0 if lo[k] is None else min(lo[k], a0)
            hi[k] = a1 if hi[k] is None else max(hi[k], a1)
    if lo[0] is None:
        return (0, 0, 0, 0)
    return (lo[0] - 1, lo[1] - 1, hi[0] - lo[0] + 2, hi[1] - lo[1] + 2)


def describe_interest_points(image, generator, ip, ctx=None):
    """describe_interest_points(view, descriptor, list) (Descriptor.h:324-354): the points are grouped by the 1024 x 1024 tile
    that holds them (by their truncated x, y), each group is described on its own crop (description_crop), which for SGrad2
    is part of the result.  Deviation: the reference reorders the list with std::partition; the caller's order is kept."""
    h, w = image.shape
    n = len(ip)
    tx, ty = ip.x.astype(np.int32), ip.y.astype(np.int32)      # Vector2i(ip.x, ip.y)
    if n and not ((tx >= 0) & (ty >= 0) & (tx < w) & (ty < h)).all():
        raise ArgumentErr("describe_interest_points: a point lies outside the image")
    ops = Operands("describe", image, ctx)
    desc = ops.zeros((n, generator.descriptor_size), np.float32)
    tile_id = (ty // TILE_SIZE) * ((int(w) + TILE_SIZE - 1) // TILE_SIZE) + tx // TILE_SIZE
    for t in np.unique(tile_id):
        index = np.flatnonzero(tile_id == t)
        part = ip.take(index)
        d = generator(image, part, description_crop(part, generator.support_size), ctx).descriptor
        if ops.tensor:
            import torch
            desc[torch.as_tensor(index, device=ops.device)] = d
        else:
            desc[index] = d
    return InterestPoints(ip.x, ip.y, desc, **{name: getattr(ip, name) for name, _ in _FIELDS[2:] if getattr(ip, name) is not None})


def normalized_input(image, nodata=None, ctx=None):
    """The image tools/ipfind.cc hands its detectors (:286-295): normalize(raw_image) to [0, 1], or with a nodata value
    apply_mask(normalize(create_mask(raw_image, nodata))): the range is taken over the pixels that differ from nodata, and
    those that equal it become 0.  On the side of `image`; a tensor never leaves the device."""
    from . import image as _image
    if nodata is None:
        return _image.normalize(image, ctx=ctx)
    valid = image != float(np.float32(nodata))
    out = _image.normalize(image, mask=valid, ctx=ctx)
    out[~valid] = 0
    return out


def ipfind(image, detector="iagd", descriptor="sgrad", ip_per_tile=250, gain=1, ctx=None, normalize=False, nodata=None):
    """What tools/ipfind.cc does to one float image without OpenCV (:328-339, :395-400): detect with "iagd" (the default) or
    "obalog", whose threshold is IDEAL_OBALOG_THRESHOLD / gain, ip_per_tile points per 1024 x 1024 tile, then describe with
    "sgrad" or "sgrad2".  The result goes to match() and write_binary_ip_file().  normalize=True first applies
    normalized_input(image, nodata), as the tool always does (:286-295); the default takes the image as it is."""
    if normalize:
        image = normalized_input(image, nodata, ctx)
    elif nodata is not None:
        raise ArgumentErr("ipfind: nodata is used by normalize=True only")
    if _code(DETECTORS, detector, "detector") == DETECTORS["obalog"]:
        det = IntegralInterestPointDetector(OBALoGInterestOperator(float(IDEAL_OBALOG_THRESHOLD / np.float32(gain))), max_points=ip_per_tile)
    else:
        det = IntegralAutoGainDetector(ip_per_tile)
    gen = SGrad2DescriptorGenerator() if _code(DESCRIPTORS, descriptor, "descriptor") == DESCRIPTORS["sgrad2"] else SGradDescriptorGenerator()
    return describe_interest_points(image, gen, detect_interest_points(image, det, ip_per_tile, ctx), ctx)


__all__ = ["integral_image", "assign_orientation", "OBALoGInterestOperator", "IntegralInterestPointDetector", "IntegralAutoGainDetector", "detect_interest_points",
           "detection_tiles", "cull_order", "SGradDescriptorGenerator", "SGrad2DescriptorGenerator", "description_crop",
           "describe_interest_points", "ipfind", "normalized_input",
           "InterestPoints", "match", "matched_pairs", "remove_duplicates", "remove_duplicates_mask", "NullConstraint",
           "ScaleOrientationConstraint", "PositionConstraint", "fit_similarity", "fit_affine", "fit_homography", "ransac", "ransac_samples",
           "iplist_to_vectorlist", "read_binary_ip_file", "write_binary_ip_file", "read_binary_match_file", "write_binary_match_file",
           "align_homography", "chunk_size", "HomographyTransform"]
