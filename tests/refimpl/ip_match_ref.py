"""ctypes binding of the CPU restatement of the interest-point matchers (ip_match_ref.cc; test infrastructure), a numpy
restatement of the three fitting functors of src/vw/Math/Geometry.h and of the RANSAC loop of src/vw/Math/RANSAC.h, and the
scenes the CPU and the GPU tests share."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
L2, HAMMING = 0, 1
SIMPLE, KNN = 0, 1
NONE, SCALE_ORIENTATION, POSITION = 0, 1, 2
SIMILARITY, AFFINE, HOMOGRAPHY = 0, 1, 2
_LIB = None


def same(got, want, what=""):
    """Exact equality of every word; NaNs by position."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), "%s: NaNs in different places" % what
        got, want = np.where(gn, 0, got), np.where(wn, 0, want)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d words differ, first at %s: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "ip_match_ref.mk"])
    return os.path.join(HERE, "libip_match_ref.so")


def lib():
    global _LIB
    if _LIB is None:
        _LIB = ctypes.CDLL(build())
        p, i, d, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_longlong
        _LIB.ipr_l2.argtypes = [p, p, i]
        _LIB.ipr_l2.restype = ctypes.c_float
        _LIB.ipr_l2_double.argtypes = [p, p, i]
        _LIB.ipr_l2_double.restype = d
        _LIB.ipr_hamming.argtypes = [p, p, i]
        _LIB.ipr_hamming.restype = ctypes.c_float
        _LIB.ipr_constraint.argtypes = [i, p, p, p]
        _LIB.ipr_match.argtypes = [i, i, p, i, ll, p, i, ll, i, p, p, p, p, d, i, p, i, p, p, p]
        _LIB.ipr_match.restype = None
        _LIB.ipr_remove_duplicates.argtypes = [p, p, ll, p]
        _LIB.ipr_remove_duplicates.restype = ll
    return _LIB


def l2(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return float(lib().ipr_l2(a.ctypes.data, b.ctypes.data, a.size))


def l2_double(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return float(lib().ipr_l2_double(a.ctypes.data, b.ctypes.data, a.size))


def hamming(a, b):
    a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
    return float(lib().ipr_hamming(a.ctypes.data, b.ctypes.data, a.size))


def constraint(kind, bounds, baseline, test):
    """ConstraintT(bounds)(baseline_ip, test_ip); a point is {x, y, scale, orientation}."""
    c = np.ascontiguousarray(bounds, np.float64)
    b, t = np.ascontiguousarray(baseline, np.float32), np.ascontiguousarray(test, np.float32)
    return bool(lib().ipr_constraint(kind, c.ctypes.data, b.ctypes.data, t.ctypes.data))


def match(desc1, desc2, threshold=0.5, metric=L2, mode=SIMPLE, pol1=None, pol2=None, attr1=None, attr2=None, ckind=NONE,
          bounds=(0, 0, 0, 0), bidirectional=False):
    """(index int32 [n1], dist float32 [n1, 2], stats [matched, queries]) of the restatement; the descriptor matrices may
    be column slices of wider ones."""
    dt = np.float32 if metric == L2 else np.uint8
    assert desc1.dtype == dt and desc2.dtype == dt and desc1.strides[1] == dt().itemsize and desc2.strides[1] == dt().itemsize
    n1, k = desc1.shape
    n2 = desc2.shape[0]
    keep = [np.ascontiguousarray(v, t) if v is not None else None for v, t in
            ((pol1, np.uint8), (pol2, np.uint8), (attr1, np.float32), (attr2, np.float32))]
    ptr = [v.ctypes.data if v is not None else None for v in keep]
    c = np.ascontiguousarray(bounds, np.float64)
    index, dist = np.full(n1, -7, np.int32), np.full((n1, 2), -7, np.float32)
    stats = (ctypes.c_longlong * 2)()
    lib().ipr_match(metric, mode, desc1.ctypes.data, n1, desc1.strides[0] // dt().itemsize, desc2.ctypes.data, n2,
                    desc2.strides[0] // dt().itemsize, k, ptr[0], ptr[1], ptr[2], ptr[3], float(threshold), ckind, c.ctypes.data,
                    int(bool(bidirectional)), index.ctypes.data, dist.ctypes.data, stats)
    return index, dist, list(stats)


def remove_duplicates(xy1, xy2):
    a, b = np.ascontiguousarray(xy1, np.float32), np.ascontiguousarray(xy2, np.float32)
    keep = np.zeros(a.shape[0], np.uint8)
    kept = lib().ipr_remove_duplicates(a.ctypes.data, b.ctypes.data, a.shape[0], keep.ctypes.data)
    assert kept == keep.sum()
    return keep != 0


# ---- the fitting functors of src/vw/Math/Geometry.h with numpy -----------------------------------------------------------

def apply(H, p):
    """proj(H (x, y, 1)) of (N, 2) points."""
    q = np.c_[np.asarray(p, np.float64), np.ones(len(p))] @ np.asarray(H, np.float64).T
    return q[:, :2] / q[:, 2:3]


def fit_similarity(p1, p2):
    """SimilarityFittingFunctorN<2> (Geometry.h:305-347), literally."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    mean1, mean2 = p1.mean(0), p2.mean(0)
    dist1 = np.linalg.norm(p1 - mean1, axis=1).sum() / len(p1)
    dist2 = np.linalg.norm(p2 - mean2, axis=1).sum() / len(p2)
    scale_factor = dist2 / dist1
    H = (p1 - mean1).T @ (p2 - mean2)
    U, S, VT = np.linalg.svd(H)
    R = VT.T @ U.T
    out = np.eye(3)
    out[:2, :2] = scale_factor * R
    out[:2, 2] = mean2 - scale_factor * R @ mean1
    return out


def fit_affine(p1, p2):
    """AffineFittingFunctorN<2> (Geometry.h:222-270): least_squares(A, y)."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    A = np.zeros((2 * len(p1), 6))
    A[0::2, 0:2], A[0::2, 2] = p1, 1
    A[1::2, 3:5], A[1::2, 5] = p1, 1
    x = np.linalg.lstsq(A, p2.reshape(-1), rcond=None)[0]
    out = np.eye(3)
    out[:2] = x.reshape(2, 3)
    return out


def _norm_similarity(p):
    t = p.mean(0)
    scale = len(p) * np.sqrt(2.) / np.linalg.norm(p - t, axis=1).sum()
    return np.array([[scale, 0, -scale * t[0]], [0, scale, -scale * t[1]], [0, 0, 1]])


def fit_homography(p1, p2, seed=None):
    """HomographyFittingFunctor (Geometry.h:116-191): four pairs by the normalised DLT (the null space from an SVD), more by
    scipy.optimize.least_squares over the first eight entries, from the seed or the DLT of the first four pairs."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    if len(p1) == 4:
        s_in, s_out = _norm_similarity(p1), _norm_similarity(p2)
        x, y = apply(s_in, p1), apply(s_out, p2)
        A = np.zeros((8, 9))
        for i in range(4):
            xi = np.array([x[i, 0], x[i, 1], 1.0])
            A[i, 3:6], A[i, 6:9] = -xi, y[i, 1] * xi
            A[i + 4, 0:3], A[i + 4, 6:9] = xi, -y[i, 0] * xi
        ns = np.linalg.svd(A)[2][-1]
        H = np.linalg.inv(s_out) @ (ns / ns[8]).reshape(3, 3) @ s_in
        return H / H[2, 2]
    from scipy.optimize import least_squares
    start = fit_homography(p1[:4], p2[:4]) if seed is None else np.asarray(seed, np.float64)

    def residual(h):
        return (p2 - apply(np.append(h, 1.0).reshape(3, 3), p1)).reshape(-1)
    res = least_squares(residual, start.reshape(9)[:8], method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return np.append(res.x, 1.0).reshape(3, 3)


FITS = {SIMILARITY: fit_similarity, AFFINE: fit_affine, HOMOGRAPHY: fit_homography}


def error(H, p1, p2):
    """HomogeneousL2NormErrorMetric<2> (RANSAC.h:77-100) of (N, 2) points."""
    q = np.c_[p1, np.ones(len(p1))] @ np.asarray(H, np.float64).T
    w = q[:, 2:3]
    q = np.where(w != 1, q / w, q)
    return np.linalg.norm(np.c_[p2, np.ones(len(p2))] - q, axis=1)


def ransac(kind, p1, p2, samples, inlier_threshold, min_inliers):
    """attempt_ransac (RANSAC.h:246-330) over a given sample table: (H, inlier mask), or None where it throws."""
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    fit = FITS[kind]
    min_err, best, num = np.finfo(np.float64).max, None, 0
    for row in samples:
        H = fit(p1[row], p2[row])
        inl = error(H, p1, p2) < inlier_threshold
        if inl.sum() < min_inliers:
            continue
        H = fit(p1[inl], p2[inl], H) if kind == HOMOGRAPHY else fit(p1[inl], p2[inl])
        err = error(H, p1[inl], p2[inl]).sum() / inl.sum()
        if err < min_err:
            min_err, best, num = err, H, int(inl.sum())
    if num < min_inliers:
        return None
    return best, error(best, p1, p2) < inlier_threshold


# ---- scenes ----------------------------------------------------------------------------------------------------------------

PLANTED = {
    SIMILARITY: np.array([[1.2 * np.cos(0.3), -1.2 * np.sin(0.3), 55.0], [1.2 * np.sin(0.3), 1.2 * np.cos(0.3), -31.0], [0, 0, 1]]),
    AFFINE: np.array([[1.1, 0.15, -40.0], [-0.07, 0.93, 25.0], [0, 0, 1]]),
    HOMOGRAPHY: np.array([[1.02, 0.03, -12.0], [-0.02, 0.98, 9.0], [2e-5, -1e-5, 1.0]]),
}


def planted(kind, sigma=0.0, seed=5, n_in=40, n_out=20):
    """(p1, p2, inlier mask): n_in pairs with coordinates in 0 .. 4096 mapped by PLANTED[kind] (plus Gaussian noise of
    sigma px), n_out outliers displaced by at least 200 px, shuffled."""
    rng = np.random.RandomState(seed + 17 * kind)
    n = n_in + n_out
    p1 = rng.uniform(0, 4096, (n, 2))
    p2 = apply(PLANTED[kind], p1)
    p2[:n_in] += sigma * rng.standard_normal((n_in, 2))
    ang = rng.uniform(0, 2 * np.pi, n_out)
    p2[n_in:] += (rng.uniform(200, 900, n_out) * np.array([np.cos(ang), np.sin(ang)])).T
    flags = np.arange(n) < n_in
    order = rng.permutation(n)
    return p1[order], p2[order], flags[order]


def sample_table(n, m, iterations, seed=11):
    rng = np.random.RandomState(seed)
    return np.ascontiguousarray(np.argsort(rng.random_sample((iterations, n)), axis=1)[:, :m], np.int32)


def uniform_scene(n1, n2, k, seed=1):
    """Two float32 descriptor matrices of uniform values in 0 .. 1: sums whose rounding depends on the order of the terms."""
    rng = np.random.RandomState(seed)
    return rng.random_sample((n1, k)).astype(np.float32), rng.random_sample((n2, k)).astype(np.float32)


def integer_scene(n1, n2, k, seed=2, top=16):
    """Integer-valued float32 descriptors: every partial sum is exact, and ties are common."""
    rng = np.random.RandomState(seed)
    return rng.randint(0, top, (n1, k)).astype(np.float32), rng.randint(0, top, (n2, k)).astype(np.float32)


def build_view_program():
    """Compiles ip_view.cc (vwlite headers + libvwgpu.so) by ip_view.mk."""
    subprocess.check_call(["make", "-s", "-C", HERE, "-f", "ip_view.mk"])
    return os.path.join(HERE, "ip_view")
