"""ip_view.cc: the C++ surface of vw::ip matching and the RANSAC alignment (vwlite vw/InterestPoint.h) on libvwgpu.so.  The
program reads files this side wrote, matches two lists with DefaultMatcher and InterestPointMatcherSimple, compares the
indices with the restatement's, and runs the match-file-to-HomographyTransform lines of tools/correlate.cc."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import ip_match_ref as ref  # noqa: E402

from visionworkbench_amd import interest_point as ipm  # noqa: E402
from visionworkbench_amd import transform as tf  # noqa: E402

pytestmark = pytest.mark.gpu


def test_cpp_surface(tmp_path):
    exe = ref.build_view_program()
    rng = np.random.RandomState(21)
    # two lists for the matchers: some true partners with small noise, polarity mixed; ix is the row number
    n1, n2, k = 70, ipm.chunk_size(1) + 9, 16
    d1 = rng.random_sample((n1, k)).astype(np.float32)
    d2 = rng.random_sample((n2, k)).astype(np.float32)
    d2[rng.permutation(n2)[:40]] = d1[:40] + 0.01 * rng.standard_normal((40, k)).astype(np.float32)
    pol1, pol2 = rng.randint(0, 2, n1).astype(np.uint8), rng.randint(0, 2, n2).astype(np.uint8)
    ip1 = ipm.InterestPoints(rng.uniform(0, 99, n1), rng.uniform(0, 99, n1), d1, ix=np.arange(n1), polarity=pol1)
    ip2 = ipm.InterestPoints(rng.uniform(0, 99, n2), rng.uniform(0, 99, n2), d2, ix=np.arange(n2), polarity=pol2)
    ipm.write_binary_ip_file(str(tmp_path / "one.vwip"), ip1)
    ipm.write_binary_ip_file(str(tmp_path / "two.vwip"), ip2)
    knn = ref.match(d1, d2, 0.5, mode=ref.KNN)[0]
    simple = ref.match(d1, d2, 0.5, mode=ref.SIMPLE, pol1=pol1, pol2=pol2)[0]
    assert (knn >= 0).sum() >= 30 and (simple >= 0).sum() >= 10 and not np.array_equal(knn, simple)
    np.concatenate([[n1], knn, simple]).astype(np.int32).tofile(str(tmp_path / "expected.bin"))
    # matched pairs for the alignment: positions on a quarter-pixel grid mapped by an integer scale and shift, so that the
    # file's float32 coordinates are exact; 20 of 60 pairs are outliers.  correlate.cc maps list 2 onto list 1.
    H = np.array([[2.0, 0, 10], [0, 2.0, -6], [0, 0, 1]])
    right = np.round(rng.uniform(0, 1500, (60, 2)) * 4) / 4
    left = ref.apply(H, right)
    left[40:] += np.round(rng.uniform(200, 500, (20, 2)))
    m1 = ipm.InterestPoints(left[:, 0], left[:, 1], np.zeros((60, 2), np.float32))
    m2 = ipm.InterestPoints(right[:, 0], right[:, 1], np.zeros((60, 2), np.float32))
    assert np.array_equal(m1.x.astype(np.float64), left[:, 0]) and np.array_equal(m2.y.astype(np.float64), right[:, 1])
    ipm.write_binary_match_file(str(tmp_path / "pairs.match"), m1, m2)
    img = rng.random_sample((24, 40)).astype(np.float32)
    img.tofile(str(tmp_path / "image.bin"))
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, str(tmp_path / "pairs.match"), str(tmp_path / "one.vwip"), str(tmp_path / "two.vwip"), str(tmp_path / "expected.bin"),
                          str(tmp_path / "image.bin"), "40", "24", prefix], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout
    meta = np.fromfile(prefix + ".meta", np.float64)
    got = meta[:9].reshape(3, 3)
    assert meta[9] == 60 and meta[10] == 40 and list(meta[11:]) == list(range(40))      # inlier_indices: the planted ones
    # exact inliers: every one mapped within 1e-6 px of its partner
    assert np.linalg.norm(ref.apply(got, right[:40]) - left[:40], axis=1).max() <= 1e-6
    # transform(right_disk_image, HomographyTransform(alignment)) equals the Python side's with the same matrix
    want = tf.transform(img, ipm.HomographyTransform(got), ctx=None)
    ref.same(np.fromfile(prefix + ".aligned", np.float32).reshape(24, 40), want, "aligned image")
