"""Interest-point detection and description on the GPU against the CPU restatement (tests/refimpl/ip_detect_ref.cc): the
integral image, the points of both detectors with every field, SGrad and SGrad2, through the device entry (torch tensors)
and the host entry (numpy), and the chain ipfind -> match -> RANSAC on a warped scene.

Tolerance of the descriptors that pass through the device's double cos / sin (orientation other than 0): measured on the
three scenes on an MI355X the largest absolute difference of an element was 0 for SGrad and for SGrad2, 4 914 and 3 494
elements (profiles/ip_detect.md): the device library's cos and sin gave the host's doubles at every orientation met.  The
bound is four times the measured maximum, so it is 0 as well; the project's ceiling for results that pass through the device's
trigonometry is 1e-5.  Everything else is equal in every word."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ip_detect_ref as ref  # noqa: E402
from ip_detect_ref import same  # noqa: E402
import ip_detect_scenes as sc  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import interest_point as ipm  # noqa: E402
from visionworkbench_amd import transform as tf  # noqa: E402
from visionworkbench_amd.core import CapacityErr, NoImplErr  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ("x", "y", "ix", "iy", "orientation", "scale", "interest")
# Four times a measured maximum of 0 is 0: the rule makes this an equality with glibc's cos / sin that DESIGN 4.22 does not promise.
# If test_descriptors_of_oriented_points fails after a change of the ROCm device library and nothing else, read it as library drift
# (measure again, the bound follows the rule) and not as a kernel bug; the words that do not pass through cos / sin stay exact.
TRIG_BOUND = min(4 * 0.0, 1e-5)


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scenes():
    return sc.scenes()


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def detector(kind, threshold=0.05, scales=8, max_points=0):
    if kind == ref.OBALOG:
        return ipm.IntegralInterestPointDetector(ipm.OBALoGInterestOperator(threshold), scales, max_points)
    return ipm.IntegralAutoGainDetector(max_points, scales)


def check_points(got, want, what):
    assert len(got) == want["x"].size, "%s: %d points, want %d" % (what, len(got), want["x"].size)
    for name in FIELDS:
        same(getattr(got, name), want[name], "%s %s" % (what, name))


# ---- integral image ----------------------------------------------------------------------------------------------------------------

# the issue's sizes, then the schedule's own edges: the 16-step chunk and the 64-row band, each less one, exactly, plus one
INTEGRAL_SIZES = [(1, 1), (1, 70), (70, 1), (63, 65), (64, 64), (130, 67), (257, 129), (15, 3), (16, 63), (17, 64), (33, 65), (48, 128), (2, 129)]


@pytest.mark.parametrize("w,h", INTEGRAL_SIZES)
def test_integral_image_every_word(ctx, w, h):
    img = np.random.RandomState(w * 1000 + h).random_sample((h, w)).astype(np.float32)
    want = ref.integral(img)
    same(ipm.integral_image(cuda(img), ctx=ctx).cpu().numpy(), want, "device %dx%d" % (w, h))
    same(ipm.integral_image(img, ctx=ctx), want, "host %dx%d" % (w, h))


def test_integral_image_1024_and_strided(ctx):
    img = np.random.RandomState(7).random_sample((1024, 1024)).astype(np.float32)
    want = ref.integral(img)
    assert (want[1:, 1:] != np.cumsum(np.cumsum(img.astype(np.float64), 0), 1).astype(np.float32)).any()
    same(ipm.integral_image(cuda(img), ctx=ctx).cpu().numpy(), want, "1024")
    view = cuda(img)[5:5 + 131, 17:17 + 200]      # rows 1024 apart
    assert not view.is_contiguous()
    same(ipm.integral_image(view, ctx=ctx).cpu().numpy(), ref.integral(img[5:5 + 131, 17:17 + 200]), "strided")


# ---- detection -------------------------------------------------------------------------------------------------------------------------

CONFIGS = [(ref.IAGD, 0.0), (ref.OBALOG, 0.05), (ref.OBALOG, 0.01)]


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("kind,threshold", CONFIGS)
def test_detection_every_field(ctx, scenes, which, kind, threshold):
    img = scenes[which]
    want, wstats = ref.detect(img, kind, threshold=threshold)
    assert wstats[2] > 0
    for side, image in (("device", cuda(img)), ("host", img)):
        stats = []
        got = detector(kind, threshold).process_image(image, ctx=ctx, stats=stats)
        check_points(got, want, "scene %d detector %d %s" % (which, kind, side))
        assert stats == [wstats]


@pytest.mark.parametrize("kind,threshold", CONFIGS)
def test_detection_limits(ctx, scenes, kind, threshold):
    """max_points 0, 5 and more than the count; desired_num_ip overriding max_points, also where OBALoG sorts without cutting."""
    img, dimg = scenes[1], cuda(scenes[1])
    count = ref.detect(img, kind, threshold=threshold)[1][1]
    for max_points, desired in ((0, 0), (5, 0), (count + 10, 0), (5, 9), (0, 7), (3, count + 5)):
        want, wstats = ref.detect(img, kind, threshold=threshold, max_points=max_points, desired=desired)
        stats = []
        got = detector(kind, threshold, max_points=max_points).process_image(dimg, desired, ctx=ctx, stats=stats)
        check_points(got, want, "limits %d %d" % (max_points, desired))
        assert stats == [wstats]


@pytest.mark.parametrize("scales", [3, 5, 8])
def test_detection_scales(ctx, scenes, scales):
    for kind, threshold in CONFIGS[:2]:
        want, _ = ref.detect(scenes[0], kind, scales=scales, threshold=0.01 if kind else 0.0)
        got = detector(kind, 0.01, scales=scales).process_image(cuda(scenes[0]), ctx=ctx)
        check_points(got, want, "scales %d detector %d" % (scales, kind))
    assert len(detector(ref.IAGD, scales=2).process_image(cuda(scenes[0]), ctx=ctx)) == 0
    with pytest.raises(NoImplErr):
        detector(ref.IAGD, scales=9).process_image(cuda(scenes[0]), ctx=ctx)


def test_detection_small_images(ctx):
    """40 x 40 is smaller than the largest boxes, so the upper planes are all zero; 2 x 2 has no interior pixel."""
    img = sc.scene(40, 40, 5)
    for kind, threshold in CONFIGS:
        want, wstats = ref.detect(img, kind, threshold=threshold / 5)
        stats = []
        got = detector(kind, threshold / 5).process_image(cuda(img), ctx=ctx, stats=stats)
        check_points(got, want, "40x40 detector %d" % kind)
        assert stats == [wstats]
        assert len(detector(kind).process_image(cuda(img[:2, :2].copy()), ctx=ctx)) == 0
        assert len(detector(kind).process_image(img[:1, :1].copy(), ctx=ctx)) == 0


def test_detection_tiles_in_one_call(ctx, scenes):
    """Two and five tiles in one call equal the single-tile calls and the restatement's tile loop."""
    img, dimg = scenes[2], cuda(scenes[2])
    for rects, desired in (([(0, 0, 128, 129), (128, 0, 129, 129)], [0, 20]),
                           ([(0, 0, 100, 60), (100, 0, 157, 60), (0, 60, 64, 69), (64, 60, 65, 69), (129, 60, 128, 69)], [9, 0, 4, 0, 50])):
        for kind, threshold in CONFIGS[:2]:
            det = detector(kind, 0.01, max_points=30)
            want = ref.detect_tiles(img, kind, rects, desired, threshold=0.01, max_points=30)
            got = det._run(dimg, rects, desired, ctx)
            check_points(got, want, "%d tiles detector %d" % (len(rects), kind))
            singles = [det._run(dimg, [r], [d], ctx) for r, d in zip(rects, desired)]
            for name in FIELDS:
                same(getattr(got, name), np.concatenate([getattr(s, name) for s in singles]), "tiles against single calls " + name)


def test_detect_interest_points_tile_loop(ctx):
    """An image wider than one 1024 tile: the tile loop of detect_interest_points, with the per-tile counts."""
    img = sc.scene(1100, 70, 8)
    rects, counts = ipm.detection_tiles(1100, 70, 40)
    assert len(rects) == 2 and counts == [3, 1]
    for kind in (ref.IAGD, ref.OBALOG):
        want = ref.detect_tiles(img, kind, rects, counts, threshold=0.01, max_points=1000)
        got = ipm.detect_interest_points(cuda(img), detector(kind, 0.01, max_points=1000), 40, ctx=ctx)
        check_points(got, want, "tile loop detector %d" % kind)


def test_batches_of_tiles(ctx, scenes):
    """A scratch budget of 1 MiB takes the five tiles in several batches (a tile of 157 x 60 needs 0.4 MiB): the same points
    as one batch, also through the host entry, and a capacity that a tile of the first batch exceeds still fills the stats rows of
    the later batches."""
    from visionworkbench_amd import core
    img, dimg = scenes[2], cuda(scenes[2])
    rects = [(0, 0, 100, 60), (100, 0, 157, 60), (0, 60, 64, 69), (64, 60, 65, 69), (129, 60, 128, 69)]
    desired = [9, 0, 4, 0, 50]
    c = vwa.Context(0)
    try:
        c.set_option(core.OPT_IP_SCRATCH_MB, 1)
        assert c.get_option(core.OPT_IP_SCRATCH_MB) == 1
        for kind in (ref.IAGD, ref.OBALOG):
            det = detector(kind, 0.01, max_points=30)
            want = ref.detect_tiles(img, kind, rects, desired, threshold=0.01, max_points=30)
            wstats = [ref.detect(img, kind, threshold=0.01, max_points=30, desired=d, rect=r)[1] for r, d in zip(rects, desired)]
            for image in (dimg, img):
                stats = []
                check_points(det._run(image, rects, desired, c, stats), want, "batches detector %d" % kind)
                assert stats == wstats
            stats = []
            with pytest.raises(CapacityErr):
                det._run(dimg, rects, desired, c, stats, capacity=1)
            assert stats == wstats and wstats[0][2] > 1
    finally:
        c.close()


def test_assign_orientation_entry(ctx, scenes):
    """vwgpu_ip_orientation[_dev] on integral_image() output, dense and as a view of a wider array, against the restatement and
    against the orientations the detector gave the same (ix, iy, scale)."""
    img = scenes[1]
    ip = detector(ref.OBALOG, 0.01).process_image(img, ctx=ctx)
    integ = ref.integral(img)
    want = np.array([ref.orientation(integ, x, y, s) for x, y, s in zip(ip.ix, ip.iy, ip.scale)], np.float32)
    same(want, ip.orientation, "the detector's own orientations")
    same(ipm.assign_orientation(integ, ip.ix, ip.iy, ip.scale, ctx=ctx), want, "host")
    dint = ipm.integral_image(cuda(img), ctx=ctx)
    same(ipm.assign_orientation(dint, ip.ix, ip.iy, ip.scale, ctx=ctx).cpu().numpy(), want, "device")
    import torch
    wide = torch.zeros((integ.shape[0] + 3, integ.shape[1] + 37), dtype=torch.float32, device="cuda")
    wide[2:2 + integ.shape[0], 5:5 + integ.shape[1]] = dint
    view = wide[2:2 + integ.shape[0], 5:5 + integ.shape[1]]
    assert not view.is_contiguous()
    same(ipm.assign_orientation(view, ip.ix, ip.iy, ip.scale, ctx=ctx).cpu().numpy(), want, "strided")
    assert ipm.assign_orientation(dint, [], [], [], ctx=ctx).shape == (0,)


def test_capacity_exceeded_keeps_the_stats(ctx, scenes):
    want, wstats = ref.detect(scenes[0], ref.IAGD)
    stats = []
    with pytest.raises(CapacityErr):
        detector(ref.IAGD).process_image(cuda(scenes[0]), ctx=ctx, stats=stats, capacity=wstats[2] - 1)
    assert stats == [wstats]
    got = detector(ref.IAGD).process_image(cuda(scenes[0]), ctx=ctx, capacity=wstats[2])
    check_points(got, want, "exact capacity")


# ---- description ---------------------------------------------------------------------------------------------------------------------

def reference_description(img, ip, gen):
    """describe_interest_points with the restatement's generator: the same tile groups and crops (host logic of the wrapper)."""
    out = np.zeros((len(ip), gen.descriptor_size), np.float32)
    if len(ip):
        crop = ipm.description_crop(ip, gen.support_size)      # the scenes are one tile
        out[:] = ref.describe(img, crop, ip.x, ip.y, ip.scale, ip.orientation, gen.kind)
    return out


@pytest.mark.parametrize("which", range(3))
def test_sgrad_of_unoriented_points_every_word(ctx, scenes, which):
    """IAGD points have orientation 0: cos(-0.0) = 1 and sin(-0.0) = -0.0 exactly, so nothing is left to the device library.
    The points near the border have supports that leave the image (the crop reaches outside it).  SGrad2 with orientation 0
    is the same case: every word equal, on any imagery."""
    img = scenes[which]
    ip = detector(ref.IAGD).process_image(img, ctx=ctx)
    for gen in (ipm.SGradDescriptorGenerator(), ipm.SGrad2DescriptorGenerator()):
        crop = ipm.description_crop(ip, gen.support_size)
        assert crop[0] < 0 and crop[1] < 0 and crop[0] + crop[2] > img.shape[1]
        want = reference_description(img, ip, gen)
        assert np.isfinite(want).all() and np.abs(want).sum() > 0
        same(ipm.describe_interest_points(cuda(img), gen, ip, ctx=ctx).descriptor.cpu().numpy(), want, "device")
        same(ipm.describe_interest_points(img, gen, ip, ctx=ctx).descriptor, want, "host")


def test_sgrad_flat_image_and_integer_imagery(ctx):
    """A flat image: the norm is 0, its reciprocal is not a normal number, the descriptor is all zero.  Integer-valued imagery
    with orientation 0 and scale 1.2: SGrad2 equal in every word."""
    flat = np.full((128, 128), 0.25, np.float32)      # the supports (at most 42 pixels to a side of the point) stay inside
    ip = ipm.InterestPoints([64.0, 60.0], [64.0, 70.0], np.zeros((2, 0), np.float32), scale=[1.2, 2.0])
    got = ipm.SGradDescriptorGenerator()(cuda(flat), ip, ctx=ctx).descriptor.cpu().numpy()
    same(got, ref.describe(flat, (0, 0, 128, 128), ip.x, ip.y, ip.scale, ip.orientation, ref.SGRAD), "flat")
    assert not got.any()
    img = np.random.RandomState(3).randint(0, 256, (90, 110)).astype(np.float32)
    ip = ipm.InterestPoints([30.0, 55.5, 100.0, 3.0], [31.0, 40.25, 80.0, 2.0], np.zeros((4, 0), np.float32), scale=[1.2] * 4)
    for gen in (ipm.SGrad2DescriptorGenerator(), ipm.SGradDescriptorGenerator()):
        want = ref.describe(img, (0, 0, 110, 90), ip.x, ip.y, ip.scale, ip.orientation, gen.kind)
        same(gen(cuda(img), ip, ctx=ctx).descriptor.cpu().numpy(), want, "integer imagery kind %d" % gen.kind)


def test_descriptors_of_oriented_points(ctx, scenes):
    """OBALoG points carry an orientation, so double cos / sin of the device library enter: SGrad and SGrad2 within TRIG_BOUND."""
    worst = {}
    for which, img in enumerate(scenes):
        ip = detector(ref.OBALOG, 0.01).process_image(img, ctx=ctx)
        assert len(ip) > 20 and np.count_nonzero(ip.orientation) > 20
        for gen in (ipm.SGradDescriptorGenerator(), ipm.SGrad2DescriptorGenerator()):
            want = reference_description(img, ip, gen)
            got = ipm.describe_interest_points(cuda(img), gen, ip, ctx=ctx).descriptor.cpu().numpy()
            assert got.shape == want.shape and np.isfinite(got).all()
            worst[(which, gen.kind)] = float(np.abs(got - want).max())
    print("largest |difference| of a descriptor element, (scene, kind): %r" % worst)
    assert max(worst.values()) <= TRIG_BOUND


# ---- end to end ----------------------------------------------------------------------------------------------------------------------

def test_ipfind_match_ransac_recovers_the_homography(ctx):
    """ipfind on a scene and on its copy warped by a known homography with transform(), then match, remove_duplicates, ransac:
    the recovered homography maps the scene's corners within 1 px of the planted one."""
    w, h = 320, 240
    img = sc.scene(w, h, 11)
    th = np.deg2rad(1.5)
    planted = np.array([[1.02 * np.cos(th), -1.02 * np.sin(th), 6.0], [1.02 * np.sin(th), 1.02 * np.cos(th), -4.0], [1e-5, -2e-5, 1.0]])
    warped = tf.transform(cuda(img), ipm.HomographyTransform(planted), ctx=ctx)
    per_tile = 5461      # detect_interest_points scales it by the tile's share of 1024 x 1024: 400 points for 320 x 240
    assert ipm.detection_tiles(w, h, per_tile)[1] == [400]
    ip1 = ipm.ipfind(cuda(img), ip_per_tile=per_tile, ctx=ctx)
    ip2 = ipm.ipfind(warped, ip_per_tile=per_tile, ctx=ctx)
    assert len(ip1) == 400 and len(ip2) == 400 and ip1.descriptor.shape[1] == 180
    index = ipm.match(ip1, ip2, 0.6, ctx=ctx)
    m1, m2 = ipm.remove_duplicates(*ipm.matched_pairs(ip1, ip2, index))
    assert len(m1) >= 100
    # the winner of RandomSampleConsensus is the model with the lowest mean inlier error among those with min_inliers, so
    # min_inliers is set high: the points are whole pixels, and a model carried by few of them is exact on those few only
    H, inliers = ipm.ransac("homography", ipm.iplist_to_vectorlist(m1), ipm.iplist_to_vectorlist(m2), 100, 1.5, int(0.8 * len(m1)), seed=3)
    corners = np.array([[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1]], np.float64)

    def apply(M, p):
        q = np.concatenate([p, np.ones((len(p), 1))], 1) @ M.T
        return q[:, :2] / q[:, 2:]
    err = np.linalg.norm(apply(H, corners) - apply(planted, corners), axis=1)
    print("pairs %d, inliers %d, corner errors %r" % (len(m1), int(inliers.sum()), err))
    assert err.max() < 1.0
