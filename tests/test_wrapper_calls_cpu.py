"""What every Python wrapper hands to the C library on the host side, pinned call by call (no GPU, no library needed).

Every wrapper of stereo.py and filters.py takes ctx=; the context here records (entry name, normalised arguments) for
every library call and answers 0, and its set_stream fails the test: the numpy side never touches a stream.  The record
of all cases is compared with tests/golden/wrapper_calls.json, which this module's own recorder wrote from the wrappers
as they were before they shared one operand helper (`PYTHONPATH=. python tests/test_wrapper_calls_cpu.py --write`).

Normalisation of an argument: ints, floats, None and strings as they are; an address that is the .ctypes.data of an
input the case passed in -> that input's label (the inputs are contiguous and of the right dtype, so a wrapper that
copied one would show as "fresh"); the address of a returned array -> "out" / "out[i]"; any other address -> "fresh";
a ctypes array, structure or byref object -> its type name and its contents, normalised the same way.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

from visionworkbench_amd import _lib, camera, filters, stereo
from visionworkbench_amd.core import BBox2i

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrapper_calls.json")
ADDRESS = 1 << 32     # every scalar a case passes is far below, every heap or stack address above


class Recorder(object):
    """Stands for ctx._lib (and, for the two wrappers that take no context, for _lib.load())."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, [_snapshot(a) for a in args]))
            return 0
        return entry


class FakeContext(object):
    _h = "ctx"

    def __init__(self):
        self._lib = Recorder()

    def check(self, rc):
        assert rc == 0

    def set_stream(self, stream):
        pytest.fail("a numpy call must not touch the stream")


def _snapshot(a):
    """What of an argument has to be taken at call time: ctypes objects are read now, a wrapper may reuse them."""
    if isinstance(a, (ctypes.Structure, ctypes.Array, ctypes._SimpleCData)):
        return _ctypes_value(a)
    if hasattr(a, "_obj"):    # ctypes.byref(x)
        return {"byref": _ctypes_value(a._obj)}
    return a


def _ctypes_value(c):
    if isinstance(c, ctypes.Structure):
        return {type(c).__name__: {f[0]: _ctypes_value(getattr(c, f[0])) for f in c._fields_}}
    if isinstance(c, ctypes.Array):
        return {type(c).__name__: [_ctypes_value(x) for x in c]}
    if isinstance(c, ctypes._SimpleCData):
        return {type(c).__name__: c.value}
    return c


def _normalise(a, inputs, outputs):
    if isinstance(a, dict):
        return {k: _normalise(v, inputs, outputs) for k, v in a.items()}
    if isinstance(a, (list, tuple)):
        return [_normalise(v, inputs, outputs) for v in a]
    if isinstance(a, bool) or a is None or isinstance(a, str):
        return a
    if isinstance(a, (int, np.integer)):
        a = int(a)
        if a < ADDRESS:
            return a
        for label, arr in inputs.items():
            if arr.ctypes.data == a:
                return label
        for label, arr in outputs.items():
            if arr.ctypes.data == a:
                return label
        return "fresh"
    if isinstance(a, (float, np.floating)):
        return float(a)
    raise AssertionError("an argument of type %s reached the library" % type(a).__name__)


def _describe(res):
    """Type, dtype and shape of a result (tuples and lists element by element)."""
    if isinstance(res, np.ndarray):
        return ["ndarray", str(res.dtype), list(res.shape)]
    if isinstance(res, (list, tuple)):
        return [type(res).__name__, [_describe(r) for r in res]]
    return [type(res).__name__]


def _arrays(res, label="out"):
    if isinstance(res, np.ndarray):
        return {label: res}
    out = {}
    if isinstance(res, (list, tuple)):
        for i, r in enumerate(res):
            out.update(_arrays(r, "%s[%d]" % (label, i)))
    return out


def make_inputs():
    """Left 20 x 24, right 22 x 30: rows differ from columns and the left image from the right one."""
    rng = np.random.RandomState(7)
    d3f = rng.uniform(-2, 2, (20, 24, 3)).astype(np.float32)
    d3f[..., 2] = 1
    d3i = rng.randint(-2, 3, (20, 24, 3)).astype(np.int32)
    return {
        "L": rng.rand(20, 24).astype(np.float32), "R": rng.rand(22, 30).astype(np.float32),
        "LM": np.ones((20, 24), np.uint8), "RM": np.ones((22, 30), np.uint8),
        "D3f": d3f, "D3i": d3i, "D3i_b": d3i[::-1].copy(), "D2f": d3f[..., 0].copy(),
        "L2R": d3i.copy(), "R2L": rng.randint(-2, 3, (22, 30, 3)).astype(np.int32),
        "DIFF": np.zeros((21, 25, 2), np.float32), "TEX": rng.rand(20, 24).astype(np.float32),
        "PREV": np.zeros((10, 12, 3), np.int32), "POINTS": rng.rand(20, 24, 4).astype(np.float64) + 1.0,
        "TILES": np.array([[0, 0, 10, 9], [10, 9, 14, 11]], np.int32),
        "XK": np.array([1, 2, 1], np.float32), "YK": np.array([1, 2, 3, 2, 1], np.float32),
        "K2D": np.arange(15, dtype=np.float32).reshape(3, 5),
    }


K, S = (3, 5), (3, 2)     # kernel (kx, ky), search (sx, sy)
BLOCK = (7, 9)            # divides neither 24 nor 20
H3 = [[1.0, 0.01, 2.0], [0.02, 1.0, -1.0], [0.0, 0.0, 1.0]]


def _cameras():
    # CAHV models fill their descriptor in Python; a PinholeModel would need the library
    return (camera.CAHVModel((0, 0, 0), (0, 0, 1), (100, 0, 12), (0, 100, 10)),
            camera.CAHVModel((1, 0, 0), (0, 0, 1), (100, 0, 12), (0, 100, 10)))


def _cases(x, ctx):
    """{case id: (function name, thunk)}; a thunk returns (result, stats list or None).  `x` are the labelled inputs."""
    c = {}

    def add(cid, fn, *args, **kw):
        stats = [] if kw.pop("_stats", False) else None
        if stats is not None:
            kw["stats"] = stats
        name = cid.split("/")[0]
        c[cid] = (name, lambda: (fn(*args, ctx=ctx, **kw), stats))

    whole, part = BBox2i(0, 0, 24, 20), BBox2i(2, 1, 20, 17)
    search = BBox2i.from_corners((-3, -2), (4, 3))
    add("calc_disparity/whole", stereo.calc_disparity, 0, x["L"], x["R"], whole, S, K)
    add("calc_disparity/region", stereo.calc_disparity, 2, x["L"], x["R"], part, S, K)
    add("fast_box_sum", stereo.fast_box_sum, x["L"], K)
    add("cross_corr_consistency_check/plain", stereo.cross_corr_consistency_check, x["L2R"], x["R2L"], 1.5)
    add("cross_corr_consistency_check/diff", stereo.cross_corr_consistency_check, x["L2R"], x["R2L"], 1.5,
        lr_disp_diff=x["DIFF"], ul_corner_offset=(1, 2))
    add("parabola_subpixel", stereo.parabola_subpixel, x["D3f"], x["L"], x["R"], 1, 1.5, K)
    for name in ("pyramid_subpixel", "affine_subpixel", "lk_subpixel", "bayes_em_subpixel", "phase_subpixel"):
        fn = getattr(stereo, name)
        add(name + "/plain", fn, x["D3f"], x["L"], x["R"], 1, 1.5, K)
        add(name + "/blocks_stats", fn, x["D3f"], x["L"], x["R"], 2, 1.25, K, max_pyramid_levels=3, block_size=BLOCK, _stats=True)
    add("pyramid_subpixel/lk", stereo.pyramid_subpixel, x["D3f"], x["L"], x["R"], 1, 1.5, K, algorithm=stereo.SUBPIXEL_LUCAS_KANADE)
    add("phase_subpixel/accuracy", stereo.phase_subpixel, x["D3f"], x["L"], x["R"], 1, 1.5, K, phase_subpixel_accuracy=10)
    add("corr_eval/plain", stereo.corr_eval, x["L"], x["R"], x["D3f"], K, "ncc")
    add("corr_eval/all", stereo.corr_eval, x["L"], x["R"], x["D3f"], K, "cramer_rao", sample_rate=2, round_to_int=True,
        prefilter_mode=2, prefilter_kernel_width=1.25, left_valid=x["LM"], right_valid=x["RM"], block_size=BLOCK, _stats=True)
    add("rm_outliers_using_thresh", stereo.rm_outliers_using_thresh, x["D3i"], 2, 3, 1.5, 0.5)
    add("disparity_cleanup_using_thresh", stereo.disparity_cleanup_using_thresh, x["D3i"], 2, 3, 1.5, 0.5)
    add("disparity_mask", stereo.disparity_mask, x["D3i"], x["LM"], x["RM"])
    add("disparity_blob_filter", stereo.disparity_blob_filter, x["D3i"], 7)
    c["subdivide_regions"] = ("subdivide_regions", lambda: (stereo.subdivide_regions(x["D3i"], K), None))

    pyr = dict(corr_timeout=3, seconds_per_op=0.5, consistency_threshold=2.0, min_consistency_level=1, filter_half_kernel=4,
               max_pyramid_levels=2, algorithm=1, collar_size=6, sgm_subpixel_mode=3, sgm_search_buffer=(5, 7),
               memory_limit_mb=123, blob_filter_area=9, sgm_num_threads=2)
    add("pyramid_correlate/plain", stereo.pyramid_correlate, x["L"], x["R"], None, None, 1, 1.5, search, K, 2)
    add("pyramid_correlate/all", stereo.pyramid_correlate, x["L"], x["R"], x["LM"], x["RM"], 2, 1.25, search, K, 1,
        bbox=BBox2i(2, 1, 15, 13), lr_disp_diff=x["DIFF"], region_ul=(1, 2), **pyr)
    boxes = [BBox2i(0, 0, 13, 11), BBox2i(13, 11, 11, 9)]
    add("pyramid_correlate_batch/plain", stereo.pyramid_correlate_batch, x["L"], x["R"], None, None, 1, 1.5, search, K, 2, boxes)
    add("pyramid_correlate_batch/all", stereo.pyramid_correlate_batch, x["L"], x["R"], x["LM"], x["RM"], 2, 1.25, search, K, 1,
        boxes, **pyr)
    add("calc_disparity_sgm/plain", stereo.calc_disparity_sgm, 3, x["L"], x["R"], whole, S, (3, 3))
    add("calc_disparity_sgm/all", stereo.calc_disparity_sgm, 4, x["L"], x["R"], part, S, (5, 5), use_mgm=True, subpixel_mode=2,
        search_buffer=(3, 4), memory_limit_mb=77, left_mask=x["LM"], right_mask=x["RM"], prev_disparity=x["PREV"], p1=11, p2=22,
        ternary_census_threshold=6, num_threads=3, with_subpixel=True, allow_block_cost=True)

    add("disparity_median_filter/plain", stereo.disparity_median_filter, x["D3f"], 5)
    add("disparity_median_filter/blocks_stats", stereo.disparity_median_filter, x["D3f"], 3, semantics="snapshot",
        block_size=BLOCK, _stats=True)
    add("disparity_median_filter/tiles", stereo.disparity_median_filter, x["D3f"], 3, tiles=x["TILES"])
    add("disparity_neighbor_filter/plain", stereo.disparity_neighbor_filter, x["D3i"])
    add("disparity_neighbor_filter/tiles_stats", stereo.disparity_neighbor_filter, x["D3i"], semantics="snapshot",
        tiles=x["TILES"], _stats=True)
    add("texture_preserving_disparity_filter/plain", stereo.texture_preserving_disparity_filter, x["D3f"], x["TEX"])
    add("texture_preserving_disparity_filter/all", stereo.texture_preserving_disparity_filter, x["D3f"], x["TEX"], 0.25, 7,
        semantics="snapshot", block_size=BLOCK, _stats=True)
    add("texture_measure/plain", stereo.texture_measure, x["L"])
    add("texture_measure/all", stereo.texture_measure, x["L"], 5, 0.25, 0.75, tiles=x["TILES"], _stats=True)
    for name in ("rm_outliers_using_mean", "disparity_cleanup_using_mean"):
        add(name + "/int32", getattr(stereo, name), x["D3i"], 2, 3, 1.5)
        add(name + "/float32_skip_stats", getattr(stereo, name), x["D3f"], 3, 2, 2.5, semantics="skip", _stats=True)
    for name in ("rm_outliers_using_stddev", "disparity_cleanup_using_stddev", "rm_outliers_using_plane",
                 "disparity_clean_using_plane"):
        add(name + "/int32", getattr(stereo, name), x["D3i"], 2, 3, 1.5, 0.5)
        add(name + "/float32_stats", getattr(stereo, name), x["D3f"], 3, 2, 2.5, 0.25, _stats=True)
    add("std_dev_image/zero", stereo.std_dev_image, x["L"], 3, 5)
    add("std_dev_image/constant", stereo.std_dev_image, x["L"], 5, 3, edge="constant")

    add("get_disparity_range/float32", stereo.get_disparity_range, x["D3f"])
    add("get_disparity_range/int32", stereo.get_disparity_range, x["D3i"])
    add("disparity_range_mask/plain", stereo.disparity_range_mask, x["D3i"], (1, 2), (20, 18))
    add("disparity_range_mask/all", stereo.disparity_range_mask, x["D3f"], (1.5, 2.5), (20, 18), semantics="fixed", x0=3, y0=4,
        _stats=True)
    add("transform_disparities/matrix", stereo.transform_disparities, x["D3f"], H3)
    add("transform_disparities/homography", stereo.transform_disparities, x["D3i"], stereo.HomographyTransform(H3), x0=1, y0=2)
    add("transform_disparities_subregion/round", stereo.transform_disparities_subregion, True, BBox2i(3, 4, 24, 20), H3, x["D3f"])
    add("transform_disparities_subregion/exact", stereo.transform_disparities_subregion, False, BBox2i(3, 4, 24, 20), H3, x["D3i"])
    for name in ("disparity_subsample", "disparity_upsample", "missing_pixel_image"):
        add(name + "/float32", getattr(stereo, name), x["D3f"])
        add(name + "/int32", getattr(stereo, name), x["D3i"])
    add("intersect_mask_and_data", stereo.intersect_mask_and_data, x["D3i"], x["D3i_b"])
    add("disparity_transform_image", stereo.disparity_transform_image, x["R"], x["D3f"])

    c1, c2 = _cameras()
    model = stereo.StereoModel(c1, c2, 0.01)
    add("stereo_triangulate/plain", stereo.stereo_triangulate, x["D3f"], c1, c2)
    add("stereo_triangulate/all", stereo.stereo_triangulate, x["D3i"], c1, c2, x0=1, y0=2, error=True, error_vector=True,
        angle_tol=0.02, _stats=True)
    add("stereo_triangulate/scalar", stereo.stereo_triangulate, x["D2f"], c1, c2, error=True)
    add("StereoModel/plain", model, x["D3f"])
    add("StereoModel/all", model, x["D3i"], x0=1, y0=2, layout="dxdyv", _stats=True)
    add("StereoModel/convergence_angle", model.convergence_angle, x["D3f"], x0=1, y0=2, semantics="view")
    add("universe_radius/plain", stereo.universe_radius, x["POINTS"], (1, 2, 3))
    add("universe_radius/all", stereo.universe_radius, x["POINTS"], (1, 2, 3), 0.5, 100.0, _stats=True)
    add("universe_radius/in_place", stereo.universe_radius, x["POINTS"], (1, 2, 3), 0.5, 100.0, out=x["POINTS"])

    c["generate_gaussian_kernel"] = ("generate_gaussian_kernel", lambda: (filters.generate_gaussian_kernel(1.5, 5), None))
    add("separable_convolution_filter/plain", filters.separable_convolution_filter, x["L"], x["XK"], x["YK"])
    add("separable_convolution_filter/all", filters.separable_convolution_filter, x["L"], x["XK"], x["YK"], cx=0, cy=4,
        edge=filters.ZeroEdgeExtension, subsample=2)
    add("gaussian_filter", filters.gaussian_filter, x["L"], 1.5, 2.5, 5, 7, edge=filters.ZeroEdgeExtension)
    add("convolution_filter/plain", filters.convolution_filter, x["L"], x["K2D"])
    add("convolution_filter/all", filters.convolution_filter, x["L"], x["K2D"], 0, 2, filters.ZeroEdgeExtension)
    add("laplacian_filter", filters.laplacian_filter, x["L"], edge=filters.ZeroEdgeExtension)
    add("subsample_mask_by_two", filters.subsample_mask_by_two, x["LM"])
    add("prefilter_image", filters.prefilter_image, x["L"], 2, 1.5)
    add("build_gaussian_pyramid", filters.build_gaussian_pyramid, x["L"], 2)
    return c


VALUE_TYPES = {"BBox2i", "CostFunctionType", "HomographyTransform"}     # arguments of the cases, not wrappers
UNLISTED = {"fast_box_sum"}                                             # public, but not in stereo.__all__
FILTER_WRAPPERS = {"generate_gaussian_kernel", "separable_convolution_filter", "gaussian_filter", "convolution_filter",
                   "laplacian_filter", "subsample_mask_by_two", "prefilter_image", "build_gaussian_pyramid"}


def record_all():
    """Runs every case on fresh inputs and returns {case id: {"calls", "result", "stats"}}, ready for json."""
    saved = _lib.load
    record = {}
    try:
        for cid in sorted(_cases(make_inputs(), FakeContext())):
            inputs, ctx = make_inputs(), FakeContext()
            _lib.load = lambda ctx=ctx: ctx._lib     # subdivide_regions and generate_gaussian_kernel take no context
            res, stats = _cases(inputs, ctx)[cid][1]()
            outputs = _arrays(res)
            record[cid] = {"calls": [[name, _normalise(args, inputs, outputs)] for name, args in ctx._lib.calls],
                           "result": _describe(res), "stats": stats}
    finally:
        _lib.load = saved
    return json.loads(json.dumps(record))


@pytest.fixture(scope="module")
def recorded():
    return record_all()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_public_wrapper_has_a_case():
    names = {name for name, _ in _cases(make_inputs(), FakeContext()).values()}
    assert names == (set(stereo.__all__) - VALUE_TYPES) | UNLISTED | FILTER_WRAPPERS
    for name in FILTER_WRAPPERS:
        assert callable(getattr(filters, name))


def test_the_same_cases_as_the_golden_file(recorded, golden):
    assert sorted(recorded) == sorted(golden)


@pytest.mark.parametrize("cid", sorted(_cases(make_inputs(), FakeContext())))
def test_calls_and_results(recorded, golden, cid):
    got, want = recorded[cid], golden[cid]
    assert got["result"] == want["result"]     # type, dtype and shape
    assert got["stats"] == want["stats"]
    assert [c[0] for c in got["calls"]] == [c[0] for c in want["calls"]]
    for (name, a), (_, b) in zip(got["calls"], want["calls"]):
        assert len(a) == len(b), name
        for i, (p, q) in enumerate(zip(a, b)):
            assert p == q, "%s: argument %d" % (name, i)


def test_in_place_wrappers_return_their_operand():
    x, ctx = make_inputs(), FakeContext()
    assert stereo.cross_corr_consistency_check(x["L2R"], x["R2L"], 1.5, ctx=ctx) is x["L2R"]
    assert stereo.cross_corr_consistency_check(x["L2R"], x["R2L"], 1.5, lr_disp_diff=x["DIFF"], ctx=ctx) is x["L2R"]
    assert stereo.universe_radius(x["POINTS"], (0, 0, 0), out=x["POINTS"], ctx=ctx) is x["POINTS"]


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        with open(GOLDEN, "w") as f:
            json.dump(record_all(), f, indent=0, sort_keys=True)
            f.write("\n")
    else:
        sys.exit("usage: PYTHONPATH=. python tests/test_wrapper_calls_cpu.py --write   (rewrites %s)" % GOLDEN)
