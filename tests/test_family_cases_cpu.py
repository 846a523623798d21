"""What keeps tests/test_fuzz_families_gpu.py from passing vacuously, without a GPU: for every generator of
tests/family_cases.py and every seed the suite uses, (a) two runs give equal cases, (b) the CPU restatement accepts every case,
(c) the stream covers what it claims (counts, with the minimum counts written here), (d) the restatements' pass over a
family takes at most 5 s."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import family_cases as fc  # noqa: E402

TIME_LIMIT = 5.0
_PASS = {}


def same_value(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and fc.differing(a, b) == 0
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def _valid(img):
    return img != 0 if img.ndim == 2 else img[..., -1] != 0


def summary(generator, c, out):
    """What the coverage asserts count, of one case and the restatement's answer to it."""
    s = dict(entry=c.get("entry"), size_class=c.get("size_class"), layout=c["layout"], base=c["base"], side_stream=c["side_stream"],
             mask_class=c.get("mask_class"))
    if generator in ("disparity_filter_cases", "outlier_filter_cases") and "disparity" in c:
        s["changed"] = fc.differing(out["out"], c["disparity"]) > 0
        s["dtype"] = c["disparity"].dtype.name
        s["semantics"] = c["semantics"]
    if generator == "disparity_map_cases":
        s["dtype"], s["semantics"], s["matrix_kind"] = c["dtype"], c.get("semantics"), c.get("matrix_kind")
        s["right_relation"] = c.get("right_relation")
    if generator == "transform_cases":
        import transform_ref
        w, h = c["out_size"]
        yy, xx = np.mgrid[c["y0"]:c["y0"] + h, c["x0"]:c["x0"] + w]
        rc, q = transform_ref.points(fc.transform_steps(c), transform_ref.REVERSE, np.stack([xx.ravel(), yy.ravel()], 1))
        assert rc == 0
        inside = (q[:, 0] >= 0) & (q[:, 0] <= c["size"][0] - 1) & (q[:, 1] >= 0) & (q[:, 1] <= c["size"][1] - 1)
        s["where"] = "all_inside" if inside.all() else "wholly_outside" if not inside.any() else "partly_outside"
        s.update(interp=c["interp"], edge=c["edge"], masked=c["mask"] is not None, steps=len(c["steps"]), out_class=c["out_class"])
    if generator == "corr_eval_cases":
        v = out["out"][..., 1] != 0
        s.update(metric=c["metric"], both=bool(v.any() and (~v).any()), big=max(c["kernel"]) > 35, right_relation=c["right_relation"])
    if generator == "hole_fill_cases":
        s["pixel_kind"], s["semantics"] = c["pixel_kind"], c.get("semantics")
        if c["entry"] == "fill_holes_grass":
            before, after = _valid(c["image"]), _valid(out["out"])
            s["fills_and_leaves"] = bool((~before & after).any() and (~after).any())
    if generator == "mosaic_cases":
        cols, rows = c["view"]
        x0, y0 = (c["total_bbox"][:2] if c["total_bbox"] else (min(o[0] for o in c["offsets"]), min(o[1] for o in c["offsets"])))
        cover = np.zeros((rows, cols), bool)
        for (x, y), (w, h) in zip(c["offsets"], c["sizes"]):
            cover[y - y0:y - y0 + h, x - x0:x - x0 + w] = True
        s.update(levels=int(out["geometry"][2]), gap=bool((~cover).any()), draft=c["draft"], channels=c["channels"], fill=c["fill_holes"],
                 count=len(c["images"]))
        assert (int(out["geometry"][0]), int(out["geometry"][1])) == (cols, rows)
    return s


def the_pass(generator):
    """One pass of the restatement over every case the suite runs of a generator: [summary, ...] and the seconds the
    restatement took."""
    if generator not in _PASS:
        n, seeds = fc.SUITE[generator]
        fc.reference(generator, fc.case_at(generator, seeds[0], 0))      # builds and loads the restatement outside the clock
        rows, seconds = [], 0.0
        for seed in seeds:
            for c in fc.GENERATORS[generator](n, seed):
                t = time.perf_counter()
                out = fc.reference(generator, c)                          # (b): raises on a refusal or an error status
                seconds += time.perf_counter() - t
                rows.append(summary(generator, c, out))
        _PASS[generator] = (rows, seconds)
    return _PASS[generator]


def count(rows, **kw):
    return sum(1 for r in rows if all(r.get(k) == v for k, v in kw.items()))


GENERATOR_NAMES = sorted(fc.GENERATORS)


def test_the_suite_runs_every_generator_with_two_seeds():
    assert sorted(fc.SUITE) == GENERATOR_NAMES
    assert all(len(set(seeds)) == 2 and n >= 60 for n, seeds in fc.SUITE.values())


@pytest.mark.parametrize("generator", GENERATOR_NAMES)
def test_deterministic_and_replayable(generator):
    n, seeds = fc.SUITE[generator]
    for seed in seeds:
        a, b = list(fc.GENERATORS[generator](n, seed)), list(fc.GENERATORS[generator](n, seed))
        assert len(a) == len(b) == n and [c["it"] for c in a] == list(range(n))
        assert all(same_value(x, y) for x, y in zip(a, b))
        for it in (0, n // 2, n - 1):                                     # a case is a function of (seed, it) alone
            assert same_value(fc.case_at(generator, seed, it), a[it])
    assert not same_value(fc.case_at(generator, seeds[0], 1), fc.case_at(generator, seeds[1], 1))


@pytest.mark.parametrize("generator", GENERATOR_NAMES)
def test_accepted_by_the_restatement_in_time(generator):
    rows, seconds = the_pass(generator)
    n, seeds = fc.SUITE[generator]
    assert len(rows) == n * len(seeds)
    print("%s: %d cases, restatement %.2f s" % (generator, len(rows), seconds))
    assert seconds <= TIME_LIMIT, "%s: the restatement took %.2f s for %d cases" % (generator, seconds, len(rows))


@pytest.mark.parametrize("generator", GENERATOR_NAMES)
def test_sizes_layouts_and_masks_occur(generator):
    rows, _ = the_pass(generator)
    if generator != "mosaic_cases":                                       # its sizes are its own (8 .. 90 a side)
        for cls in fc.SIZE_CLASSES:
            assert count(rows, size_class=cls) >= 5, cls
        for cls in fc.MASK_CLASSES:
            assert count(rows, mask_class=cls) >= 4, cls
    for base in fc.LAYOUTS[:4]:
        assert count(rows, base=base) >= 35, base
    device = [r for r in rows if r["base"].startswith("dev")]
    assert len(device) // 5 <= count(device, side_stream=True) <= len(device) // 2
    assert count([r for r in rows if not r["base"].startswith("dev")], side_stream=True) == 0


def test_disparity_filter_coverage():
    rows, _ = the_pass("disparity_filter_cases")
    for e in fc.DISPARITY_FILTER_ENTRIES:
        assert count(rows, entry=e) >= 100, e
        if e != "texture_measure":
            for sem in ("reference", "snapshot"):
                assert count(rows, entry=e, semantics=sem) >= 40, (e, sem)
    filters = [r for r in rows if "changed" in r]
    assert count(filters, changed=True) * 2 >= len(filters)


def test_outlier_filter_coverage():
    rows, _ = the_pass("outlier_filter_cases")
    for e in fc.OUTLIER_ENTRIES:
        assert count(rows, entry=e) >= 50, e
    for dtype in ("int32", "float32"):
        assert count(rows, dtype=dtype) >= 180
    for sem in ("reference", "skip"):
        assert count(rows, semantics=sem) >= 50
    filters = [r for r in rows if "changed" in r]
    assert count(filters, changed=True) * 2 >= len(filters)


def test_disparity_map_coverage():
    rows, _ = the_pass("disparity_map_cases")
    for e in fc.DISPARITY_MAP_ENTRIES:
        assert count(rows, entry=e) >= 60, e
        for dtype in ("int32", "float32") if e != "disparity_transform_image" else ("float32",):
            assert count(rows, entry=e, dtype=dtype) >= 25, (e, dtype)
    for sem in ("reference", "fixed"):
        assert count(rows, entry="disparity_range_mask", semantics=sem) >= 25
    for kind in ("translation", "affine", "projective"):
        assert count(rows, matrix_kind=kind) >= 35
    for rel in ("larger", "equal", "smaller"):
        assert count(rows, right_relation=rel) >= 15


def test_transform_coverage():
    rows, _ = the_pass("transform_cases")
    for where in ("all_inside", "partly_outside", "wholly_outside"):
        assert count(rows, where=where) >= 80, where
    for interp in fc.TRANSFORM_INTERPS:
        for edge in fc.TRANSFORM_EDGES:
            assert count(rows, interp=interp, edge=edge) >= 15, (interp, edge)
    for steps in (1, 2, 3, 4):
        assert count(rows, steps=steps) >= 60
    for masked in (False, True):
        assert count(rows, masked=masked) >= 250
    for e in ("transform", "transform_nodata"):
        assert count(rows, entry=e) >= 150
    for cls in fc.SIZE_CLASSES:
        assert count(rows, out_class=cls) >= 15


def test_corr_eval_coverage():
    rows, _ = the_pass("corr_eval_cases")
    for metric in fc.CORR_EVAL_METRICS:
        assert count(rows, metric=metric) >= 50, metric
    assert count(rows, both=True) * 2 >= len(rows)
    assert 1 <= count(rows, big=True) <= len(rows) // 10
    for rel in ("larger", "equal", "smaller"):
        assert count(rows, right_relation=rel) >= 70


def test_hole_fill_coverage():
    rows, _ = the_pass("hole_fill_cases")
    for e in fc.HOLE_FILL_ENTRIES:
        assert count(rows, entry=e) >= 50, e
    for kind in fc.PIXEL_KINDS:
        assert count(rows, pixel_kind=kind) >= 60, kind
    for sem in ("reference", "fixed"):
        for e in ("inpaint", "fill_holes_grass"):
            assert count(rows, entry=e, semantics=sem) >= 35
    assert count(rows, size_class="scan") >= 15
    assert count(rows, layout="inplace") >= 25
    fills = [r for r in rows if r["entry"] == "fill_holes_grass"]
    assert count(fills, fills_and_leaves=True) * 3 >= len(fills)


def test_mosaic_coverage():
    rows, _ = the_pass("mosaic_cases")
    for levels in (1, 2, 3, 4):
        assert count(rows, levels=levels) >= 20, levels
    assert count(rows, gap=True) >= 40
    for n in range(1, 7):
        assert count(rows, count=n) >= 20
    assert count(rows, draft=True) >= 35 and count(rows, draft=False, fill=True) >= 60 and count(rows, draft=False, fill=False) >= 60
    for channels in (1, 2, 4):
        assert count(rows, channels=channels) >= 12
