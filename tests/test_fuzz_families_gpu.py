"""Seeded random parity of the image and disparity kernel families under pytest -m gpu (the long-running version is
tools/fuzz_families.py): the disparity post-filters, the local outlier filters, the rest of DisparityMap.h, transform,
corr_eval, hole filling and the multi-band blend against the CPU restatements of tests/refimpl on the cases of
tests/family_cases.py.  Every word of every output must be IDENTICAL (==, validity included; two NaNs in one place are equal).

All families share ONE context on purpose: its grow-only arenas are dirty with another family's data when the next call
comes.  Operands are passed as the case's `layout` says (host, a view of a wider host array, device, a strided device view, in
place where the wrapper has out=), and the device cases with `side_stream` run uploads and call on a stream of their own.
After the call every operand that was not to be written must hold what it held, and the surroundings of every strided view
their sentinel.  A failure prints generator(seed): [(it, entry, shape, differing words), ...] for tools/replay_family_case.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import family_cases as fc  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import image, mosaic, stereo  # noqa: E402
from visionworkbench_amd import transform as tf  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 77


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    c = vwa.Context(0)
    yield c
    c.close()


# ---- operands as the case's layout says ------------------------------------------------------------------------------------------

class Placed(object):
    """The operands of one call, each with what it must hold afterwards."""

    def __init__(self, case):
        self.case, self.device, self.strided = case, case["base"].startswith("dev"), case["base"] in ("host_view", "dev_strided")
        self.held = []          # (the array or tensor that owns the memory, a host copy of what it held, columns of the view, written)
        self.pinned = []        # the host side of uploads that may still be under way

    def put(self, a, written=False):
        """`a` on the case's side and with its row stride; written: the call may write the view (never its surroundings)."""
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        cols = a.shape[1]
        if self.strided:
            big = np.full((a.shape[0], cols + self.case["pad"]) + a.shape[2:], SENTINEL, a.dtype)
            big[:, :cols] = a
        else:
            big = a.copy()
        owner = big
        if self.device:
            import torch
            if self.case["side_stream"]:        # from pinned memory: the copy is queued on the side stream, behind its delay
                self.pinned.append(torch.from_numpy(big).pin_memory())
                owner = self.pinned[-1].cuda(non_blocking=True)
            else:
                owner = torch.from_numpy(big).cuda()
        self.held.append((owner, big.copy(), cols, written))
        return owner[:, :cols] if self.strided else owner

    def untouched(self):
        """The names of what the call changed although it was not its to change."""
        bad = []
        for k, (owner, before, cols, written) in enumerate(self.held):
            now = owner.cpu().numpy() if self.device else owner
            if written:
                now, before = now[:, cols:], before[:, cols:]
            if fc.differing(now, before):
                bad.append("operand %d %s" % (k, "surroundings" if written else "changed"))
        return bad


def host(x):
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.asarray(x)


# ---- one call per family ----------------------------------------------------------------------------------------------------------------

def call_disparity_filter(ctx, c, p):
    e, st = c["entry"], []
    kw = dict(block_size=c["block_size"], tiles=c["tiles"], ctx=ctx, stats=st)
    if e == "disparity_median_filter":
        out = stereo.disparity_median_filter(p.put(c["disparity"]), c["kernel_size"], c["semantics"], **kw)
    elif e == "disparity_neighbor_filter":
        out = stereo.disparity_neighbor_filter(p.put(c["disparity"]), c["semantics"], **kw)
    elif e == "texture_measure":
        out = stereo.texture_measure(p.put(c["image"]), c["kernel_size"], c["gradient_weight"], c["stddev_weight"], **kw)
        return {"out": out, "stats": np.array(st, np.float32)}
    else:
        out = stereo.texture_preserving_disparity_filter(p.put(c["disparity"]), p.put(c["texture"]), c["texture_max"], c["max_kernel_size"],
                                                         c["semantics"], **kw)
    return {"out": out, "stats": np.array(st, np.int64)}


def call_outlier_filter(ctx, c, p):
    e, st = c["entry"], []
    if e == "std_dev_image":
        return {"out": stereo.std_dev_image(p.put(c["image"]), c["kernel"][0], c["kernel"][1], c["edge"], ctx=ctx)}
    kw = {"semantics": c["semantics"]} if e.endswith("mean") else {}
    out = getattr(stereo, e)(p.put(c["disparity"]), c["half"][0], c["half"][1], *c["args"], ctx=ctx, stats=st, **kw)
    return {"out": out, "stats": np.array(st, np.int64)}


def call_disparity_map(ctx, c, p):
    e, d = c["entry"], p.put(c["disparity"])
    if e == "get_disparity_range":
        return {"out": stereo.get_disparity_range(d, ctx=ctx, device_result=p.device and c["it"] % 2 == 1)}
    if e == "disparity_range_mask":
        st = []
        out = stereo.disparity_range_mask(d, c["min"], c["max"], c["semantics"], c["x0"], c["y0"], ctx=ctx, stats=st)
        return {"out": out, "stats": np.array(st, np.int64)}
    if e == "transform_disparities":
        return {"out": stereo.transform_disparities(d, c["matrix"], c["x0"], c["y0"], ctx=ctx)}
    if e == "transform_disparities_subregion":
        box = vwa.BBox2i(c["x0"], c["y0"], c["size"][0], c["size"][1])
        return {"out": stereo.transform_disparities_subregion(c["do_round"], box, c["matrix"], d, ctx=ctx)}
    if e == "intersect_mask_and_data":
        return {"out": stereo.intersect_mask_and_data(d, p.put(c["mask"]), ctx=ctx)}
    if e == "disparity_transform_image":
        return {"out": stereo.disparity_transform_image(p.put(c["right"]), d, ctx=ctx)}
    return {"out": getattr(stereo, e)(d, ctx=ctx)}


INTERP_TAGS = {"nearest": tf.NearestPixelInterpolation, "bilinear": tf.BilinearInterpolation, "bicubic": tf.BicubicInterpolation}
EDGE_TAGS = {"zero": tf.ZeroEdgeExtension, "constant": tf.ConstantEdgeExtension, "periodic": tf.PeriodicEdgeExtension,
             "cylindrical": tf.CylindricalEdgeExtension, "reflect": tf.ReflectEdgeExtension, "linear": tf.LinearEdgeExtension}


def call_transform(ctx, c, p):
    edge = tf.ValueEdgeExtension(*c["edge_value"]) if c["edge"] == "value" else EDGE_TAGS[c["edge"]]
    img, mask, steps = p.put(c["image"]), p.put(c["mask"]), fc.transform_steps(c)
    if c["nodata"] is None:
        got = tf.transform(img, steps, size=c["out_size"], x0=c["x0"], y0=c["y0"], edge=edge, interp=INTERP_TAGS[c["interp"]], mask=mask, ctx=ctx)
    else:
        got = tf.transform_nodata(img, steps, c["out_size"], edge, INTERP_TAGS[c["interp"]], c["nodata"][0], c["nodata"][1], mask=mask,
                                  x0=c["x0"], y0=c["y0"], ctx=ctx)
    return {"out": got} if mask is None else {"out": got[0], "mask": got[1]}


def call_corr_eval(ctx, c, p):
    st = []
    out = stereo.corr_eval(p.put(c["left"]), p.put(c["right"]), p.put(c["disparity"]), c["kernel"], c["metric"], c["sample_rate"], c["round_to_int"],
                           0, c["prefilter_width"], p.put(c["left_valid"]), p.put(c["right_valid"]), block_size=c["block_size"], ctx=ctx, stats=st)
    return {"out": out, "stats": np.array(st, np.int64)}


def call_hole_fill(ctx, c, p):
    e, inplace = c["entry"], c["layout"] == "inplace"
    img = p.put(c["image"], written=inplace)
    kw = {"out": img} if inplace else {}
    if e == "grassfire":
        return {"out": image.grassfire(img, c["ignore_borders"], ctx=ctx)}
    if e == "blob_index":
        bi = image.blob_index(img, invert=c["invert"], max_area=c["max_area"], wipe_size=c["wipe_size"], ctx=ctx)
        return {"labels": bi.labels, "table": bi.table, "count": np.array([bi.count])}
    if e == "get_blob_sizes":
        return {"out": image.get_blob_sizes(img, c["limit"], ctx=ctx)}
    if e == "erode_blobs":
        return {"out": image.erode_blobs(img, c["max_area"], ctx=ctx, **kw)}
    if e == "inpaint":
        bi = image.blob_index(img, ctx=ctx, **c["index"])
        return {"out": image.inpaint(img, bi, c["use_grassfire"], c["default"], c["semantics"], ctx=ctx, **kw), "count": np.array([bi.count])}
    if e == "fill_holes_grass":
        return {"out": image.fill_holes_grass(img, c["L"], c["semantics"], ctx=ctx, **kw)}
    return {"out": image.fill_nodata_with_avg(img, c["kernel_size"], ctx=ctx)}


def call_mosaic(ctx, c, p):
    comp = mosaic.ImageComposite(ctx)
    try:
        comp.set_draft_mode(c["draft"])
        comp.set_fill_holes(c["fill_holes"])
        for img, (x, y) in zip(c["images"], c["offsets"]):
            comp.insert(p.put(img), x, y)
        comp.prepare(c["total_bbox"])
        b, v = comp.bbox(), comp.source_data_bbox()
        out = {"geometry": np.array((comp.cols(), comp.rows(), comp.levels) + tuple(b.min) + tuple(b.max) + tuple(v.min) + tuple(v.max))}
        out["whole"] = comp.generate()
        if not c["draft"]:
            for k in range(len(c["images"])):
                out["mask%d" % k] = comp.mask(k)
        out["patch0"] = comp.generate_patch(c["patches"][0])
        x0, y0, x1, y1 = c["patches"][1]                                # the second patch into an image of the case's layout
        target = p.put(np.zeros((y1 - y0, x1 - x0, c["channels"]), np.float32), written=True)
        out["patch1"] = comp.generate_patch(c["patches"][1], out=target)
        out = {k: host_after(c, v) for k, v in out.items()}             # before the composite's memory goes
    finally:
        comp.close()
    return out


def host_after(c, v):
    if hasattr(v, "cpu") and c["side_stream"]:
        import torch
        torch.cuda.current_stream().synchronize()
    return host(v)


CALLS = {"disparity_filter_cases": call_disparity_filter, "outlier_filter_cases": call_outlier_filter,
         "disparity_map_cases": call_disparity_map, "transform_cases": call_transform, "corr_eval_cases": call_corr_eval,
         "hole_fill_cases": call_hole_fill, "mosaic_cases": call_mosaic}


_SPIN = []       # cycles of torch.cuda._sleep that take about a millisecond here, measured once


def delay_stream():
    """About a millisecond of spinning on the current stream.  Everything a side-stream case queues after it (the uploads
    included) is late, so a step of the library that lands on another stream finds operands or scratch that are not there yet."""
    import time
    import torch
    if not hasattr(torch.cuda, "_sleep"):
        x = torch.zeros(1 << 22, device="cuda")
        for _ in range(200):
            x += 1
        return
    if not _SPIN:                     # the counter's rate differs between parts
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        t = time.perf_counter()
        torch.cuda._sleep(100000)
        torch.cuda.synchronize()
        _SPIN.append(int(min(max(100000 * 1e-3 / max(time.perf_counter() - t, 1e-6), 1e4), 1e8)))
    torch.cuda._sleep(_SPIN[0])


def run_case(generator, c, ctx):
    """The case on the GPU: (name -> numpy array of every output, names of operands the call should have left alone)."""
    p = Placed(c)
    if p.device:
        import torch
        if c["side_stream"]:
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                delay_stream()
                got = CALLS[generator](ctx, c, p)
            side.synchronize()
        else:
            got = CALLS[generator](ctx, c, p)
            torch.cuda.synchronize()
    else:
        got = CALLS[generator](ctx, c, p)
    out = {}
    for k, v in got.items():
        v = host(v)
        if v.dtype == np.int32 and c.get("entry") == "get_blob_sizes":      # the device entry's words travel as int32
            v = v.view(np.uint32)
        out[k] = v
    return out, p.untouched()


def compare(generator, c, ctx):
    """None, or (it, entry, shape, {output: differing words, -1 for another shape or type}) of a case that differs."""
    want = fc.reference(generator, c)
    got, touched = run_case(generator, c, ctx)
    bad = {k: fc.differing(got[k], want[k]) if k in got else -1 for k in want}
    bad = {k: n for k, n in bad.items() if n}
    for t in touched:
        bad[t] = 1
    shape = c.get("size") or c.get("view")
    return (c["it"], c.get("entry"), shape, bad) if bad else None


def failures(generator, seed, n, ctx, start=0):
    bad = []
    for c in fc.GENERATORS[generator](n, seed, start):
        r = compare(generator, c, ctx)
        if r:
            bad.append(r)
    return bad


def check(generator, seed, ctx):
    bad = failures(generator, seed, fc.SUITE[generator][0], ctx)
    assert not bad, "%s(%d): (it, entry, shape, differing words) %s" % (generator, seed, bad)


@pytest.mark.parametrize("seed", fc.SUITE["disparity_filter_cases"][1])
def test_fuzz_disparity_filters(ctx, seed):
    """disparity_median_filter, disparity_neighbor_filter, texture_measure, texture_preserving_disparity_filter."""
    check("disparity_filter_cases", seed, ctx)


@pytest.mark.parametrize("seed", fc.SUITE["outlier_filter_cases"][1])
def test_fuzz_outlier_filters(ctx, seed):
    """rm_outliers_using_mean / _stddev / _plane, their clean-up forms and std_dev_image."""
    check("outlier_filter_cases", seed, ctx)


@pytest.mark.parametrize("seed", fc.SUITE["disparity_map_cases"][1])
def test_fuzz_disparity_map(ctx, seed):
    """The range, the range mask, the transforms, the resampling pair, the missing-pixel image, the intersection, the warp."""
    check("disparity_map_cases", seed, ctx)


@pytest.mark.parametrize("seed", fc.SUITE["transform_cases"][1])
def test_fuzz_transform(ctx, seed):
    """transform and transform_nodata: every interpolation with every edge extension over chains of one to four steps."""
    check("transform_cases", seed, ctx)


@pytest.mark.parametrize("seed", fc.SUITE["corr_eval_cases"][1])
def test_fuzz_corr_eval(ctx, seed):
    check("corr_eval_cases", seed, ctx)


@pytest.mark.parametrize("seed", fc.SUITE["hole_fill_cases"][1])
def test_fuzz_hole_fill(ctx, seed):
    """grassfire, blob_index, get_blob_sizes, erode_blobs, inpaint, fill_holes_grass, fill_nodata_with_avg."""
    check("hole_fill_cases", seed, ctx)


@pytest.mark.parametrize("seed", fc.SUITE["mosaic_cases"][1])
def test_fuzz_mosaic(ctx, seed):
    """ImageComposite: geometry, level-0 masks, the whole view and two patches, draft and blend, fill_holes on and off."""
    check("mosaic_cases", seed, ctx)
