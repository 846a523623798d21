"""Both sides of every Python wrapper on the GPU: the same small inputs once as numpy arrays (host entries) and once as
CUDA tensors (device entries) must give the same bytes, and the same stats where a wrapper reports any.

Left 40 x 48, right 44 x 60 (the left image is the right one moved by (3, 2)), kernels 3 to 7, search (4, 3), tile boxes
(13, 11) that divide neither side; SGM at 48 x 64, kernel 3, search (8, 0).

Comparisons another test already makes are not repeated here:
  the operators of DisparityMap.h (get_disparity_range, disparity_range_mask, transform_disparities[_subregion],
  disparity_subsample / _upsample, missing_pixel_image, intersect_mask_and_data, disparity_transform_image):
      test_disparity_map_gpu.py::test_device_entries
  rm_outliers_using_* / disparity_clean[up]_using_* and std_dev_image:
      test_outlier_filters_gpu.py::test_device_entries_equal_host_entries
  disparity_median_filter, disparity_neighbor_filter, texture_measure, texture_preserving_disparity_filter:
      test_disparity_filters_gpu.py::test_device_entries_equal_host_entries
  stereo_triangulate and StereoModel: test_triangulate_gpu.py::test_device_entry
  universe_radius on both sides, copying and with out=points (the same data_ptr comes back):
      test_triangulate_gpu.py::test_universe_radius
  separable_convolution_filter, prefilter_image, subsample_mask_by_two and build_gaussian_pyramid on contiguous images:
      test_filters_gpu.py (_both)
"""
import numpy as np
import pytest

import visionworkbench_amd as vwa
from visionworkbench_amd import camera, core, filters, stereo
from visionworkbench_amd._operands import Operands

pytestmark = pytest.mark.gpu

K5, SEARCH, BLOCK = (5, 5), (4, 3), (13, 11)
VALID = core.VALID_I32


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    rng = np.random.RandomState(11)
    base = np.floor(rng.rand(44, 60) * 256).astype(np.float32)
    x = {"R": base, "L": base[2:42, 3:51].copy()}
    holes = rng.rand(40, 48) < 0.1
    d3f = np.zeros((40, 48, 3), np.float32)
    d3f[..., 0], d3f[..., 1], d3f[..., 2] = 3, 2, 1
    d3f[holes] = 0
    d3i = np.zeros((40, 48, 3), np.int32)
    d3i[..., 0], d3i[..., 1], d3i[..., 2] = rng.randint(0, 4, (40, 48)), rng.randint(0, 3, (40, 48)), VALID
    d3i[holes] = 0
    r2l = np.zeros((44, 60, 3), np.int32)
    r2l[..., 0], r2l[..., 1], r2l[..., 2] = -rng.randint(0, 4, (44, 60)), -rng.randint(0, 3, (44, 60)), VALID
    r2l[rng.rand(44, 60) < 0.1] = 0
    x.update(D3f=d3f, D3i=d3i, R2L=r2l, LM=(rng.rand(40, 48) > 0.05).astype(np.uint8), RM=(rng.rand(44, 60) > 0.05).astype(np.uint8))
    sgm = np.floor(rng.rand(48, 72) * 256).astype(np.float32)
    # SGM masks have the size of the output (46 x 62 at kernel 3), the right one grown by the search; the previous
    # disparity is the output at half the size
    prev = np.zeros((23, 31, 3), np.int32)
    prev[..., 0], prev[..., 2] = 2, VALID
    prev[5:9, 8:20, 2] = 0
    x.update(SR=sgm, SL=sgm[:, 4:68].copy(), SLM=(rng.rand(46, 62) > 0.05).astype(np.uint8) * 255,
             SRM=(rng.rand(46, 70) > 0.05).astype(np.uint8) * 255, PREV=prev)
    return x


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(a).cuda()


def host(t):
    return t.cpu().numpy()


def same(got_dev, got_host, what=""):
    """Bit for bit, with the type, dtype and shape of the host result."""
    if isinstance(got_host, (list, tuple)):
        assert type(got_dev) is type(got_host) and len(got_dev) == len(got_host), what
        for i, (a, b) in enumerate(zip(got_dev, got_host)):
            same(a, b, "%s[%d]" % (what, i))
        return
    assert got_dev.is_cuda, what
    a = host(got_dev)
    assert a.dtype == got_host.dtype and a.shape == got_host.shape, what
    assert a.tobytes() == got_host.tobytes(), what


def both(fn, arrays, *args, **kw):
    """fn(*arrays, *args, **kw) with the arrays as numpy arrays and as CUDA tensors; stats=True adds a stats list to each
    call and compares the two."""
    import torch
    want_stats = kw.pop("stats", False)
    sh, sd = ([], []) if want_stats else (None, None)
    on_host = fn(*arrays, *args, **(dict(kw, stats=sh) if want_stats else kw))
    on_dev = fn(*[dev(a) for a in arrays], *args, **(dict(kw, stats=sd) if want_stats else kw))
    torch.cuda.synchronize()
    same(on_dev, on_host, getattr(fn, "__name__", "call"))
    if want_stats:
        assert sd == sh and len(sh) > 0
    return on_host


def test_matchers(ctx, data):
    L, R = data["L"], data["R"]
    got = both(lambda l, r: stereo.calc_disparity(0, l, r, vwa.bounding_box(L), SEARCH, (7, 7), ctx=ctx), (L, R))
    both(lambda l, r: stereo.calc_disparity(2, l, r, vwa.BBox2i(5, 3, 37, 30), SEARCH, (3, 5), ctx=ctx), (L, R))
    assert got.shape == (34, 42, 3) and (got[..., 0] == 3).mean() > 0.9 and (got[..., 1] == 2).mean() > 0.9
    both(stereo.fast_box_sum, (L,), (3, 7), ctx=ctx)


def test_sub_pixel_refiners(ctx, data):
    arrays = (data["D3f"], data["L"], data["R"])
    both(stereo.parabola_subpixel, arrays, 0, 0.0, K5, ctx=ctx)
    for fn in (stereo.pyramid_subpixel, stereo.affine_subpixel, stereo.lk_subpixel, stereo.bayes_em_subpixel):
        both(fn, arrays, 2, 1.4, K5, max_pyramid_levels=1, block_size=BLOCK, ctx=ctx, stats=True)
    both(stereo.phase_subpixel, arrays, 2, 1.4, (7, 7), max_pyramid_levels=0, phase_subpixel_accuracy=10, block_size=BLOCK,
         ctx=ctx, stats=True)


def test_corr_eval(ctx, data):
    arrays = (data["L"], data["R"], data["D3f"])
    both(stereo.corr_eval, arrays, K5, "ncc", ctx=ctx, stats=True)
    both(lambda l, r, d, lv, rv, stats: stereo.corr_eval(l, r, d, (3, 7), "stddev", sample_rate=2, left_valid=lv, right_valid=rv,
                                                         block_size=BLOCK, ctx=ctx, stats=stats),
         arrays + (data["LM"], data["RM"]), stats=True)


def test_integer_disparity_filters(ctx, data):
    d = data["D3i"]
    both(stereo.rm_outliers_using_thresh, (d,), 2, 3, 1.0, 0.3, ctx=ctx)
    both(stereo.disparity_cleanup_using_thresh, (d,), 3, 2, 1.0, 0.3, ctx=ctx)
    both(stereo.disparity_mask, (d, data["LM"], data["RM"]), ctx=ctx)
    both(stereo.disparity_blob_filter, (d,), 6, ctx=ctx)


def test_pyramid_correlate_and_batch(ctx, data):
    import torch
    search = vwa.BBox2i.from_corners((-1, -1), (5, 4))
    kw = dict(consistency_threshold=2, filter_half_kernel=2, max_pyramid_levels=1, ctx=ctx)
    images = (data["L"], data["R"], data["LM"], data["RM"])
    both(stereo.pyramid_correlate, images[:2], None, None, 0, 0.0, search, K5, 0, **kw)
    both(stereo.pyramid_correlate, images, 2, 1.4, search, K5, 2, bbox=vwa.BBox2i(3, 5, 41, 33), **kw)
    boxes = [vwa.BBox2i(0, 0, 29, 23), vwa.BBox2i(29, 0, 19, 23), vwa.BBox2i(0, 23, 48, 17)]
    both(stereo.pyramid_correlate_batch, images[:2], None, None, 0, 0.0, search, K5, 0, boxes, **kw)
    both(stereo.pyramid_correlate_batch, images, 2, 1.4, search, K5, 2, boxes, **kw)
    # lr_disp_diff is written in place on either side
    dh = np.full((42, 50, 2), -7.0, np.float32)
    dd = dev(dh)
    kw["bbox"] = vwa.BBox2i(3, 5, 41, 33)     # inside the image pixels [1, 51) x [1, 43) that lr_disp_diff covers
    on_host = stereo.pyramid_correlate(*images, 0, 0.0, search, K5, 0, lr_disp_diff=dh, region_ul=(1, 1), **kw)
    on_dev = stereo.pyramid_correlate(*[dev(a) for a in images], 0, 0.0, search, K5, 0, lr_disp_diff=dd, region_ul=(1, 1), **kw)
    torch.cuda.synchronize()
    same(on_dev, on_host, "pyramid_correlate with lr_disp_diff")
    same(dd, dh, "lr_disp_diff")
    assert (dh != -7.0).any()
    with pytest.raises(core.ArgumentErr):     # the images are tensors, lr_disp_diff is not
        stereo.pyramid_correlate(*[dev(a) for a in images], 0, 0.0, search, K5, 0, lr_disp_diff=dh, region_ul=(1, 1), **kw)
    with pytest.raises(core.ArgumentErr):     # modified in place: never copied
        stereo.pyramid_correlate(*images, 0, 0.0, search, K5, 0, lr_disp_diff=np.zeros((42, 50, 4), np.float32)[..., ::2],
                                 region_ul=(1, 1), **kw)


def test_calc_disparity_sgm(ctx, data):
    L, R = data["SL"], data["SR"]
    box = vwa.bounding_box(L)
    both(lambda l, r: stereo.calc_disparity_sgm(3, l, r, box, (8, 0), (3, 3), ctx=ctx), (L, R))
    got = both(lambda l, r, lm, rm, prev: stereo.calc_disparity_sgm(3, l, r, box, (8, 0), (3, 3), left_mask=lm, right_mask=rm,
                                                                    prev_disparity=prev, with_subpixel=True, ctx=ctx),
               (L, R, data["SLM"], data["SRM"], data["PREV"]))
    assert got[0].shape == (46, 62, 3) and got[1].dtype == np.float32


def test_convergence_angle_and_filters(ctx, data):
    c1 = camera.CAHVModel((0, 0, 0), (0, 0, 1), (100, 0, 24), (0, 100, 20))
    c2 = camera.CAHVModel((1, 0, 0), (0, 0, 1), (100, 0, 24), (0, 100, 20))
    model = stereo.StereoModel(c1, c2)
    for d in (data["D3f"], data["D3i"]):
        both(model.convergence_angle, (d,), x0=2, y0=1, ctx=ctx)
    L = data["L"]
    both(filters.convolution_filter, (L,), np.arange(15, dtype=np.float32).reshape(3, 5) / 100, ctx=ctx)
    both(filters.laplacian_filter, (L,), edge=filters.ZeroEdgeExtension, ctx=ctx)
    both(filters.gaussian_filter, (L,), 1.5, ctx=ctx)


def test_row_strided_views_are_not_copied(ctx, data):
    """A tensor view whose last stride is 1 goes to the library as it is (pointer of the view, stride of the wider
    tensor) and gives the result of its contiguous copy."""
    import torch
    big_l = torch.full((40, 56), -1.0, dtype=torch.float32, device="cuda")
    big_r = torch.full((44, 66), -1.0, dtype=torch.float32, device="cuda")
    lv, rv = big_l[:, 3:51], big_r[:, 3:63]
    lv.copy_(dev(data["L"]))
    rv.copy_(dev(data["R"]))
    assert not lv.is_contiguous() and lv.stride(1) == 1
    ops = Operands("test", lv)
    for v in (lv, rv):
        a = ops.image(v, np.float32, rows=True)
        assert a.data_ptr() == v.data_ptr() and ops.row_stride(a) == v.stride(0) != v.shape[1]
    assert ops.image(lv, np.float32).data_ptr() != lv.data_ptr()     # every other operand is made contiguous
    assert ops.image(lv.t(), np.float32, rows=True).is_contiguous()  # and so is a view with another last stride
    for fn, views in ((lambda l, r: stereo.calc_disparity(0, l, r, vwa.BBox2i(0, 0, 48, 40), SEARCH, K5, ctx=ctx), (lv, rv)),
                      (lambda l: stereo.fast_box_sum(l, (3, 7), ctx=ctx), (lv,)),
                      (lambda l: filters.separable_convolution_filter(l, [1, 2, 1], [1, 4, 6, 4, 1], subsample=2, ctx=ctx), (lv,)),
                      (lambda l: filters.prefilter_image(l, 2, 1.4, ctx=ctx), (lv,))):
        got, want = fn(*views), fn(*[v.contiguous() for v in views])
        torch.cuda.synchronize()
        assert got.shape == want.shape and host(got).tobytes() == host(want).tobytes()
    assert (big_l[:, :3] == -1).all() and (big_l[:, 51:] == -1).all()


def test_cross_corr_consistency_check_in_place(ctx, data):
    import torch
    l2r, r2l = data["D3i"], data["R2L"]
    for diff in (False, True):
        ah, ad = l2r.copy(), dev(l2r)
        dh = np.full((44, 52, 2), -7.0, np.float32) if diff else None
        dd = dev(dh)
        kw = dict(lr_disp_diff=dh, ul_corner_offset=(2, 1)) if diff else {}
        kd = dict(lr_disp_diff=dd, ul_corner_offset=(2, 1)) if diff else {}
        assert stereo.cross_corr_consistency_check(ah, r2l, 1, ctx=ctx, **kw) is ah         # the very object
        assert stereo.cross_corr_consistency_check(ad, dev(r2l), 1, ctx=ctx, **kd) is ad
        torch.cuda.synchronize()
        same(ad, ah, "l2r")
        assert (ah[..., 2] != l2r[..., 2]).any()
        if diff:
            same(dd, dh, "lr_disp_diff")
    wide_h = np.zeros((40, 48, 4), np.int32)
    for wide in (wide_h, dev(wide_h)):
        with pytest.raises(core.ArgumentErr):     # a non-contiguous l2r is refused, never copied
            stereo.cross_corr_consistency_check(wide[..., :3], r2l if wide is wide_h else dev(r2l), 1, ctx=ctx)
    with pytest.raises(core.ArgumentErr):
        stereo.cross_corr_consistency_check(l2r.astype(np.float32), r2l, 1, ctx=ctx)
