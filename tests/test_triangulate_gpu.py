"""stereo_triangulate / StereoModel / convergence_angle / universe_radius on the GPU against the CPU restatement
(tests/refimpl/triangulate_ref.cc): every word with ==, NaNs by position.  The scenes and the conditions they meet are
checked without a GPU in test_triangulate_cpu.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import triangulate_ref as ref  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import _lib, camera, stereo, synth  # noqa: E402

pytestmark = pytest.mark.gpu
TYPES = [np.int32, np.float32]
SIZES = [(1, 1), (2, 9), (17, 1), (37, 29), (70, 45), (1024, 768)]


def same(got, want, what=""):
    """Exact equality of every word; NaNs by position."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaNs in different places" % what
    g, w = got.copy(), want.copy()
    g[gn], w[wn] = 0, 0
    bits = {8: np.uint64, 4: np.uint32}[got.dtype.itemsize]
    bad = np.argwhere(g.view(bits) != w.view(bits))
    assert bad.size == 0, "%s: %d words differ, first at %s: got %r, want %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def sum_error_close(got, want, n):
    """Two orderings of n non-negative doubles with sum S differ by at most 2 (n - 1) 2^-53 S to first order."""
    assert abs(got - want) <= 2 * max(n - 1, 0) * 2.0 ** -53 * want, (got, want, n)


def check_all(got_xyz, got_err, got_vec, got_stats, want, what=""):
    same(got_xyz, want["xyz"], what + " xyz")
    same(got_err, want["error"], what + " error")
    same(got_vec, want["errvec"], what + " errvec")
    if got_stats is not None:
        assert got_stats[0] == want["stats"][0], what
        assert got_stats[1] == want["stats"][1], what
        sum_error_close(got_stats[2], want["stats"][2], want["stats"][0])


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def main():
    """The main scene in both pixel types with the restatement's results for both semantics."""
    out = {}
    for t in TYPES:
        d, c1, c2 = ref.main_scene(dtype=t)
        out[t] = (d, c1, c2, {s: ref.stereo_triangulate(d, c1, c2, semantics=s) for s in ("view", "model")})
    return out


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("size", SIZES)
def test_sizes(ctx, size, dtype):
    """Partial and multiple workgroups, and reductions across the wavefront, workgroup and fold boundaries."""
    w, h = size
    d, c1, c2 = ref.main_scene(w, h, seed=20 + w, dtype=dtype)
    want = ref.stereo_triangulate(d, c1, c2)
    st = []
    xyz, err, vec = stereo.stereo_triangulate(d, c1, c2, error=True, error_vector=True, stats=st, ctx=ctx)
    check_all(xyz, err, vec, st, want, "%dx%d" % size)
    assert st[0] == int(np.sum(want["classes"][..., 0] != ref.PX_INVALID))
    # without the optional outputs and without statistics: the other kernel
    same(stereo.stereo_triangulate(d, c1, c2, ctx=ctx), want["xyz"], "xyz only")


def camera_pairs():
    p1, p2 = ref.pinhole_pair(37, 29)
    return {
        "pinhole": (p1, p2),
        "cahv_flipped": (ref.cahv_of(p1), ref.cahv_of(p2)),
        "cahv_plain": (ref.cahv_of(p1, flip_v=True), ref.cahv_of(p2, flip_v=True)),
        "pinhole_cahv": (p1, ref.cahv_of(p2)),
        "cahv_pinhole": (ref.cahv_of(p1, flip_v=True), p2),
        "tsai_cahv": (ref.pinhole_pair(37, 29, distortion1=camera.TsaiLensDistortion(*ref.MILD_TSAI))[0], ref.cahv_of(p2)),
    }


@pytest.mark.parametrize("dtype", TYPES)
@pytest.mark.parametrize("semantics", ["view", "model"])
@pytest.mark.parametrize("pair", ["pinhole", "cahv_flipped", "cahv_plain", "pinhole_cahv", "cahv_pinhole", "tsai_cahv"])
def test_camera_kinds_and_semantics(ctx, pair, semantics, dtype):
    cams = camera_pairs()[pair]
    d, c1, c2 = ref.main_scene(37, 29, seed=31, dtype=dtype, cams=cams)
    want = ref.stereo_triangulate(d, c1, c2, semantics=semantics)
    assert np.any(want["xyz"] != 0)
    st = []
    if semantics == "view":
        xyz, err, vec = stereo.stereo_triangulate(d, c1, c2, error=True, error_vector=True, stats=st, ctx=ctx)
        check_all(xyz, err, vec, st, want, pair)
        same(stereo.stereo_triangulate(d, c1, c2, ctx=ctx), want["xyz"], pair + " xyz only")      # the kernel without statistics
    else:
        xyz, err = stereo.StereoModel(c1, c2)(d, stats=st, ctx=ctx)
        same(xyz, want["xyz"], pair + " xyz")
        same(err, want["error"], pair + " error")
        assert st[:2] == want["stats"][:2]
        sum_error_close(st[2], want["stats"][2], st[0])


@pytest.mark.parametrize("semantics", ["view", "model"])
def test_tsai_pair(ctx, semantics):
    """Every exit of the Newton solver (test_triangulate_cpu.py::test_tsai_scene_conditions) with the same bits."""
    d, c1, c2 = ref.tsai_scene()
    want = ref.stereo_triangulate(d, c1, c2, semantics=semantics)
    st = []
    xyz, err, vec = stereo._triangulate("test", d, c1, c2, 0, 0, 0.0, semantics, None, True, True, st, ctx)
    check_all(xyz, err, vec, st, want, "tsai " + semantics)
    same(stereo._triangulate("test", d, c1, c2, 0, 0, 0.0, semantics, None, False, False, None, ctx)[0], want["xyz"], "tsai xyz only")


def test_semantics_differ(ctx, main):
    d, c1, c2, want = main[np.float32]
    view = stereo.stereo_triangulate(d, c1, c2, ctx=ctx)
    model, _ = stereo.StereoModel(c1, c2)(d, ctx=ctx)
    same(view, want["view"]["xyz"])
    same(model, want["model"]["xyz"])
    assert np.any(view != model)


@pytest.mark.parametrize("layout", ["dxdy", "dv", "d"])
@pytest.mark.parametrize("dtype", TYPES)
def test_pixel_forms(ctx, main, layout, dtype):
    """The unmasked and scalar forms of DispHelper, on the host and on the device."""
    import torch
    full, c1, c2, _ = main[dtype]
    d = ref.relayout(full, layout)
    want = ref.stereo_triangulate(d, c1, c2, layout=layout)
    xyz, err = stereo.stereo_triangulate(d, c1, c2, error=True, layout=layout, ctx=ctx)
    same(xyz, want["xyz"], layout)
    same(err, want["error"], layout)
    t = stereo.stereo_triangulate(torch.from_numpy(d).cuda(), c1, c2, layout=layout, ctx=ctx)
    assert t.is_cuda
    same(t.cpu().numpy(), want["xyz"], layout + " device")


def test_angle_tol(ctx, main):
    d, c1, c2, want = main[np.float32]
    tol = 4e-3   # 1 - cos(5.1 degrees): most of the scene's rays converge by less
    w2 = ref.stereo_triangulate(d, c1, c2, angle_tol=tol)
    n_default = int(np.sum(want["view"]["classes"][..., 0] == ref.PX_PARALLEL))
    n_tol = int(np.sum(w2["classes"][..., 0] == ref.PX_PARALLEL))
    assert n_default < n_tol < d.shape[0] * d.shape[1]
    st = []
    xyz, err, vec = stereo.stereo_triangulate(d, c1, c2, error=True, error_vector=True, stats=st, angle_tol=tol, ctx=ctx)
    check_all(xyz, err, vec, st, w2, "angle_tol")
    xyz_m, _ = stereo.StereoModel(c1, c2, angle_tol=tol)(d, ctx=ctx)
    same(xyz_m, ref.stereo_triangulate(d, c1, c2, angle_tol=tol, semantics="model")["xyz"])
    # a negative tolerance is the default one (angle_tol > 0 overrides)
    same(stereo.stereo_triangulate(d, c1, c2, angle_tol=-1.0, ctx=ctx), want["view"]["xyz"])


@pytest.mark.parametrize("dtype", TYPES)
def test_device_entry(ctx, main, dtype):
    """Tensors stay on the device; the statistics too when a device tensor is handed in."""
    import torch
    d, c1, c2, want = main[dtype]
    dt = torch.from_numpy(d).cuda()
    words = torch.zeros(3, dtype=torch.int64, device="cuda")
    xyz, err, vec = stereo.stereo_triangulate(dt, c1, c2, error=True, error_vector=True, stats=words, ctx=ctx)
    assert xyz.is_cuda and err.is_cuda and vec.is_cuda and xyz.dtype == torch.float64
    st = [int(words[0].item())] + words[1:].view(torch.float64).cpu().tolist()
    check_all(xyz.cpu().numpy(), err.cpu().numpy(), vec.cpu().numpy(), st, want["view"], "device")
    st2 = []
    stereo.stereo_triangulate(dt, c1, c2, stats=st2, ctx=ctx)
    assert st2 == st
    # on a side stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xyz2, err2 = stereo.StereoModel(c1, c2)(dt, ctx=ctx)
    s.synchronize()
    same(xyz2.cpu().numpy(), want["model"]["xyz"])
    same(err2.cpu().numpy(), want["model"]["error"])


def test_two_calls_same_bits(ctx):
    import torch
    d, c1, c2 = ref.main_scene(333, 257, seed=5)
    dt = torch.from_numpy(d).cuda()
    runs = []
    for _ in range(2):
        st = []
        xyz, err, vec = stereo.stereo_triangulate(dt, c1, c2, error=True, error_vector=True, stats=st, ctx=ctx)
        runs.append((xyz.cpu().numpy(), err.cpu().numpy(), vec.cpu().numpy(), st))
    for a, b in zip(runs[0][:3], runs[1][:3]):
        same(a, b)
    assert runs[0][3] == runs[1][3]
    assert np.float64(runs[0][3][2]).view(np.uint64) == np.float64(runs[1][3][2]).view(np.uint64)


def _abi_triangulate(ctx, entry, d, c1, c2, x0, y0, dstride, xyz, xstride, err, estride, vec, vstride, stats, semantics=0):
    t = 1   # float32 pixels
    ptr = (lambda a: None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data))
    return entry(ctx._h, t, ptr(d), 37, 29, dstride, x0, y0, ctypes.byref(camera.descriptor_of(c1)),
                 ctypes.byref(camera.descriptor_of(c2)), 0.0, semantics, ptr(xyz), xstride, ptr(err), estride, ptr(vec), vstride, stats)


@pytest.mark.parametrize("device", [False, True])
def test_strided(ctx, device):
    """Row strides on every image: a 37 x 29 window of larger buffers, whose surroundings stay untouched."""
    import torch
    d, c1, c2 = ref.main_scene(37, 29, seed=31)
    want = ref.stereo_triangulate(d, c1, c2)
    big_d = np.full((29, 41, 3), 7.0, np.float32)
    big_d[:, :37] = d
    xyz, err, vec = np.full((29, 40, 3), -5.0), np.full((29, 45), -5.0), np.full((29, 38, 3), -5.0)
    st = _lib.TriangulateStats()
    if device:
        big_t, xyz_t, err_t, vec_t = (torch.from_numpy(a).cuda() for a in (big_d, xyz, err, vec))
        st_t = torch.zeros(3, dtype=torch.int64, device="cuda")
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.check(_abi_triangulate(ctx, ctx._lib.vwgpu_stereo_triangulate_dev, big_t, c1, c2, 0, 0, 41, xyz_t, 40, err_t, 45, vec_t, 38,
                                   st_t.data_ptr()))
        xyz, err, vec = xyz_t.cpu().numpy(), err_t.cpu().numpy(), vec_t.cpu().numpy()
        assert int(st_t[0].item()) == want["stats"][0]
    else:
        ctx.check(_abi_triangulate(ctx, ctx._lib.vwgpu_stereo_triangulate, big_d, c1, c2, 0, 0, 41, xyz, 40, err, 45, vec, 38,
                                   ctypes.addressof(st)))
        assert st.point_count == want["stats"][0] and st.max_error == want["stats"][1]
    same(xyz[:, :37], want["xyz"])
    same(err[:, :37], want["error"])
    same(vec[:, :37], want["errvec"])
    assert np.all(xyz[:, 37:] == -5.0) and np.all(err[:, 37:] == -5.0) and np.all(vec[:, 37:] == -5.0)


@pytest.mark.parametrize("semantics", ["view", "model"])
def test_tiles_equal_whole_map(ctx, main, semantics):
    """Tiles and row strips through x0, y0 equal the same region of the whole map."""
    d, c1, c2, want = main[np.float32]
    whole = want[semantics]
    boxes = [(0, 0, 70, 13), (0, 13, 70, 32), (0, 0, 33, 45), (33, 7, 37, 20), (8, 16, 1, 1), (60, 40, 10, 5)]
    for x, y, w, h in boxes:
        tile = np.ascontiguousarray(d[y:y + h, x:x + w])
        xyz, err, vec = stereo._triangulate("test", tile, c1, c2, x, y, 0.0, semantics, None, True, True, None, ctx)
        same(xyz, whole["xyz"][y:y + h, x:x + w], "tile %r" % ((x, y, w, h),))
        same(err, whole["error"][y:y + h, x:x + w])
        same(vec, whole["errvec"][y:y + h, x:x + w])
        same(xyz, ref.stereo_triangulate(tile, c1, c2, x0=x, y0=y, semantics=semantics)["xyz"])
    # a tile far from the origin: the pixel position enters as int32 + float in the model semantics
    xyz, _, _ = stereo._triangulate("test", d, c1, c2, 1 << 24, -(1 << 20), 0.0, semantics, None, False, False, None, ctx)
    same(xyz, ref.stereo_triangulate(d, c1, c2, x0=1 << 24, y0=-(1 << 20), semantics=semantics)["xyz"])


# The dot product of the two rays is bit-identical to the restatement's; the angle differs by the device's acos against
# glibc's.  Largest absolute difference measured on an MI355X over the scenes of this test (profiles/triangulate.md):
# 5.55e-17 (the Tsai scene; 1.39e-17 on the other two), one unit in the last place of the angle.  The bar is 4 x that.
CONVERGENCE_ANGLE_MEASURED = 5.55e-17


@pytest.mark.parametrize("pair", ["pinhole", "tsai", "cahv_pinhole", "pinhole_cahv", "cahv_flipped", "cahv_plain"])
def test_convergence_angle(ctx, pair):
    import torch
    if pair == "tsai":
        d, c1, c2 = ref.tsai_scene()
    else:
        d, c1, c2 = ref.main_scene(37, 29, seed=31, cams=camera_pairs()[pair])
    worst = 0.0
    for semantics in ("model", "view"):
        want = ref.convergence_angle(d, c1, c2, semantics=semantics)
        got = stereo.StereoModel(c1, c2).convergence_angle(d, semantics=semantics, ctx=ctx)
        got_t = stereo.StereoModel(c1, c2).convergence_angle(torch.from_numpy(d).cuda(), semantics=semantics, ctx=ctx)
        same(got_t.cpu().numpy(), got)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert np.array_equal(got[d[..., 2] == 0], np.zeros(int(np.sum(d[..., 2] == 0))))
        ok = ~np.isnan(want)
        worst = max(worst, float(np.abs(got[ok] - want[ok]).max()))
    print("convergence_angle %s: largest absolute difference to the restatement %.3g" % (pair, worst))
    assert worst <= 4 * CONVERGENCE_ANGLE_MEASURED


def _points(ch, seed=3):
    d, c1, c2 = ref.main_scene(70, 45, seed=seed)
    r = ref.stereo_triangulate(d, c1, c2)
    p = np.concatenate([r["xyz"]] + ([r["error"][..., None]] if ch == 4 else [r["errvec"]] if ch == 6 else []), axis=2)
    p[5, 5, 3:] = 1.0    # zero xyz with a non-zero tail
    return np.ascontiguousarray(p), c1


@pytest.mark.parametrize("ch", [3, 4, 6])
def test_universe_radius(ctx, ch):
    import torch
    p, c1 = _points(ch)
    origin = c1.camera_center() + (0.1, -0.2, 0.3)
    for near, far in ((11.0, 13.0), (0.0, 12.5), (11.5, ref.universe_radius.__defaults__[1]), (0.0, 0.0)):
        ws, gs = [], []
        want = ref.universe_radius(p, origin, near, far, stats=ws)
        got = stereo.universe_radius(p, origin, near, far, stats=gs, ctx=ctx)
        same(got, want, "universe %r" % ((near, far),))
        assert gs == ws and gs[0] == 70 * 45
        if (near, far) == (11.0, 13.0):
            assert 0 < gs[1] < np.sum(np.any(p[..., :3] != 0, axis=2))
        # on the device, and in place
        t = torch.from_numpy(p).cuda()
        gs2 = []
        out = stereo.universe_radius(t, origin, near, far, stats=gs2, ctx=ctx)
        assert out.is_cuda and out.data_ptr() != t.data_ptr()
        same(out.cpu().numpy(), want)
        same(t.cpu().numpy(), p)
        res = stereo.universe_radius(t, origin, near, far, ctx=ctx, out=t)
        assert res.data_ptr() == t.data_ptr()
        same(t.cpu().numpy(), want)
        assert gs2 == ws
    q = p.copy()
    stereo.universe_radius(q, origin, 11.0, 13.0, ctx=ctx, out=q)
    same(q, ref.universe_radius(p, origin, 11.0, 13.0))


def test_device_chain(ctx):
    """Sub-pixel disparity -> triangulate -> universe radius without a host copy: every intermediate is a CUDA tensor."""
    import torch
    left, right, _ = synth.stereo_pair(160, 96, 17, 1, block=64)
    lt, rt = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    di = stereo.calc_disparity(0, lt, rt, vwa.bounding_box(left), (17, 1), (7, 7), ctx=ctx)
    oh, ow = int(di.shape[0]), int(di.shape[1])      # the matcher's output is smaller than the left image by its kernel
    sub = stereo.parabola_subpixel(di.to(torch.float32), lt[:oh, :ow].contiguous(), rt, 0, 0.0, (7, 7), ctx=ctx)
    sub[..., 0] -= 8.0    # around zero disparity the converging pair sees the surface in front of it
    c1, c2 = ref.pinhole_pair(ow, oh)
    words = torch.zeros(3, dtype=torch.int64, device="cuda")
    xyz, err = stereo.stereo_triangulate(sub, c1, c2, error=True, stats=words, ctx=ctx)
    pts = stereo.universe_radius(torch.cat([xyz, err[..., None]], dim=2), (0, 0, 0), 2.0, 40.0, ctx=ctx)
    assert sub.is_cuda and xyz.is_cuda and pts.is_cuda and words.is_cuda
    host = sub.cpu().numpy()
    want = ref.stereo_triangulate(host, c1, c2)
    same(xyz.cpu().numpy(), want["xyz"])
    assert np.any(want["xyz"] != 0)
    want_pts = ref.universe_radius(np.concatenate([want["xyz"], want["error"][..., None]], axis=2), (0, 0, 0), 2.0, 40.0)
    same(pts.cpu().numpy(), want_pts)
    assert int(words[0].item()) == want["stats"][0]


def _write_raw(path, a):
    np.ascontiguousarray(a).tofile(path)


def test_cpp_surface(ctx, tmp_path):
    """vw::stereo::stereo_triangulate, StereoModel and UniverseRadiusFunc of vwlite (tests/refimpl/triangulate_view.cc)
    give the Python call's bits."""
    exe = ref.build_view_program()
    w, h = 70, 45
    d, c1, c2 = ref.main_scene(w, h)
    _write_raw(tmp_path / "d.bin", d)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    for kind, cams in (("pinhole", (c1, c2)), ("cahv", (ref.cahv_of(c1), ref.cahv_of(c2)))):
        out = run("view", kind, tmp_path / "d.bin", w, h, tmp_path / "xyz.bin")
        got = np.fromfile(tmp_path / "xyz.bin", np.float64).reshape(h, w, 3)
        same(got, stereo.stereo_triangulate(d, cams[0], cams[1], ctx=ctx), "C++ view " + kind)
        assert "triangulate_view ok" in out
    # the view rasterises per box through x0, y0
    run("boxes", "pinhole", tmp_path / "d.bin", w, h, tmp_path / "xyz.bin")
    same(np.fromfile(tmp_path / "xyz.bin", np.float64).reshape(h, w, 3), stereo.stereo_triangulate(d, c1, c2, ctx=ctx), "C++ boxes")
    # StereoModel: (xyz, error) in the model semantics
    run("model", "pinhole", tmp_path / "d.bin", w, h, tmp_path / "xyz.bin", tmp_path / "err.bin")
    xyz, err = stereo.StereoModel(c1, c2)(d, ctx=ctx)
    same(np.fromfile(tmp_path / "xyz.bin", np.float64).reshape(h, w, 3), xyz, "C++ model")
    same(np.fromfile(tmp_path / "err.bin", np.float64).reshape(h, w), err, "C++ model error")
    # a Tsai pair, and the universe radius with its counters
    dt, t1, t2 = ref.tsai_scene()
    _write_raw(tmp_path / "t.bin", dt)
    run("view", "tsai", tmp_path / "t.bin", w, h, tmp_path / "xyz.bin")
    txyz = stereo.stereo_triangulate(dt, t1, t2, ctx=ctx)
    same(np.fromfile(tmp_path / "xyz.bin", np.float64).reshape(h, w, 3), txyz, "C++ tsai")
    pts = stereo.stereo_triangulate(d, c1, c2, ctx=ctx)
    _write_raw(tmp_path / "p.bin", pts)
    out = run("universe", tmp_path / "p.bin", w, h, 0.1, -0.2, 0.3, 11.0, 13.0, tmp_path / "u.bin")
    st = []
    want = stereo.universe_radius(pts, (0.1, -0.2, 0.3), 11.0, 13.0, stats=st, ctx=ctx)
    same(np.fromfile(tmp_path / "u.bin", np.float64).reshape(h, w, 3), want, "C++ universe")
    assert "rejected %d of %d" % (st[1], st[0]) in out


def test_argument_errors(ctx):
    d, c1, c2 = ref.main_scene(37, 29, seed=31)
    lib, E = ctx._lib, -1
    xyz, err, vec = np.zeros((29, 37, 3)), np.zeros((29, 37)), np.zeros((29, 37, 3))

    def tri(**kw):
        a = dict(d=d, c1=c1, c2=c2, dstride=0, xyz=xyz, xstride=0, err=err, estride=0, vec=vec, vstride=0, semantics=0, type=1,
                 w=37, h=29, tol=0.0)
        a.update(kw)
        P = (lambda x: None if x is None else x.ctypes.data)
        C = (lambda c: None if c is None else ctypes.byref(camera.descriptor_of(c)))
        return lib.vwgpu_stereo_triangulate(ctx._h, a["type"], P(a["d"]), a["w"], a["h"], a["dstride"], 0, 0, C(a["c1"]), C(a["c2"]),
                                            a["tol"], a["semantics"], P(a["xyz"]), a["xstride"], P(a["err"]), a["estride"],
                                            P(a["vec"]), a["vstride"], None)

    assert tri() == 0
    assert tri(err=None, vec=None) == 0
    bad_kind, bad_dist = _lib.Camera(), _lib.Camera()
    ctypes.memmove(ctypes.addressof(bad_kind), ctypes.addressof(c1.descriptor), ctypes.sizeof(_lib.Camera))
    ctypes.memmove(ctypes.addressof(bad_dist), ctypes.addressof(c1.descriptor), ctypes.sizeof(_lib.Camera))
    bad_kind.kind = 2
    bad_dist.distortion_kind = 5
    for kw in (dict(d=None), dict(xyz=None), dict(c1=None), dict(c2=None), dict(type=2), dict(type=-1), dict(w=0), dict(h=-3),
               dict(tol=float("nan")), dict(semantics=2), dict(semantics=-1), dict(semantics=0x400), dict(semantics=0x101 + 0x1000),
               dict(dstride=36), dict(xstride=36), dict(estride=10), dict(vstride=1), dict(c1=bad_kind), dict(c2=bad_dist),
               dict(err=xyz), dict(vec=xyz)):
        assert tri(**kw) == E, kw
        assert ctx._lib.vwgpu_last_error(ctx._h)
    assert lib.vwgpu_stereo_triangulate(None, 1, d.ctypes.data, 37, 29, 0, 0, 0, ctypes.byref(c1.descriptor), ctypes.byref(c2.descriptor),
                                        0.0, 0, xyz.ctypes.data, 0, None, 0, None, 0, None) == E
    # convergence_angle
    ang = np.zeros((29, 37))
    cv = (lambda t=1, dd=d, a=c1, b=c2, s=1, o=ang, os=0: lib.vwgpu_convergence_angle(
        ctx._h, t, None if dd is None else dd.ctypes.data, 37, 29, 0, 0, 0, None if a is None else ctypes.byref(camera.descriptor_of(a)),
        None if b is None else ctypes.byref(camera.descriptor_of(b)), s, None if o is None else o.ctypes.data, os))
    assert cv() == 0
    assert cv(t=3) == E and cv(dd=None) == E and cv(a=None) == E and cv(b=bad_kind) == E and cv(s=7) == E and cv(o=None) == E and cv(os=5) == E
    # universe_radius
    p = np.zeros((29, 37, 3))
    o3 = np.zeros(3)
    ur = (lambda pts=p, ch=3, org=o3, near=1.0, far=2.0, out=p, stride=0: lib.vwgpu_universe_radius(
        ctx._h, None if pts is None else pts.ctypes.data, ch, 37, 29, stride, None if org is None else org.ctypes.data, near, far,
        None if out is None else out.ctypes.data, 0, None))
    assert ur() == 0
    for kw in (dict(pts=None), dict(out=None), dict(org=None), dict(ch=5), dict(ch=0), dict(near=-1.0), dict(far=-1.0),
               dict(near=3.0, far=2.0), dict(near=1.0, far=0.0), dict(near=float("nan")), dict(far=float("nan")), dict(stride=3)):
        assert ur(**kw) == E, kw
    # the Python layer raises the project's exceptions
    with pytest.raises(vwa.ArgumentErr):
        stereo.stereo_triangulate(d[..., :1], c1, c2, ctx=ctx)
    with pytest.raises(vwa.ArgumentErr):
        stereo.stereo_triangulate(d.astype(np.float64), c1, c2, ctx=ctx)
    with pytest.raises(vwa.ArgumentErr):
        stereo.stereo_triangulate(d, c1, "camera", ctx=ctx)
    with pytest.raises(vwa.ArgumentErr):
        stereo.universe_radius(np.zeros((4, 4, 5)), (0, 0, 0), ctx=ctx)
    with pytest.raises(vwa.ArgumentErr):
        stereo.universe_radius(np.zeros((4, 4, 3)), (0, 0, 0), 5.0, 1.0, ctx=ctx)
    with pytest.raises(vwa.ArgumentErr):
        stereo.StereoModel(c1, c2, angle_tol=float("nan"))(d, ctx=ctx)
