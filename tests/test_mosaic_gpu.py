"""GPU: vw::mosaic::ImageComposite (libvwgpu.so, mosaic.hip) equal to the CPU restatement tests/refimpl/mosaic_ref.cc word
for word (== on all channels, no tolerance, no pixel left out): blends with and without fill_holes, draft mode, 1, 2 and 4
channels, alpha that is 1, fractional and 0 in an interior rectangle, host and device entries, strided buffers, the whole
view and patches at even and odd origins down to 1 x 1, the level-0 masks, a view enlarged through prepare(total_bbox),
negative offsets, the C++ surface, the argument errors, the image-count cap and a chain that stays on the device.  Finite
values only."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
import mosaic_ref as ref  # noqa: E402

import visionworkbench_amd as vwa  # noqa: E402
from visionworkbench_amd import core, mosaic  # noqa: E402

pytestmark = pytest.mark.gpu

# name: ([(cols, rows), ...], [(x, y), ...], total_bbox)
SCENES = {
    "pair16_overlap5": ([(16, 16), (16, 16)], [(0, 0), (11, 0)], None),                    # 2 levels
    "pair24x40_odd_offsets": ([(24, 40), (24, 40)], [(0, 0), (3, 7)], None),              # the parity branches of reduce()
    "edges_and_inside": ([(50, 40), (17, 13)], [(0, 0), (20, 11)], None),                 # all four canvas edges; strictly inside
    "three33x20_ties": ([(33, 20), (33, 20), (33, 20)], [(0, 0), (20, 0), (10, 11)], None),
    "gap": ([(20, 18), (20, 18)], [(0, 0), (27, 2)], None),                               # msum == 0 between them
    "big_next_to_9x9": ([(70, 45), (9, 9)], [(0, 0), (70, 36)], None),                    # mindim 9: one level
    "pair130x66": ([(130, 66), (130, 66)], [(0, 0), (71, 13)], None),                     # 4 levels, several workgroups, a partial one
    "total_bbox": ([(16, 16), (16, 16)], [(0, 0), (11, 0)], (-3, -2, 33, 21)),
    "negative_offsets": ([(24, 17), (19, 22)], [(-7, -3), (2, 4)], None),
}
LEVELS = {"pair16_overlap5": 2, "big_next_to_9x9": 1, "pair130x66": 4}


def images_of(name, channels, alpha):
    sizes = SCENES[name][0]
    out = []
    for k, (w, h) in enumerate(sizes):
        hole = (w // 3, h // 3, w // 3 + max(2, w // 5), h // 3 + max(2, h // 6)) if alpha == "mixed_with_hole" and k == 0 else None
        kind = {"one": "one", "fraction": "fraction", "mixed_with_hole": "one" if k % 2 == 0 else "fraction"}[alpha]
        out.append(ref.textured(w, h, channels, 10 * k + len(name), alpha=kind, hole=hole))
    return out


_REF = {}


def reference(name, channels, alpha, fill=False, draft=False):
    """The restatement's composite of a scene, computed once."""
    key = (name, channels, alpha, fill, draft)
    if key not in _REF:
        _REF[key] = ref.compose(images_of(name, channels, alpha), SCENES[name][1], fill_holes=fill, draft=draft, total_bbox=SCENES[name][2])
    return _REF[key]


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s against %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d words differ, first at %s: got %s want %s" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available()
    c = vwa.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def wide(a, pad=5):
    """`a` as a view of a wider array: rows further apart than the width (numpy or torch)."""
    if hasattr(a, "cpu"):
        import torch
        big = torch.full((a.shape[0], a.shape[1] + pad) + tuple(a.shape[2:]), 77.0, dtype=a.dtype, device=a.device)
    else:
        big = np.full((a.shape[0], a.shape[1] + pad) + a.shape[2:], 77, a.dtype)
    big[:, :a.shape[1]] = a
    return big[:, :a.shape[1]]


def gpu_composite(ctx, name, channels, alpha, fill=False, draft=False, device=True, strided=False):
    c = mosaic.ImageComposite(ctx)
    c.set_draft_mode(draft)
    c.set_fill_holes(fill)
    for img, (x, y) in zip(images_of(name, channels, alpha), SCENES[name][1]):
        a = dev(img) if device else img
        c.insert(wide(a) if strided else a, x, y)
    c.prepare(SCENES[name][2])
    return c


def patches_of(cols, rows):
    """(x0, y0, x1, y1): even and odd origins, a 1 x 1 patch, the last pixel."""
    out = [(2, 2, min(cols, 13), min(rows, 11)), (1, 3, min(cols, 12), min(rows, 10)), (cols // 2, rows // 2, cols // 2 + 1, rows // 2 + 1),
           (cols - 1, rows - 1, cols, rows), (cols // 2 - 1, 0, cols, rows)]
    return [p for p in out if p[0] < p[2] and p[1] < p[3]]


# ---- blending -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [False, True], ids=["trim", "fill_holes"])
@pytest.mark.parametrize("channels", [2, 4])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_blend_device(ctx, name, channels, fill):
    want = reference(name, channels, "mixed_with_hole", fill)
    c = gpu_composite(ctx, name, channels, "mixed_with_hole", fill)
    assert (c.cols(), c.rows(), c.levels) == (want.cols(), want.rows(), want.levels)
    if name in LEVELS:
        assert c.levels == LEVELS[name]
    b, v = c.bbox(), c.source_data_bbox()
    assert tuple(b.min + b.max) == want.bbox() and tuple(v.min + v.max) == want.source_data_bbox()
    for p in range(len(SCENES[name][0])):
        same(c.mask(p), want.mask(p), "mask %d" % p)
    whole = want.generate()
    same(host(c.generate()), whole, "whole view")
    for x0, y0, x1, y1 in patches_of(c.cols(), c.rows()):
        # patch by patch against the restatement's own patch (which the CPU tests show equal to the crop of the whole view)
        same(host(c.generate_patch((x0, y0, x1, y1))), want.generate_patch(x0, y0, x1 - x0, y1 - y0), "patch %s" % ((x0, y0, x1, y1),))
    c.close()


@pytest.mark.parametrize("alpha", ["one", "fraction"])
@pytest.mark.parametrize("channels", [2, 4])
@pytest.mark.parametrize("name", ["pair24x40_odd_offsets", "three33x20_ties", "pair130x66"])
def test_blend_alpha_kinds(ctx, name, channels, alpha):
    for fill in (False, True):
        c = gpu_composite(ctx, name, channels, alpha, fill)
        same(host(c.generate()), reference(name, channels, alpha, fill).generate(), "fill_holes %s" % fill)
        c.close()


@pytest.mark.parametrize("channels", [2, 4])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_blend_host_and_strided(ctx, name, channels):
    want = reference(name, channels, "mixed_with_hole").generate()
    c = gpu_composite(ctx, name, channels, "mixed_with_hole", device=False, strided=True)
    got = c.generate()
    assert isinstance(got, np.ndarray)
    same(got, want, "host entry, strided inputs")
    out = wide(np.zeros_like(want))
    c.generate_patch((0, 0, c.cols(), c.rows()), out=out)
    same(out, want, "host entry, strided output")
    assert np.all(out.base[:, want.shape[1]:] == 77)
    x, y = c.cols() // 2, c.rows() // 3
    same(c(x, y), want[y, x], "operator()")
    c.close()
    d = gpu_composite(ctx, name, channels, "mixed_with_hole", device=True, strided=True)
    dout = wide(dev(np.zeros_like(want)))
    d.generate_patch((0, 0, d.cols(), d.rows()), out=dout)
    same(host(dout), want, "device entry, strided input and output")
    d.close()


def test_fill_holes_set_after_prepare(ctx):
    name = "pair24x40_odd_offsets"
    c = gpu_composite(ctx, name, 4, "mixed_with_hole", fill=False)
    same(host(c.generate()), reference(name, 4, "mixed_with_hole", False).generate(), "before")
    c.set_fill_holes(True)      # the pyramids are built again
    same(host(c.generate()), reference(name, 4, "mixed_with_hole", True).generate(), "after")
    c.close()


def test_blend_one_call(ctx):
    name = "three33x20_ties"
    imgs = images_of(name, 4, "mixed_with_hole")
    got = mosaic.blend([dev(i) for i in imgs], SCENES[name][1], ctx=ctx)
    same(host(got), reference(name, 4, "mixed_with_hole").generate(), "blend()")


# ---- draft mode -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 2, 4])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_draft(ctx, name, channels):
    want = reference(name, channels, "fraction", draft=True)
    whole = want.generate()
    for device in (True, False):
        c = gpu_composite(ctx, name, channels, "fraction", draft=True, device=device, strided=not device)
        same(host(c.generate()), whole, "draft, device %s" % device)
        for x0, y0, x1, y1 in patches_of(c.cols(), c.rows())[:3]:
            same(host(c.generate_patch((x0, y0, x1, y1))), whole[y0:y1, x0:x1], "draft patch")
        c.close()


def test_known_answer(ctx):
    c = mosaic.ImageComposite(ctx)
    c.set_draft_mode(True)
    c.insert(np.full((8, 8), 2, np.float32), 3, 0)
    assert (c.cols(), c.rows()) == (8, 8)
    c.insert(np.full((8, 8), 3, np.float32), 0, 0)
    assert (c.cols(), c.rows()) == (11, 8)
    c.prepare()
    out = c.generate()
    assert np.all(out[:, :8] == 3) and np.all(out[:, 8:] == 2)
    c.close()


# ---- the C++ surface --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [2, 4])
def test_vwlite_program_equals_python(ctx, tmp_path, channels):
    exe = ref.build_view_program()
    name = "pair24x40_odd_offsets"
    imgs = images_of(name, channels, "mixed_with_hole")
    args = []
    for k, (img, (x, y)) in enumerate(zip(imgs, SCENES[name][1])):
        path = str(tmp_path / ("img%d.bin" % k))
        img.tofile(path)
        args += [path, str(img.shape[1]), str(img.shape[0]), str(x), str(y)]
    c = gpu_composite(ctx, name, channels, "mixed_with_hole")
    py = host(c.generate())
    out = str(tmp_path / "out.bin")
    text = subprocess.check_output([exe, str(channels), "0", "0", out, "5", "9"] + args).decode().split("\n")
    assert text[0].split() == [str(c.cols()), str(c.rows()), str(c.levels)] and "mosaic_view ok" in text
    assert [int(v) for v in text[1].split()] == list(reference(name, channels, "mixed_with_hole").bbox())
    same(np.fromfile(out, np.float32).reshape(py.shape), py, "vwlite")
    same(np.array([float(v) for v in text[3].split()], np.float32), py[9, 5], "operator()")
    c.close()


# ---- argument errors ----------------------------------------------------------------------------------------------------------------

def test_argument_errors(ctx):
    a2, a4, a1 = ref.textured(16, 16, 2, 1), ref.textured(16, 16, 4, 1), ref.textured(16, 16, 1, 1)
    c = mosaic.ImageComposite(ctx)
    with pytest.raises(core.ArgumentErr):
        c.prepare()                                     # nothing inserted
    c.insert(a2, 0, 0)
    with pytest.raises(core.ArgumentErr):
        c.insert(a4, 3, 3)                              # mixed channel counts
    with pytest.raises(core.ArgumentErr):
        c.generate_patch((0, 0, 4, 4))                  # generate before prepare
    with pytest.raises(core.ArgumentErr):
        c.prepare((1, 0, 20, 20))                       # a total box that does not contain every image
    c.prepare((-2, -2, 20, 20))
    with pytest.raises(core.ArgumentErr):
        c.insert(a2, 1, 1)                              # insert after prepare
    with pytest.raises(core.ArgumentErr):
        c.prepare()                                     # twice
    for box in ((-1, 0, 4, 4), (0, 0, 23, 4), (0, 19, 4, 23), (4, 4, 4, 8)):
        with pytest.raises(core.ArgumentErr):
            c.generate_patch(box)                       # outside the view, or empty
    with pytest.raises(core.ArgumentErr):
        c.mask(2)
    c.close()
    d = mosaic.ImageComposite(ctx)
    d.insert(a1, 0, 0)
    with pytest.raises(core.ArgumentErr):
        d.prepare()                                     # blending one channel
    d.close()
    e = mosaic.ImageComposite(ctx)
    e.set_draft_mode(True)
    e.insert(a2, 0, 0)
    e.prepare()
    e.set_draft_mode(False)
    with pytest.raises(core.ArgumentErr):
        e.generate_patch((0, 0, 4, 4))                  # no masks were made
    with pytest.raises(core.ArgumentErr):
        e.mask(0)
    e.close()
    f = mosaic.ImageComposite(ctx)
    with pytest.raises(core.ArgumentErr):
        f.insert(np.zeros((4, 4, 3), np.float32), 0, 0)   # three channels
    f.close()


def test_image_count_cap(ctx):
    """VWGPU_COMPOSITE_MAX_IMAGES = 64: the 65th insert is NoImpl, and the 64 blend."""
    c = mosaic.ImageComposite(ctx)
    tile = np.ones((4, 4, 2), np.float32)
    for k in range(64):
        c.insert(tile, k % 8, k // 8)
    with pytest.raises(core.NoImplErr):
        c.insert(tile, 0, 0)
    c.prepare()
    want = ref.compose([tile] * 64, [(k % 8, k // 8) for k in range(64)]).generate()
    same(c.generate(), want, "64 images")     # up to 48 overlapping images: several tables of the mask kernel
    c.close()


# ---- a chain that stays on the device -------------------------------------------------------------------------------------------------

def test_transform_then_blend_stays_on_the_device(ctx):
    import torch
    from visionworkbench_amd import transform as tf
    base = ref.textured(48, 40, 2, 3)
    other = dev(ref.textured(48, 40, 2, 4)[..., 0].copy())
    ang = 0.03   # a translation plus a small rotation
    H = np.array([[np.cos(ang), -np.sin(ang), 2.5], [np.sin(ang), np.cos(ang), -1.25], [0, 0, 1]])
    warped, valid = tf.transform(other, tf.HomographyTransform(H), mask=torch.ones_like(other, dtype=torch.uint8), ctx=ctx)
    assert 0 < int((valid == 0).sum()) < valid.numel()      # the warp leaves part of the frame empty
    alpha = (valid != 0).to(torch.float32)
    img = torch.stack([warped * alpha, alpha], dim=2).contiguous()      # premultiplied, alpha from the validity mask
    got = mosaic.blend([dev(base), img], [(0, 0), (17, 5)], ctx=ctx)
    want = ref.compose([base, img.cpu().numpy()], [(0, 0), (17, 5)]).generate()
    same(host(got), want, "transform -> alpha -> blend")
