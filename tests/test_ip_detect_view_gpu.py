"""ip_detect_view.cc: the C++ surface of vw::ip detection and description (vwlite vw/InterestPoint.h) on libvwgpu.so, written as
tools/ipfind.cc calls it.  The program reads an image this side wrote, detects with detect_interest_points, describes with
describe_interest_points and writes a .vwip file; every field and every descriptor word equals what the Python module returns
for the same image (both go through the library's host entries), and its IntegralImage equals integral_image()."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ip_detect_ref as ref  # noqa: E402
import ip_detect_scenes as sc  # noqa: E402

from visionworkbench_amd import interest_point as ipm  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ("x", "y", "ix", "iy", "orientation", "scale", "interest", "polarity", "octave", "scale_lvl", "descriptor")


def same_points(got, want, what):
    assert len(got) == len(want) and len(want) > 0, "%s: %d points, want %d" % (what, len(got), len(want))
    for name in FIELDS:
        ref.same(getattr(got, name), getattr(want, name), "%s %s" % (what, name))


@pytest.mark.parametrize("operator,generator,gain", [("iagd", "sgrad", 1.0), ("obalog", "sgrad", 4.0), ("obalog", "sgrad2", 4.0), ("iagd", "sgrad2", 1.0)])
def test_cpp_surface(tmp_path, operator, generator, gain):
    exe = ref.build_view_program()
    img = sc.scene(1200, 70, 8)      # two tiles of detect_interest_points and of describe_interest_points
    img.tofile(str(tmp_path / "image.bin"))
    per_tile = 700
    prefix = str(tmp_path / "out")
    run = subprocess.run([exe, str(tmp_path / "image.bin"), "1200", "70", operator, generator, str(per_tile), repr(gain), prefix],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
    want = ipm.ipfind(img, detector=operator, descriptor=generator, ip_per_tile=per_tile, gain=gain)
    assert len(np.unique(want.x.astype(np.int32) // 1024)) == 2
    if operator == "obalog":
        assert np.count_nonzero(want.orientation) > 5
    same_points(ipm.read_binary_ip_file(prefix + ".vwip"), want, "ipfind")
    # process_image on the whole image as one tile, described by the generator's operator() on the whole image
    if operator == "obalog":
        det = ipm.IntegralInterestPointDetector(ipm.OBALoGInterestOperator(float(ipm.IDEAL_OBALOG_THRESHOLD / np.float32(gain))), max_points=per_tile)
    else:
        det = ipm.IntegralAutoGainDetector(per_tile)
    gen = ipm.SGradDescriptorGenerator() if generator == "sgrad" else ipm.SGrad2DescriptorGenerator()
    same_points(ipm.read_binary_ip_file(prefix + ".whole.vwip"), gen(img, det.process_image(img, per_tile)), "process_image")
    ref.same(np.fromfile(prefix + ".integral", np.float32).reshape(71, 1201), ipm.integral_image(img), "IntegralImage")
