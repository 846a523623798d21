"""The host plan of the pyramid correlator (csrc/pyramid_plan.h: level counts, slice layout, zone tasks, margins, zone rescale) on its own:
tests/cpp/test_pyramid_plan.cc is a plain C++ program built with the address and undefined-behaviour sanitizers and run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_pyramid_plan_program():
    subprocess.check_call(["make", "-s", "-C", CPP, "test_pyramid_plan"])
    p = subprocess.run([os.path.join(CPP, "test_pyramid_plan")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "0 failures" in p.stdout
