"""Replays one case of tests/family_cases.py: prints its parameters and, output by output, the positions where the GPU and the
CPU restatement differ.  GPU box only.  usage: python tools/replay_family_case.py <generator> <seed> <it> [COLSxROWS as given to fuzz_families.py --max-size]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import family_cases as fc  # noqa: E402
import test_fuzz_families_gpu as runner  # noqa: E402
import visionworkbench_amd as vwa  # noqa: E402


def describe(v):
    if isinstance(v, np.ndarray):
        return "%s %s" % (v.dtype.name, v.shape)
    if isinstance(v, list) and v and isinstance(v[0], np.ndarray):
        return "[%s]" % ", ".join(describe(x) for x in v)
    return repr(v)


def main():
    generator, seed, it = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    if len(sys.argv) > 4:
        fc.MAX_COLS, fc.MAX_ROWS = (int(v) for v in sys.argv[4].split("x"))
        fc.MOSAIC_MAX = max(fc.MOSAIC_MAX, fc.MAX_COLS)
    c = fc.case_at(generator, seed, it)
    print("case (%s, %d, %d)" % (generator, seed, it))
    for k in sorted(c):
        print("  %-16s %s" % (k, describe(c[k])))
    want = fc.reference(generator, c)
    ctx = vwa.Context(0)
    try:
        got, touched = runner.run_case(generator, c, ctx)
    finally:
        ctx.close()
    total = len(touched)
    for t in touched:
        print("the call changed what was not its to change:", t)
    for name in sorted(want):
        g, w = got.get(name), want[name]
        n = -1 if g is None else fc.differing(g, w)
        total += abs(n)
        if n < 0:
            print("%s: GPU %s, restatement %s" % (name, None if g is None else describe(g), describe(w)))
        elif n:
            ne = (g != w) & ~(np.isnan(g) & np.isnan(w)) if g.dtype.kind == "f" else g != w
            where = np.argwhere(ne)
            print("%s: %d of %d words differ" % (name, n, w.size))
            for pos in where[:16]:
                print("   %s gpu %r restatement %r" % (tuple(int(v) for v in pos), g[tuple(pos)], w[tuple(pos)]))
        else:
            print("%s: identical (%s)" % (name, describe(w)))
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
