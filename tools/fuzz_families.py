"""The long-running version of tests/test_fuzz_families_gpu.py: seeded random cases of tests/family_cases.py through the Python
wrappers on one context, every word of every output against the CPU restatement.  GPU box only.

usage: python tools/fuzz_families.py --family F --seed S --n N [--start I] [--shuffle] [--max-size COLSxROWS]

F is a generator of tests/family_cases.py (disparity_filter_cases, outlier_filter_cases, disparity_map_cases, transform_cases,
corr_eval_cases, hole_fill_cases, mosaic_cases) or `all`.  --shuffle takes N cases of EVERY family and interleaves them in a
random order (a function of the seed) on the one context, so that each call finds the arenas as another family left them.
--max-size raises the
largest image of the size sampler above the suite's 140 x 48 (and the largest mosaic image to COLS): other cases than the suite's,
so pass it to the replay too.  Stops at the first failing case, prints (generator, seed, it) and what differs, and exits 1; tools/replay_family_case.py shows
the case."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import family_cases as fc  # noqa: E402
import test_fuzz_families_gpu as runner  # noqa: E402
import visionworkbench_amd as vwa  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", required=True, choices=sorted(fc.GENERATORS) + ["all"])
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--start", type=int, default=0)
    ap.add_argument("--shuffle", action="store_true")
    ap.add_argument("--max-size", default=None)
    a = ap.parse_args()
    if a.max_size:
        fc.MAX_COLS, fc.MAX_ROWS = (int(v) for v in a.max_size.split("x"))
        fc.MOSAIC_MAX = max(fc.MOSAIC_MAX, fc.MAX_COLS)
    families = sorted(fc.GENERATORS) if a.family == "all" or a.shuffle else [a.family]
    order = [(g, it) for g in families for it in range(a.start, a.n)]
    if a.shuffle:
        order = [order[k] for k in np.random.default_rng([a.seed, 0x5F]).permutation(len(order))]
    ctx = vwa.Context(0)
    t0, done = time.time(), {g: 0 for g in families}
    try:
        for g, it in order:
            bad = runner.compare(g, fc.case_at(g, a.seed, it), ctx)
            if bad:
                print("MISMATCH (generator, seed, it) = (%s, %d, %d): entry %s shape %s differing words %s" % (g, a.seed, it, bad[1], bad[2], bad[3]))
                print("replay: python tools/replay_family_case.py %s %d %d%s" % (g, a.seed, it, " " + a.max_size if a.max_size else ""))
                return 1
            done[g] += 1
    finally:
        ctx.close()
    print("identical: seed %d %s%s in %.1f s" % (a.seed, " ".join("%s %d" % kv for kv in sorted(done.items())), " shuffled" if a.shuffle else "",
                                                  time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
