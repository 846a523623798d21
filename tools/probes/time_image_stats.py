"""Times of the image statistics family (csrc/image_stats.hip) at 4096^2 with HIP events after a warm-up, next to a device copy
of the same bytes measured in the same run.  GPU box only.

    python tools/probes/time_image_stats.py [--size 4096] [--repeat 20] [--out FILE.md]

Images: "natural" (smooth + noise), "one bin" (a constant: every valid pixel in one histogram bin) and "two bins" (two values
in neighbouring bins, alternating by column): the last two are the worst cases of the LDS adds.  Every entry reads the image
once per pass: the table gives the passes, the time per call and the image bytes read per second, beside the copy's."""
import argparse
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests/refimpl")
import image_stats_ref as ref  # noqa: E402
from visionworkbench_amd import core, image  # noqa: E402


def timed(fn, repeat):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(3):            # three windows of `repeat` calls: the spread says what a difference is worth
        a.record()
        for _ in range(repeat):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / repeat)
    return min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = args.size
    ctx = core.default_context(0)
    natural = ref.natural(n, n, 1, 0.1, 0.9)
    one = np.full((n, n), 0.5, np.float32)
    two = one.copy()
    two[:, 1::2] = 0.5 + 1.0 / 255
    mask = torch.from_numpy(ref.random_mask(n, n, 1, 0.9)).cuda()
    lines = ["| image | entry | passes over the image | ms (best of 3 windows) | ms (worst) | image GB/s read (best) | of the copy's read rate |",
             "|---|---|---|---|---|---|---|"]
    nbytes = n * n * 4
    src = torch.from_numpy(natural).cuda()
    dst = torch.empty_like(src)
    copy_best, copy_worst = timed(lambda: dst.copy_(src), args.repeat)
    copy_rate = nbytes / copy_best / 1e6
    lines.append("| natural | device copy (read + write of the same bytes) | 1 | %.4f | %.4f | %.0f | 1.00 |" % (copy_best, copy_worst, copy_rate))
    for name, img in (("natural", natural), ("one bin", one), ("two bins", two)):
        a = torch.from_numpy(img).cuda()
        mn, mx = image.min_max(a, ctx=ctx)[:2]
        entries = [
            ("min_max", 1, lambda: image.min_max(a, ctx=ctx)),
            ("min_max, masked", 1, lambda: image.min_max(a, mask, ctx=ctx)),
            ("moments", 1, lambda: image.moments(a, ctx=ctx)),
            ("histogram, 256 bins", 1, lambda: image.histogram(a, 256, mn, mx, ctx=ctx)),
            ("histogram, 4096 bins", 1, lambda: image.histogram(a, 4096, mn, mx, ctx=ctx)),
            ("histogram, 256 bins, masked", 1, lambda: image.histogram(a, 256, mn, mx, mask=mask, ctx=ctx)),
            ("median (radix select)", 5, lambda: image.median(a, ctx=ctx)),
            ("percentile 98 (radix select)", 3, lambda: image.percentile(a, 98.0, ctx=ctx)),
            ("normalize to float", 1, lambda: image.normalize(a, mn, mx, 0.0, 255.0, ctx=ctx)),
            ("clamp + normalize to uint8", 1, lambda: image.normalize(a, mn, mx, 0.0, 255.0, clamp=(mn, mx), dtype=np.uint8, ctx=ctx)),
            ("percentile_scale_convert to float, no host round trip", 3, lambda: image.percentile_scale_convert(a, dtype=np.float32, ctx=ctx)),
            ("u8_convert to uint8", 2, lambda: image.u8_convert(a, ctx=ctx)),
            ("otsu_threshold (two host round trips)", 2, lambda: image.otsu_threshold(a, ctx=ctx)),
        ]
        if name != "natural":
            entries = [e for e in entries if e[0].startswith(("histogram", "median", "percentile_scale"))]
        for what, passes, fn in entries:
            best, worst = timed(fn, args.repeat)
            rate = passes * nbytes / best / 1e6
            lines.append("| %s | %s | %d | %.4f | %.4f | %.0f | %.2f |" % (name, what, passes, best, worst, rate, rate / copy_rate))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write("%d x %d float32, %d calls per window, torch %s\n\n%s\n" % (n, n, args.repeat, torch.__version__, text))


if __name__ == "__main__":
    main()
