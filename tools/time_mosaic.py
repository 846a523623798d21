#!/usr/bin/env python
"""Times the stages of a multi-band blend (visionworkbench_amd.mosaic) with HIP events: the
library's own event brackets (Context.profile_read) for masks, pyramids, collapse and trim, torch events around insert,
prepare and generate_patch, for two RGBA scenes: 2 x 4096^2 overlapping by a quarter and 8 x 2048^2 in a 4 x 2 grid.
Next to every stage stands the least number of bytes it has to move and the time that takes at 8 TB/s; the serial CPU
restatement (tests/refimpl/mosaic_ref.cc) is timed on a smaller scene and scaled by the pixel count.

    python tools/time_mosaic.py [--repeat 5] [--cpu-side 512] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "refimpl"))

PEAK = 8e12     # bytes / s


def scene(kind, side):
    """(sizes, offsets) of a scene of RGBA images of side x side."""
    if kind == "pair":
        return [(side, side)] * 2, [(0, 0), (side * 3 // 4, side // 16)]
    step = side - side // 8
    return [(side, side)] * 8, [(i * step, j * step) for j in range(2) for i in range(4)]


def device_image(torch, w, h, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    img = torch.rand((h, w, 4), generator=g, device="cuda")
    img[..., 3] = 0.5 + 0.5 * img[..., 3]
    img[..., :3] *= img[..., 3:4]
    return img


def least_bytes(sizes, view, levels):
    """The bytes every stage must move at least, 4 channels: n source pixels, v view pixels; a pyramid holds 4/3 n."""
    n = float(sum(w * h for w, h in sizes))
    v = float(view[0] * view[1])
    pyr = n * (1 - 0.25 ** levels) / 0.75
    return {
        "mosaic_masks": n * (16 + 4) + n * (4 + 4) * 2 + n * (4 + 4),      # alpha out of the pixels, two grassfire passes, the compare
        "mosaic_pyramids": 16 * pyr * 2 + 4 * pyr * 2 + 16 * (pyr - n),       # read G and mask, write diff and mask, write G
        "mosaic_collapse": 20 * pyr + 16 * v * (1 - 0.25 ** levels) / 0.75 * 2,
        "mosaic_trim": 32 * v + 4 * n,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--cpu-side", type=int, default=512)
    ap.add_argument("--small", action="store_true", help="scenes a sixteenth the size, for a quick look")
    args = ap.parse_args()
    import torch
    import visionworkbench_amd as vwa
    from visionworkbench_amd import mosaic
    import mosaic_ref as ref

    ctx = vwa.Context(0)
    results = []
    for kind, side in (("pair", 4096), ("grid8", 2048)):
        if args.small:
            side //= 4
        sizes, offsets = scene(kind, side)
        images = [device_image(torch, w, h, k) for k, (w, h) in enumerate(sizes)]
        best = {}
        for rep in range(args.repeat + 1):      # the first pass allocates
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ctx.profile_reset()
            ctx.profile_enable(True)
            c = mosaic.ImageComposite(ctx)
            ev[0].record()
            for img, (x, y) in zip(images, offsets):
                c.insert(img, x, y)
            ev[1].record()
            c.prepare()
            ev[2].record()
            out = c.generate()
            ev[3].record()
            torch.cuda.synchronize()
            stages = {"insert": ev[0].elapsed_time(ev[1]), "prepare": ev[1].elapsed_time(ev[2]), "generate_patch": ev[2].elapsed_time(ev[3])}
            stages["whole"] = ev[0].elapsed_time(ev[3])
            for name, ms in ctx.profile_read():
                if name.startswith("mosaic_"):
                    stages[name] = stages.get(name, 0.0) + ms
            ctx.profile_enable(False)
            view, levels = (c.cols(), c.rows()), c.levels
            del out
            c.close()
            if rep:
                for k, v in stages.items():
                    best[k] = min(best.get(k, v), v)
        need = least_bytes(sizes, view, levels)
        row = {"scene": "%d x %d^2" % (len(sizes), side), "view": view, "levels": levels, "ms": {k: round(v, 3) for k, v in best.items()},
               "least_MB": {k: round(v / 1e6, 1) for k, v in need.items()}, "ms_at_8TBps": {k: round(v / PEAK * 1e3, 3) for k, v in need.items()}}
        results.append(row)
        print(json.dumps(row))
        del images
        torch.cuda.empty_cache()
    # the restatement, serial, on a scene small enough to wait for
    s = args.cpu_side
    sizes, offsets = scene("pair", s)
    rng = np.random.RandomState(1)
    imgs = []
    for w, h in sizes:
        a = rng.uniform(0, 1, (h, w, 4)).astype(np.float32)
        a[..., 3] = 0.5 + 0.5 * a[..., 3]
        a[..., :3] *= a[..., 3:4]
        imgs.append(a)
    t0 = time.time()
    ref.compose(imgs, offsets).generate()
    dt = time.time() - t0
    px = sum(w * h for w, h in sizes)
    print(json.dumps({"restatement": "2 x %d^2" % s, "seconds": round(dt, 3), "ns_per_source_pixel": round(dt / px * 1e9, 1),
                      "scaled_to_2x4096^2_seconds": round(dt / px * 2 * 4096 * 4096, 1)}))
    ctx.close()


if __name__ == "__main__":
    main()
