#!/usr/bin/env python3
"""Which first-round workgroups of the packed-u8 SAD matcher share a CU, and what the first-round hand-off does to them.

Reads the stamp records that tools/sad_timeline.py saves (its sad_stamps_WxH_SX.npy, one row of 16 u64 per tile) and prints
  * for the first round of dispatch (blockIdx.x < 2 x CUs): how many CUs hold exactly two of its workgroups, and on how many of those
    each candidate index rule on j = blockIdx.x >> 3 marks exactly one of the two (parity of j; j >= CUs per XCD);
  * staging time and byte phase 0 of the first round, split into the workgroups the rule lets start at once and those it delays;
  * per CU, how far apart its two slots end.
usage: python tools/sad_handoff_pairs.py file.npy [rule: 0 = parity (default), 1 = upper half]"""
import sys

import numpy as np

st = np.load(sys.argv[1])
rule = int(sys.argv[2]) if len(sys.argv) > 2 else 0
n = len(st)
assert n % 8 == 0 and (st[:, 0] != 0).all(), "expects a full grid (a multiple of 8 tiles, every one stamped)"
per_xcd = n // 8
wg = np.arange(n)
block = (wg % per_xcd) * 8 + wg // per_xcd                       # the kernel's tile order, inverted
j = block >> 3
hw = st[:, 2]
xcc = ((hw >> np.uint64(32)) & np.uint64(0xf)).astype(np.int64)
cu = ((hw >> np.uint64(8)) & np.uint64(0xf)).astype(np.int64)
sh = ((hw >> np.uint64(12)) & np.uint64(1)).astype(np.int64)
se = ((hw >> np.uint64(13)) & np.uint64(7)).astype(np.int64)
key = xcc * 1000 + se * 100 + sh * 50 + cu
cus = np.unique(key)
slots = 2 * len(cus)
first = block < slots
half = slots // 16                                                # CUs per XCD
base = st[:, 0].astype(np.float64).min()
us = lambda col: (st[:, col].astype(np.float64) - base) / 100.0   # noqa: E731
start, staged, ph0, end = us(0), us(3), us(4), us(8)
q = lambda a: "%.1f / %.1f / %.1f" % (np.percentile(a, 5), np.median(a), np.percentile(a, 95)) if len(a) else "-"   # noqa: E731

two = par = up = 0
dj = {}
for c in cus:
    js = np.sort(j[(key == c) & first])
    if len(js) != 2:
        continue
    two += 1
    par += (js[0] & 1) != (js[1] & 1)
    up += (js[0] >= half) != (js[1] >= half)
    dj[int(js[1] - js[0])] = dj.get(int(js[1] - js[0]), 0) + 1
print("%d CUs, %d tiles; first round = blockIdx.x < %d; XCD of block i is i %% 8 on %d of %d first-round workgroups" %
      (len(cus), n, slots, int((xcc[first] == (block[first] & 7)).sum()), int(first.sum())))
print("CUs with exactly two first-round workgroups: %d (%.1f %%)" % (two, 100.0 * two / len(cus)))
print("  exactly one of the two marked by the parity rule: %d (%.1f %% of all CUs); by the upper-half rule (j >= %d): %d (%.1f %%)" %
      (par, 100.0 * par / len(cus), half, up, 100.0 * up / len(cus)))
print("  j distance of the two: %s" % ", ".join("%d: %d" % kv for kv in sorted(dj.items(), key=lambda kv: -kv[1])[:6]))
late = ((j & 1) != 0) if rule == 0 else (j >= half)
for name, m in (("first round, starts at once", first & ~late), ("first round, delayed by the rule", first & late), ("later rounds", ~first)):
    print("%-34s n = %4d | start %s | staging (start -> staged) %s | staged at %s | byte phase 0 %s | end %s" %
          (name, int(m.sum()), q(start[m]), q((staged - start)[m]), q(staged[m]), q((ph0 - staged)[m]), q(end[m])))
gap, last = [], []
for c in cus:
    idx = np.where(key == c)[0]
    e = np.sort(end[idx])
    if len(e) >= 2:
        gap.append(e[-1] - e[-2])
        last.append(e[-1])
print("end of the two slots of a CU: the last two ends differ by %s us; last end per CU %s us; launch ends at %.1f us" % (q(np.array(gap)), q(np.array(last)), end.max()))
