#!/usr/bin/env python3
"""Split a batch of wide stripes in one launch (hbec_split_plan_wide) against
hbec_split_plan on the same sources, which above k = 12 queues a copy per data
shard, a memset per padded one and an apply in accumulate passes per entry, at
16+4 and 20+4.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
each at an odd address of one source arena, split into a stripe plan whose
stripes lie at odd offsets.  Each leg has a shard arena and a plan of its own
over the same layout, so the two results can be compared afterwards.

Legs, in one process on the same sources:

  w    hbec_split_plan_wide: the new call
  p    hbec_split_plan: the per-entry route of the same library

Method: a warm-up, then `rounds` rounds in which the legs run in
alternating order, each timed by HIP events around `reps` back-to-back calls
(w: 20; p: 1, a call being tens of thousands of copies, memsets and applies);
medians, with the smallest and largest round and their spread (max - min) /
median.  The rate is over bytes read plus bytes written, (2 k + m) S per entry,
for both legs.  Nothing is gated.

After the timing each leg splits into its own arena, filled with a sentinel
beforehand, and the two arenas are compared: they must be equal.

    python scripts/bench_split_wide.py [--out FILE] [--rounds N] [--shape 16+4|20+4] [--objects N]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from hummingbird_amd import _native as N  # noqa: E402
from hummingbird_amd import batch as B  # noqa: E402
from hummingbird_amd import reedsolomon as RS  # noqa: E402

PEAK = 8000.0
U64P = C.POINTER(C.c_uint64)
REPS = {"w": 20, "p": 1}


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(legs, rounds):
    for name, fn in legs.items():
        for _ in range(3 if name == "w" else 1):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    names = list(legs)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            ms[name].append(timed(legs[name], REPS[name]))
    return ms


def run(k, m, n, rounds, emit):
    enc = RS.New(k, m)
    L = k + m
    lib = N.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(100 * k + m + 7)
    sizes = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = [-(-x // k) for x in sizes]
    nbytes = (2 * k + m) * sum(ss)

    # the pieces 3 bytes apart from an odd address
    soffs, pos = [], 1
    for x in sizes:
        soffs.append(pos)
        pos += x + 3
    src = torch.empty((1, pos + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(src, src.shape[1])
    srcs = (C.c_void_p * n)(*[src.data_ptr() + o for o in soffs])
    lens = np.ascontiguousarray(sizes, np.uint64)
    # the stripes (k + m) S + 3 bytes apart from an odd offset, one arena and one plan per leg
    offs, pos = [], 1
    for s in ss:
        offs.append(pos)
        pos += L * s + 3
    arena = {q: torch.empty(pos + 16, dtype=torch.uint8, device="cuda") for q in ("w", "p")}
    plan = {q: B.StripePlan(enc, stripes=[(arena[q].data_ptr() + o, s) for o, s in zip(offs, ss)]) for q in arena}

    def w():
        RS.check(lib.hbec_split_plan_wide(enc.handle, plan["w"]._h, srcs, lens.ctypes.data_as(U64P), stream))

    def p():
        RS.check(lib.hbec_split_plan(enc.handle, plan["p"]._h, srcs, lens.ctypes.data_as(U64P), stream))

    legs = {"w": w, "p": p}
    ms = measure(legs, rounds)
    s0, r0 = B.split_wide_stats(), B.split_plan_stats()
    for q, fn in legs.items():
        arena[q].fill_(0xC3)
        fn()
    torch.cuda.synchronize()
    s1, r1 = B.split_wide_stats(), B.split_plan_stats()
    assert torch.equal(arena["w"], arena["p"]), "the two calls write different bytes"
    med = {q: statistics.median(x) for q, x in ms.items()}
    for q in legs:
        gbs = nbytes / (med[q] * 1e-3) / 1e9
        d = {"shape": f"{k}+{m} {n} objects", "layout": "stripes", "leg": q, "ms": round(med[q], 5),
             "ms_min": round(min(ms[q]), 5), "ms_max": round(max(ms[q]), 5),
             "spread": round((max(ms[q]) - min(ms[q])) / med[q], 4), "rounds": rounds, "reps": REPS[q],
             "bytes_read_plus_written": nbytes, "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK, 4)}
        if q == "w":
            d["launches_per_call"] = s1["kernel_launches"] - s0["kernel_launches"]
            d["time_ratio_p_over_w"] = round(med["p"] / med["w"], 2)
            d["slowest_w_below_fastest_p"] = max(ms["w"]) < min(ms["p"])
        else:
            d["per_stripe_calls"] = r1["per_stripe_calls"] - r0["per_stripe_calls"]
        emit(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "split_wide.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default=None, choices=["16+4", "20+4"])
    ap.add_argument("--objects", type=int, default=4096)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(a.out, "w") as out:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for k, m in ((16, 4), (20, 4)):
            if a.shape in (None, f"{k}+{m}"):
                run(k, m, a.objects, a.rounds, emit)


if __name__ == "__main__":
    main()
