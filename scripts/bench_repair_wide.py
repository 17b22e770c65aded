#!/usr/bin/env python3
"""Repair a sweep of wide stripes in one launch (hbec_repair_plan_wide) against
hbec_repair_plan_mixed on the same plan, which above k = 12 repairs one stripe
at a time, at 16+4 and 20+4.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
as a stripe plan (databufs at odd offsets).  Two mask sets: `single_loss`, one
shard lost per stripe, drawn uniformly; `all_present`, where the call is a
Verify.  Legs, in one run on the same buffers and flags:

  w    hbec_repair_plan_wide: the new call
  p    hbec_repair_plan_mixed: the per-stripe route of the same library

Method: a warm-up, then `rounds` rounds in which the legs run in
alternating order, each timed by HIP events around `reps` back-to-back calls
(w: 20; p: 1, a call being thousands of launches); medians, with the smallest
and largest round and their spread (max - min) / median.  Rates are over the
algorithmic bytes, (k + checked + rebuilt) S = (k + m) S per stripe, for both
legs: what p moves beyond them is its own cost.  Nothing is gated.

After the timing the lost shards are overwritten with garbage, each leg runs
once more, and buffers and flags of the two are compared: they must be equal,
and the flags those of clean codewords.

    python scripts/bench_repair_wide.py [--out FILE] [--rounds N] [--shape 16+4|20+4] [--objects N]
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
U32P = C.POINTER(C.c_uint32)
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
    rng = np.random.default_rng(100 * k + m)
    pats = np.ascontiguousarray([[1] * L] + [[0 if i == j else 1 for i in range(L)] for j in range(L)], np.uint8)
    runs = {"single_loss": np.ascontiguousarray(rng.integers(1, L + 1, n), np.uint32),
            "all_present": np.zeros(n, np.uint32)}
    lens = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = np.array([-(-x // k) for x in lens], np.int64)
    buf = torch.empty((1, int(L * ss.sum()) + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, buf.shape[1])
    offs, pos = [], 1
    for s in ss:
        offs.append(pos)
        pos += L * int(s) + 3
    plan = B.StripePlan(enc, stripes=[(buf.data_ptr() + o, int(s)) for o, s in zip(offs, ss)])
    plan.encode()
    torch.cuda.synchronize()
    flat = buf.view(-1)
    flags = {q: torch.zeros(n, dtype=torch.int32, device="cuda") for q in ("w", "p")}
    nbytes = int((L * ss).sum())
    for name, idx in runs.items():
        head = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0], idx.ctypes.data_as(U32P), 0)

        def w(a=head + (C.c_void_p(flags["w"].data_ptr()), stream)):
            RS.check(lib.hbec_repair_plan_wide(*a))

        def p(a=head + (C.c_void_p(flags["p"].data_ptr()), stream)):
            RS.check(lib.hbec_repair_plan_mixed(*a))

        legs = {"w": w, "p": p}
        ms = measure(legs, rounds)
        s0, r0 = B.repair_wide_stats(), B.repair_plan_stats()
        # garbage into every lost shard; each leg must leave the same buffers and clean flags
        after = {}
        for q, fn in legs.items():
            for e in np.nonzero(idx)[0]:
                s, i = int(ss[e]), int(idx[e]) - 1
                flat[offs[e] + i * s:offs[e] + (i + 1) * s].random_(0, 256)
            flags[q].zero_()
            fn()
            torch.cuda.synchronize()
            after[q] = flat.clone()
            assert not flags[q].cpu().numpy().any(), f"leg {q}: clean codewords flagged"
        s1, r1 = B.repair_wide_stats(), B.repair_plan_stats()
        assert torch.equal(after["w"], after["p"]), "the two calls leave different bytes"
        del after
        med = {q: statistics.median(x) for q, x in ms.items()}
        for q in legs:
            gbs = nbytes / (med[q] * 1e-3) / 1e9
            d = {"shape": f"{k}+{m} {n} objects", "layout": "stripes", "run": name, "leg": q, "ms": round(med[q], 5),
                 "ms_min": round(min(ms[q]), 5), "ms_max": round(max(ms[q]), 5),
                 "spread": round((max(ms[q]) - min(ms[q])) / med[q], 4), "rounds": rounds, "reps": REPS[q],
                 "algorithmic_bytes": nbytes, "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK, 4)}
            if q == "w":
                d["launches_per_call"] = s1["kernel_launches"] - s0["kernel_launches"]
                d["time_ratio_p_over_w"] = round(med["p"] / med["w"], 2)
            else:
                d["per_stripe_calls"] = r1["per_stripe_calls"] - r0["per_stripe_calls"]
            emit(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "repair_wide.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
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
