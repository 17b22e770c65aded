#!/usr/bin/env python3
"""Glue a batch of wide stripes in one launch (hbec_glue_plan_wide) against
hbec_glue_plan_mixed on the same plan and destinations, which above k = 12 queues
a copy per present data shard and an apply per degraded entry, at 16+4 and 20+4.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
as a stripe plan (buffers at odd offsets), each glued to a destination at an odd
address.  Runs:

  healthy         every shard present, whole entries
  one_lost        one data shard lost per entry, drawn uniformly, whole entries
  lost_past_end   one data shard i >= 1 lost per entry and lens[e] = i S: the range
                  ends before the lost shard, so the wide call gathers
  healthy_ranged  every shard present with lost_past_end's lens: the same bytes
                  read and written as lost_past_end

Legs, in one process on the same buffers:

  w    hbec_glue_plan_wide: the new call
  p    hbec_glue_plan_mixed: the per-entry route of the same library

Method: a warm-up, then `rounds` rounds in which the legs run in
alternating order, each timed by HIP events around `reps` back-to-back calls
(w: 20; p: 1, a call being tens of thousands of copies); medians, with the
smallest and largest round and their spread (max - min) / median.  Rates are over
bytes read plus bytes written: written, lens[e]; read, lens[e] where nothing is
decoded and k min(S, lens[e]) where something is, for both legs.  Nothing is gated.

After the timing each leg writes to a destination arena of its own, filled with a
sentinel, and the two arenas are compared: they must be equal.

    python scripts/bench_glue_wide.py [--out FILE] [--rounds N] [--shape 16+4|20+4] [--objects N]
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
    rng = np.random.default_rng(100 * k + m)
    # pattern 0: every shard present; pattern 1 + j: data shard j lost
    pats = np.ascontiguousarray([[1] * L] + [[0 if i == j else 1 for i in range(L)] for j in range(k)], np.uint8)
    sizes = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = np.array([-(-x // k) for x in sizes], np.int64)
    whole = np.array(sizes, np.uint64)
    any_lost = np.ascontiguousarray(rng.integers(0, k, n), np.uint32)
    late_lost = np.ascontiguousarray(rng.integers(1, k, n), np.uint32)
    ranged = (late_lost.astype(np.int64) * ss).astype(np.uint64)  # ends where the lost shard begins
    zeros = np.zeros(n, np.uint32)
    runs = {"healthy": (zeros, whole), "one_lost": (any_lost + 1, whole),
            "lost_past_end": (late_lost + 1, ranged), "healthy_ranged": (zeros, ranged)}

    buf = torch.empty((1, int(L * ss.sum()) + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, buf.shape[1])
    offs, pos = [], 1
    for s in ss:
        offs.append(pos)
        pos += L * int(s) + 3
    plan = B.StripePlan(enc, stripes=[(buf.data_ptr() + o, int(s)) for o, s in zip(offs, ss)])
    plan.encode()
    torch.cuda.synchronize()
    # destinations k S + 3 bytes apart from an odd address, one arena per leg
    doffs, pos = [], 1
    for s in ss:
        doffs.append(pos)
        pos += k * int(s) + 3
    arena = {q: torch.empty(pos + 16, dtype=torch.uint8, device="cuda") for q in ("w", "p")}
    dsts = {q: (C.c_void_p * n)(*[arena[q].data_ptr() + o for o in doffs]) for q in ("w", "p")}

    for name, (idx, lens) in runs.items():
        idx = np.ascontiguousarray(idx, np.uint32)
        lens = np.ascontiguousarray(lens, np.uint64)
        decoded = np.array([p > 0 and (p - 1) * s < ln for p, s, ln in zip(idx.tolist(), ss.tolist(), lens.tolist())])
        read = np.where(decoded, k * np.minimum(ss, lens.astype(np.int64)), lens.astype(np.int64))
        nbytes = int(read.sum() + lens.astype(np.int64).sum())
        head = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0], idx.ctypes.data_as(U32P))

        def w(a=head + (dsts["w"], lens.ctypes.data_as(U64P), stream)):
            RS.check(lib.hbec_glue_plan_wide(*a))

        def p(a=head + (dsts["p"], lens.ctypes.data_as(U64P), stream)):
            RS.check(lib.hbec_glue_plan_mixed(*a))

        legs = {"w": w, "p": p}
        ms = measure(legs, rounds)
        s0, r0 = B.glue_wide_stats(), B.glue_plan_stats()
        for q, fn in legs.items():
            arena[q].fill_(0xC3)
            fn()
        torch.cuda.synchronize()
        s1, r1 = B.glue_wide_stats(), B.glue_plan_stats()
        assert torch.equal(arena["w"], arena["p"]), f"{name}: the two calls write different bytes"
        med = {q: statistics.median(x) for q, x in ms.items()}
        for q in legs:
            gbs = nbytes / (med[q] * 1e-3) / 1e9
            d = {"shape": f"{k}+{m} {n} objects", "layout": "stripes", "run": name, "leg": q, "ms": round(med[q], 5),
                 "ms_min": round(min(ms[q]), 5), "ms_max": round(max(ms[q]), 5),
                 "spread": round((max(ms[q]) - min(ms[q])) / med[q], 4), "rounds": rounds, "reps": REPS[q],
                 "bytes_read_plus_written": nbytes, "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK, 4)}
            if q == "w":
                d["launches_per_call"] = s1["kernel_launches"] - s0["kernel_launches"]
                d["time_ratio_p_over_w"] = round(med["p"] / med["w"], 2)
            else:
                d["per_stripe_calls"] = r1["per_stripe_calls"] - r0["per_stripe_calls"]
            emit(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "glue_wide.jsonl"))
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
