#!/usr/bin/env python3
"""Verify of a repair sweep whose stripes are missing different shards, in one
call (hbec_verify_plan_mixed), against the two existing calls that bound it, at
4+2 and 8+3.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
as a stripe plan (databufs at odd offsets) and as an object plan (data arena +
parity arena).  Three runs per layout: `degraded`, a mask per stripe drawn
uniformly from all single and double losses (at 4+2 a double loss leaves exactly
k shards: v reads nothing of those stripes and sets bit 1); `single_loss`, from
the single losses alone, where v and r move the same bytes per stripe; and
`all_present`.  Legs, all on the same buffers in the same run:

  v   hbec_verify_plan_mixed with the masks: the new call
  r   hbec_reconstruct_plan_mixed with the same masks (degraded runs): it reads
      k S and writes (lost) S per stripe where v reads (present) S, the same
      bytes for a single loss in 4+2 and more for a double loss
  p   hbec_verify_plan (all_present run): the read-only upper bound

Method: a warm-up, then `rounds` rounds in which the legs run in
alternating order, each timed by HIP events around `reps` back-to-back calls
(the calls' host side is inside the bracket); medians, with the smallest and
largest round and their spread (max - min) / median beside them.  Rates are over
the algorithmic bytes of each leg.  Nothing is gated: the v line carries its
time ratio to r (or p) and whether it is slower than r by more than the larger
of the two legs' spreads.

    python scripts/bench_verify_mixed.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N]
"""
from __future__ import annotations

import argparse
import ctypes as C
import itertools
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
REPS = 20


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
    for fn, _ in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    names = list(legs)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            ms[name].append(timed(legs[name][0], REPS))
    return ms


def run(k, m, n, rounds, emit):
    enc = RS.New(k, m)
    L = k + m
    lib = N.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(100 * k + m)
    masks = [[1] * L]
    for c in (1, 2):
        for lost in itertools.combinations(range(L), c):
            masks.append([0 if i in lost else 1 for i in range(L)])
    pats = np.ascontiguousarray(masks, np.uint8)
    lost_of = (L - pats.sum(axis=1)).astype(np.int64)
    runs = {"degraded": np.ascontiguousarray(rng.integers(1, len(masks), n), np.uint32),
            "single_loss": np.ascontiguousarray(rng.integers(1, L + 1, n), np.uint32),
            "all_present": np.zeros(n, np.uint32)}
    lens = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = np.array([-(-x // k) for x in lens], np.int64)
    shape = f"{k}+{m} {n} objects"

    for layout in ("stripes", "objects"):
        if layout == "stripes":
            buf = torch.empty((1, int(L * ss.sum()) + 3 * n + 16), dtype=torch.uint8, device="cuda")
            B.fill_splitmix(buf, buf.shape[1])
            offs, pos = [], 1
            for s in ss:
                offs.append(pos)
                pos += L * int(s) + 3
            plan = B.StripePlan(enc, stripes=[(buf.data_ptr() + o, int(s)) for o, s in zip(offs, ss)])
            keep = [buf]
        else:
            data = torch.empty((1, int(k * ss.sum()) + 16), dtype=torch.uint8, device="cuda")
            B.fill_splitmix(data, data.shape[1])
            par = torch.empty(int(m * ss.sum()) + 16, dtype=torch.uint8, device="cuda")
            items, do, po = [], 1, 3
            for s in ss:
                items.append((data.data_ptr() + do, par.data_ptr() + po, int(s)))
                do += k * int(s)
                po += m * int(s)
            plan = B.StripePlan(enc, objects=items)
            keep = [data, par]
        plan.encode()
        torch.cuda.synchronize()
        flags = torch.zeros(n, dtype=torch.int32, device="cuda")
        pflags = torch.zeros(n, dtype=torch.int32, device="cuda")
        for name, idx in runs.items():
            lost = lost_of[idx]
            v_args = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0], idx.ctypes.data_as(U32P),
                      C.c_void_p(flags.data_ptr()), stream)
            r_args = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0], idx.ctypes.data_as(U32P), 0,
                      stream)
            # a stripe with exactly k present is not read at all
            v_bytes = int((np.where(lost < m, L - lost, 0) * ss).sum())
            legs = {"v": (lambda a=v_args: RS.check(lib.hbec_verify_plan_mixed(*a)), v_bytes)}
            if name != "all_present":
                legs["r"] = (lambda a=r_args: RS.check(lib.hbec_reconstruct_plan_mixed(*a)), int(((k + lost) * ss).sum()))
            else:
                legs["p"] = (lambda: plan.verify(pflags), int((L * ss).sum()))
            flags.zero_()
            ms = measure(legs, rounds)
            s0 = B.verify_mixed_plan_stats()
            legs["v"][0]()
            s1 = B.verify_mixed_plan_stats()
            torch.cuda.synchronize()
            # the codewords are clean: bit 1 exactly where m shards are lost, nothing else
            got = flags.cpu().numpy()
            assert np.array_equal(got, np.where(lost == m, 2, 0)), "flags of the new call are wrong"
            assert int(pflags.count_nonzero()) == 0
            med = {q: statistics.median(v) for q, v in ms.items()}
            spread = {q: (max(v) - min(v)) / med[q] for q, v in ms.items()}
            other = "p" if name == "all_present" else "r"
            for q, (_, nb) in legs.items():
                gbs = nb / (med[q] * 1e-3) / 1e9
                d = {"shape": shape, "layout": layout, "run": name, "leg": q, "ms": round(med[q], 5),
                     "ms_min": round(min(ms[q]), 5), "ms_max": round(max(ms[q]), 5), "spread": round(spread[q], 4),
                     "rounds": rounds, "reps": REPS, "algorithmic_bytes": nb, "GB_s": round(gbs, 1),
                     "frac_of_8TBs": round(gbs / PEAK, 4)}
                if q == "v":
                    d["launches_per_call"] = s1["kernel_launches"] - s0["kernel_launches"]
                    d["per_stripe_calls"] = s1["per_stripe_calls"] - s0["per_stripe_calls"]
                    d[f"time_ratio_v_over_{other}"] = round(med["v"] / med[other], 3)
                    if other == "r":
                        d["slower_than_r_beyond_spread"] = bool(
                            med["v"] > med["r"] * (1 + max(spread["v"], spread["r"])))
                emit(d)
        del plan, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "verify_mixed_plan.jsonl"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shape", default=None, choices=["4+2", "8+3"])
    ap.add_argument("--objects", type=int, default=4096)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(a.out, "w") as out:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for k, m in ((4, 2), (8, 3)):
            if a.shape in (None, f"{k}+{m}"):
                run(k, m, a.objects, a.rounds, emit)


if __name__ == "__main__":
    main()
