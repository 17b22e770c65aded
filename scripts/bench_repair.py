#!/usr/bin/env python3
"""Rebuild the missing shards of a repair sweep and check its surplus shards in
one pass (hbec_repair_plan_mixed), against the pair of calls it replaces, at 4+2
and 8+3.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
as a stripe plan (databufs at odd offsets) and as an object plan (data arena +
parity arena).  Three mask sets per layout: `single_loss`, a mask per stripe
drawn uniformly from the single losses; `single_double`, from all single and
double losses (at 4+2 a double loss leaves exactly k shards: nothing to check);
and `all_present`.  Legs, all in one run on the same buffers:

  p    hbec_repair_plan_mixed: the new call
  vr   hbec_verify_plan_mixed then hbec_reconstruct_plan_mixed, timed as a pair:
       what a caller pays today for the same result
  v    hbec_verify_plan_mixed alone
  r    hbec_reconstruct_plan_mixed alone

Method: a warm-up, then `rounds` rounds in which the legs run in
alternating order, each timed by HIP events around `reps` back-to-back calls
(the calls' host side is inside the bracket); medians, with the smallest and
largest round and their spread (max - min) / median beside them.  `host_ms` is
the wall time the caller spends inside one call (queueing only, nothing waited
for), `host_share` its part of the leg's time.  Rates are over the algorithmic
bytes of each leg; p's are (k + checked + rebuilt) S per stripe.  Nothing is
gated: the p line carries its time ratios to vr, r and v and whether it beats the
pair by more than the larger of the two legs' spreads (mask sets with something
to rebuild) or stays within the spread of v (all present).

After the timing the lost shards of every stripe are overwritten with garbage
and one p call is checked: every flag against what clean codewords must give,
and the rebuilt shards of a sample of stripes against the oracle
(coracle.apply of lagrange_row on the survivors' bytes).

    python scripts/bench_repair.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N]
"""
from __future__ import annotations

import argparse
import ctypes as C
import itertools
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from hummingbird_amd import _native as N  # noqa: E402
from hummingbird_amd import batch as B  # noqa: E402
from hummingbird_amd import reedsolomon as RS  # noqa: E402
from oracle import coracle as CO  # noqa: E402
from oracle import lagrange as LG  # noqa: E402

PEAK = 8000.0
U32P = C.POINTER(C.c_uint32)
REPS = 20
SAMPLE = 24


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_time(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) * 1e3 / reps


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


def check_against_oracle(k, m, plan_call, flags, shard_addr, ss, pats, idx, lost, rng):
    """Garbage into every lost shard, one p call, then the flags of all stripes
    and the rebuilt shards of SAMPLE stripes against the oracle."""
    L = k + m
    sample = rng.choice(len(ss), size=min(SAMPLE, len(ss)), replace=False)
    survivors = {}
    for e in range(len(ss)):
        for i in np.nonzero(pats[idx[e]] == 0)[0]:
            shard_addr(e, int(i)).random_(0, 256)
    for e in sample:
        here = [i for i in range(L) if pats[idx[e]][i]]
        survivors[int(e)] = (here[:k], [shard_addr(int(e), i).cpu().numpy().copy() for i in here[:k]])
    flags.zero_()
    torch.cuda.synchronize()
    plan_call()
    torch.cuda.synchronize()
    got = flags.cpu().numpy()
    assert np.array_equal(got, np.where(lost == m, 2, 0)), "flags of the new call are wrong"
    n_checked = 0
    for e, (surv, data) in survivors.items():
        gone = [i for i in range(L) if not pats[idx[e]][i]]
        if not gone:
            continue
        want = CO.apply([LG.lagrange_row(surv, g) for g in gone], data)
        for g, w in zip(gone, want):
            assert np.array_equal(shard_addr(e, g).cpu().numpy(), w), f"stripe {e} shard {g} rebuilt wrong"
            n_checked += 1
    return n_checked


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
    runs = {"single_loss": np.ascontiguousarray(rng.integers(1, L + 1, n), np.uint32),
            "single_double": np.ascontiguousarray(rng.integers(1, len(masks), n), np.uint32),
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
            flat = buf.view(-1)

            def shard_addr(e, i, flat=flat, offs=offs):
                s = int(ss[e])
                return flat[offs[e] + i * s:offs[e] + (i + 1) * s]
            keep = [buf]
        else:
            data = torch.empty((1, int(k * ss.sum()) + 16), dtype=torch.uint8, device="cuda")
            B.fill_splitmix(data, data.shape[1])
            par = torch.empty(int(m * ss.sum()) + 16, dtype=torch.uint8, device="cuda")
            items, where, do, po = [], [], 1, 3
            for s in ss:
                items.append((data.data_ptr() + do, par.data_ptr() + po, int(s)))
                where.append((do, po))
                do += k * int(s)
                po += m * int(s)
            plan = B.StripePlan(enc, objects=items)
            dflat = data.view(-1)

            def shard_addr(e, i, dflat=dflat, par=par, where=where):
                s = int(ss[e])
                do, po = where[e]
                return dflat[do + i * s:do + (i + 1) * s] if i < k else par[po + (i - k) * s:po + (i - k + 1) * s]
            keep = [data, par]
        plan.encode()
        torch.cuda.synchronize()
        flags = torch.zeros(n, dtype=torch.int32, device="cuda")
        vflags = torch.zeros(n, dtype=torch.int32, device="cuda")
        for name, idx in runs.items():
            lost = lost_of[idx]
            head = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0], idx.ctypes.data_as(U32P))
            p_args = head + (0, C.c_void_p(flags.data_ptr()), stream)
            v_args = head + (C.c_void_p(vflags.data_ptr()), stream)
            r_args = head + (0, stream)

            def p(a=p_args):
                RS.check(lib.hbec_repair_plan_mixed(*a))

            def v(a=v_args):
                RS.check(lib.hbec_verify_plan_mixed(*a))

            def r(a=r_args):
                RS.check(lib.hbec_reconstruct_plan_mixed(*a))

            def vr():
                v()
                r()

            # a stripe with exactly k present is not read by v; one with nothing lost not by r
            v_bytes = int((np.where(lost < m, L - lost, 0) * ss).sum())
            r_bytes = int((np.where(lost > 0, k + lost, 0) * ss).sum())
            p_bytes = int((L * ss).sum())  # k + (m - lost) checked + lost rebuilt
            legs = {"p": (p, p_bytes), "vr": (vr, v_bytes + r_bytes), "v": (v, v_bytes)}
            if name != "all_present":
                legs["r"] = (r, r_bytes)
            flags.zero_()
            vflags.zero_()
            ms = measure(legs, rounds)
            host = {q: host_time(fn, REPS) for q, (fn, _) in legs.items()}
            s0 = B.repair_plan_stats()
            p()
            s1 = B.repair_plan_stats()
            torch.cuda.synchronize()
            rebuilt_checked = check_against_oracle(k, m, p, flags, shard_addr, ss, pats, idx, lost, rng)
            assert np.array_equal(vflags.cpu().numpy(), np.where(lost == m, 2, 0))
            med = {q: statistics.median(x) for q, x in ms.items()}
            spread = {q: (max(x) - min(x)) / med[q] for q, x in ms.items()}
            for q, (_, nb) in legs.items():
                gbs = nb / (med[q] * 1e-3) / 1e9
                d = {"shape": shape, "layout": layout, "run": name, "leg": q, "ms": round(med[q], 5),
                     "ms_min": round(min(ms[q]), 5), "ms_max": round(max(ms[q]), 5), "spread": round(spread[q], 4),
                     "rounds": rounds, "reps": REPS, "host_ms": round(host[q], 5),
                     "host_share": round(host[q] / med[q], 4), "algorithmic_bytes": nb, "GB_s": round(gbs, 1),
                     "frac_of_8TBs": round(gbs / PEAK, 4)}
                if q == "p":
                    d["launches_per_call"] = s1["kernel_launches"] - s0["kernel_launches"]
                    d["per_stripe_calls"] = s1["per_stripe_calls"] - s0["per_stripe_calls"]
                    d["time_ratio_p_over_vr"] = round(med["p"] / med["vr"], 3)
                    d["time_ratio_p_over_v"] = round(med["p"] / med["v"], 3)
                    d["rebuilt_shards_checked"] = rebuilt_checked
                    if name != "all_present":
                        d["time_ratio_p_over_r"] = round(med["p"] / med["r"], 3)
                        d["faster_than_vr_beyond_spread"] = bool(
                            med["p"] < med["vr"] * (1 - max(spread["p"], spread["vr"])))
                    else:
                        d["within_spread_of_v"] = bool(
                            abs(med["p"] - med["v"]) <= med["v"] * max(spread["p"], spread["v"]))
                emit(d)
        del plan, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "repair_plan.jsonl"))
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
