#!/usr/bin/env python3
"""Reconstruct of a repair sweep that is mixed in both size and erasure
pattern, in one call (hbec_reconstruct_plan_mixed), against what a caller
could do before, at 4+2 and 8+3.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
as a stripe plan (databufs at odd offsets) and as an object plan (data arena +
parity arena); a pattern per stripe drawn uniformly from all single and double
losses.  Legs, per layout:

  a       hbec_reconstruct_plan, one double-loss pattern over all stripes: the ceiling
  b       one plan per distinct pattern and one hbec_reconstruct_plan each: the
          best a caller could do with plans; `b_build` also builds the plans
          inside the bracket
  c       one hbec_reconstruct_batch per stripe (stripe layout only)
  d       hbec_reconstruct_plan_mixed, the random patterns
  e       hbec_reconstruct_plan_mixed, the same patterns sorted into runs
  f_plan / f_batch   (once per shape) 4096 aligned 1 MiB objects with random
          patterns: the new call, and hbec_reconstruct_batch_mixed on the same bytes

Method: a warm-up, then `rounds` rounds in which the legs run in
alternating order, each timed by HIP events around `reps` back-to-back calls
(the calls' host side is inside the bracket); medians.  Rates are over the
algorithmic bytes (k + r_i) S_i of the stripes, r_i the shards rebuilt.  The
host time of a d call (the call returns without waiting) is the wall clock
around the same 20 calls before the device is waited for.

    python scripts/bench_mixed_plan.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N]
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

PEAK = 8000.0
U32P = C.POINTER(C.c_uint32)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t = (time.perf_counter() - t0) * 1e3 / reps
    torch.cuda.synchronize()
    return t


def mixed_call(enc, plan, pats, idx, stream):
    args = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0], idx.ctypes.data_as(U32P), 0, stream)
    f = N.lib().hbec_reconstruct_plan_mixed
    return lambda: RS.check(f(*args))


def measure(legs, rounds):
    for name, (fn, _, reps) in legs.items():
        for _ in range(1 if reps == 1 else 3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    names = list(legs)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            fn, _, reps = legs[name]
            ms[name].append(timed(fn, reps))
    return ms


def run(k, m, n, rounds, emit):
    enc = RS.New(k, m)
    L = k + m
    lib = N.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(100 * k + m)
    masks = []
    for c in (1, 2):
        for lost in itertools.combinations(range(L), c):
            masks.append([0 if i in lost else 1 for i in range(L)])
    pats = np.ascontiguousarray(masks, np.uint8)
    r_of = (L - pats.sum(axis=1)).astype(np.int64)
    idx = np.ascontiguousarray(rng.integers(0, len(masks), n), np.uint32)
    idx_sorted = np.ascontiguousarray(np.sort(idx), np.uint32)
    double = [0, 1] + [1] * (L - 3) + [0]  # a data and a parity shard lost

    lens = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = np.array([-(-x // k) for x in lens], np.int64)
    bytes_d = int(((k + r_of[idx]) * ss).sum())
    bytes_e = int(((k + r_of[idx_sorted]) * ss).sum())
    bytes_a = int(((k + 2) * ss).sum())
    shape = f"{k}+{m} {n} objects"
    results = {}

    for layout in ("stripes", "objects"):
        if layout == "stripes":
            buf = torch.empty((1, int(L * ss.sum()) + 3 * n + 16), dtype=torch.uint8, device="cuda")
            B.fill_splitmix(buf, buf.shape[1])
            offs, pos = [], 1
            for s in ss:
                offs.append(pos)
                pos += L * int(s) + 3
            items = [(buf.data_ptr() + o, int(s)) for o, s in zip(offs, ss)]
            mk = lambda sub: B.StripePlan(enc, stripes=sub)  # noqa: E731
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
            mk = lambda sub: B.StripePlan(enc, objects=sub)  # noqa: E731
            keep = [data, par]
        plan = mk(items)
        plan.encode()
        torch.cuda.synchronize()
        groups = [(masks[p], [items[i] for i in np.nonzero(idx == p)[0]]) for p in sorted(set(idx.tolist()))]
        gplans = [(mask, mk(sub)) for mask, sub in groups]

        def leg_b():
            for mask, gp in gplans:
                gp.reconstruct(mask)

        def leg_b_build():
            for mask, sub in groups:
                mk(sub).reconstruct(mask)
            torch.cuda.synchronize()  # the plans are freed on return: their work must be done

        leg_d = mixed_call(enc, plan, pats, idx, stream)
        legs = {
            "a": (lambda: plan.reconstruct(double), bytes_a, 20),
            "b": (leg_b, bytes_d, 20),
            "b_build": (leg_b_build, bytes_d, 1),
            "d": (leg_d, bytes_d, 20),
            "e": (mixed_call(enc, plan, pats, idx_sorted, stream), bytes_e, 20),
        }
        if layout == "stripes":
            c_args = []
            for (base, s), p in zip(items, idx):
                pres = (C.c_uint8 * L)(*masks[p])
                c_args.append((enc.handle, B._views([(base + i * s, 0) for i in range(L)]), pres, 1, s, 0, stream))

            def leg_c():
                f = lib.hbec_reconstruct_batch
                for x in c_args:
                    rc = f(*x)
                    if rc:
                        RS.check(rc)

            legs["c"] = (leg_c, bytes_d, 1)
        ms = measure(legs, rounds)
        host_d = statistics.median(host_ms(leg_d, 20) for _ in range(rounds))
        s0 = B.mixed_plan_stats()
        leg_d()
        s1 = B.mixed_plan_stats()
        flags = torch.zeros(n, dtype=torch.int32, device="cuda")
        plan.verify(flags)
        torch.cuda.synchronize()
        assert int(flags.count_nonzero()) == 0, "a stripe does not verify after the legs"
        med = {name: statistics.median(v) for name, v in ms.items()}
        rate = {name: legs[name][1] / (med[name] * 1e-3) / 1e9 for name in legs}
        for name, (fn, nb, reps) in legs.items():
            d = {"shape": shape, "layout": layout, "leg": name, "ms": round(med[name], 5),
                 "ms_min": round(min(ms[name]), 5), "ms_max": round(max(ms[name]), 5), "rounds": rounds, "reps": reps,
                 "algorithmic_bytes": nb, "GB_s": round(rate[name], 1), "frac_of_8TBs": round(rate[name] / PEAK, 4)}
            if name in ("b", "b_build"):
                d["plans"] = len(gplans)
            if name == "c":
                d["calls_per_rep"] = n
            if name == "d":
                d["launches_per_call"] = s1["kernel_launches"] - s0["kernel_launches"]
                d["per_stripe_calls"] = s1["per_stripe_calls"] - s0["per_stripe_calls"]
                d["host_ms_per_call"] = round(host_d, 5)
                d["host_share"] = round(host_d / med["d"], 4)
                d["rate_ratio_to_a"] = round(rate["d"] / rate["a"], 3)
                d["time_ratio_b_over_d"] = round(med["b"] / med["d"], 3)
                if "c" in med:
                    d["time_ratio_c_over_d"] = round(med["c"] / med["d"], 1)
            emit(d)
        results[layout] = med
        del plan, gplans, groups, legs, keep

    # f: aligned 1 MiB objects, random patterns
    s_eq = (1 << 20) // k
    eq = torch.empty((n, L * s_eq), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(eq, L * s_eq)
    views = B.shard_views(eq, L, s_eq)
    B.encode_views(enc, views, n, s_eq)
    eq_plan = B.StripePlan(enc, stripes=[(eq.data_ptr() + o * L * s_eq, s_eq) for o in range(n)])
    bytes_f = int(((k + r_of[idx]) * s_eq).sum())
    bm_args = (enc.handle, B._views(views), pats.ctypes.data_as(N._U8P), pats.shape[0], idx.ctypes.data_as(U32P), n,
               s_eq, 0, stream)
    legs = {
        "f_plan": (mixed_call(enc, eq_plan, pats, idx, stream), bytes_f, 20),
        "f_batch": (lambda: RS.check(lib.hbec_reconstruct_batch_mixed(*bm_args)), bytes_f, 20),
    }
    ms = measure(legs, rounds)
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, (fn, nb, reps) in legs.items():
        gbs = nb / (med[name] * 1e-3) / 1e9
        emit({"shape": shape, "layout": "aligned 1 MiB stripes", "leg": name, "ms": round(med[name], 5),
              "ms_min": round(min(ms[name]), 5), "ms_max": round(max(ms[name]), 5), "rounds": rounds, "reps": reps,
              "algorithmic_bytes": nb, "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK, 4),
              "time_ratio_to_f_batch": round(med[name] / med["f_batch"], 3)})
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default=None, choices=["4+2", "8+3"])
    ap.add_argument("--objects", type=int, default=4096)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = open(a.out, "a") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    res = {}
    for k, m in ((4, 2), (8, 3)):
        if a.shape in (None, f"{k}+{m}"):
            res[f"{k}+{m}"] = run(k, m, a.objects, a.rounds, emit)
    # what must hold, on both shapes of the same run: d no slower than b (plan
    # builds excluded) and faster than one call per stripe
    for shape, by_layout in res.items():
        for layout, med in by_layout.items():
            assert med["d"] <= med["b"], (shape, layout, med)
            if "c" in med:
                assert med["d"] < med["c"], (shape, layout, med)


if __name__ == "__main__":
    main()
