#!/usr/bin/env python3
"""The locate pass of a repair sweep (hbec_locate_plan_mixed) against the
degraded Verify it follows (hbec_verify_plan_mixed, the yardstick: same masks,
same buffers, same run), at 4+2 and 8+3.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
as a stripe plan (databufs at odd offsets) and as an object plan (data arena +
parity arena).  Masks: 4+2 every shard present (two checked shards, the fewest
that can name a shard); 8+3 drawn uniformly from all present and the 11 single
losses (three and two checked).  Three states of the same buffers, one after the
other, and in each the legs interleaved:

  clean      v   verify_mixed
             l   locate, d_flags = NULL: detect and locate in one pass
             z   locate filtered by all-zero flags: the cost of the list walk
  one_pct    v   verify_mixed (1 % of the stripes have one flipped byte)
             f   locate filtered by the flags v wrote: reads the flagged 1 %
             l   locate, d_flags = NULL
  all_bad    v   verify_mixed (every stripe has one flipped byte)
             f   locate filtered by v's flags (all set)
             l   locate, d_flags = NULL

Method: a warm-up, then `rounds` rounds in which the legs run in
alternating order, each timed by HIP events around `reps` back-to-back calls
(the calls' host side is inside the bracket); medians, with the smallest and
largest round and their spread (max - min) / median beside them.  Every locate
leg carries its time ratio to v of the same state.  Rates are over the bytes a
leg must read: every present shard of every examined stripe.  Nothing is gated.
After each state the words are decoded and must name exactly the flipped shards.

    python scripts/bench_locate.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N]
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
    if m >= 3:
        masks += [[0 if i == j else 1 for i in range(L)] for j in range(L)]
    pats = np.ascontiguousarray(masks, np.uint8)
    idx = np.ascontiguousarray(rng.integers(0, len(masks), n), np.uint32)
    present = pats[idx]
    lens = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = np.array([-(-x // k) for x in lens], np.int64)
    stripe_bytes = present.sum(axis=1).astype(np.int64) * ss
    shape = f"{k}+{m} {n} objects"
    # the flips: one byte of one present shard per stripe, the 1 % first
    order = rng.permutation(n)
    hit_shard = np.array([int(rng.choice(np.nonzero(present[i])[0])) for i in range(n)], np.int64)
    hit_pos = np.array([int(rng.integers(s)) for s in ss], np.int64)
    states = {"clean": order[:0], "one_pct": order[:max(1, n // 100)], "all_bad": order}

    for layout in ("stripes", "objects"):
        if layout == "stripes":
            buf = torch.empty((1, int(L * ss.sum()) + 3 * n + 16), dtype=torch.uint8, device="cuda")
            B.fill_splitmix(buf, buf.shape[1])
            offs, pos = [], 1
            for s in ss:
                offs.append(pos)
                pos += L * int(s) + 3
            plan = B.StripePlan(enc, stripes=[(buf.data_ptr() + o, int(s)) for o, s in zip(offs, ss)])
            where_of = [(buf.view(-1), np.array(offs, np.int64) + hit_shard * ss + hit_pos, np.ones(n, bool))]
            keep = [buf]
        else:
            data = torch.empty((1, int(k * ss.sum()) + 16), dtype=torch.uint8, device="cuda")
            B.fill_splitmix(data, data.shape[1])
            par = torch.empty(int(m * ss.sum()) + 16, dtype=torch.uint8, device="cuda")
            items, do, po, dos, pos_ = [], 1, 3, [], []
            for s in ss:
                items.append((data.data_ptr() + do, par.data_ptr() + po, int(s)))
                dos.append(do)
                pos_.append(po)
                do += k * int(s)
                po += m * int(s)
            plan = B.StripePlan(enc, objects=items)
            in_data = hit_shard < k
            where_of = [(data.view(-1), np.array(dos, np.int64) + hit_shard * ss + hit_pos, in_data),
                        (par, np.array(pos_, np.int64) + (hit_shard - k) * ss + hit_pos, ~in_data)]
            keep = [data, par]
        plan.encode()
        torch.cuda.synchronize()
        flags = torch.zeros(n, dtype=torch.int32, device="cuda")
        zero_flags = torch.zeros(n, dtype=torch.int32, device="cuda")
        where = torch.zeros(n, dtype=torch.int32, device="cuda")
        common = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0], idx.ctypes.data_as(U32P))
        v_args = common + (C.c_void_p(flags.data_ptr()), stream)

        def loc(f):
            a = common + (None if f is None else C.c_void_p(f.data_ptr()), C.c_void_p(where.data_ptr()), stream)
            return lambda: RS.check(lib.hbec_locate_plan_mixed(*a))

        done = np.zeros(n, bool)
        for name, chosen in states.items():
            todo = np.array([i for i in chosen if not done[i]], np.int64)
            for t, addr, sel in where_of:  # flip the stripes this state adds
                at = todo[sel[todo]] if todo.size else todo
                if at.size:
                    t[torch.from_numpy(addr[at]).cuda()] ^= 0x5A
            done[todo] = True
            flags.zero_()
            RS.check(lib.hbec_verify_plan_mixed(*v_args))
            torch.cuda.synchronize()
            assert np.array_equal(flags.cpu().numpy() & 1, done.astype(np.int32)), "verify_mixed flags are wrong"
            all_bytes, bad_bytes = int(stripe_bytes.sum()), int(stripe_bytes[done].sum())
            legs = {"v": (lambda: RS.check(lib.hbec_verify_plan_mixed(*v_args)), all_bytes),
                    "l": (loc(None), all_bytes)}
            if name == "clean":
                legs["z"] = (loc(zero_flags), 0)
            else:
                legs["f"] = (loc(flags), bad_bytes)
            ms = measure(legs, rounds)
            # what the words say: exactly the flipped shards
            for q in ("l", "f"):
                if q not in legs:
                    continue
                where.zero_()
                s0 = B.locate_plan_stats()
                legs[q][0]()
                s1 = B.locate_plan_stats()
                torch.cuda.synchronize()
                named = B.locate_decode(k, m, present, where.cpu().numpy())
                assert np.array_equal(named, np.where(done, hit_shard, N.LOC_CLEAN)), f"leg {q} names wrong shards"
                assert s1["kernel_launches"] - s0["kernel_launches"] == 1 and s1["skipped_entries"] == s0["skipped_entries"]
            med = {q: statistics.median(v) for q, v in ms.items()}
            spread = {q: (max(v) - min(v)) / med[q] for q, v in ms.items()}
            for q, (_, nb) in legs.items():
                gbs = nb / (med[q] * 1e-3) / 1e9
                d = {"shape": shape, "layout": layout, "state": name, "bad_stripes": int(done.sum()), "leg": q,
                     "ms": round(med[q], 5), "ms_min": round(min(ms[q]), 5), "ms_max": round(max(ms[q]), 5),
                     "spread": round(spread[q], 4), "rounds": rounds, "reps": REPS, "read_bytes": nb,
                     "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK, 4)}
                if q != "v":
                    d["time_ratio_over_v"] = round(med[q] / med["v"], 3)
                    d["beyond_spread"] = bool(abs(med[q] - med["v"]) > med["v"] * max(spread[q], spread["v"]))
                emit(d)
        del plan, keep, where_of


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "locate_plan.jsonl"))
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
