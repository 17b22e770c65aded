#!/usr/bin/env python3
"""The object bytes of a plan's entries in one call (hbec_glue_plan_mixed)
against what a caller had to do without it, at 4+2 and 8+3.

Workload: that of scripts/bench_mixed_plan.py, 4096 objects of random odd sizes,
4 KiB to 1 MiB (S = ceil(len / k)), databufs at odd offsets, encoded.  Every
object is glued whole (its own length, so the last data shard is cut by up to
k - 1 bytes) into an output arena, objects k S + 3 bytes apart.

Mask sets: `healthy` (every shard present), `one_data` (one data shard lost per
entry, drawn uniformly), `single_double` (drawn uniformly from all single and
double losses, as bench_mixed_plan.py draws them).

Arms, the same bytes each:

  a        hbec_glue_plan_mixed on a stripe plan over the databufs
  a_again  the same call on a second plan over the same databufs: a against
           itself, whose spread in this run is the margin the others are read with
  b        what a caller does without the call: a shards plan whose missing data
           shards point into the output arena (built outside the bracket, as it
           is rebuilt only when the masks change), hbec_reconstruct_plan_mixed
           (data_only) on it, and one device-to-device hipMemcpyAsync per present
           data shard per stripe (inside the bracket).  Its rebuilt shards are
           written whole, so it writes up to k - 1 bytes past the object: the
           arena's spacing leaves room for that
  c        hbec_reconstruct_plan_mixed (data_only) alone on a's plan with the same
           masks, for scale: it writes e S bytes per entry where a writes k S

Method: a warm-up, then `rounds` rounds in which the arms run in
alternating order, each timed by HIP events around `reps` back-to-back calls of
the C entry points (masks matched to pattern rows once, outside the bracket);
medians, min and max.  The rate of a is over 2 k S bytes per entry, read and
written.

    python scripts/bench_glue.py [--out FILE] [--rounds N] [--reps N] [--shape 4+2|8+3] [--objects N]
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
U64P = C.POINTER(C.c_uint64)
D2D = 3  # hipMemcpyDeviceToDevice


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(k, m, n, rounds, reps, emit):
    enc = RS.New(k, m)
    L = k + m
    rng = np.random.default_rng(100 * k + m)
    lens = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = [-(-x // k) for x in lens]
    total = L * sum(ss)
    shape = f"{k}+{m} {n} objects"

    buf = torch.empty((1, total + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, buf.shape[1])
    offs, pos = [], 1
    for s in ss:
        offs.append(pos)
        pos += L * s + 3
    stripes = [(buf.data_ptr() + o, s) for o, s in zip(offs, ss)]
    plan_a, plan_a2 = B.StripePlan(enc, stripes=stripes), B.StripePlan(enc, stripes=stripes)
    plan_a.encode()
    out = torch.zeros(k * sum(ss) + 3 * n + 16, dtype=torch.uint8, device="cuda")
    outs, pos = [], 1
    for s in ss:
        outs.append(pos)
        pos += k * s + 3
    torch.cuda.synchronize()

    lib = N.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dsts = (C.c_void_p * n)(*[out.data_ptr() + o for o in outs])
    dlens = np.ascontiguousarray(lens, np.uint64)

    singles = [[0 if i in lost else 1 for i in range(L)] for c in (1, 2) for lost in itertools.combinations(range(L), c)]
    one = rng.integers(0, k, n)
    sets = {
        "healthy": np.ones((n, L), np.uint8),
        "one_data": np.array([[0 if i == one[e] else 1 for i in range(L)] for e in range(n)], np.uint8),
        "single_double": np.ascontiguousarray(np.array(singles, np.uint8)[rng.integers(0, len(singles), n)]),
    }
    for name, present in sets.items():
        pats, pat_of = np.unique(present, axis=0, return_inverse=True)
        pats = np.ascontiguousarray(pats, np.uint8)
        pat_of = np.ascontiguousarray(pat_of.reshape(-1), np.uint32)
        pp, po, npat = pats.ctypes.data_as(N._U8P), pat_of.ctypes.data_as(U32P), pats.shape[0]
        # b: the plan a caller builds when the masks change, and the copies it issues per call
        rows, copies = [], []
        for e in range(n):
            row = [buf.data_ptr() + offs[e] + j * ss[e] for j in range(L)]
            for j in range(k):
                if present[e][j]:
                    v = min(ss[e], lens[e] - j * ss[e])
                    if v > 0:
                        copies.append((out.data_ptr() + outs[e] + j * ss[e], row[j], v))
                else:
                    row[j] = out.data_ptr() + outs[e] + j * ss[e]
            rows.append((row, ss[e]))
        plan_b = B.StripePlan(enc, shards=rows)
        failed = []

        def glue(p):
            return lambda: RS.check(lib.hbec_glue_plan_mixed(enc.handle, p._h, pp, npat, po, dsts,
                                                             dlens.ctypes.data_as(U64P), stream))

        def by_hand():
            RS.check(lib.hbec_reconstruct_plan_mixed(enc.handle, plan_b._h, pp, npat, po, 1, stream))
            for d, s, v in copies:
                rc = hip.hipMemcpyAsync(d, s, v, D2D, stream)
                if rc:
                    failed.append(rc)

        legs = {"a": glue(plan_a), "a_again": glue(plan_a2), "b": by_hand,
                "c": lambda: RS.check(lib.hbec_reconstruct_plan_mixed(enc.handle, plan_a._h, pp, npat, po, 1, stream))}
        # each arm writes the objects: checked once against the databufs' data shards
        for arm in ("a", "b"):
            out.zero_()
            legs[arm]()
            torch.cuda.synchronize()
            for e in range(0, n, max(1, n // 64)):
                want = buf[0, offs[e]:offs[e] + lens[e]]
                assert torch.equal(out[outs[e]:outs[e] + lens[e]], want), (name, arm, e)
        assert not failed, failed[:4]
        for fn in legs.values():
            for _ in range(2):
                fn()
        ms = {arm: [] for arm in legs}
        names = list(legs)
        for r in range(rounds):
            for arm in (names if r % 2 == 0 else names[::-1]):
                ms[arm].append(timed(legs[arm], reps))
        assert not failed, failed[:4]
        med = {arm: statistics.median(v) for arm, v in ms.items()}
        moved = 2 * k * sum(ss)
        spread = max(med["a_again"] / med["a"], med["a"] / med["a_again"])
        for arm in legs:
            d = {"shape": shape, "masks": name, "arm": arm, "ms": round(med[arm], 5),
                 "ms_min": round(min(ms[arm]), 5), "ms_max": round(max(ms[arm]), 5), "rounds": rounds, "reps": reps,
                 "patterns": int(npat)}
            if arm in ("a", "a_again"):
                gbs = moved / (med[arm] * 1e-3) / 1e9
                d.update({"bytes_2kS": moved, "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK, 4)})
            if arm == "b":
                d["copies_per_call"] = len(copies)
            emit(d)
        emit({"shape": shape, "masks": name, "arm": "ratios", "a_again_over_a": round(med["a_again"] / med["a"], 4),
              "spread": round(spread, 4), "a_over_b": round(med["a"] / med["b"], 4),
              "a_over_c": None if name == "healthy" else round(med["a"] / med["c"], 4),  # healthy: c launches nothing
              "a_not_slower_than_b_within_spread": bool(med["a"] <= med["b"] * spread)})
        del plan_b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", default=None, choices=["4+2", "8+3"])
    ap.add_argument("--objects", type=int, default=4096)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    torch.cuda.set_device(0)
    for shape in [s for s in ("4+2", "8+3") if a.shape in (None, s)]:
        k, m = map(int, shape.split("+"))
        run(k, m, a.objects, a.rounds, a.reps, emit)


if __name__ == "__main__":
    main()
