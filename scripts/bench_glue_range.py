#!/usr/bin/env python3
"""Any byte range of a plan's entries in one call (hbec_glue_plan_range) against
what a caller had to do without it, at 4+2 and 8+3.

Workload: 4096 entries of S = 256 KiB plus an odd remainder (1..127 bytes),
databufs at odd offsets, encoded.  Mask sets: `healthy` (every shard present),
`one_data` (one data shard lost per entry, drawn uniformly), `single_double`
(drawn uniformly from all single and double losses).  Range sets, per entry of
D = k S bytes: `r64k` 64 KiB at a random odd start, `half2` the second half
[k S / 2, k S), `whole` [0, k S).

Arms, the same bytes each:

  a        hbec_glue_plan_range on a stripe plan over the databufs
  a_again  the same call on a second plan over the same databufs: a against
           itself, whose spread in this run is the margin the others are read with
  b        what a caller does without the call: hbec_glue_plan_mixed of the prefix
           [0, start + len) of every entry into a scratch arena, then one
           device-to-device hipMemcpyAsync of the slice per entry
  c        hbec_glue_plan_mixed of whole entries, for scale
  d        (r64k only) hbec_glue_plan_range on a shards plan that holds nothing but
           the wanted shard positions: per entry one sub-entry of the positions
           [lo, hi) of every shard when the range lies in one data shard, two (the
           end of the shards and their beginning) when it straddles a junction.
           GF coding is bytewise, so such a sub-entry is a codeword.  a - d is what
           a pays to walk past the tiles it does not touch

Method: a warm-up, then `rounds` rounds in which the arms run in
alternating order, each timed by HIP events around `reps` back-to-back calls of
the C entry points (masks matched to pattern rows once, outside the bracket);
medians, min and max.

    python scripts/bench_glue_range.py [--out FILE] [--rounds N] [--reps N] [--shape 4+2|8+3] [--objects N]
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


def u64(a):
    return np.ascontiguousarray(a, np.uint64)


def run(k, m, n, rounds, reps, emit):
    enc = RS.New(k, m)
    L = k + m
    rng = np.random.default_rng(300 * k + m)
    ss = [(256 << 10) + (int(x) | 1) for x in rng.integers(0, 127, n)]
    shape = f"{k}+{m} {n} entries"

    buf = torch.empty((1, L * sum(ss) + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, buf.shape[1])
    offs, pos = [], 1
    for s in ss:
        offs.append(pos)
        pos += L * s + 3
    stripes = [(buf.data_ptr() + o, s) for o, s in zip(offs, ss)]
    plan_a, plan_a2 = B.StripePlan(enc, stripes=stripes), B.StripePlan(enc, stripes=stripes)
    plan_a.encode()
    arena = k * sum(ss) + 3 * n + 16
    out = torch.zeros(arena, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(arena, dtype=torch.uint8, device="cuda")
    at, pos = [], 1
    for s in ss:
        at.append(pos)
        pos += k * s + 3
    torch.cuda.synchronize()

    lib = N.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dsts = (C.c_void_p * n)(*[out.data_ptr() + o for o in at])
    tmps = (C.c_void_p * n)(*[scratch.data_ptr() + o for o in at])
    whole = u64([k * s for s in ss])

    losses = [[0 if i in lost else 1 for i in range(L)] for c in (1, 2) for lost in itertools.combinations(range(L), c)]
    one = rng.integers(0, k, n)
    mask_sets = {
        "healthy": np.ones((n, L), np.uint8),
        "one_data": np.array([[0 if i == one[e] else 1 for i in range(L)] for e in range(n)], np.uint8),
        "single_double": np.ascontiguousarray(np.array(losses, np.uint8)[rng.integers(0, len(losses), n)]),
    }
    r64 = [int(x) | 1 for x in rng.integers(0, k * min(ss) - (64 << 10) - 1, n)]
    range_sets = {
        "r64k": (r64, [64 << 10] * n),
        "half2": ([k * s // 2 for s in ss], [k * s - k * s // 2 for s in ss]),
        "whole": ([0] * n, [k * s for s in ss]),
    }
    for (mname, present), (rname, (starts, lens)) in itertools.product(mask_sets.items(), range_sets.items()):
        pats, pat_of = np.unique(present, axis=0, return_inverse=True)
        pats = np.ascontiguousarray(pats, np.uint8)
        pat_of = np.ascontiguousarray(pat_of.reshape(-1), np.uint32)
        pp, po, npat = pats.ctypes.data_as(N._U8P), pat_of.ctypes.data_as(U32P), pats.shape[0]
        st, ln = u64(starts), u64(lens)
        pre = u64([a + b for a, b in zip(starts, lens)])
        copies = [(out.data_ptr() + at[e], scratch.data_ptr() + at[e] + starts[e], lens[e]) for e in range(n)]
        failed = []

        def ranged(p, d=dsts, s=st, l_=ln, q=po):
            return lambda: RS.check(lib.hbec_glue_plan_range(enc.handle, p._h, pp, npat, q, d, s.ctypes.data_as(U64P),
                                                             l_.ctypes.data_as(U64P), stream))

        def by_hand():
            RS.check(lib.hbec_glue_plan_mixed(enc.handle, plan_a._h, pp, npat, po, tmps, pre.ctypes.data_as(U64P),
                                              stream))
            for d, s, v in copies:
                rc = hip.hipMemcpyAsync(d, s, v, D2D, stream)
                if rc:
                    failed.append(rc)

        legs = {"a": ranged(plan_a), "a_again": ranged(plan_a2), "b": by_hand,
                "c": lambda: RS.check(lib.hbec_glue_plan_mixed(enc.handle, plan_a._h, pp, npat, po, dsts,
                                                               whole.ctypes.data_as(U64P), stream))}
        plan_d = None
        if rname == "r64k":  # the wanted shard positions alone, as sub-entries
            rows, d_dst, d_st, d_ln, d_of = [], [], [], [], []
            for e in range(n):
                s, a, b = ss[e], starts[e], starts[e] + lens[e]
                j0, j1 = a // s, (b - 1) // s
                parts = [(j0, a - j0 * s, b - j0 * s, 0)] if j0 == j1 else \
                    [(j0, a - j0 * s, s, 0), (j1, 0, b - j1 * s, s - (a - j0 * s))]
                for j, lo, hi, skip in parts:
                    rows.append(([buf.data_ptr() + offs[e] + i * s + lo for i in range(L)], hi - lo))
                    d_dst.append(out.data_ptr() + at[e] + skip)
                    d_st.append(j * (hi - lo))
                    d_ln.append(hi - lo)
                    d_of.append(pat_of[e])
            plan_d = B.StripePlan(enc, shards=rows)
            legs["d"] = ranged(plan_d, (C.c_void_p * len(rows))(*d_dst), u64(d_st), u64(d_ln),
                               np.ascontiguousarray(d_of, np.uint32).ctypes.data_as(U32P))
        # each arm writes the ranges: checked once against the databufs' data shards
        for arm in [x for x in legs if x != "c"]:
            out.zero_()
            legs[arm]()
            torch.cuda.synchronize()
            for e in range(0, n, max(1, n // 64)):
                want = buf[0, offs[e] + starts[e]:offs[e] + starts[e] + lens[e]]
                assert torch.equal(out[at[e]:at[e] + lens[e]], want), (mname, rname, arm, e)
                assert int(out[at[e] + lens[e]]) == 0, (mname, rname, arm, e)
        assert not failed, failed[:4]
        for fn in legs.values():
            fn()
        ms = {arm: [] for arm in legs}
        names = list(legs)
        for r in range(rounds):
            for arm in (names if r % 2 == 0 else names[::-1]):
                ms[arm].append(timed(legs[arm], reps))
        assert not failed, failed[:4]
        med = {arm: statistics.median(v) for arm, v in ms.items()}
        wanted = int(sum(lens))
        spread = max(med["a_again"] / med["a"], med["a"] / med["a_again"])
        for arm in legs:
            d = {"shape": shape, "masks": mname, "ranges": rname, "arm": arm, "ms": round(med[arm], 5),
                 "ms_min": round(min(ms[arm]), 5), "ms_max": round(max(ms[arm]), 5), "rounds": rounds, "reps": reps,
                 "patterns": int(npat)}
            if arm in ("a", "a_again", "d"):
                d.update({"bytes_wanted": wanted, "GB_s_wanted_x2": round(2 * wanted / (med[arm] * 1e-3) / 1e9, 1)})
            if arm == "b":
                d["copies_per_call"] = len(copies)
            emit(d)
        emit({"shape": shape, "masks": mname, "ranges": rname, "arm": "ratios",
              "a_again_over_a": round(med["a_again"] / med["a"], 4), "spread": round(spread, 4),
              "a_over_b": round(med["a"] / med["b"], 4), "a_over_c": round(med["a"] / med["c"], 4),
              "a_beats_b_by_more_than_spread": bool(med["a"] * spread < med["b"]),
              "a_minus_d_over_a": round((med["a"] - med["d"]) / med["a"], 4) if "d" in med else None})
        del plan_d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
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
