#!/usr/bin/env python3
"""Chosen shards of a plan's entries from their object bytes in one call
(hbec_split_plan_select) against what a caller had to do without it, at 4+2 and
8+3.

Workload: that of scripts/bench_split.py, 4096 objects of random odd sizes, 4 KiB
to 1 MiB, in a source arena at odd offsets; the shards are those of a databuf
per object at odd offsets in a shard arena, named shard by shard in a shards
plan.  A second arena of the same layout is the scratch of the hand-made routes.

Arms, in four groups, each group's arms writing the same bytes:

  a  all_select    every shard selected
     split         hbec_split_plan, the yardstick
     split_again   the same call on a second plan over the same buffers: the
                   yardstick against itself, whose spread in this run is the
                   margin all_select is read with
  b  one_data      one data shard per object selected (shard e mod k of object e)
     hand_data     hbec_split_plan into the scratch arena, then one
                   device-to-device hipMemcpyAsync per wanted shard
  c  one_parity    one parity shard per object selected (row e mod m)
     hand_parity   the same hand-made route for those shards
  d  parity_inplace  parity alone selected, the source the entry's own data region
     encode        hbec_encode_plan on the same plan

Method: a warm-up that also sizes every arm's window to 6 ms or
more of back-to-back calls, then `rounds` rounds in which the arms run in
alternating order, each window timed by HIP events; medians with the smallest
and largest round.  Bytes read and written per arm are counted from the lengths
and masks, not measured.

    python scripts/bench_split_select.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N] [--groups abcd] [--label TEXT]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
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

U64P = C.POINTER(C.c_uint64)
U32P = C.POINTER(C.c_uint32)
D2D = 3  # hipMemcpyDeviceToDevice
WINDOW_MS = 6.0


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def traffic(k, m, masks, lens, ss):
    """Bytes the select kernel reads and writes: every needed input's bytes of the
    piece once (csrc/splitselect.h ss_needed_inputs), every selected shard whole."""
    rd = wr = 0
    for mk, ln, s in zip(masks, lens, ss):
        coded = bool(mk[k:].any())
        for j in range(k):
            v = max(0, min(s, ln - j * s))
            if mk[j] or (coded and v):
                rd += v
        wr += int(mk.sum()) * s
    return rd, wr


def run(k, m, n, rounds, only, emit):
    enc = RS.New(k, m)
    L = k + m
    rng = np.random.default_rng(100 * k + m)
    lens = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = [-(-x // k) for x in lens]
    shape = f"{k}+{m} {n} objects"

    src = torch.empty((1, sum(lens) + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(src, src.shape[1])
    src_at, pos = [], 1
    for ln in lens:
        src_at.append(pos)
        pos += ln + 3
    arena = L * sum(ss) + 3 * n + 16
    buf = torch.zeros(arena, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(arena, dtype=torch.uint8, device="cuda")
    offs, pos = [], 1
    for s in ss:
        offs.append(pos)
        pos += L * s + 3

    def rows(t):
        return [([t.data_ptr() + o + j * s for j in range(L)], s) for o, s in zip(offs, ss)]

    plan, plan2, plan_scratch = (B.StripePlan(enc, shards=rows(t)) for t in (buf, buf, scratch))
    torch.cuda.synchronize()

    lib = N.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    srcs = (C.c_void_p * n)(*[src.data_ptr() + o for o in src_at])
    in_place = (C.c_void_p * n)(*[buf.data_ptr() + o for o in offs])
    slens = np.ascontiguousarray(lens, np.uint64)
    e = np.arange(n)
    sel = {"all": np.ones((n, L), np.uint8), "data": np.zeros((n, L), np.uint8), "parity": np.zeros((n, L), np.uint8),
           "rows": np.zeros((n, L), np.uint8)}
    sel["data"][e, e % k] = 1
    sel["parity"][e, k + e % m] = 1
    sel["rows"][:, k:] = 1
    sel["no_rows"] = 1 - sel["rows"]
    failed = []

    def select(which, p=plan, sources=srcs):
        pats, of = np.unique(sel[which], axis=0, return_inverse=True)
        pats, of = np.ascontiguousarray(pats, np.uint8), np.ascontiguousarray(of.reshape(-1), np.uint32)
        return lambda: RS.check(lib.hbec_split_plan_select(
            enc.handle, p._h, sources, slens.ctypes.data_as(U64P), pats.ctypes.data_as(N._U8P),
            of.ctypes.data_as(U32P), pats.shape[0], stream))

    def split(p):
        return lambda: RS.check(lib.hbec_split_plan(enc.handle, p._h, srcs, slens.ctypes.data_as(U64P), stream))

    def by_hand(which):
        wanted = [(offs[i] + int(j) * ss[i], ss[i]) for i in range(n) for j in np.flatnonzero(sel[which][i])]
        to_scratch = split(plan_scratch)

        def go():
            to_scratch()
            for o, s in wanted:
                rc = hip.hipMemcpyAsync(buf.data_ptr() + o, scratch.data_ptr() + o, s, D2D, stream)
                if rc:
                    failed.append(rc)
        return go

    data_in_place = select("no_rows")
    groups = {
        "a": {"all_select": select("all"), "split": split(plan), "split_again": split(plan2)},
        "b": {"one_data": select("data"), "hand_data": by_hand("data")},
        "c": {"one_parity": select("parity"), "hand_parity": by_hand("parity")},
        "d": {"parity_inplace": select("rows", sources=in_place),
              "encode": lambda: RS.check(lib.hbec_encode_plan(enc.handle, plan._h, stream))},
    }
    moved = {"all_select": traffic(k, m, sel["all"], lens, ss), "one_data": traffic(k, m, sel["data"], lens, ss),
             "one_parity": traffic(k, m, sel["parity"], lens, ss), "parity_inplace": traffic(k, m, sel["rows"], lens, ss)}
    full = (sum(lens), L * sum(ss))
    moved.update({"split": full, "split_again": full, "encode": (k * sum(ss), m * sum(ss)),
                  "hand_data": (full[0] + sum(ss), full[1] + sum(ss)),
                  "hand_parity": (full[0] + sum(ss), full[1] + sum(ss))})

    for grp, legs in groups.items():
        if only and grp not in only:
            continue
        # the arms of a group write the same bytes: checked once over the whole arena.  Group d
        # codes from data shards a data-only select put in place.
        kept = []
        for arm, fn in legs.items():
            buf.fill_(0xC3)
            if grp == "d":
                data_in_place()  # the parity stays 0xC3 for the arm to write
            fn()
            torch.cuda.synchronize()
            kept.append(buf.clone())
        assert not failed, failed[:4]
        assert all(torch.equal(kept[0], x) for x in kept[1:]), (shape, grp)
        del kept
        reps = {}
        for arm, fn in legs.items():
            fn()
            reps[arm] = max(4, math.ceil(WINDOW_MS / max(timed(fn, 2), 1e-3)))
        ms = {arm: [] for arm in legs}
        names = list(legs)
        for r in range(rounds):
            for arm in (names if r % 2 == 0 else names[::-1]):
                ms[arm].append(timed(legs[arm], reps[arm]))
        assert not failed, failed[:4]
        med = {arm: statistics.median(v) for arm, v in ms.items()}
        for arm in legs:
            rd, wr = moved[arm]
            emit({"shape": shape, "group": grp, "arm": arm, "ms": round(med[arm], 5), "ms_min": round(min(ms[arm]), 5),
                  "ms_max": round(max(ms[arm]), 5), "rounds": rounds, "reps": reps[arm],
                  "window_ms": round(med[arm] * reps[arm], 2), "bytes_read": rd, "bytes_written": wr,
                  "GB_s": round((rd + wr) / (med[arm] * 1e-3) / 1e9, 1)})
        first, rest = names[0], names[1:]
        d = {"shape": shape, "group": grp, "arm": "ratios"}
        for other in rest:
            d[f"{first}_over_{other}"] = round(med[first] / med[other], 4)
        if grp == "a":
            spread = max(med["split_again"] / med["split"], med["split"] / med["split_again"])
            d["split_spread"] = round(spread, 4)
            d["all_select_within_split_spread"] = bool(1 / spread <= med["all_select"] / med["split"] <= spread)
        emit(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "split_select.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default=None, choices=["4+2", "8+3"])
    ap.add_argument("--objects", type=int, default=4096)
    ap.add_argument("--groups", default=None, help="a subset of the groups, e.g. ab")
    ap.add_argument("--label", default=None, help="a tag for every row, for a run of a tuning build")
    a = ap.parse_args()
    out = open(a.out, "a")

    def emit(d):
        line = json.dumps(dict(d, label=a.label) if a.label else d)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    torch.cuda.set_device(0)
    for shape in [s for s in ("4+2", "8+3") if a.shape in (None, s)]:
        k, m = map(int, shape.split("+"))
        run(k, m, a.objects, a.rounds, a.groups, emit)


if __name__ == "__main__":
    main()
