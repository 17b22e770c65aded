#!/usr/bin/env python3
"""The k+m shards of a plan's entries from their object bytes in one call
(hbec_split_plan) against what a caller had to do without it, at 4+2 and 8+3.

Workload: that of scripts/bench_glue.py, 4096 objects of random odd sizes, 4 KiB
to 1 MiB (S = ceil(len / k), so every object's last data shard ends in 1..k-1
bytes of ecSplit's pad), in a source arena at odd offsets, len + 3 bytes apart.
The shards are those of a databuf per object, at odd offsets in a shard arena,
named shard by shard in a shards plan.

Arms, the same bytes each:

  a        hbec_split_plan on the shards plan
  a_again  the same call on a second plan over the same buffers: a against
           itself, whose spread in this run is the margin the others are read with
  b        what a caller does without the call: one clipped device-to-device
           hipMemcpyAsync per data shard per entry, a hipMemsetAsync per pad, and
           hbec_encode_plan on that plan, which reads the k S bytes again
  c        hbec_encode_plan alone on the same plan, for scale: it moves (k + m) S
           bytes per entry where a moves (2 k + m) S

Method: a warm-up, then `rounds` rounds in which the arms run in
alternating order, each timed by HIP events around `reps` back-to-back calls of
the C entry points; medians, min and max.  The rate of a is over (2 k + m) S
bytes per entry, read and written.

    python scripts/bench_split.py [--out FILE] [--rounds N] [--reps N] [--shape 4+2|8+3] [--objects N] [--label TEXT]
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


def run(k, m, n, rounds, reps, label, emit):
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
    buf = torch.zeros(L * sum(ss) + 3 * n + 16, dtype=torch.uint8, device="cuda")
    offs, pos = [], 1
    for s in ss:
        offs.append(pos)
        pos += L * s + 3
    rows = [([buf.data_ptr() + o + j * s for j in range(L)], s) for o, s in zip(offs, ss)]
    plan_a, plan_a2 = B.StripePlan(enc, shards=rows), B.StripePlan(enc, shards=rows)
    torch.cuda.synchronize()

    lib = N.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipMemsetAsync.restype = C.c_int
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    srcs = (C.c_void_p * n)(*[src.data_ptr() + o for o in src_at])
    slens = np.ascontiguousarray(lens, np.uint64)
    copies, pads = [], []
    for e in range(n):
        for j in range(k):
            v = max(0, min(ss[e], lens[e] - j * ss[e]))
            to = buf.data_ptr() + offs[e] + j * ss[e]
            if v:
                copies.append((to, src.data_ptr() + src_at[e] + j * ss[e], v))
            if v < ss[e]:
                pads.append((to + v, ss[e] - v))
    failed = []

    def split(p):
        return lambda: RS.check(lib.hbec_split_plan(enc.handle, p._h, srcs, slens.ctypes.data_as(U64P), stream))

    def encode():
        RS.check(lib.hbec_encode_plan(enc.handle, plan_a._h, stream))

    def by_hand():
        for d, s, v in copies:
            rc = hip.hipMemcpyAsync(d, s, v, D2D, stream)
            if rc:
                failed.append(rc)
        for d, v in pads:
            rc = hip.hipMemsetAsync(d, 0, v, stream)
            if rc:
                failed.append(rc)
        encode()

    legs = {"a": split(plan_a), "a_again": split(plan_a2), "b": by_hand, "c": encode}
    # a and b write the same shards: checked once, entry by entry over a sample, pads and parity included
    sample = list(range(0, n, max(1, n // 64)))
    kept = {}
    for arm in ("a", "b"):
        buf.fill_(0xC3)
        legs[arm]()
        torch.cuda.synchronize()
        kept[arm] = [buf[offs[e] - 1:offs[e] + L * ss[e] + 1].clone() for e in sample]
    assert not failed, failed[:4]
    for e, x, y in zip(sample, kept["a"], kept["b"]):
        assert torch.equal(x, y), (shape, e)
        assert torch.equal(x[1:1 + lens[e]], src[0, src_at[e]:src_at[e] + lens[e]]), (shape, e)
    del kept
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
    moved = (2 * k + m) * sum(ss)
    spread = max(med["a_again"] / med["a"], med["a"] / med["a_again"])
    for arm in legs:
        d = {"shape": shape, "arm": arm, "ms": round(med[arm], 5), "ms_min": round(min(ms[arm]), 5),
             "ms_max": round(max(ms[arm]), 5), "rounds": rounds, "reps": reps}
        if label:
            d["label"] = label
        if arm in ("a", "a_again"):
            gbs = moved / (med[arm] * 1e-3) / 1e9
            d.update({"bytes_2kS_mS": moved, "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK, 4)})
        if arm == "b":
            d.update({"copies_per_call": len(copies), "memsets_per_call": len(pads)})
        if arm == "c":
            gbs = (k + m) * sum(ss) / (med[arm] * 1e-3) / 1e9
            d.update({"bytes_kS_mS": (k + m) * sum(ss), "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK, 4)})
        emit(d)
    d = {"shape": shape, "arm": "ratios", "a_again_over_a": round(med["a_again"] / med["a"], 4),
         "spread": round(spread, 4), "a_over_b": round(med["a"] / med["b"], 4),
         "a_over_c": round(med["a"] / med["c"], 4), "byte_ratio_a_over_c": round((2 * k + m) / (k + m), 4),
         "a_quicker_than_b_by_more_than_spread": bool(med["a"] * spread < med["b"])}
    if label:
        d["label"] = label
    emit(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", default=None, choices=["4+2", "8+3"])
    ap.add_argument("--objects", type=int, default=4096)
    ap.add_argument("--label", default=None, help="a tag for every row, for a run of a tuning build")
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
        run(k, m, a.objects, a.rounds, a.reps, a.label, emit)


if __name__ == "__main__":
    main()
