#!/usr/bin/env python3
"""What a pointer per shard costs: the plan calls on a shards plan
(hbec_plan_shards) against the same bytes in a stripe plan, at 4+2 and 8+3.

Workload: that of scripts/bench_mixed_plan.py, 4096 objects of random odd sizes,
4 KiB to 1 MiB (S = ceil(len / k)), databufs at odd offsets; a mask per stripe
drawn uniformly from all single and double losses.  Arms, the same bytes each:

  a        a stripe plan over the databufs
  a_again  a second stripe plan over the same databufs: a against itself, whose
           spread in this run is the margin every other ratio is read with
  b        a shards plan whose pointers describe that same databuf placement
  c        a shards plan with every shard scattered: its own offset in a second
           buffer, the (stripe, shard) pairs shuffled, odd gaps between them

Ops: repair_mixed, verify_mixed, encode and hash_mixed (every shard, digests
written).  `encode` on b and c runs the mixed reconstruct kernel with one mask;
on a it is hbec_encode_plan's own kernels.

Method: a warm-up, then `rounds` rounds in which the arms run in
alternating order, each timed by HIP events around `reps` back-to-back calls of
the C entry points (masks matched to pattern rows once, outside the bracket);
medians, min and max.  Rates are over the bytes of every shard of the plan.

--parent-lib PATH also runs arm a in fresh child processes, alternately on this
build and on the library at PATH (a build of the commit before shards plans),
to show that the existing kernels did not move: per op the ratio parent / this,
beside the ratio of this build's two children against each other.

    python scripts/bench_shard_plan.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N]
                                       [--parent-lib PATH]
"""
from __future__ import annotations

import argparse
import ctypes as C
import itertools
import json
import os
import statistics
import subprocess
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
OPS = ("repair_mixed", "verify_mixed", "encode", "hash_mixed")


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(k, m, n, rounds, reps, only_a, emit):
    enc = RS.New(k, m)
    L = k + m
    rng = np.random.default_rng(100 * k + m)
    masks = [[0 if i in lost else 1 for i in range(L)] for c in (1, 2) for lost in itertools.combinations(range(L), c)]
    present = np.ascontiguousarray(np.array(masks, np.uint8)[rng.integers(0, len(masks), n)])
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
    plans = {"a": B.StripePlan(enc, stripes=stripes), "a_again": B.StripePlan(enc, stripes=stripes)}
    plans["a"].encode()
    torch.cuda.synchronize()
    keep = [buf]
    if not only_a:
        plans["b"] = B.StripePlan(enc, shards=[([buf.data_ptr() + o + j * s for j in range(L)], s)
                                               for o, s in zip(offs, ss)])
        # c: the same shard bytes, every shard at a place of its own
        pairs = [(e, j) for e in range(n) for j in range(L)]
        order = rng.permutation(len(pairs))
        gaps = rng.integers(1, 14, len(pairs))
        scat = torch.empty(total + int(gaps.sum()) + 16, dtype=torch.uint8, device="cuda")
        at = [[0] * L for _ in range(n)]
        flat = buf[0]
        pos = 0
        for q, g in zip(order, gaps):
            e, j = pairs[q]
            pos += int(g)
            at[e][j] = pos
            src = offs[e] + j * ss[e]
            scat[pos:pos + ss[e]].copy_(flat[src:src + ss[e]])
            pos += ss[e]
        plans["c"] = B.StripePlan(enc, shards=[([scat.data_ptr() + at[e][j] for j in range(L)], ss[e])
                                               for e in range(n)])
        keep.append(scat)
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    dig = torch.empty(n * L * 16, dtype=torch.uint8, device="cuda")

    # the C calls themselves, on rows matched once: the wrapper's np.unique per call
    # (1-2 ms for 4096 masks) would sit inside the bracket and hide the kernels
    lib = N.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pats, pat_of = np.unique(present, axis=0, return_inverse=True)
    pats = np.ascontiguousarray(pats, np.uint8)
    pat_of = np.ascontiguousarray(pat_of.reshape(-1), np.uint32)
    every = np.ones((1, L), np.uint8)
    sel_of = np.zeros(n, np.uint32)
    pp, po = pats.ctypes.data_as(N._U8P), pat_of.ctypes.data_as(U32P)
    fl, dg = C.c_void_p(flags.data_ptr()), C.c_void_p(dig.data_ptr())

    def call(op, p):
        if op == "repair_mixed":
            return lambda: RS.check(lib.hbec_repair_plan_mixed(enc.handle, p._h, pp, pats.shape[0], po, 0, fl, stream))
        if op == "verify_mixed":
            return lambda: RS.check(lib.hbec_verify_plan_mixed(enc.handle, p._h, pp, pats.shape[0], po, fl, stream))
        if op == "encode":
            return lambda: RS.check(lib.hbec_encode_plan(enc.handle, p._h, stream))
        return lambda: RS.check(lib.hbec_hash_plan_mixed(enc.handle, p._h, every.ctypes.data_as(N._U8P), 1,
                                                         sel_of.ctypes.data_as(U32P), None, 1, None, dg, None, None,
                                                         stream))

    med = {}
    for op in OPS:
        legs = {arm: call(op, p) for arm, p in plans.items()}
        for fn in legs.values():
            for _ in range(3):
                fn()
        ms = {arm: [] for arm in legs}
        names = list(legs)
        for r in range(rounds):
            for arm in (names if r % 2 == 0 else names[::-1]):
                ms[arm].append(timed(legs[arm], reps))
        med[op] = {arm: statistics.median(v) for arm, v in ms.items()}
        for arm in legs:
            gbs = total / (med[op][arm] * 1e-3) / 1e9
            d = {"shape": shape, "op": op, "arm": arm, "ms": round(med[op][arm], 5),
                 "ms_min": round(min(ms[arm]), 5), "ms_max": round(max(ms[arm]), 5), "rounds": rounds, "reps": reps,
                 "shard_bytes": total, "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK, 4),
                 "time_ratio_to_a": round(med[op][arm] / med[op]["a"], 4)}
            emit(d)
    # the stripes still verify, whichever plan wrote them last
    flags.zero_()
    for p in plans.values():
        p.verify(flags)
    torch.cuda.synchronize()
    assert int(flags.count_nonzero()) == 0, "a stripe does not verify after the arms"
    del plans, keep
    return med


def child(lib, shape, n, rounds, reps):
    env = dict(os.environ)
    if lib:
        env["HBEC_LIB"] = str(lib)
    else:
        env.pop("HBEC_LIB", None)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--only-a", "--shape", shape, "--objects", str(n),
           "--rounds", str(rounds), "--reps", str(reps)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode:
        raise RuntimeError(out.stdout[-2000:] + out.stderr[-2000:])
    rows = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    return {r["op"]: r["ms"] for r in rows if r["arm"] == "a"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shape", default=None, choices=["4+2", "8+3"])
    ap.add_argument("--objects", type=int, default=4096)
    ap.add_argument("--only-a", action="store_true", help="arms a and a_again only (what --parent-lib runs)")
    ap.add_argument("--parent-lib", default=None)
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    shapes = [s for s in ("4+2", "8+3") if a.shape in (None, s)]
    if a.parent_lib:
        # fresh processes, this build and the parent's by turns; nothing of the GPU is open here
        for shape in shapes:
            runs = {"this": [], "parent": []}
            for _ in range(2):
                runs["this"].append(child(None, shape, a.objects, a.rounds, a.reps))
                runs["parent"].append(child(a.parent_lib, shape, a.objects, a.rounds, a.reps))
            for op in OPS:
                this = statistics.mean(r[op] for r in runs["this"])
                parent = statistics.mean(r[op] for r in runs["parent"])
                emit({"shape": f"{shape} {a.objects} objects", "op": op, "arm": "a, parent build against this build",
                      "ms_this": [r[op] for r in runs["this"]], "ms_parent": [r[op] for r in runs["parent"]],
                      "parent_over_this": round(parent / this, 4),
                      "this_over_this": round(runs["this"][1][op] / runs["this"][0][op], 4),
                      "parent_over_parent": round(runs["parent"][1][op] / runs["parent"][0][op], 4)})
        return
    torch.cuda.set_device(0)
    for shape in shapes:
        k, m = map(int, shape.split("+"))
        run(k, m, a.objects, a.rounds, a.reps, a.only_a, emit)


if __name__ == "__main__":
    main()
