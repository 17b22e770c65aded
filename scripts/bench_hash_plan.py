#!/usr/bin/env python3
"""The ShardHash audit of a plan (hbec_hash_plan_mixed) against the way the same
job was done without it, at 4+2 and 8+3.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
as a stripe plan with the databufs at odd offsets, so shard starts fall on every
residue.  Legs, interleaved round by round in alternating order:

  a      hash_mixed over every shard, digests only
  list   hbec_md5_list over the same shard pointers: the yardstick of a and b
  b      a with expected, bad and where
  c      b filtered to 1 % of the entries
  c1     b filtered to the one longest of those entries: a call lasts at least
         as long as its longest examined chain, and this is that bound
  d      the r = 1 sweep: every entry has lost m - 1 shards, 1 % have one
         flipped bit; repair_mixed -> hash_mixed(filter=flags) -> heal_mixed and
         a synchronize, on the wall clock
  dy     the host trip for the same: repair_mixed, flags.cpu(), hbec_md5_list
         over the present shards of the flagged entries, digests.cpu(), compare
         on the host, a plan of the flagged entries, repair_mixed on it with the
         differing shard cleared, synchronize

a, list, b, c and c1 are timed with HIP events around `reps` back-to-back calls,
the calls' host side inside the bracket.  d and dy heal what they find, so the
bits are flipped again before every pass, outside the clock.  Medians with the
smallest and largest round and their spread (max - min) / median.  Nothing is
gated.  Before the timing every digest is compared with hashlib on 32 sampled
shards, and after d and dy 24 sampled stripes are compared with their snapshot.

With --only-a the script times leg a alone: run it under HBEC_LIB with a library
built with -DHBEC_HASH_PLAN_BYTE_LOADER=1 for the loader A/B (tag: --tag).

    python scripts/bench_hash_plan.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N]
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
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

REPS = 3
U32P = C.POINTER(C.c_uint32)


def timed_events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, (t1 - t0) * 1e3 / reps


def timed_wall(fn, before):
    before()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, 0.0


def measure(legs, rounds):
    """legs: name -> (fn, 'events' | setup function of a wall-clock leg)."""
    for fn, how in legs.values():
        if how != "events":
            how()
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in legs}
    names = list(legs)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            fn, how = legs[name]
            out[name].append(timed_events(fn, REPS) if how == "events" else timed_wall(fn, how))
    return out


def summary(samples):
    ms = [s[0] for s in samples]
    med = statistics.median(ms)
    return {"ms": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5),
            "spread": round((max(ms) - min(ms)) / med, 4),
            "host_ms": round(statistics.median(s[1] for s in samples), 5)}


def run(k, m, n, rounds, emit, only_a, tag):
    enc = RS.New(k, m)
    L = k + m
    rng = np.random.default_rng(300 * k + m)
    lib = N.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lens = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = np.array([-(-x // k) for x in lens], np.int64)
    shape = f"{k}+{m} {n} objects"
    buf = torch.empty((1, int(L * ss.sum()) + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, buf.shape[1])
    offs, pos = [], 1
    for s in ss:
        offs.append(pos)
        pos += L * int(s) + 3
    items = [(buf.data_ptr() + o, int(s)) for o, s in zip(offs, ss)]
    plan = B.StripePlan(enc, stripes=items)
    plan.encode()
    torch.cuda.synchronize()
    flat = buf.view(-1)
    shard_off = lambda i, j: offs[i] + j * int(ss[i])  # noqa: E731
    residues = sorted({(buf.data_ptr() + shard_off(i, j)) % 16 for i in range(n) for j in range(L)})
    shard_bytes = int(L * ss.sum())

    # ---- the stored hashes: this call's own digests, sampled against hashlib ----
    expected = torch.zeros(n * L * 16, dtype=torch.uint8, device="cuda")
    plan.hash_mixed(None, digests=expected)
    torch.cuda.synchronize()
    exp_host = expected.cpu().numpy().reshape(n, L, 16)
    for i, j in zip(rng.integers(0, n, 32), rng.integers(0, L, 32)):
        o = shard_off(int(i), int(j))
        want = hashlib.md5(flat[o:o + int(ss[i])].cpu().numpy().tobytes()).digest()
        assert bytes(exp_host[i, j]) == want, "digest differs from hashlib"

    all_rows = np.ones((1, L), np.uint8)
    zeros_idx = np.zeros(n, np.uint32)
    digests = torch.zeros(n * L * 16, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(n, dtype=torch.int32, device="cuda")
    where = torch.zeros(n, dtype=torch.int32, device="cuda")

    def hash_call(rows, idx, flt=None, exp=None, dig=None, b=None, w=None):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        a = (enc.handle, plan._h, rows.ctypes.data_as(N._U8P), rows.shape[0], idx.ctypes.data_as(U32P), p(flt), 1,
             p(exp), p(dig), p(b), p(w), stream)
        return lambda: RS.check(lib.hbec_hash_plan_mixed(*a))

    # hbec_md5_list over the same chains
    addrs = (C.c_void_p * (n * L))(*[buf.data_ptr() + shard_off(i, j) for i in range(n) for j in range(L)])
    lens64 = (C.c_uint64 * (n * L))(*[int(ss[i]) for i in range(n) for _ in range(L)])
    list_dig = torch.zeros(n * L * 16, dtype=torch.uint8, device="cuda")

    def list_leg():
        RS.check(lib.hbec_md5_list(addrs, lens64, n * L, C.c_void_p(list_dig.data_ptr()), stream))

    def emit_leg(leg, samples, **more):
        d = {"shape": shape, "leg": leg, **summary(samples), "rounds": rounds, "reps": REPS}
        if tag:
            d["tag"] = tag
        d.update(more)
        emit(d)
        return d

    common = dict(chains=n * L, shard_bytes=shard_bytes, longest_chain=int(ss.max()), start_residues=len(residues))
    if only_a:
        ms = measure({"a": (hash_call(all_rows, zeros_idx, dig=digests), "events")}, rounds)
        a = emit_leg("a", ms["a"], **common)
        emit({"shape": shape, "tag": tag, "GBps": round(shard_bytes / a["ms"] / 1e6, 2)})
        return

    # ---- a, b against hbec_md5_list ----
    legs = {"a": (hash_call(all_rows, zeros_idx, dig=digests), "events"),
            "list": (list_leg, "events"),
            "b": (hash_call(all_rows, zeros_idx, exp=expected, dig=digests, b=bad, w=where), "events")}
    ms = measure(legs, rounds)
    assert torch.equal(digests, expected) and torch.equal(list_dig, expected) and not bad.any() and not where.any()
    a = emit_leg("a", ms["a"], **common)
    li = emit_leg("list", ms["list"], **common)
    b = emit_leg("b", ms["b"], **common)
    for name, x in (("a", a), ("b", b)):
        emit({"shape": shape, "compare": f"list / {name}", "ratio": round(li["ms"] / x["ms"], 3),
              "not_slower_beyond_list_spread": bool(x["ms"] - li["ms"] <= li["spread"] * li["ms"]),
              "GBps": round(shard_bytes / x["ms"] / 1e6, 2), "list_GBps": round(shard_bytes / li["ms"] / 1e6, 2)})

    # ---- c: 1 % of the entries examined; c1: the longest of them alone ----
    order = rng.permutation(n)
    one_pct = order[:max(1, n // 100)]
    f1 = np.zeros(n, np.int32)
    f1[one_pct] = 1
    longest = int(one_pct[np.argmax(ss[one_pct])])
    f2 = np.zeros(n, np.int32)
    f2[longest] = 1
    flt1, flt2 = torch.from_numpy(f1).cuda(), torch.from_numpy(f2).cuda()
    legs = {"c": (hash_call(all_rows, zeros_idx, flt=flt1, exp=expected, dig=digests, b=bad, w=where), "events"),
            "c1": (hash_call(all_rows, zeros_idx, flt=flt2, exp=expected, dig=digests, b=bad, w=where), "events")}
    ms = measure(legs, rounds)
    c = emit_leg("c", ms["c"], examined=int(one_pct.size), longest_examined_chain=int(ss[longest]))
    c1 = emit_leg("c1", ms["c1"], examined=1, longest_examined_chain=int(ss[longest]))
    emit({"shape": shape, "compare": "c / c1", "ratio": round(c["ms"] / c1["ms"], 3),
          "c_over_b": round(c["ms"] / b["ms"], 4)})

    # ---- d: the r = 1 sweep against the host trip ----
    present = np.ones((n, L), np.uint8)
    for i in range(n):
        present[i][rng.choice(L, size=m - 1, replace=False)] = 0
    pats, idx = np.unique(present, axis=0, return_inverse=True)
    pats = np.ascontiguousarray(pats, np.uint8)
    idx = np.ascontiguousarray(idx.reshape(-1), np.uint32)
    plan.reconstruct_mixed(present)  # missing shards hold what the others imply
    torch.cuda.synchronize()
    sample = order[-24:]
    snap = {int(i): flat[offs[i]:offs[i] + L * int(ss[i])].clone() for i in list(sample) + list(one_pct[:8])}
    hit_shard = np.array([int(rng.choice(np.nonzero(present[i])[0])) for i in range(n)], np.int64)
    hit_at = torch.tensor([shard_off(int(i), int(hit_shard[i])) + int(rng.integers(ss[i])) for i in one_pct],
                          device="cuda")
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    healed = torch.zeros(n, dtype=torch.int32, device="cuda")

    def flip():
        flat[hit_at] ^= 0x10
        for t in (flags, bad, where, healed):
            t.zero_()

    mix = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0], idx.ctypes.data_as(U32P))
    sweep_hash = hash_call(pats, idx, flt=flags, exp=expected, b=bad, w=where)

    def sweep():
        RS.check(lib.hbec_repair_plan_mixed(*mix, 0, C.c_void_p(flags.data_ptr()), stream))
        sweep_hash()
        RS.check(lib.hbec_heal_plan_mixed(*mix, C.c_void_p(where.data_ptr()), C.c_void_p(healed.data_ptr()), stream))

    def host_trip():
        RS.check(lib.hbec_repair_plan_mixed(*mix, 0, C.c_void_p(flags.data_ptr()), stream))
        sel = np.nonzero(flags.cpu().numpy() & 1)[0]
        chains = [(int(i), int(j)) for i in sel for j in np.nonzero(present[i])[0]]
        a_ = (C.c_void_p * len(chains))(*[buf.data_ptr() + shard_off(i, j) for i, j in chains])
        l_ = (C.c_uint64 * len(chains))(*[int(ss[i]) for i, _ in chains])
        dig = torch.empty(len(chains) * 16, dtype=torch.uint8, device="cuda")
        RS.check(lib.hbec_md5_list(a_, l_, len(chains), C.c_void_p(dig.data_ptr()), stream))
        got = dig.cpu().numpy().reshape(-1, 16)
        again = present[sel].copy()
        row = {int(i): q for q, i in enumerate(sel)}
        for (i, j), d in zip(chains, got):
            if not np.array_equal(d, exp_host[i, j]):
                again[row[i], j] = 0
        sub = B.StripePlan(enc, stripes=[items[i] for i in sel])
        f2_ = torch.zeros(sel.size, dtype=torch.int32, device="cuda")
        sub.repair_mixed(again, f2_)

    ms = measure({"d": (sweep, flip), "dy": (host_trip, flip)}, rounds)
    d = emit_leg("d", ms["d"], flagged=int(one_pct.size))
    dy = emit_leg("dy", ms["dy"], flagged=int(one_pct.size))
    emit({"shape": shape, "compare": "dy / d", "ratio": round(dy["ms"] / d["ms"], 2),
          "faster_beyond_spread": bool(dy["ms"] - d["ms"] > max(dy["spread"] * dy["ms"], d["spread"] * d["ms"]))})
    # the sweep once more, checked
    flip()
    sweep()
    torch.cuda.synchronize()
    named = B.locate_decode(k, m, present, where.cpu().numpy())
    assert np.array_equal(named[one_pct], hit_shard[one_pct]) and (np.delete(named, one_pct) == N.LOC_CLEAN).all()
    want_h = np.zeros(n, np.int32)
    want_h[one_pct] = N.HEAL_DONE | 2
    assert np.array_equal(healed.cpu().numpy(), want_h), "heal flags are wrong"
    for i, s in snap.items():
        assert torch.equal(flat[offs[i]:offs[i] + L * int(ss[i])], s), f"stripe {i} is not what it was"
    emit({"shape": shape, "state": "checked", "stripes_compared": len(snap), "named": int(one_pct.size)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hash_plan.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default=None, choices=["4+2", "8+3"])
    ap.add_argument("--objects", type=int, default=4096)
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--tag", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with open(a.out, "a" if a.append else "w") as out:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()

        for k, m in ((4, 2), (8, 3)):
            if a.shape in (None, f"{k}+{m}"):
                run(k, m, a.objects, a.rounds, emit, a.only_a, a.tag)


if __name__ == "__main__":
    main()
