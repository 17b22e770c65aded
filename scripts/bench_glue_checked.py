#!/usr/bin/env python3
"""The checked glue of a GET (hbec_glue_plan_checked) against the calls it
replaces, at 4+2 and 8+3, on a shards plan.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
every shard named by its own pointer, destinations back to back.  Three arms,
the legs of an arm interleaved:

  clean    g    glue_mixed alone: reads k shards, checks nothing
           vg   verify_mixed, then glue_mixed: the survivors read twice
           c    glue_checked: every present shard read once
  one      x    XOR one byte into one shard of 1 % of the entries of a scratch copy, and out again
           cg   the XOR, correct_mixed filtered by Verify's flags, glue_mixed, all on the scratch copy
           c    glue_checked on the corrupt shards themselves, which it leaves as they are
  lost     g    glue_mixed with one data shard of every entry lost, the rest clean
           c    glue_checked with the same masks (m - 1 shards checked)

correct_mixed removes the error it is timed on, so cg puts it back inside the
bracket; x times that step alone, twice, and the JSON carries cg less half of x
(ms_less_setup).  Method: a warm-up, then `rounds` rounds with
the legs in alternating order, each timed by HIP events around `reps`
back-to-back calls, so that no window is under 5 ms; medians with the smallest
and largest round.  Nothing is gated.  After every arm the destination must
hold the objects byte for byte and the shards must be what they were.

    python scripts/bench_glue_checked.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N]
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

REPS = 10         # calls per timed window: every leg but x takes 0.5 ms or more
REPS_SHORT = 200  # of x: a window of 10 such steps would time the scheduler
U32P, U64P = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


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
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    names = list(legs)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            ms[name].append(timed(*legs[name]))
    return ms


def run(k, m, n, rounds, emit):
    enc = RS.New(k, m)
    L = k + m
    rng = np.random.default_rng(100 * k + m)
    lens = np.array([int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)], np.uint64)
    ss = -(-lens.astype(np.int64) // k)
    offs = 1 + np.concatenate([[0], np.cumsum(L * ss + 3)[:-1]])
    buf = torch.empty((1, int(L * ss.sum()) + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, buf.shape[1])
    B.StripePlan(enc, stripes=[(buf.data_ptr() + int(o), int(s)) for o, s in zip(offs, ss)]).encode()
    torch.cuda.synchronize()
    work = buf.clone()  # the scratch copy correct_mixed may write

    def shards_plan(t):
        return B.StripePlan(enc, shards=[([t.data_ptr() + int(o) + j * int(s) for j in range(L)], int(s))
                                         for o, s in zip(offs, ss)])

    plan, wplan = shards_plan(buf), shards_plan(work)
    d_offs = np.concatenate([[0], np.cumsum(lens.astype(np.int64) + 5)[:-1]]) + 3
    dst = torch.zeros(int(d_offs[-1]) + int(lens[-1]) + 16, dtype=torch.uint8, device="cuda")
    dsts = (C.c_void_p * n)(*[dst.data_ptr() + int(o) for o in d_offs])
    hit = np.sort(rng.permutation(n)[:max(1, n // 100)])  # 1 % of the entries: shard j bad at p < min(S, len)
    j1 = rng.integers(0, L, hit.size)
    p1 = np.array([int(rng.integers(s)) for s in ss[hit]], np.int64)
    at = torch.from_numpy(offs[hit] + j1 * ss[hit] + p1).cuda()
    flags, fixed, wfixed = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))  # wfixed: the cg leg's own
    idx = np.arange(n, dtype=np.uint32) % k  # arm `lost`: entry i has lost data shard i % k
    full, lost = np.ones((1, L), np.uint8), np.ones((k, L), np.uint8)
    lost[np.arange(k), np.arange(k)] = 0
    zero_idx = np.zeros(n, np.uint32)

    lib, stream = N.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(fn, p, pats, of, *rest):
        a = (enc.handle, p._h, pats.ctypes.data_as(N._U8P), pats.shape[0], of.ctypes.data_as(U32P)) + rest + (stream,)
        return lambda: RS.check(fn(*a))

    ln = lens.ctypes.data_as(U64P)
    fx, fl = C.c_void_p(fixed.data_ptr()), C.c_void_p(flags.data_ptr())
    glue = call(lib.hbec_glue_plan_mixed, plan, full, zero_idx, dsts, ln)
    verify = call(lib.hbec_verify_plan_mixed, plan, full, zero_idx, fl)
    checked = call(lib.hbec_glue_plan_checked, plan, full, zero_idx, dsts, ln, fx)
    wglue = call(lib.hbec_glue_plan_mixed, wplan, full, zero_idx, dsts, ln)
    wcorrect = call(lib.hbec_correct_plan_mixed, wplan, full, zero_idx, fl, C.c_void_p(wfixed.data_ptr()))
    glue_lost = call(lib.hbec_glue_plan_mixed, plan, lost, idx, dsts, ln)
    checked_lost = call(lib.hbec_glue_plan_checked, plan, lost, idx, dsts, ln, fx)

    def xor(t):
        t.view(-1)[at] ^= 0x5A

    def objects_written(last):
        dst.zero_()
        last()
        torch.cuda.synchronize()
        flat = work.view(-1)  # clean again after every arm
        for i in range(0, n, 37):
            got = dst[int(d_offs[i]):int(d_offs[i]) + int(lens[i])]
            assert torch.equal(got, flat[int(offs[i]):int(offs[i]) + int(lens[i])]), f"object {i} differs"
        for i in hit:
            got = dst[int(d_offs[i]):int(d_offs[i]) + int(lens[i])]
            assert torch.equal(got, flat[int(offs[i]):int(offs[i]) + int(lens[i])]), f"object {i} differs"

    def arm(name, legs, last, base, bad=0):
        ms = measure(legs, rounds)
        objects_written(last)
        med = {q: statistics.median(v) for q, v in ms.items()}
        for q in legs:
            d = {"shape": f"{k}+{m} {n} objects", "arm": name, "leg": q, "ms": round(med[q], 5),
                 "ms_min": round(min(ms[q]), 5), "ms_max": round(max(ms[q]), 5), "rounds": rounds, "reps": legs[q][1],
                 "bad_entries": bad, "shard_bytes": int(L * ss.sum()), "object_bytes": int(lens.sum())}
            if q == "cg":
                d["ms_less_setup"] = round(med[q] - med["x"] / 2, 5)
            if q != base and q != "x":
                d["time_ratio_over_" + base] = round(d.get("ms_less_setup", med[q]) / med[base], 3)
            emit(d)

    arm("clean", {"g": (glue, REPS), "vg": (lambda: (verify(), glue()), REPS), "c": (checked, REPS)}, checked, "g")
    assert not flags.any() and not fixed.any()
    xor(buf)
    verify()
    torch.cuda.synchronize()
    assert set(np.nonzero(flags.cpu().numpy() & 1)[0]) == set(hit.tolist())
    arm("one", {"x": (lambda: (xor(work), xor(work)), REPS_SHORT),
                "cg": (lambda: (xor(work), wcorrect(), wglue()), REPS), "c": (checked, REPS)}, checked, "c",
        bad=int(hit.size))
    want = np.zeros(n, np.uint32)
    want[hit] = N.COR_BAD | (1 << j1).astype(np.uint32)
    for name, words in (("glue_checked", fixed), ("correct_mixed", wfixed)):  # each call's own words
        assert np.array_equal(words.cpu().numpy().view(np.uint32), want), f"one: wrong words from {name}"
    xor(buf)  # the shards as they were
    assert torch.equal(buf, work), "the shards differ from the encoded ones"
    fixed.zero_()
    arm("lost", {"g": (glue_lost, REPS), "c": (checked_lost, REPS)}, checked_lost, "g")
    assert not fixed.any() and torch.equal(buf, work)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "glue_checked.jsonl"))
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
