#!/usr/bin/env python3
"""The checked glue of a ranged GET (hbec_glue_plan_range_checked) against the
calls around it, at 4+2 and 8+3, on a shards plan.

Workload: 4096 entries of S = 256 KiB, every shard named by its own pointer,
destinations back to back.  Three ranges, the legs of a range interleaved:

  (i)   64 KiB inside data shard 1      (ii)  the second half of D      (iii)  all of D

  c     glue_range_checked, clean, every shard present
  g, g2 glue_range, the unchecked yardstick, twice: its spread against itself
  vg    verify_mixed, then glue_range
  w     the work-around: glue_checked of the prefix up to the range's end into
        scratch, then one device-to-device copy per entry
  gc    (iii) only: glue_checked
  bad   c with one bad byte inside the range in 1 % of the entries
  lost  c with one data shard of every entry lost (m - 1 shards checked)

Method (as scripts/bench_glue_checked.py): a warm-up, then
`rounds` rounds with the legs in alternating order, each timed by HIP events
around enough back-to-back calls that no window is under 5 ms; medians with the
smallest and largest round.  Nothing is gated.  Before a leg's time is reported
its bytes and words are compared with the clean objects.

    python scripts/bench_glue_range_checked.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N]
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

S = 256 * 1024
WINDOW_MS = 6.0
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
    reps = {}
    for name, fn in legs.items():  # warm-up, and the calls a window of WINDOW_MS needs
        fn()
        reps[name] = max(2, math.ceil(WINDOW_MS / max(timed(fn, 2), 1e-3)))
    ms = {name: [] for name in legs}
    names = list(legs)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            ms[name].append(timed(legs[name], reps[name]))
    return ms, reps


def run(k, m, n, rounds, emit):
    enc = RS.New(k, m)
    L = k + m
    rng = np.random.default_rng(200 * k + m)
    offs = 1 + np.arange(n, dtype=np.int64) * (L * S + 3)
    buf = torch.empty((1, n * (L * S + 3) + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, buf.shape[1])
    B.StripePlan(enc, stripes=[(buf.data_ptr() + int(o), S) for o in offs]).encode()
    torch.cuda.synchronize()
    flat = buf.view(-1)
    plan = B.StripePlan(enc, shards=[([buf.data_ptr() + int(o) + j * S for j in range(L)], S) for o in offs])
    dst = torch.zeros(n * (k * S + 5) + 16, dtype=torch.uint8, device="cuda")
    scr = torch.zeros(n * k * S + 16, dtype=torch.uint8, device="cuda")  # the work-around's prefixes
    flags, fixed = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    idx = np.arange(n, dtype=np.uint32) % k  # `lost`: entry i has lost data shard i % k
    full, lost = np.ones((1, L), np.uint8), np.ones((k, L), np.uint8)
    lost[np.arange(k), np.arange(k)] = 0
    zero_idx = np.zeros(n, np.uint32)
    hit = np.sort(rng.permutation(n)[:max(1, n // 100)])  # 1 % of the entries: shard j1 bad at p1, inside every range
    j1 = rng.integers(0, L, hit.size)
    p1 = S // 4 + rng.integers(0, 64 * 1024, hit.size)
    at = torch.from_numpy(offs[hit] + j1 * S + p1).cuda()
    lib, stream = N.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fx, fl = C.c_void_p(fixed.data_ptr()), C.c_void_p(flags.data_ptr())

    def call(fn, pats, of, *rest):
        a = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0], of.ctypes.data_as(U32P)) + rest + (stream,)
        return lambda: RS.check(fn(*a))

    verify = call(lib.hbec_verify_plan_mixed, full, zero_idx, fl)
    for name, s, e in (("i", S + S // 4, S + S // 4 + 64 * 1024), ("ii", k * S // 2, k * S), ("iii", 0, k * S)):
        ln = e - s
        d_offs = 3 + np.arange(n, dtype=np.int64) * (ln + 5)
        dsts = (C.c_void_p * n)(*[dst.data_ptr() + int(o) for o in d_offs])
        sdsts = (C.c_void_p * n)(*[scr.data_ptr() + int(i) * e for i in range(n)])
        starts, lens, ends = (np.full(n, v, np.uint64) for v in (s, ln, e))
        st, lp, ep = (x.ctypes.data_as(U64P) for x in (starts, lens, ends))
        grange = call(lib.hbec_glue_plan_range, full, zero_idx, dsts, st, lp)
        checked = call(lib.hbec_glue_plan_range_checked, full, zero_idx, dsts, st, lp, fx)
        checked_lost = call(lib.hbec_glue_plan_range_checked, lost, idx, dsts, st, lp, fx)
        prefix = call(lib.hbec_glue_plan_checked, full, zero_idx, sdsts, ep, fx)

        def around():
            prefix()
            for i in range(n):
                dst[int(d_offs[i]):int(d_offs[i]) + ln].copy_(scr[i * e + s:(i + 1) * e], non_blocking=True)

        def xor():
            flat[at] ^= 0x5A

        def written(fn, words):
            """fn's bytes and words against the clean objects (the shards are clean when this compares)."""
            dst.zero_()
            fixed.zero_()
            fn()
            torch.cuda.synchronize()
            if words is not None:
                xor()  # the shards as they were
                torch.cuda.synchronize()
            for i in sorted(set(range(0, n, 37)) | set(hit.tolist())):
                got = dst[int(d_offs[i]):int(d_offs[i]) + ln]
                assert torch.equal(got, flat[int(offs[i]) + s:int(offs[i]) + e]), f"{name}: entry {i} differs"
            want = np.zeros(n, np.uint32)
            if words is not None:
                want[hit] = words
            assert np.array_equal(fixed.cpu().numpy().view(np.uint32), want), f"{name}: wrong words"

        legs = {"c": checked, "g": grange, "g2": grange, "vg": lambda: (verify(), grange()), "w": around}
        if name == "iii":
            legs["gc"] = call(lib.hbec_glue_plan_checked, full, zero_idx, dsts, lp, fx)
        legs["lost"] = checked_lost
        for fn in legs.values():
            written(fn, None)
        ms, reps = measure(legs, rounds)
        assert not flags.any()
        xor()
        written(checked, N.COR_BAD | (1 << j1).astype(np.uint32))  # leaves the shards clean again
        xor()
        bad_ms, bad_reps = measure({"bad": checked}, rounds)
        xor()
        fixed.zero_()
        ms.update(bad_ms)
        reps.update(bad_reps)
        med = {q: statistics.median(v) for q, v in ms.items()}
        for q in ms:
            d = {"shape": f"{k}+{m} {n} entries of {S} B", "range": name, "range_bytes": ln, "leg": q,
                 "ms": round(med[q], 5), "ms_min": round(min(ms[q]), 5), "ms_max": round(max(ms[q]), 5),
                 "rounds": rounds, "reps": reps[q], "bad_entries": int(hit.size) if q == "bad" else 0}
            for base in ("g", "vg", "w", "gc"):
                if base in med and q in ("c", "bad", "lost", "g2") and not (q == "g2" and base != "g"):
                    d["time_ratio_over_" + base] = round(med[q] / med[base], 3)
            emit(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "glue_range_checked.jsonl"))
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
