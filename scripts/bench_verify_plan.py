#!/usr/bin/env python3
"""Encoder.Verify of a sweep of objects in one call (hbec_verify_plan,
hbec_verify_host) against what a caller could do before, at 4+2 and 8+3.

Legs (device-resident unless said otherwise; all stripes hold valid codewords,
so no flag is written):

  a          hbec_verify_batch over 4096 equal 1 MiB objects (ecSplit databufs
             back to back): the existing uniform entry, the yardstick
  b          hbec_verify_plan over the same stripes (a stripe plan)
  c_stripes  hbec_verify_plan over 4096 objects of random odd sizes, 4 KiB to
             1 MiB, as a stripe plan (databufs at odd offsets)
  c_objects  the same objects as an object plan (data arena + parity arena)
  d          one hbec_verify_batch call per object of c_stripes: what a caller
             can do without the plan entry
  e_*        hbec_verify_host over the first --host-objects (1024) of the c sizes
             in host memory, pinned (hbec_host_alloc, zero-copy) and pageable
             (staged), next to hbec_encode_host on the same stripes; wall clock

Method: a warm-up, then `rounds` rounds in which the device
legs run in alternating order, each timed by HIP events around `reps` calls;
the median over the rounds is reported, as a fraction of 8 TB/s over the
algorithmic bytes (k + m) S per stripe, and as a ratio to leg a's rate.  The
argument arrays and plans are built before the clock starts.

    python scripts/bench_verify_plan.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--host-objects N]
"""
from __future__ import annotations

import argparse
import ctypes as C
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


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(k, m, n, size, rounds, host_objects, emit):
    enc = RS.New(k, m)
    L = k + m
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(100 * k + m)

    # a / b: n equal objects, one databuf each
    s_eq = size // k
    eq = torch.empty((n, L * s_eq), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(eq, L * s_eq)
    eq_views = B.shard_views(eq, L, s_eq)
    B.encode_views(enc, eq_views, n, s_eq)
    eq_plan = B.StripePlan(enc, stripes=[(eq.data_ptr() + o * L * s_eq, s_eq) for o in range(n)])
    eq_bytes = n * L * s_eq

    # c / d: random odd object sizes, S = ceil(len / k)
    lens = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = [-(-x // k) for x in lens]
    odd_bytes = sum(L * s for s in ss)
    buf = torch.empty((1, odd_bytes + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, buf.shape[1])
    offs, pos = [], 1
    for s in ss:
        offs.append(pos)
        pos += L * s + 3
    st_plan = B.StripePlan(enc, stripes=[(buf.data_ptr() + o, s) for o, s in zip(offs, ss)])
    st_plan.encode()
    data = torch.empty((1, sum(k * s for s in ss) + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(data, data.shape[1])
    par = torch.empty(sum(m * s for s in ss) + 16, dtype=torch.uint8, device="cuda")
    objs, do, po = [], 1, 3
    for s in ss:
        objs.append((data.data_ptr() + do, par.data_ptr() + po, s))
        do += k * s
        po += m * s
    ob_plan = B.StripePlan(enc, objects=objs)
    ob_plan.encode()
    torch.cuda.synchronize()

    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    fptr = C.c_void_p(flags.data_ptr())
    a_args = (enc.handle, B._views(eq_views), n, s_eq, fptr, stream)
    d_args = [(enc.handle, B._views([(buf.data_ptr() + o + i * s, 0) for i in range(L)]), 1, s,
               C.c_void_p(flags.data_ptr() + 4 * e), stream) for e, (o, s) in enumerate(zip(offs, ss))]
    lib = N.lib()

    def leg_a():
        RS.check(lib.hbec_verify_batch(*a_args))

    def leg_d():
        f = lib.hbec_verify_batch
        for x in d_args:
            rc = f(*x)
            if rc:
                RS.check(rc)

    legs = {
        "a": (leg_a, eq_bytes, 20),
        "b": (lambda: eq_plan.verify(flags), eq_bytes, 20),
        "c_stripes": (lambda: st_plan.verify(flags), odd_bytes, 20),
        "c_objects": (lambda: ob_plan.verify(flags), odd_bytes, 20),
        "d": (leg_d, odd_bytes, 1),
    }
    for name, (fn, _, reps) in legs.items():
        for _ in range(1 if name == "d" else 5):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    names = list(legs)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            fn, _, reps = legs[name]
            ms[name].append(timed(fn, reps))
    assert int(flags.count_nonzero()) == 0, "valid codewords were flagged"
    s0 = B.verify_plan_stats()
    st_plan.verify(flags)
    s1 = B.verify_plan_stats()
    med = {name: statistics.median(v) for name, v in ms.items()}
    rate = {name: legs[name][1] / (med[name] * 1e-3) / 1e9 for name in legs}
    shape = f"{k}+{m} {n} objects"
    for name, (fn, nb, reps) in legs.items():
        d = {"shape": shape, "leg": name, "ms": round(med[name], 5), "ms_min": round(min(ms[name]), 5),
             "ms_max": round(max(ms[name]), 5), "rounds": rounds, "reps": reps, "algorithmic_bytes": nb,
             "GB_s": round(rate[name], 1), "frac_of_8TBs": round(rate[name] / PEAK, 4),
             "rate_ratio_to_a": round(rate[name] / rate["a"], 3)}
        if name == "c_stripes":
            d["launches_per_call"] = s1["plan_launches"] - s0["plan_launches"]
            d["per_stripe_calls"] = s1["per_stripe_calls"] - s0["per_stripe_calls"]
            d["speedup_over_d"] = round(med["d"] / med[name], 1)
        if name == "d":
            d["calls_per_rep"] = len(d_args)
            d["note"] = "all objects of c_stripes, not a subset"
        emit(d)
    assert med["c_stripes"] < med["d"] and med["c_objects"] < med["d"], med

    # e: host stripes (the first host_objects of the c sizes), wall clock
    del eq, buf, data, par, eq_plan, st_plan, ob_plan
    hs = ss[:host_objects]
    hbytes = sum(L * s for s in hs)
    hoffs, pos = [], 1
    for s in hs:
        hoffs.append(pos)
        pos += L * s + 3
    pinned = RS.HostBuffer(pos + 16)
    pageable = np.empty(pos + 16, np.uint8)
    for mem, arr in (("pinned", pinned.array), ("pageable", pageable)):
        arr[:] = rng.integers(0, 256, arr.size, dtype=np.uint8)
        stripes = [arr[o:o + L * s] for o, s in zip(hoffs, hs)]
        sa = enc._stripes(stripes)
        out = np.zeros(len(hs), np.uint8)
        calls = {
            "encode_host": lambda: RS.check(lib.hbec_encode_host(enc.handle, sa, len(hs))),
            "verify_host": lambda: RS.check(lib.hbec_verify_host(enc.handle, sa, len(hs), out.ctypes.data_as(N._U8P))),
        }
        for what, fn in calls.items():
            fn()
            ts = []
            for _ in range(max(3, rounds)):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            t = statistics.median(ts)
            gbs = hbytes / (t * 1e-3) / 1e9
            emit({"shape": shape, "leg": f"e_{what}_{mem}", "ms": round(t, 3), "ms_min": round(min(ts), 3),
                  "ms_max": round(max(ts), 3), "rounds": len(ts), "stripes": len(hs),
                  "note": f"first {len(hs)} of the c sizes; wall clock", "algorithmic_bytes": hbytes,
                  "GB_s": round(gbs, 1), "frac_of_8TBs": round(gbs / PEAK, 4),
                  "rate_ratio_to_a": round(gbs / rate["a"], 4)})
        assert not out.any(), "encoded host stripes were flagged"
        del stripes, sa
    pinned.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default=None, choices=["4+2", "8+3"])
    ap.add_argument("--objects", type=int, default=4096)
    ap.add_argument("--host-objects", type=int, default=1024)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = open(a.out, "a") if a.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for k, m in ((4, 2), (8, 3)):
        if a.shape in (None, f"{k}+{m}"):
            run(k, m, a.objects, 1 << 20, a.rounds, a.host_objects, emit)


if __name__ == "__main__":
    main()
