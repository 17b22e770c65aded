#!/usr/bin/env python
"""The ETag of a plan's objects from their shards (hbec_etag_plan_mixed,
hbec_etag_plan_files) against the way the same job was done without it: glue the
object into a scratch buffer, then hbec_md5_list over that buffer.  4+2 and 8+3.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB.  Three cases, the
arms of each interleaved round by round in alternating order:

  healthy   a stripe plan (S = ceil(len / k), databufs at odd offsets), nothing
            lost.  etag: etag_mixed, digests only.  list / list_again:
            hbec_md5_list over the same [a, a + len) runs, twice, so the spread
            of the yardstick against itself is in the same run: with one
            segment per entry etag walks what list walks.
  files     a files plan of 1-16 stripes of 64 KiB an object, nothing lost.
            etag: etag_files.  glue_list: glue_files into scratch, then
            hbec_md5_list over the scratch.
  one_data  the stripe plan with one data shard lost per object (overwritten).
            etag: etag_mixed with the masks.  glue_list: glue_mixed into
            scratch, then hbec_md5_list.

A call cannot be shorter than its longest chain (one lane, serial MD5): the
times here are bounded below by the 1 MiB objects, not by bandwidth.  Each arm's
digests are compared with the other arm's in full and with hashlib on a sample.

Method: a warm-up, then `rounds` rounds in which the arms run in
alternating order, each timed by HIP events around `reps` back-to-back calls;
medians, min and max.

    python scripts/bench_etag.py [--out FILE] [--rounds N] [--reps N] [--shape 4+2|8+3] [--objects N]
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
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

U64P = C.POINTER(C.c_uint64)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(legs, rounds, reps):
    for fn in legs.values():
        fn()
    ms = {arm: [] for arm in legs}
    names = list(legs)
    for r in range(rounds):
        for arm in (names if r % 2 == 0 else names[::-1]):
            ms[arm].append(timed(legs[arm], reps))
    return ms


def run(k, m, n, rounds, reps, emit):
    enc = RS.New(k, m)
    L = k + m
    rng = np.random.default_rng(500 * k + m)
    lens = [int(x) | 1 for x in rng.integers(4 << 10, 1 << 20, n)]
    lens[0] = (1 << 20) - 1  # the longest chain is in every run
    ss = [(ln + k - 1) // k for ln in lens]
    shape = f"{k}+{m} {n} objects"
    lib = N.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    total = int(sum(lens))

    def list_leg(addrs, dig):
        a = (C.c_void_p * n)(*addrs)
        ln = (C.c_uint64 * n)(*lens)
        return lambda: RS.check(lib.hbec_md5_list(a, ln, n, C.c_void_p(dig.data_ptr()), stream))

    def report(case, ms, yard, scratch, **more):
        med = {arm: statistics.median(v) for arm, v in ms.items()}
        for arm, v in ms.items():
            emit({"shape": shape, "case": case, "arm": arm, "ms": round(med[arm], 4), "ms_min": round(min(v), 4),
                  "ms_max": round(max(v), 4), "rounds": rounds, "reps": reps, "object_bytes": total,
                  "scratch_bytes": int(scratch[arm]), "us_per_block_longest": round(med[arm] * 1e3 / (lens[0] // 64), 4)})
        emit({"shape": shape, "case": case, "arm": "ratios", "etag_over_" + yard: round(med["etag"] / med[yard], 4), **more})
        return med

    def same(case, x, y):
        torch.cuda.synchronize()
        assert torch.equal(x, y), case

    def sample_ok(case, dig, obj_of):
        got = dig.cpu().numpy().tobytes()
        for e in range(0, n, max(1, n // 32)):
            assert got[16 * e:16 * e + 16] == hashlib.md5(obj_of(e)).digest(), (case, e)

    # ---- healthy: a stripe plan against md5_list over the same runs ----
    buf = torch.empty((1, L * sum(ss) + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, buf.shape[1])
    offs, pos = [], 1
    for s in ss:
        offs.append(pos)
        pos += L * s + 3
    plan = B.StripePlan(enc, stripes=[(buf.data_ptr() + o, s) for o, s in zip(offs, ss)])
    plan.encode()
    torch.cuda.synchronize()
    dig_e = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    dig_l = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    ones = np.ones((n, L), np.uint8)
    s0 = B.etag_plan_stats()
    legs = {"etag": lambda: plan.etag_mixed(ones, lens, digests=dig_e),
            "list": list_leg([buf.data_ptr() + o for o in offs], dig_l),
            "list_again": list_leg([buf.data_ptr() + o for o in offs], dig_l)}
    legs["etag"]()
    s1 = B.etag_plan_stats()
    assert s1["segments"] - s0["segments"] == n and s1["decoded_entries"] == s0["decoded_entries"]
    legs["list"]()
    same("healthy", dig_e, dig_l)
    sample_ok("healthy", dig_e, lambda e: buf[0, offs[e]:offs[e] + lens[e]].cpu().numpy().tobytes())
    ms = measure(legs, rounds, reps)
    med = report("healthy", ms, "list", {"etag": 0, "list": 0, "list_again": 0})
    spread = max(med["list_again"] / med["list"], med["list"] / med["list_again"])
    emit({"shape": shape, "case": "healthy", "arm": "spread", "list_again_over_list": round(med["list_again"] / med["list"], 4),
          "spread": round(spread, 4), "etag_inside_spread": bool(1 / spread <= med["etag"] / med["list"] <= spread)})

    # ---- one_data: the same plan with a data shard lost per object, against glue_mixed + md5_list ----
    keep = {e: buf[0, offs[e]:offs[e] + lens[e]].cpu().numpy().tobytes() for e in range(0, n, max(1, n // 32))}
    lost = rng.integers(0, k, n)
    masks = np.ones((n, L), np.uint8)
    span = 0
    for e in range(n):
        j, s = int(lost[e]), ss[e]
        masks[e, j] = 0
        buf[0, offs[e] + j * s:offs[e] + (j + 1) * s] = 0xEE
        span += max(0, min(s, lens[e] - j * s))
    scratch = torch.zeros(total + 3 * n + 16, dtype=torch.uint8, device="cuda")
    at, pos = [], 1
    for ln in lens:
        at.append(pos)
        pos += ln + 3
    dsts = [scratch.data_ptr() + o for o in at]
    glue_list = list_leg(dsts, dig_l)

    def glue_then_list():
        plan.glue_mixed(masks, dsts, lens)
        glue_list()

    dig_e.zero_(), dig_l.zero_()
    s0 = B.etag_plan_stats()
    legs = {"etag": lambda: plan.etag_mixed(masks, lens, digests=dig_e), "glue_list": glue_then_list}
    legs["etag"]()
    decoded = B.etag_plan_stats()["decoded_entries"] - s0["decoded_entries"]
    legs["glue_list"]()
    same("one_data", dig_e, dig_l)
    sample_ok("one_data", dig_e, lambda e: keep[e])
    ms = measure(legs, rounds, reps)
    report("one_data", ms, "glue_list", {"etag": span, "glue_list": total}, decoded_entries=int(decoded))
    del scratch, buf, plan

    # ---- files: objects of 1-16 stripes as their shard files, against glue_files + md5_list ----
    chunk = (64 << 10) // k
    objs = torch.empty((1, total + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(objs, objs.shape[1])
    flen = [sum(min(chunk, (rest + k - 1) // k) for rest in range(ln, 0, -k * chunk)) for ln in lens]
    fbuf = torch.zeros(L * sum(flen) + 3 * n * L + 16, dtype=torch.uint8, device="cuda")
    files, pos = [], 1
    for e in range(n):
        row = []
        for _ in range(L):
            row.append(fbuf.data_ptr() + pos)
            pos += flen[e] + 3
        files.append((row, lens[e]))
    fplan = B.StripePlan(enc, files=files, chunk_size=chunk)
    fplan.split_files([objs.data_ptr() + o for o in at])
    torch.cuda.synchronize()
    n_entries = int(fplan.object_start[-1])
    present = np.ones((n_entries, L), np.uint8)
    scratch = torch.zeros(total + 3 * n + 16, dtype=torch.uint8, device="cuda")
    dsts = [scratch.data_ptr() + o for o in at]
    glue_list = list_leg(dsts, dig_l)

    def glue_files_then_list():
        fplan.glue_files(present, dsts)
        glue_list()

    dig_e.zero_(), dig_l.zero_()
    legs = {"etag": lambda: fplan.etag_files(present, digests=dig_e), "glue_list": glue_files_then_list}
    legs["etag"]()
    legs["glue_list"]()
    same("files", dig_e, dig_l)
    sample_ok("files", dig_e, lambda e: objs[0, at[e]:at[e] + lens[e]].cpu().numpy().tobytes())
    ms = measure(legs, rounds, reps)
    report("files", ms, "glue_list", {"etag": 0, "glue_list": total}, entries=n_entries)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
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
