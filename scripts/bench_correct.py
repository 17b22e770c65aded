#!/usr/bin/env python3
"""The column-by-column correction of a sweep (hbec_correct_plan_mixed) against
the calls it stands beside, at 4+2 and 8+3, every shard present.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
as a stripe plan at odd offsets.  Four groups of legs, the legs of a group
interleaved:

  clean    v    verify_mixed
           l    locate_mixed, flags = None
           c    correct_mixed, flags = None: detect and correct in one pass
           z    correct_mixed filtered by all-zero flags: the cost of the list walk
  one      x1   XOR one byte into one shard of 1 % of the stripes, and out again (the set-up, twice)
           f1   the XOR, then correct_mixed filtered by Verify's flags
  two      x2   XOR one byte each into two shards of those stripes, at different offsets, and out again
           f2   the XOR, then correct_mixed filtered by Verify's flags
           alt  the only other way today: flags copied back, a plan built of the
                flagged stripes, reconstruct_mixed with the two shards left out
                (the host is told which two; no call can name them)

A correction removes the error it is timed on, so f1 and f2 put it back inside
the bracket; x1 and x2 time that step alone, twice so that the buffers end
clean, and the JSON carries f less half of x (ms_less_setup).  Method
(DESIGN.md §5): a warm-up, then `rounds` rounds with the legs in alternating
order, each timed by HIP events around `reps` back-to-back calls (the calls'
host side is inside the bracket; 10 calls for the legs of 0.3 ms and more, 200
for the short ones, so that no window is under 5 ms); medians with the smallest
and largest round.  Nothing is gated.  After every group the buffers must equal
the encoded ones byte for byte.

    python scripts/bench_correct.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N]
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

REPS = 10         # calls per timed window of the legs that take 0.3 ms or more
REPS_SHORT = 200  # of the legs below 0.1 ms: a window of 10 such calls would time the scheduler
U32P = C.POINTER(C.c_uint32)


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
    ss = np.array([-(-(int(x) | 1) // k) for x in rng.integers(4096, (1 << 20) + 1, n)], np.int64)
    offs = 1 + np.concatenate([[0], np.cumsum(L * ss + 3)[:-1]])
    buf = torch.empty((1, int(L * ss.sum()) + 3 * n + 16), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, buf.shape[1])
    flat = buf.view(-1)
    stripes = [(buf.data_ptr() + int(o), int(s)) for o, s in zip(offs, ss)]
    plan = B.StripePlan(enc, stripes=stripes)
    plan.encode()
    torch.cuda.synchronize()
    clean = buf.clone()
    # 1 % of the stripes: shard j1 bad at p1, and for `two` shard j2 at p2 != p1 as well
    hit = np.sort(rng.permutation(n)[:max(1, n // 100)])
    j1 = rng.integers(0, L, hit.size)
    j2 = (j1 + 1 + rng.integers(0, L - 1, hit.size)) % L
    p1 = np.array([int(rng.integers(s)) for s in ss[hit]], np.int64)
    p2 = (p1 + 1 + np.array([int(rng.integers(s - 1)) for s in ss[hit]], np.int64)) % ss[hit]
    at1 = torch.from_numpy(offs[hit] + j1 * ss[hit] + p1).cuda()
    at2 = torch.cat([at1, torch.from_numpy(offs[hit] + j2 * ss[hit] + p2).cuda()])
    flags, zero, fixed, where = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4))
    two_out = np.ones((hit.size, L), np.uint8)
    two_out[np.arange(hit.size), j1] = 0
    two_out[np.arange(hit.size), j2] = 0

    # the calls through the ABI with the masks resolved once, as a sweep holds them
    lib, stream = N.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pats, idx = np.ones((1, L), np.uint8), np.zeros(n, np.uint32)
    common = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), 1, idx.ctypes.data_as(U32P))

    def verify():
        RS.check(lib.hbec_verify_plan_mixed(*common, C.c_void_p(flags.data_ptr()), stream))

    def call(fn, out, f=None):
        a = common + (None if f is None else C.c_void_p(f.data_ptr()), C.c_void_p(out.data_ptr()), stream)
        return lambda: RS.check(fn(*a))

    correct_all, correct_zero = call(lib.hbec_correct_plan_mixed, fixed), call(lib.hbec_correct_plan_mixed, fixed, zero)
    correct_flagged = call(lib.hbec_correct_plan_mixed, fixed, flags)

    def xor(at):
        flat[at] ^= 0x5A

    def alt():
        bad = np.nonzero(flags.cpu().numpy() & 1)[0]
        B.StripePlan(enc, stripes=[stripes[i] for i in bad]).reconstruct_mixed(two_out)
        torch.cuda.synchronize()  # the small plan is freed when the call returns

    def group(name, legs, at, bits=None):
        ms = measure(legs, rounds)
        if at is not None:  # one more pass, looked at: exactly the bad shards corrected, nothing left
            xor(at)
            fixed.zero_()
            correct_flagged()
            want = np.zeros(n, np.uint32)
            want[hit] = N.COR_BAD | bits
            assert np.array_equal(fixed.cpu().numpy().view(np.uint32), want), f"{name}: wrong words"
        assert torch.equal(buf, clean), f"{name}: the buffers differ from the encoded ones"
        med = {q: statistics.median(v) for q, v in ms.items()}
        for q in legs:
            d = {"shape": f"{k}+{m} {n} objects", "group": name, "leg": q, "ms": round(med[q], 5),
                 "ms_min": round(min(ms[q]), 5), "ms_max": round(max(ms[q]), 5), "rounds": rounds, "reps": legs[q][1],
                 "bad_stripes": 0 if at is None else int(hit.size), "shard_bytes": int(L * ss.sum())}
            if name == "clean" and q != "v":
                d["time_ratio_over_v"] = round(med[q] / med["v"], 3)
            if q in ("f1", "f2", "alt"):
                d["ms_less_setup"] = round(med[q] - (med["x" + q[1]] / 2 if q != "alt" else 0.0), 5)
            emit(d)

    group("clean", {"v": (verify, REPS), "l": (call(lib.hbec_locate_plan_mixed, where), REPS),
                    "c": (correct_all, REPS), "z": (correct_zero, REPS_SHORT)}, None)
    assert not flags.any() and not fixed.any() and not where.any()
    for name, tag, at, bits in (("one", "1", at1, 1 << j1), ("two", "2", at2, (1 << j1) | (1 << j2))):
        xor(at)
        flags.zero_()
        verify()
        xor(at)  # every leg puts the errors in itself
        assert set(np.nonzero(flags.cpu().numpy() & 1)[0]) == set(hit.tolist())
        legs = {"x" + tag: (lambda at=at: (xor(at), xor(at)), REPS_SHORT),
                "f" + tag: (lambda at=at: (xor(at), correct_flagged()), REPS_SHORT)}
        if name == "two":
            legs["alt"] = (alt, REPS)
        group(name, legs, at, bits.astype(np.uint32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "correct_plan.jsonl"))
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
