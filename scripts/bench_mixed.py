#!/usr/bin/env python3
"""Device-resident reconstruct of a batch whose objects lost DIFFERENT shards
(hbec_reconstruct_batch_mixed), at 4096 x 1 MiB 4+2 and 65 536 x 4 KiB 8+3.

Legs, every one rebuilding in place over the same encoded batch:

  a         one hbec_reconstruct_batch, one pattern ({0, 1} lost) for the whole
            batch: the ceiling
  b_random  what a caller can do without the mixed entry: one
            hbec_reconstruct_batch per run of consecutive equal-pattern objects
            (views advanced to the run), patterns drawn per object uniformly
            from all single and double losses
  b_sorted  the same with the objects' patterns sorted into contiguous runs
  c_random  one hbec_reconstruct_batch_mixed, the b_random patterns
  c_sorted  one hbec_reconstruct_batch_mixed, the b_sorted patterns

All argument arrays are built before the clock starts, so a leg's time is its
C calls and the GPU work.  Method: a warm-up, then `rounds`
rounds in which the legs run in alternating order, each timed by HIP events
around `reps` calls back to back; the median over the rounds is reported.
The events bracket the host side of the calls too, so a call whose host
preparation outlasts its kernels is charged for it.  Afterwards the c_random
patterns are erased for real, rebuilt, and checked (Encoder.Verify flags and
the regenerated data).

    python scripts/bench_mixed.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--no-runs] [--tag TEXT]

--no-runs leaves out the b legs (an A/B of two builds of the kernel needs
only a and c); --tag adds a "tag" field to every line.
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

PEAK = 8000.0


def losses(k, m, upto=2):
    out = []
    for e in range(1, upto + 1):
        for miss in itertools.combinations(range(k + m), e):
            out.append([0 if i in miss else 1 for i in range(k + m)])
    return np.array(out, dtype=np.uint8)


class Mixed:
    """Prebuilt arguments of one hbec_reconstruct_batch_mixed call."""

    def __init__(self, enc, views, present, n, s):
        pat, idx = np.unique(present, axis=0, return_inverse=True)
        self.pat = np.ascontiguousarray(pat, dtype=np.uint8)
        self.idx = np.ascontiguousarray(idx.reshape(-1), dtype=np.uint32)
        self.args = (enc.handle, B._views(views), self.pat.ctypes.data_as(N._U8P), self.pat.shape[0],
                     self.idx.ctypes.data_as(C.POINTER(C.c_uint32)), n, s, 0)

    def __call__(self, stream):
        RS.check(N.lib().hbec_reconstruct_batch_mixed(*self.args, stream))


class Runs:
    """Prebuilt arguments of one hbec_reconstruct_batch per run of equal patterns."""

    def __init__(self, enc, views, present, n, s):
        self.calls = []
        cut = np.flatnonzero((present[1:] != present[:-1]).any(axis=1)) + 1
        for o0, o1 in zip(np.concatenate([[0], cut]), np.concatenate([cut, [n]])):
            v = B._views([(b + int(o0) * st, st) for b, st in views])
            p = (C.c_uint8 * present.shape[1])(*present[o0].tolist())
            self.calls.append((enc.handle, v, p, int(o1 - o0), s, 0))

    def __call__(self, stream):
        f = N.lib().hbec_reconstruct_batch
        for a in self.calls:
            rc = f(*a, stream)
            if rc:
                RS.check(rc)


def timed(fn, stream, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn(stream)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def run(k, m, n, size, rounds, emit, runs=True):
    s = size // k
    enc = RS.New(k, m)
    objs = torch.empty((n, size), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(objs, size)
    par = torch.empty((n, m * s), dtype=torch.uint8, device="cuda")
    views = B.shard_views(objs, k, s) + B.shard_views(par, m, s)
    B.encode_views(enc, views, n, s)
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    lost = losses(k, m)
    rng = np.random.default_rng(k * 100 + m)
    random = lost[rng.integers(0, len(lost), n)]
    order = np.lexsort(random.T[::-1])
    sorted_ = random[order]
    uniform = np.array([[0, 0] + [1] * (k + m - 2)] * n, dtype=np.uint8)

    def nbytes(present):
        return int(((k + (present == 0).sum(axis=1)) * s).sum())

    legs = {
        "a": (Runs(enc, views, uniform, n, s), nbytes(uniform), 20),
        "b_sorted": (Runs(enc, views, sorted_, n, s), nbytes(sorted_), 5),
        "c_sorted": (Mixed(enc, views, sorted_, n, s), nbytes(sorted_), 20),
        "c_random": (Mixed(enc, views, random, n, s), nbytes(random), 20),
        "b_random": (Runs(enc, views, random, n, s), nbytes(random), 1),
    }
    assert len(legs["a"][0].calls) == 1
    if not runs:
        del legs["b_sorted"], legs["b_random"]
    for name, (fn, _, reps) in legs.items():  # warm-up (b_random once: it takes the longest)
        for _ in range(1 if name == "b_random" else 10):
            fn(stream)
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    names = list(legs)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            fn, _, reps = legs[name]
            ms[name].append(timed(fn, stream, reps))
    st0 = B.mixed_stats()
    legs["c_random"][0](stream)
    st1 = B.mixed_stats()
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, (fn, nb, reps) in legs.items():
        d = {"shape": f"{k}+{m} {n}x{size}", "leg": name, "ms": round(med[name], 5),
             "ms_min": round(min(ms[name]), 5), "ms_max": round(max(ms[name]), 5), "rounds": rounds, "reps": reps,
             "calls_per_rep": len(fn.calls) if isinstance(fn, Runs) else 1, "algorithmic_bytes": nb,
             "GB_s": round(nb / (med[name] * 1e-3) / 1e9, 1),
             "frac_of_8TBs": round(nb / (med[name] * 1e-3) / 1e9 / PEAK, 4)}
        if isinstance(fn, Mixed):
            d["patterns"] = int(fn.pat.shape[0])
            d["ratio_to_a"] = round(med[name] / med["a"], 3)
        if name == "c_random":
            d["launches_per_call"] = st1["mixed"] - st0["mixed"]
            if runs:
                d["speedup_over_b_random"] = round(med["b_random"] / med[name], 1)
        emit(d)

    # self-check: erase the c_random losses for real, rebuild, compare
    shards = [objs[:, i * s:(i + 1) * s] for i in range(k)] + [par[:, i * s:(i + 1) * s] for i in range(m)]
    gone = torch.from_numpy(random == 0).cuda()
    for i, t in enumerate(shards):
        t[gone[:, i]] = 0x6B
    legs["c_random"][0](stream)
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    B.verify_views(enc, views, n, s, flags)
    ref = torch.empty_like(objs)
    B.fill_splitmix(ref, size)
    torch.cuda.synchronize()
    assert int(flags.count_nonzero()) == 0, "rebuilt batch does not verify"
    assert torch.equal(objs, ref), "rebuilt data differs"
    if runs:
        assert med["c_random"] < med["b_random"], (med["c_random"], med["b_random"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default=None, choices=["4+2", "8+3"])
    ap.add_argument("--no-runs", action="store_true")
    ap.add_argument("--tag", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = open(a.out, "a") if a.out else None

    def emit(d):
        if a.tag:
            d["tag"] = a.tag
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    if a.shape in (None, "4+2"):
        run(4, 2, 4096, 1 << 20, a.rounds, emit, not a.no_runs)
    if a.shape in (None, "8+3"):
        run(8, 3, 65536, 4096, a.rounds, emit, not a.no_runs)


if __name__ == "__main__":
    main()
