#!/usr/bin/env python3
"""The ShardHash of multi-stripe shard files on a plan (hbec_hash_plan_files)
against the ways the same job was done without it, at 4+2 and 8+3.

(a) One-stripe objects: the workload of bench_hash_plan.py (4096 objects of
    random odd sizes, 4 KiB to 1 MiB), every object one entry.  Legs `mixed`
    (hbec_hash_plan_mixed, the yardstick) and `files` (hbec_hash_plan_files on
    the same plan), digests only, both through the C ABI with the arguments
    built once.
(b) Multi-stripe objects: 1024 objects of 1..16 stripes, odd piece lengths near
    64 KiB.  Legs `files` (one hash_files call) and `stream` (per object
    hbec_md5_new(k + m, 1), one hbec_md5_update per stripe, hbec_md5_final).
    The call is bounded by its longest chain: `files1` is hash_files filtered to
    the longest object alone, `plan1` hash_mixed over ONE chain of the same
    length on a plan of its own, both as us per 64-B block of that chain.
(c) The sweep on (b)'s plan: every object has lost m - 1 shard files, 1 % of
    the stripes have one flipped bit.  `sweep` is repair_mixed ->
    hash_files(filter=flags) -> heal_mixed and a synchronize; `trip` the host
    trip: repair_mixed, flags.cpu(), the flagged objects' present files through
    the streaming API, digests.cpu(), compare on the host, a plan of the flagged
    entries, repair_mixed on it with the differing file cleared, synchronize.
    Both on the wall clock, the bits flipped again before every pass.

Method as bench_hash_plan.py: legs interleaved round by round in alternating
order, 5 rounds of 3 back-to-back calls between HIP events (the calls' host side
inside the bracket; `host_ms` is that share), median [min - max].  Nothing is
gated.  32 sampled digests are compared with hashlib, and after the sweep the
named files, the healed words and sampled stripes are checked.

    python scripts/bench_hash_files.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--part a|b|c]
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from bench_hash_plan import measure, summary  # noqa: E402
from hummingbird_amd import _native as N  # noqa: E402
from hummingbird_amd import batch as B  # noqa: E402
from hummingbird_amd import reedsolomon as RS  # noqa: E402
from hummingbird_amd import shardhash as H  # noqa: E402

REPS = 3


class Sweep:
    """A stripe plan over `pieces` (one shard length per entry), databufs at odd
    offsets in one filled buffer, encoded."""

    def __init__(self, enc, pieces):
        self.enc, self.L = enc, enc.DataShards + enc.ParityShards
        self.ss = np.asarray(pieces, np.int64)
        n = len(self.ss)
        self.buf = torch.empty((1, int(self.L * self.ss.sum()) + 3 * n + 16), dtype=torch.uint8, device="cuda")
        B.fill_splitmix(self.buf, self.buf.shape[1])
        self.offs, pos = [], 1
        for s in self.ss:
            self.offs.append(pos)
            pos += self.L * int(s) + 3
        self.items = [(self.buf.data_ptr() + o, int(s)) for o, s in zip(self.offs, self.ss)]
        self.plan = B.StripePlan(enc, stripes=self.items)
        self.plan.encode()
        torch.cuda.synchronize()
        self.flat = self.buf.view(-1)

    def off(self, i, j):
        return self.offs[i] + j * int(self.ss[i])

    def file_md5(self, ents, j):
        h = hashlib.md5()
        for i in ents:
            o = self.off(int(i), j)
            h.update(self.flat[o:o + int(self.ss[i])].cpu().numpy().tobytes())
        return h.digest()


def emitter(emit, shape, rounds):
    def leg(part, name, samples, **more):
        d = {"shape": shape, "part": part, "leg": name, **summary(samples), "rounds": rounds, "reps": REPS, **more}
        emit(d)
        return d
    return leg


def part_a(k, m, rounds, emit):
    enc, L, n = RS.New(k, m), k + m, 4096
    rng = np.random.default_rng(300 * k + m)
    lens = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    w = Sweep(enc, [-(-x // k) for x in lens])
    shape = f"{k}+{m} {n} one-stripe objects"
    leg = emitter(emit, shape, rounds)
    starts = np.arange(n + 1, dtype=np.uint32)
    d_mixed = torch.zeros(n * L * 16, dtype=torch.uint8, device="cuda")
    d_files = torch.zeros(n * L * 16, dtype=torch.uint8, device="cuda")
    # the C calls, arguments built once, as bench_hash_plan.py times hash_mixed
    lib, u32p = N.lib(), C.POINTER(C.c_uint32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows, zeros = np.ones((1, L), np.uint8), np.zeros(n, np.uint32)
    sel = (rows.ctypes.data_as(N._U8P), 1, zeros.ctypes.data_as(u32p), None, 1, None)
    mixed = (enc.handle, w.plan._h, *sel, C.c_void_p(d_mixed.data_ptr()), None, None, stream)
    files = (enc.handle, w.plan._h, starts.ctypes.data_as(u32p), n, *sel, C.c_void_p(d_files.data_ptr()), None, None,
             stream)
    ms = measure({"mixed": (lambda: RS.check(lib.hbec_hash_plan_mixed(*mixed)), "events"),
                  "files": (lambda: RS.check(lib.hbec_hash_plan_files(*files)), "events")}, rounds)
    assert torch.equal(d_mixed, d_files), "hash_files differs from hash_mixed"
    got = d_files.cpu().numpy().reshape(n, L, 16)
    for i, j in zip(rng.integers(0, n, 32), rng.integers(0, L, 32)):
        assert bytes(got[i, j]) == w.file_md5([i], int(j)), "digest differs from hashlib"
    common = dict(chains=n * L, shard_bytes=int(L * w.ss.sum()), longest_chain=int(w.ss.max()))
    a = leg("a", "mixed", ms["mixed"], **common)
    f = leg("a", "files", ms["files"], **common)
    emit({"shape": shape, "part": "a", "compare": "files / mixed", "ratio": round(f["ms"] / a["ms"], 4),
          "behind_beyond_mixed_spread": bool(f["ms"] - a["ms"] > a["spread"] * a["ms"])})


def part_bc(k, m, rounds, emit, parts):
    enc, L, n_obj = RS.New(k, m), k + m, 1024
    rng = np.random.default_rng(500 * k + m)
    lib = N.lib()
    stripes = rng.integers(1, 17, n_obj)
    pieces = [int(x) | 1 for x in rng.integers(60000, 70000, int(stripes.sum()))]
    w = Sweep(enc, pieces)
    ne = len(pieces)
    starts = np.concatenate([[0], np.cumsum(stripes)]).astype(np.uint32)
    obj_of = np.repeat(np.arange(n_obj), stripes)
    totals = np.array([int(w.ss[starts[g]:starts[g + 1]].sum()) for g in range(n_obj)])
    shape = f"{k}+{m} {n_obj} objects of 1..16 stripes"
    leg = emitter(emit, shape, rounds)
    base = w.buf.data_ptr()

    expected = torch.zeros(n_obj * L * 16, dtype=torch.uint8, device="cuda")
    w.plan.hash_files(starts, None, digests=expected)
    torch.cuda.synchronize()
    exp_host = expected.cpu().numpy().reshape(n_obj, L, 16)
    for g, j in zip(rng.integers(0, n_obj, 32), rng.integers(0, L, 32)):
        assert bytes(exp_host[g, j]) == w.file_md5(range(starts[g], starts[g + 1]), int(j)), "digest differs from hashlib"

    def stream_hash(objects, shards_of, out):
        """The parent's way: per object a chain set, one update per stripe.  out: [len(objects), L, 16]."""
        for q, g in enumerate(objects):
            js = shards_of(g)
            ch = H.MD5Chains(len(js), 1)
            for i in range(starts[g], starts[g + 1]):
                ch.update([(base + w.off(i, j), 0) for j in js], int(w.ss[i]))
            ch.final(out[q, :len(js)])
            ch.close()

    if "b" in parts:
        d_files = torch.zeros(n_obj * L * 16, dtype=torch.uint8, device="cuda")
        d_stream = torch.zeros((n_obj, L, 16), dtype=torch.uint8, device="cuda")
        every = list(range(L))
        g_long = int(np.argmax(totals))
        f_long = np.zeros(ne, np.int32)
        f_long[starts[g_long]] = 1
        f_long = torch.from_numpy(f_long).cuda()
        d_one = torch.zeros(n_obj * L * 16, dtype=torch.uint8, device="cuda")
        one_sel = np.zeros((n_obj, L), np.uint8)
        one_sel[g_long, 0] = 1
        # one chain of the same length, contiguous, on a plan of its own
        single = Sweep(enc, [int(totals[g_long])])
        s_sel = np.zeros((1, L), np.uint8)
        s_sel[0, 0] = 1
        d_single = torch.zeros(L * 16, dtype=torch.uint8, device="cuda")
        legs = {"files": (lambda: w.plan.hash_files(starts, None, digests=d_files), "events"),
                "stream": (lambda: stream_hash(range(n_obj), lambda g: every, d_stream), "events"),
                "files1": (lambda: w.plan.hash_files(starts, one_sel, digests=d_one, filter=f_long), "events"),
                "plan1": (lambda: single.plan.hash_mixed(s_sel, digests=d_single), "events")}
        ms = measure(legs, rounds)
        assert torch.equal(d_files, expected) and torch.equal(d_stream.view(-1), expected)
        common = dict(chains=n_obj * L, entries=ne, shard_bytes=int(L * w.ss.sum()), longest_chain=int(totals.max()))
        f = leg("b", "files", ms["files"], **common)
        s = leg("b", "stream", ms["stream"], host_calls=int(n_obj * 2 + ne), **common)
        blocks = int(totals.max()) // 64
        f1 = leg("b", "files1", ms["files1"], chains=1, us_per_block=round(1e3 * summary(ms["files1"])["ms"] / blocks, 5))
        p1 = leg("b", "plan1", ms["plan1"], chains=1, us_per_block=round(1e3 * summary(ms["plan1"])["ms"] / blocks, 5))
        emit({"shape": shape, "part": "b", "compare": "stream / files", "ratio": round(s["ms"] / f["ms"], 2),
              "stream_host_share": round(s["host_ms"] / s["ms"], 3), "files_host_share": round(f["host_ms"] / f["ms"], 3),
              "files_over_longest_alone": round(f["ms"] / f1["ms"], 3),
              "files1_over_plan1": round(f1["ms"] / p1["ms"], 4), "GBps": round(common["shard_bytes"] / f["ms"] / 1e6, 2)})

    if "c" not in parts:
        return
    present_obj = np.ones((n_obj, L), np.uint8)
    for g in range(n_obj):
        present_obj[g][rng.choice(L, size=m - 1, replace=False)] = 0
    present = present_obj[obj_of]
    pats, idx = np.unique(present, axis=0, return_inverse=True)
    pats = np.ascontiguousarray(pats, np.uint8)
    idx = np.ascontiguousarray(idx.reshape(-1), np.uint32)
    w.plan.reconstruct_mixed(present)  # missing files hold what the others imply
    torch.cuda.synchronize()
    hit_ents = rng.permutation(ne)[:max(1, ne // 100)]
    hit_ents = np.array(sorted({int(obj_of[e]): int(e) for e in hit_ents}.values()))  # one per object
    hit_file = {int(e): int(rng.choice(np.nonzero(present[e])[0])) for e in hit_ents}
    hit_at = torch.tensor([w.off(e, j) + int(rng.integers(w.ss[e])) for e, j in hit_file.items()], device="cuda")
    sample = [int(e) for e in rng.permutation(ne)[:16]] + [int(e) for e in hit_ents[:8]]
    snap = {e: w.flat[w.offs[e]:w.offs[e] + L * int(w.ss[e])].clone() for e in sample}
    flags, where, healed = (torch.zeros(ne, dtype=torch.int32, device="cuda") for _ in range(3))
    bad = torch.zeros(n_obj, dtype=torch.int32, device="cuda")

    def flip():
        w.flat[hit_at] ^= 0x10
        for t in (flags, bad, where, healed):
            t.zero_()

    def sweep():
        w.plan.repair_mixed(present, flags)
        w.plan.hash_files(starts, present_obj, expected=expected, bad=bad, where=where, filter=flags)
        w.plan.heal_mixed(present, where, healed)

    def trip():
        w.plan.repair_mixed(present, flags)
        sel = np.nonzero(flags.cpu().numpy() & 1)[0]
        objs = sorted({int(obj_of[e]) for e in sel})
        dig = torch.empty((len(objs), L, 16), dtype=torch.uint8, device="cuda")
        stream_hash(objs, lambda g: [int(j) for j in np.nonzero(present_obj[g])[0]], dig)
        got = dig.cpu().numpy()
        again = present[sel].copy()
        for q, g in enumerate(objs):
            for r, j in enumerate(np.nonzero(present_obj[g])[0]):
                if not np.array_equal(got[q, r], exp_host[g, j]):
                    again[obj_of[sel] == g, j] = 0
        sub = B.StripePlan(enc, stripes=[w.items[e] for e in sel])
        f2 = torch.zeros(sel.size, dtype=torch.int32, device="cuda")
        sub.repair_mixed(again, f2)

    ms = measure({"sweep": (sweep, flip), "trip": (trip, flip)}, rounds)
    d = leg("c", "sweep", ms["sweep"], flagged=int(hit_ents.size), entries=ne)
    dy = leg("c", "trip", ms["trip"], flagged=int(hit_ents.size), entries=ne)
    emit({"shape": shape, "part": "c", "compare": "trip / sweep", "ratio": round(dy["ms"] / d["ms"], 2),
          "faster_beyond_spread": bool(dy["ms"] - d["ms"] > max(dy["spread"] * dy["ms"], d["spread"] * d["ms"]))})
    # the sweep once more, checked
    flip()
    sweep()
    torch.cuda.synchronize()
    named = B.locate_decode(k, m, present, where.cpu().numpy())
    assert all(int(named[e]) == j for e, j in hit_file.items()), "a file is not named"
    assert (np.delete(named, hit_ents) == N.LOC_CLEAN).all()
    want_b = np.zeros(n_obj, np.int32)
    for e, j in hit_file.items():
        want_b[obj_of[e]] = 1 << j
    assert np.array_equal(bad.cpu().numpy(), want_b), "bad words are wrong"
    want_h = np.zeros(ne, np.int32)
    want_h[hit_ents] = N.HEAL_DONE | 2
    assert np.array_equal(healed.cpu().numpy(), want_h), "healed words are wrong"
    for e, s in snap.items():
        assert torch.equal(w.flat[w.offs[e]:w.offs[e] + L * int(w.ss[e])], s), f"stripe {e} is not what it was"
    bad.zero_()
    w.plan.hash_files(starts, None, expected=expected, bad=bad)
    assert not bad.any(), "a file's hash differs after the sweep"
    emit({"shape": shape, "part": "c", "state": "checked", "stripes_compared": len(snap), "named": int(hit_ents.size)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hash_files.jsonl"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", default=None, choices=["4+2", "8+3"])
    ap.add_argument("--part", default="abc")
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
                if "a" in a.part:
                    part_a(k, m, a.rounds, emit)
                if "b" in a.part or "c" in a.part:
                    part_bc(k, m, a.rounds, emit, a.part)


if __name__ == "__main__":
    main()
