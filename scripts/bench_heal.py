#!/usr/bin/env python3
"""The heal pass of a repair sweep (hbec_heal_plan_mixed) against what a caller
had to do without it, at 4+2 and 8+3.

Workload: 4096 objects of random odd sizes, 4 KiB to 1 MiB (S = ceil(len / k)),
as a stripe plan (databufs at odd offsets) and as an object plan (data arena +
parity arena).  Masks as scripts/bench_locate.py: 4+2 every shard present; 8+3
drawn uniformly from all present and the 11 single losses.  Three states of the
same buffers, one after the other, and in each the legs interleaved:

  one_pct    1 % of the stripes have one flipped byte; repair_mixed and
             locate_mixed(flags=flags) have run once, so `where` names them.
             h    heal_mixed, HIP events around the calls
             hw   heal_mixed and a synchronize, on the wall clock
             y    the yardstick, unchanged code, on the wall clock: where.cpu(),
                  locate_decode, a StripePlan of the flagged entries,
                  repair_mixed on it with the named shard cleared (new masks,
                  so their patterns are built here), synchronize
  zero       `where` all zero: nothing to do but walk the list.
             h    heal_mixed
             z    locate_mixed filtered by all-zero flags (the yardstick)
  all_named  every stripe has one flipped byte and is named.
             h    heal_mixed
             r    repair_mixed on the same plan with the named shard cleared in
                  every mask (the yardstick: the same bytes moved)

Method: a warm-up, then `rounds` rounds in which the legs run in
alternating order.  Event legs time `reps` back-to-back calls, the calls' host
side inside the bracket, and note beside it how long the calls took to return
(host share).  Wall-clock legs time one pass each.  Medians, with the smallest
and largest round and their spread (max - min) / median.  Nothing is gated.
After the timing every stripe is flipped again, the sweep repair_mixed ->
locate_mixed -> heal_mixed runs once with no synchronisation in between, and
every flag and all shards of 24 sampled stripes are checked: the stripes were
snapshotted after encode and shown to be codewords by the oracle.

    python scripts/bench_heal.py [--out FILE] [--rounds N] [--shape 4+2|8+3] [--objects N]
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
from oracle import coracle as CO  # noqa: E402

REPS = 20
U32P = C.POINTER(C.c_uint32)


def timed_events(fn, reps):
    """(device ms per call, host ms per call until the calls returned)"""
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


def timed_wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    extra = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, extra


def measure(legs, rounds):
    """legs: name -> (fn, 'events' | 'wall').  Returns name -> [(ms, extra)]."""
    for fn, _ in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in legs}
    names = list(legs)
    for r in range(rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            fn, how = legs[name]
            out[name].append(timed_events(fn, REPS) if how == "events" else timed_wall(fn))
    return out


def summary(samples):
    ms = [s[0] for s in samples]
    med = statistics.median(ms)
    return {"ms": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5),
            "spread": round((max(ms) - min(ms)) / med, 4)}


def run(k, m, n, rounds, emit):
    enc = RS.New(k, m)
    L = k + m
    rng = np.random.default_rng(100 * k + m)
    masks = [[1] * L]
    if m >= 3:
        masks += [[0 if i == j else 1 for i in range(L)] for j in range(L)]
    pats = np.ascontiguousarray(masks, np.uint8)
    idx = np.ascontiguousarray(rng.integers(0, len(masks), n), np.uint32)
    present = pats[idx]
    lib = N.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lens = [int(x) | 1 for x in rng.integers(4096, (1 << 20) + 1, n)]
    ss = np.array([-(-x // k) for x in lens], np.int64)
    shape = f"{k}+{m} {n} objects"
    order = rng.permutation(n)
    hit_shard = np.array([int(rng.choice(np.nonzero(present[i])[0])) for i in range(n)], np.int64)
    hit_pos = np.array([int(rng.integers(s)) for s in ss], np.int64)
    one_pct = order[:max(1, n // 100)]
    sample = order[-24:]
    parity_rows = CO.build_matrix(k, m)[k:]

    for layout in ("stripes", "objects"):
        if layout == "stripes":
            buf = torch.empty((1, int(L * ss.sum()) + 3 * n + 16), dtype=torch.uint8, device="cuda")
            B.fill_splitmix(buf, buf.shape[1])
            offs, pos = [], 1
            for s in ss:
                offs.append(pos)
                pos += L * int(s) + 3
            items = [(buf.data_ptr() + o, int(s)) for o, s in zip(offs, ss)]
            plan = B.StripePlan(enc, stripes=items)
            flat = [buf.view(-1)]
            shard_at = lambda i, j: (0, offs[i] + j * int(ss[i]))  # noqa: E731
            sub_plan = lambda sel: B.StripePlan(enc, stripes=[items[i] for i in sel])  # noqa: E731
        else:
            data = torch.empty((1, int(k * ss.sum()) + 16), dtype=torch.uint8, device="cuda")
            B.fill_splitmix(data, data.shape[1])
            par = torch.empty(int(m * ss.sum()) + 16, dtype=torch.uint8, device="cuda")
            items, do, po, dos, pos_ = [], 1, 3, [], []
            for s in ss:
                items.append((data.data_ptr() + do, par.data_ptr() + po, int(s)))
                dos.append(do)
                pos_.append(po)
                do += k * int(s)
                po += m * int(s)
            plan = B.StripePlan(enc, objects=items)
            flat = [data.view(-1), par]
            shard_at = lambda i, j: ((0, dos[i] + j * int(ss[i])) if j < k  # noqa: E731
                                     else (1, pos_[i] + (j - k) * int(ss[i])))
            sub_plan = lambda sel: B.StripePlan(enc, objects=[items[i] for i in sel])  # noqa: E731
        plan.encode()
        torch.cuda.synchronize()

        def shard_bytes(i, j):
            b, o = shard_at(i, j)
            return flat[b][o:o + int(ss[i])].cpu().numpy()

        snap = {int(i): [shard_bytes(i, j) for j in range(L)] for i in sample}
        for i, shards in snap.items():  # codewords, says the oracle
            for want, got in zip(CO.apply(parity_rows, shards[:k]), shards[k:]):
                assert np.array_equal(want, got), "encode differs from the oracle"

        def flip(chosen):
            for b in range(len(flat)):
                at = [shard_at(i, int(hit_shard[i])) for i in chosen]
                idx = [o + int(hit_pos[i]) for (bb, o), i in zip(at, chosen) if bb == b]
                if idx:
                    flat[b][torch.tensor(idx, device="cuda")] ^= 0x5A

        flags = torch.zeros(n, dtype=torch.int32, device="cuda")
        zero_flags = torch.zeros(n, dtype=torch.int32, device="cuda")
        where = torch.zeros(n, dtype=torch.int32, device="cuda")
        zero_where = torch.zeros(n, dtype=torch.int32, device="cuda")
        hflags = torch.zeros(n, dtype=torch.int32, device="cuda")

        def locate_state(chosen):
            """Flip `chosen`, then repair and locate once: `where` names them."""
            flip(chosen)
            flags.zero_()
            where.zero_()
            plan.repair_mixed(present, flags)
            plan.locate_mixed(present, where, flags=flags)
            torch.cuda.synchronize()
            named = B.locate_decode(k, m, present, where.cpu().numpy())
            want = np.full(n, N.LOC_CLEAN, np.int64)
            want[chosen] = hit_shard[chosen]
            assert np.array_equal(named, want), "locate names wrong shards"
            return named

        # the timed calls go to the library as bench_locate.py's do: the masks are the
        # ones locate was given, so their patterns are not built again per call
        common = (enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0], idx.ctypes.data_as(U32P))

        def heal_leg(w):
            a = common + (C.c_void_p(w.data_ptr()), C.c_void_p(hflags.data_ptr()), stream)
            return lambda: RS.check(lib.hbec_heal_plan_mixed(*a))

        def yardstick():
            """The parent commit's way; returns the device ms of its repair."""
            w = where.cpu().numpy()
            named = B.locate_decode(k, m, present, w)
            sel = np.nonzero(named >= 0)[0]
            again = present[sel].copy()
            again[np.arange(sel.size), named[sel]] = 0
            sub = sub_plan(sel)
            f2 = torch.zeros(sel.size, dtype=torch.int32, device="cuda")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sub.repair_mixed(again, f2)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def emit_leg(state, leg, samples, **more):
            d = {"shape": shape, "layout": layout, "state": state, "leg": leg, **summary(samples), "rounds": rounds}
            d.update(more)
            emit(d)
            return d

        # ---- 1. 1 % of the stripes corrupt ----
        locate_state(one_pct)
        legs = {"h": (heal_leg(where), "events"), "hw": (heal_leg(where), "wall"), "y": (yardstick, "wall")}
        ms = measure(legs, rounds)
        h = emit_leg("one_pct", "h", ms["h"], reps=REPS, named=int(one_pct.size),
                     host_ms=round(statistics.median(s[1] for s in ms["h"]), 5))
        hw = emit_leg("one_pct", "hw", ms["hw"], named=int(one_pct.size))
        y_dev = statistics.median(s[1] for s in ms["y"])
        y = emit_leg("one_pct", "y", ms["y"], named=int(one_pct.size), repair_device_ms=round(y_dev, 5))
        emit({"shape": shape, "layout": layout, "state": "one_pct", "compare": "y / hw",
              "ratio": round(y["ms"] / hw["ms"], 2), "host_share_of_y": round(1 - y_dev / y["ms"], 4),
              "faster_beyond_spread": bool(y["ms"] - hw["ms"] > max(y["spread"] * y["ms"], hw["spread"] * hw["ms"])),
              "h_device_ms": h["ms"]})

        # ---- 2. nothing named ----
        z_args = common + (C.c_void_p(zero_flags.data_ptr()), C.c_void_p(where.data_ptr()), stream)
        legs = {"h": (heal_leg(zero_where), "events"),
                "z": (lambda: RS.check(lib.hbec_locate_plan_mixed(*z_args)), "events")}
        ms = measure(legs, rounds)
        h = emit_leg("zero", "h", ms["h"], reps=REPS, host_ms=round(statistics.median(s[1] for s in ms["h"]), 5))
        z = emit_leg("zero", "z", ms["z"], reps=REPS, host_ms=round(statistics.median(s[1] for s in ms["z"]), 5))
        emit({"shape": shape, "layout": layout, "state": "zero", "compare": "h / z", "ratio": round(h["ms"] / z["ms"], 3),
              "inside_z_spread": bool(abs(h["ms"] - z["ms"]) <= z["spread"] * z["ms"])})

        # ---- 3. every stripe named ----
        plan.heal_mixed(present, where, hflags)  # the 1 % are clean again
        named = locate_state(np.arange(n))
        cleared = present.copy()
        cleared[np.arange(n), named] = 0
        rflags = torch.zeros(n, dtype=torch.int32, device="cuda")
        cpats, cidx = np.unique(cleared, axis=0, return_inverse=True)
        cpats = np.ascontiguousarray(cpats, np.uint8)
        cidx = np.ascontiguousarray(cidx.reshape(-1), np.uint32)
        r_args = (enc.handle, plan._h, cpats.ctypes.data_as(N._U8P), cpats.shape[0], cidx.ctypes.data_as(U32P), 0,
                  C.c_void_p(rflags.data_ptr()), stream)
        legs = {"h": (heal_leg(where), "events"), "r": (lambda: RS.check(lib.hbec_repair_plan_mixed(*r_args)), "events")}
        ms = measure(legs, rounds)
        moved = int(L * ss.sum())  # k + r_c shards read, r_o written: every shard of every stripe once
        h = emit_leg("all_named", "h", ms["h"], reps=REPS, host_ms=round(statistics.median(s[1] for s in ms["h"]), 5),
                     bytes_moved=moved)
        r = emit_leg("all_named", "r", ms["r"], reps=REPS, host_ms=round(statistics.median(s[1] for s in ms["r"]), 5),
                     bytes_moved=moved)
        emit({"shape": shape, "layout": layout, "state": "all_named", "compare": "h / r",
              "ratio": round(h["ms"] / r["ms"], 3), "inside_r_spread": bool(abs(h["ms"] - r["ms"]) <= r["spread"] * r["ms"]),
              "host_share_h": round(h["host_ms"] / h["ms"], 4), "host_share_r": round(r["host_ms"] / r["ms"], 4),
              "masks": int(len(np.unique(present, axis=0))), "cleared_masks": int(len(np.unique(cleared, axis=0)))})

        # ---- the sweep once more, checked ----
        plan.heal_mixed(present, where, hflags)
        torch.cuda.synchronize()
        flip(np.arange(n))
        flags.zero_()
        where.zero_()
        hflags.zero_()
        s0 = B.heal_plan_stats()
        plan.repair_mixed(present, flags)
        plan.locate_mixed(present, where, flags=flags)
        plan.heal_mixed(present, where, hflags)
        torch.cuda.synchronize()
        s1 = B.heal_plan_stats()
        assert s1["kernel_launches"] - s0["kernel_launches"] == 1 and s1["skipped_entries"] == s0["skipped_entries"]
        assert (flags.cpu().numpy() & 1).all(), "repair_mixed missed a flipped stripe"
        assert np.array_equal(hflags.cpu().numpy(), np.full(n, N.HEAL_DONE, np.int32)), "heal flags are wrong"
        for i, shards in snap.items():
            for j in range(L):
                assert np.array_equal(shard_bytes(i, j), shards[j]), f"stripe {i} shard {j} is not the codeword's"
        emit({"shape": shape, "layout": layout, "state": "checked", "flags": n, "stripes_compared": len(snap),
              "launches_per_heal": 1})
        del plan, flat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "heal_plan.jsonl"))
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
