"""Child process of tests/test_gpu_host_seams.py (run as a script, not collected).

The seams of the host path (csrc/hostpath.cpp) at a 1 MiB staging slot and a
1 MiB hash arena setting: column pieces of stripes wider than a slot, chunks
closed by bytes and by tile records, slot reuse beyond kSlots, pinned stripes
that straddle a record slot, hash arenas filled, flushed and reused.  The ring
reads its capacities when it is made, so the parent starts this script afresh
per mode with HBEC_HOST_SLOT_MB=1 and HBEC_HASH_ARENA_MB=1.

Every stripe is a slice of a larger backing buffer (pageable numpy memory or
pinned RS.HostBuffer) with 1..13 sentinel bytes before and after it, and after
every call the whole backing buffers are compared with the oracle image
(coracle build_matrix / apply; after a reconstruct the codeword).  Each batch
runs EncodeStripes and then ReconstructStripes for the loss patterns (0,),
(0, k) and range(min(m, 3)), lost shards garbled first; zero-length stripes
stand first, between and last.  Digests are compared with hashlib.md5.

The capacities and the cutting rules are restated here (not read from the
library) and the counters hbec_host_run_stats, hbec_stripes_kernel_stats and
hbec_host_md5_stats are read around every call.  Prints one JSON line.

    HBEC_HOST_SLOT_MB=1 HBEC_HASH_ARENA_MB=1 python tests/host_seams_child.py MODE
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import stripes_sweep_cases as SC  # noqa: E402
from hummingbird_amd import _native as N  # noqa: E402
from hummingbird_amd import batch as B  # noqa: E402
from hummingbird_amd import reedsolomon as RS  # noqa: E402
from oracle import coracle as CO  # noqa: E402

FILL, GARBLE = 0xA7, 0x5C
K_SLOTS = 3
SLOT = int(os.environ["HBEC_HOST_SLOT_MB"]) << 20
IN_CAP = OUT_CAP = SLOT
TILE_CAP = SLOT // 1024 + 1024
ARENA = max(int(os.environ["HBEC_HASH_ARENA_MB"]) << 20, IN_CAP + OUT_CAP)
N_ARENAS = 2
ODD_MIN_MAIN = 160  # odd_impl.h kOddMinMain: shorter shards have edge records only


def piece_width(K, R):
    return (min(IN_CAP // K, OUT_CAP // R) // 16) * 16


def ring_cut(K, R, lens):
    """(pieces, chunks) of the staged stripes of one call, as host_run_on cuts them"""
    T = SC.tile_bytes(K)
    W = piece_width(K, R)
    pieces = chunks = 0
    in_used = out_used = tiles = 0
    sizes = []  # in + out bytes of every chunk (md5: what it takes of an arena)
    for S in lens:
        for col in range(0, S, W):
            lpad = -(-min(W, S - col) // 16) * 16
            nt = -(-lpad // T)
            if in_used + K * lpad > IN_CAP or out_used + R * lpad > OUT_CAP or tiles + nt > TILE_CAP:
                if in_used:
                    chunks += 1
                    sizes.append(in_used + out_used)
                in_used = out_used = tiles = 0
            in_used += K * lpad
            out_used += R * lpad
            tiles += nt
            pieces += 1
    if in_used:
        chunks += 1
        sizes.append(in_used + out_used)
    return pieces, chunks, sizes


def flushes_of(sizes, rounded=False):
    """non-empty ArenaCursor flushes of a call that appends blocks of these
    sizes (finish included); the zero-copy runners ask for the block rounded
    up to 256 B, the ring for its bytes"""
    used = n = 0
    for b in sizes:
        if used + (((b + 255) & ~255) if rounded else b) > ARENA:
            n += 1
            used = 0
        used += (b + 255) & ~255
    return n + (1 if sizes else 0)


def zc_slots(K, lens):
    """record slots zero_copy_run fills: tiles run on from slot to slot"""
    T = SC.tile_bytes(K)
    return -(-sum(-(-S // T) for S in lens) // TILE_CAP)


def stats():
    s = dict(B.host_run_stats())
    s.update(B.stripes_kernel_stats())
    zc, ring = N.C.c_uint64(), N.C.c_uint64()
    assert N.lib().hbec_host_md5_stats(N.C.byref(zc), N.C.byref(ring)) == 0
    s["md5_zero_copy"], s["md5_ring"] = zc.value, ring.value
    return s


def delta(s0, s1):
    return {f: s1[f] - s0[f] for f in s0 if s1[f] != s0[f]}


class Batch:
    """Stripes of one shape in backing buffers.  specs: (S, where) with where
    'page' (pageable, even and odd addresses in turn), 'pin' (pinned, 16-B
    aligned) or 'pinodd' (pinned, at an odd address)."""

    def __init__(self, k, m, specs, seed):
        self.k, self.m, self.specs = k, m, list(specs)
        n = k + m
        need = {"page": 64, "pin": 64}
        for S, where in self.specs:
            need["page" if where == "page" else "pin"] += n * S + 48
        self.hb = RS.HostBuffer(need["pin"]) if need["pin"] > 64 else None
        self.back = {"page": np.empty(need["page"], np.uint8)}
        if self.hb is not None:
            self.back["pin"] = self.hb.array
        pos = {"page": 0, "pin": 0}
        self.slices = []
        for i, (S, where) in enumerate(self.specs):
            b = "page" if where == "page" else "pin"
            base = self.back[b].ctypes.data
            p = pos[b] + 1 + (5 * i) % 13  # 1..13 sentinel bytes
            if where == "pin":
                p += -(base + p) % 16
            elif where == "pinodd":
                p += (1 + 2 * (i % 8) - (base + p)) % 16
            else:
                p += (i - (base + p)) % 2
            self.slices.append((b, p, n * S))
            pos[b] = p + n * S
        for b in self.back:
            assert pos[b] + 13 <= self.back[b].size
        # the codeword image
        lens = [S for S, _ in self.specs]
        col = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rng = np.random.default_rng(seed)
        data = rng.integers(0, 256, (k, max(1, int(col[-1]))), dtype=np.uint8)
        par = CO.apply(CO.build_matrix(k, m)[k:], list(data))
        cw = np.concatenate([data, np.stack(par)])
        self.want = {b: np.full(a.size, FILL, np.uint8) for b, a in self.back.items()}
        for (b, p, ln), S, c in zip(self.slices, lens, col):
            self.want[b][p:p + ln].reshape(n, S)[:] = cw[:, c:c + S] if S else 0
        self.errors = []

    def stripes(self):
        return [self.back[b][p:p + ln] for b, p, ln in self.slices]

    def start(self, lost):
        for b, a in self.back.items():
            a[:] = self.want[b]
        for (b, p, ln), (S, _) in zip(self.slices, self.specs):
            for i in lost:
                self.back[b][p + i * S:p + (i + 1) * S] = GARBLE

    def check(self, what):
        for b, a in self.back.items():
            bad = np.flatnonzero(a != self.want[b])
            if bad.size:
                o = int(bad[0])
                where = "sentinel"
                for j, ((bb, p, ln), (S, w)) in enumerate(zip(self.slices, self.specs)):
                    if bb == b and p <= o < p + ln:
                        where = f"stripe {j} ({w}, S={S}) shard {(o - p) // S} position {(o - p) % S}"
                self.errors.append(f"{self.k}+{self.m} {what}: {bad.size} bytes of the {b} buffer differ; first at "
                                   f"{where}: got {int(a[o])} want {int(self.want[b][o])}")
                return False
        return True

    def patterns(self):
        k, m = self.k, self.m
        out = []
        for lost in ((0,), (0, k), tuple(range(min(m, 3)))):
            if len(lost) <= m and lost not in out:
                out.append(lost)
        return out

    def run_all(self, enc=None):
        """encode, then every reconstruct pattern: [(what, lost, counter deltas)]"""
        k, m = self.k, self.m
        enc = enc or RS.New(k, m)
        log = []
        st = self.stripes()
        self.start(tuple(range(k, k + m)))
        s0 = stats()
        enc.EncodeStripes(st)
        log.append(("encode", m, delta(s0, stats())))
        self.check("encode")
        for lost in self.patterns():
            self.start(lost)
            s0 = stats()
            enc.ReconstructStripes(st, [0 if i in lost else 1 for i in range(k + m)])
            log.append((f"reconstruct{list(lost)}", len(lost), delta(s0, stats())))
            self.check(f"reconstruct lost={list(lost)}")
        return log

    def lens(self, *wheres):
        return [S for S, w in self.specs if w in wheres and S]

    def free(self):
        self.back = self.want = None
        if self.hb is not None:
            self.hb.free()


def with_empties(specs, where):
    """zero-length stripes first, between and last"""
    specs = list(specs)
    mid = len(specs) // 2
    return [(0, where)] + specs[:mid] + [(0, where)] + specs[mid:] + [(0, where)]


def expect(cond, msg, errors):
    if not cond:
        errors.append(msg)


def ring_checks(bt, log, errors, label):
    """pageable batches: pieces and chunks as restated, staged launches per chunk"""
    lens = bt.lens("page")
    out = []
    for what, R, d in log:
        pieces, chunks, _ = ring_cut(bt.k, R, lens)
        want = {"ring_pieces": pieces, "ring_chunks": chunks}
        for v, n in SC.launches(bt.k, R).items():
            if n:
                want[v] = n * chunks
        expect(d == want, f"{label} {what}: counters {d}, restated {want}", errors)
        out.append({"op": what, "pieces": pieces, "chunks": chunks})
    return out


def mode_pieces():
    errors, res = [], []
    for k, m, mult in ((4, 2, None), (3, 5, "out"), (10, 4, "two")):
        W = piece_width(k, m)
        T = SC.tile_bytes(k)
        if mult is None:
            big = [W - 16, W - 1, W, W + 1, W + 15, W + 16, W + 17, 2 * W, 2 * W + 1, 3 * W + T + 5]
        elif mult == "out":
            assert OUT_CAP // m < IN_CAP // k  # the OUT slot binds the width
            big = [W - 1, W + 1, 2 * W + 1]
        else:
            big = [W + 1, 2 * W - 1]
        specs = []
        for i, S in enumerate(big):
            specs.append((S, "page"))
            specs.append(((1, 16, 17, 1000)[i % 4], "page"))
        bt = Batch(k, m, with_empties(specs, "page"), 11 * k + m)
        log = bt.run_all()
        res.append({"shape": f"{k}+{m}", "W": W, "lengths": big, "ops": ring_checks(bt, log, errors, f"pieces {k}+{m}")})
        enc_pieces = res[-1]["ops"][0]["pieces"]
        expect(enc_pieces == sum(-(-S // W) for S in bt.lens("page")) > len(bt.lens("page")),
               f"pieces {k}+{m}: {enc_pieces} pieces", errors)
        errors += bt.errors
        bt.free()
    return {"cases": res, "errors": errors}


def mode_chunks():
    errors, res = [], []
    k, m = 4, 2
    # (a) >= 2 kSlots + 1 chunks; four stripes of S = 65536 fill the IN slot exactly, a fifth opens the next
    specs = [(65536, "page")] * (4 * (2 * K_SLOTS + 1) + 1)
    bt = Batch(k, m, with_empties(specs, "page"), 1)
    log = bt.run_all()
    ops = ring_checks(bt, log, errors, "chunks bytes")
    expect(4 * k * 65536 == IN_CAP and ops[0]["chunks"] == 2 * K_SLOTS + 2, f"chunks bytes: {ops[0]}", errors)
    res.append({"case": "bytes", "stripes": len(specs), "ops": ops})
    errors += bt.errors
    bt.free()
    # (b) tile_cap closes a chunk before the bytes do: one tile per 16-byte stripe
    n = TILE_CAP + 1 + 700
    bt = Batch(k, m, with_empties([(16, "page")] * n, "page"), 2)
    log = bt.run_all()
    ops = ring_checks(bt, log, errors, "chunks tiles")
    expect(TILE_CAP * k * 16 < IN_CAP and ops[0]["chunks"] == 2, f"chunks tiles: {ops[0]}", errors)
    res.append({"case": "tile_cap", "stripes": n, "ops": ops})
    errors += bt.errors
    bt.free()
    return {"cases": res, "errors": errors}


def mode_zerocopy():
    errors, res = [], []
    k, m = 3, 1
    T = SC.tile_bytes(k)
    assert T == 1024 and TILE_CAP == 2048
    # 1000 + 1048 tiles: the second stripe's last tile is the slot's last record; 1501 tiles, then
    # 1001 that straddle the next boundary with a ragged last tile; one stripe of more than two slots
    lens = [1000 * T, 1048 * T, 1500 * T + 400, 1000 * T + 16, (2 * TILE_CAP + 300) * T + 48]
    bt = Batch(k, m, with_empties([(S, "pin") for S in lens], "pin"), 3)
    expect(all(RS.host_device_addr(s) for s in bt.stripes() if s.size), "zerocopy: a stripe is not pinned", errors)
    log = bt.run_all()
    slots = zc_slots(k, lens)
    for what, R, d in log:
        want = {"zc_record_slots": slots, "plain": slots}
        expect(d == want, f"zerocopy {what}: counters {d}, restated {want}", errors)
    expect(slots >= K_SLOTS + 2, f"zerocopy: {slots} record slots", errors)
    res.append({"shape": "3+1", "lengths": lens, "slots": slots, "ops": [w for w, _, _ in log],
                "pinned_bytes": bt.hb.nbytes})
    errors += bt.errors
    bt.free()
    # accumulate passes over PCIe
    k, m = 11, 3
    bt = Batch(k, m, with_empties([(S, "pin") for S in SC.seams(k)], "pin"), 4)
    log = bt.run_all()
    for what, R, d in log:
        want = {"zc_record_slots": 1, "plain": 1, "accumulate": 1}
        expect(d == want, f"zerocopy 11+3 {what}: counters {d}, restated {want}", errors)
    res.append({"shape": "11+3", "lengths": list(SC.seams(k)), "slots": 1, "ops": [w for w, _, _ in log]})
    errors += bt.errors
    bt.free()
    return {"cases": res, "errors": errors}


def mode_zerocopy_unaligned():
    errors = []
    k, m = 2, 1
    # edge records only (S <= 160): 2047 stripes fill a slot of 2048 records
    tiny = [(1 + (37 * i) % ODD_MIN_MAIN, "pinodd") for i in range(4 * (TILE_CAP - 1) + 12)]
    # 9 MiB + 5: longer than a slot of 2048 records whatever the record tile (<= 4 KiB), at an odd
    # address; and 16-B aligned stripes of S % 16 != 0
    specs = tiny[:3000] + [((9 << 20) + 5, "pinodd")] + tiny[3000:] + [(4099, "pin"), (2017, "pinodd"), (161, "pin")]
    bt = Batch(k, m, with_empties(specs, "pinodd"), 5)
    log = bt.run_all()
    slots = []
    for what, R, d in log:
        slots.append(d.get("zc_record_slots", 0))
        expect(set(d) == {"zc_record_slots"} and d["zc_record_slots"] >= K_SLOTS + 2,
               f"zerocopy-unaligned {what}: counters {d}", errors)
    errors += bt.errors
    n = len(specs)
    bt.free()
    return {"cases": [{"shape": "2+1", "stripes": n, "tiny": len(tiny), "slots": slots, "ops": [w for w, _, _ in log]}],
            "errors": errors}


def md5_call(bt, enc, label, errors):
    """EncodeStripesMD5 over the batch: parity against the oracle image, digests against hashlib"""
    k, m = bt.k, bt.m
    bt.start(tuple(range(k, k + m)))
    st = bt.stripes()
    s0 = stats()
    digs = enc.EncodeStripesMD5(st)
    d = delta(s0, stats())
    bt.check(label)
    bad = 0
    for (b, p, ln), (S, _), dg in zip(bt.slices, bt.specs, digs):
        w = bt.want[b][p:p + ln]
        bad += dg != [hashlib.md5(w[i * S:(i + 1) * S].tobytes()).hexdigest() for i in range(k + m)]
    expect(bad == 0, f"{label}: {bad} stripes with a wrong digest", errors)
    errors += bt.errors
    bt.errors = []
    return d


def mode_md5_ring():
    errors, res = [], []
    k, m = 4, 2
    enc = RS.New(k, m)
    W = piece_width(k, m)
    assert k * W == IN_CAP
    lens = [65536] * 9 + [W] + [65536 + 16, 17, 1000, 4096 + 5] * 3 + [W - 16] + [65536] * 8
    bt = Batch(k, m, [(S, "page") for S in lens], 6)
    d = md5_call(bt, enc, "md5-ring", errors)
    pieces, chunks, sizes = ring_cut(k, m, lens)
    want = {"ring_pieces": pieces, "ring_chunks": chunks, "arena_flushes": flushes_of(sizes), "plain": chunks,
            "md5_ring": 1}
    expect(d == want and want["arena_flushes"] >= 2 * N_ARENAS + 1, f"md5-ring: counters {d}, restated {want}", errors)
    res.append({"shape": "4+2", "stripes": len(lens), "counters": want})
    bt.free()
    # 16 bytes over the slot bound: refused, nothing written, and the ring still works
    bt = Batch(k, m, [(4096, "page"), (W + 16, "page"), (1000, "page")], 7)
    bt.start(tuple(range(k, k + m)))
    keep = {b: a.copy() for b, a in bt.back.items()}
    s0 = stats()
    try:
        enc.EncodeStripesMD5(bt.stripes())
        errors.append("md5-ring: a stripe wider than a slot was accepted")
    except RS.ErrInvalidArg:
        pass
    d = delta(s0, stats())
    expect(all(np.array_equal(bt.back[b], keep[b]) for b in keep), "md5-ring: a refused call wrote to a buffer", errors)
    expect(set(d) <= {"md5_ring"}, f"md5-ring refused call: counters {d}", errors)
    bt.free()
    bt = Batch(k, m, [(W, "page"), (4096, "page")], 8)
    md5_call(bt, enc, "md5-ring after a refusal", errors)
    bt.free()
    return {"cases": res, "errors": errors}


def mode_md5_pinned():
    errors, res = [], []
    seen = {"mirror": set(), "mirror_accumulate": set()}
    for c in SC.HASH_CASES:
        bt = Batch(c.k, c.m, [(S, "pin") for S in c.lengths], 100 * c.k + c.m)
        d = md5_call(bt, RS.New(c.k, c.m), f"md5-pinned {c.k}+{c.m}", errors)
        want = {v: n for v, n in SC.hash_launches(c).items() if n}
        want.update({"zc_record_slots": 1, "arena_flushes": 1, "md5_zero_copy": 1})
        expect(d == want, f"md5-pinned {c.k}+{c.m}: counters {d}, restated {want}", errors)
        if d == want:
            for v, K, R in SC.hash_passes(c):
                seen[v].add((K, R))
        bt.free()
    res.append({"case": "instances", "mirror": len(seen["mirror"]), "mirror_accumulate": len(seen["mirror_accumulate"])})
    # arena switching: 6 x 65536 B per stripe, five stripes per 2 MiB arena
    k, m = 4, 2
    enc = RS.New(k, m)
    lens = [65536] * 14 + [16, 65536 + 1024, 1008] + [65536] * 14
    bt = Batch(k, m, [(S, "pin") for S in lens], 9)
    d = md5_call(bt, enc, "md5-pinned arenas", errors)
    fl = flushes_of([(k + m) * S for S in lens], rounded=True)
    expect(d.get("arena_flushes") == fl >= 2 * N_ARENAS + 1 and d.get("md5_zero_copy") == 1 and "md5_ring" not in d
           and d.get("mirror") == d.get("zc_record_slots") and "plain" not in d,
           f"md5-pinned arenas: counters {d}, restated flushes {fl}", errors)
    res.append({"case": "arenas", "stripes": len(lens), "counters": d})
    bt.free()
    # the unaligned twin: odd addresses and lengths, stripes with edge records only
    lens = [65537] * 12 + [1, 17, 160, 100, 161, 2017] + [65521] * 12 + [33] * 40
    bt = Batch(k, m, [(S, "pinodd") for S in lens], 10)
    d = md5_call(bt, enc, "md5-pinned unaligned", errors)
    expect(d.get("arena_flushes", 0) >= 2 * N_ARENAS + 1 and d.get("md5_zero_copy") == 1 and "md5_ring" not in d
           and "mirror" not in d and d.get("zc_record_slots", 0) >= 1,
           f"md5-pinned unaligned: counters {d}", errors)
    res.append({"case": "unaligned", "stripes": len(lens), "counters": d})
    bt.free()
    return {"cases": res, "errors": errors}


def mode_mixed():
    errors = []
    k, m = 6, 3
    W = piece_width(k, m)
    kinds = ("pin", "pinodd", "page", "pin")
    lens = [16, 1000, 4096, 1024 + 16, 160, 33, W + 17, 65536, 2048 + 368, 4099, 2 * W + 1, 48]
    specs = [(S + (0 if kinds[i % 4] == "pin" else i % 2), kinds[i % 4]) for i, S in enumerate(lens)]
    specs = [(S - S % 16 if w == "pin" and S >= 16 else S, w) for S, w in specs]
    bt = Batch(k, m, with_empties(specs, "page"), 12)
    enc = RS.New(k, m)
    log = []
    st = bt.stripes()
    for what, lost in (("encode", tuple(range(k, k + m))), ("reconstruct[0, 6]", (0, k))):
        bt.start(lost)
        s0 = stats()
        if what == "encode":
            enc.EncodeStripes(st)
        else:
            enc.ReconstructStripes(st, [0 if i in lost else 1 for i in range(k + m)])
        d = delta(s0, stats())
        bt.check(what)
        R = len(lost)
        pieces, chunks, _ = ring_cut(k, R, bt.lens("page"))
        zs = zc_slots(k, bt.lens("pin"))
        expect(d.get("ring_pieces") == pieces and d.get("ring_chunks") == chunks and d.get("plain") == zs + chunks
               and d.get("zc_record_slots", 0) >= zs + 1, f"mixed {what}: counters {d}, restated pieces {pieces} "
               f"chunks {chunks} aligned slots {zs}", errors)
        log.append({"op": what, "counters": d})
    errors += bt.errors
    specs = [[S, w] for S, w in bt.specs]
    bt.free()
    return {"cases": [{"shape": "6+3", "specs": specs, "ops": log}], "errors": errors}


MODES = {"pieces": mode_pieces, "chunks": mode_chunks, "zerocopy": mode_zerocopy,
         "zerocopy-unaligned": mode_zerocopy_unaligned, "md5-ring": mode_md5_ring, "md5-pinned": mode_md5_pinned,
         "mixed": mode_mixed}


def main():
    mode = sys.argv[1]
    out = MODES[mode]()
    out["mode"] = mode
    out["caps"] = {"in_cap": IN_CAP, "tile_cap": TILE_CAP, "arena": ARENA}
    out["errors"] = out["errors"][:12]
    print(json.dumps(out), flush=True)
    return 0 if not out["errors"] else 1


if __name__ == "__main__":
    sys.exit(main())
