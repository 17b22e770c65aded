"""Exhaustive single-flip sweeps of every Verify kernel: one object per
(parity row, byte position), one per position in a data shard, one bit each.

A wrong compare predicate in a Verify kernel produces no wrong byte, only a
corrupt byte that is never reported, so the sweeps walk every position across
every window seam, tile seam, main/tail hand-off and column-piece seam, in
every parity row (a data flip changes all rows, so a skipped row only shows on
a parity flip), and demand exact flags: 1 on every flipped object, 0 on every
control and on the all-clean replica.  No parity coefficient of the codec
matrix is zero (asserted per case), so any single-bit flip makes the codeword
invalid; the oracle's recompute-and-compare flags all of them and nothing
else.  There is no tolerance anywhere in this file.

One clean codeword per case comes from the oracle (coracle build_matrix /
apply), is replicated on the device, and one byte per non-control object is
XORed with 1 << ((p + p // 8 + r) % 8) (r = the parity row, m for the data
sweep), in a seeded random order with every 61st object left clean.  A case
whose objects exceed 4 GiB is verified in consecutive object ranges over one
resident replica (flags[o0:]); every position is still swept.  Each case
asserts from hbec_verify_route_stats / hbec_odd_path_stats /
hbec_verify_plan_stats that the call took the kernel it names.

Shard lengths are two full tiles and a ragged third: 2 tile + 37 at any
alignment (base offset 3, odd row pitch, so all 16 byte alignments occur
across objects), 2 tile + 48 on the 16-B-aligned routes.  Tiles, from the code:
  packed  shards below max(verify_tile_bytes(k), 2048)          (verify.hip)
  pipe    verify_tile_bytes(k): 4096 for k <= 4, 1024 above     (verify.hip)
  odd     k <= 4: (64 HBEC_ODD_U_VERIFY - 1) 16 = 4080 chained;  register and
          LDS-table kernels one 63-column window = 1008;  bit-plane
          (64 HBEC_ODD_BP_U - 1) 16 = 2032                       (odd.hip odd_tiles_per_obj)
  wide    kWideTile = HBEC_WIDE_U x 992 = 1984                   (wide.hip)
  plans   verify_plan_tile_bytes(k) (kVpTile) and the aligned tile of plan.info()

Routes as the counters show them (hbec.cpp verify_views): every shape with a
compiled bit-plane Verify (6+3, 8+3, 10+4, 12+4, 10+2, ...) takes it at any
alignment, so the register-table kernel is swept with 7+2 and 5+4 and the
LDS-table record kernel with 11+4 and 9+4; 9+1 has no schedule and takes
gf_verify_wide; verify_supported accepts no k > 8, so the third pipe shape is
8+4 below HBEC_REC_ROUTE_MIN_S.  gf_verify_unaligned and the scratch recompute
are only reached from 2^31 - 2^16 bytes per shard, too large for a sweep:
tests/test_gpu_large.py covers them.

The aligned-to-records case (8+4 at HBEC_REC_ROUTE_MIN_S + 16, objects of
590 KB) is the only one that samples: the first and last 8192 positions and
every 7th between them (7 is coprime to every seam period).

Column pieces run in a fresh child process with HBEC_HOST_SLOT_MB=1
(`python tests/test_gpu_verify_sweep.py`).
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
else:
    import torch  # before libhbec is loaded, so both use one HIP runtime (the child needs no torch)

from hummingbird_amd import batch as B  # noqa: E402
from hummingbird_amd import reedsolomon as RS  # noqa: E402
from oracle import coracle as CO  # noqa: E402

pytestmark = pytest.mark.gpu

CONTROL_EVERY = 61
CAP = 4 << 30          # bytes resident per verify call
FILL = 0xA5            # bytes that belong to no shard
REC_ROUTE_MIN_S = 49152  # tuning.h HBEC_REC_ROUTE_MIN_S


# ---- the object set (host, numpy only) --------------------------------------

def codeword(k, m, S, seed):
    """One clean codeword, (k+m) S bytes, parity from the oracle."""
    rows = CO.build_matrix(k, m)[k:]
    assert np.all(rows != 0), "a zero parity coefficient: single flips need not be detected"
    data = np.random.default_rng(seed).integers(0, 256, (k, S), dtype=np.uint8)
    return np.concatenate([data.reshape(-1)] + CO.apply(rows, [data[j] for j in range(k)]))


def flip_list(k, m, S, positions=None, data=True):
    """(shard, position, xor value) of every flip: each parity row at each
    position, then (data=True) data shard p % k at each position p."""
    P = np.arange(S, dtype=np.int64) if positions is None else np.asarray(positions, dtype=np.int64)
    assert P.size == 0 or (P.min() >= 0 and P.max() < S)
    groups = m + (1 if data else 0)
    shard = np.concatenate([np.full(P.size, k + r, np.int64) for r in range(m)] + ([P % k] if data else []))
    pos = np.tile(P, groups)
    r = np.repeat(np.arange(groups, dtype=np.int64), P.size)
    val = (1 << ((pos + pos // 8 + r) % 8)).astype(np.uint8)
    return shard, pos, val


def placement(n_flips, seed):
    """(n, object of flip i): a seeded permutation over the objects that are not
    controls; object o is a control when o % 61 == 60 (and the spare ones at the end)."""
    n = n_flips + max(1, -(-n_flips // (CONTROL_EVERY - 1)))
    free = np.nonzero(np.arange(n) % CONTROL_EVERY != CONTROL_EVERY - 1)[0]
    assert free.size >= n_flips and n > n_flips
    return n, free[:n_flips][np.random.default_rng(seed).permutation(n_flips)]


class Layout:
    """Where shard i of object o lives: parts = [(first shard, end shard, base
    offset, pitch)], one per buffer (split: data and parity apart).  Aligned:
    offset 0 and back-to-back rows; else offset 3 and an odd pitch (5 or 6
    slack bytes per row), plus 11 bytes after the last row."""

    def __init__(self, k, m, S, aligned, split=False):
        self.k, self.m, self.S, self.aligned = k, m, S, aligned
        self.parts = []
        for a, b in ([(0, k), (k, k + m)] if split else [(0, k + m)]):
            w = (b - a) * S
            if aligned:
                assert S % 16 == 0
                self.parts.append((a, b, 0, w))
            else:
                self.parts.append((a, b, 3, w + 5 + (w + 5 + 1) % 2))
        self.pad = 0 if aligned else 11
        self.obj_bytes = sum(p[3] for p in self.parts)

    def part_of(self, shard):
        return np.searchsorted(np.array([p[1] for p in self.parts]), shard, side="right")


# ---- device side ------------------------------------------------------------

def replicate(cw, lay, n):
    """n replicas of the codeword on the device, one tensor per part."""
    bufs = []
    for a, b, off, pitch in lay.parts:
        row = np.full(pitch, FILL, np.uint8)
        row[:(b - a) * lay.S] = cw[a * lay.S:b * lay.S]
        t = torch.empty(off + n * pitch + lay.pad, dtype=torch.uint8, device="cuda")
        t[:off] = FILL
        t[off + n * pitch:] = FILL
        t[off:off + n * pitch].view(n, pitch).copy_(torch.from_numpy(row).cuda())
        bufs.append(t)
    return bufs


def xor_flips(bufs, lay, obj, shard, pos, val):
    """XOR one byte per listed object, one advanced-index operation per buffer."""
    part = lay.part_of(shard)
    for i, (a, b, off, pitch) in enumerate(lay.parts):
        sel = part == i
        if not sel.any():
            continue
        idx = torch.from_numpy(off + obj[sel] * pitch + (shard[sel] - a) * lay.S + pos[sel]).cuda()
        bufs[i][idx] = bufs[i][idx] ^ torch.from_numpy(val[sel]).cuda()


def batch_run(enc, bufs, lay):
    """run(n, flags): hbec_verify_batch over the first n objects."""
    views = []
    for (a, b, off, pitch), t in zip(lay.parts, bufs):
        views += [(t.data_ptr() + off + (i - a) * lay.S, pitch) for i in range(a, b)]
    return lambda n, flags: B.verify_views(enc, views, n, lay.S, flags)


def plan_run(enc, bufs, lay, n_plan, layout):
    """run(n, flags): hbec_verify_plan of one plan over all n_plan objects."""
    S = lay.S
    if layout == "stripes":
        (_, _, off, pitch), = lay.parts
        plan = B.StripePlan(enc, stripes=[(bufs[0].data_ptr() + off + o * pitch, S) for o in range(n_plan)])
    else:
        (_, _, od, pd), (_, _, op, pp) = lay.parts
        d0, p0 = bufs[0].data_ptr() + od, bufs[1].data_ptr() + op
        plan = B.StripePlan(enc, objects=[(d0 + o * pd, p0 + o * pp, S) for o in range(n_plan)])

    def run(n, flags):
        assert n == n_plan
        plan.verify(flags)

    run.plan = plan
    return run


def counters():
    c = dict(B.verify_route_stats())
    c.update({"odd_" + f: v for f, v in B.odd_path_stats().items() if f in ("bitplane", "records", "strided")})
    c.update(B.verify_plan_stats())
    return c


def changed(c0, c1):
    return {f: c1[f] - c0[f] for f in c0 if c1[f] != c0[f]}


def expect_route(delta, calls, route, family=None):
    """`calls` verify calls all took `route` (and, for the odd route, launched
    only `family` main kernels); nothing else was counted."""
    want = {"records": ("records", "odd")}.get(route, (route,))
    got_routes = {f: v for f, v in delta.items() if not f.startswith("odd_")}
    assert got_routes == {f: calls for f in want}, (delta, calls, route)
    fam = {f for f in delta if f.startswith("odd_")}
    assert fam == ({"odd_" + family} if family else set()), (delta, family)


def sweep(label, k, m, S, aligned, make_run, positions=None, data=True, split=False, fp=False, seed=0, quiet=False):
    """The sweep of one case.  Returns (counter changes, verify calls made)."""
    lay = Layout(k, m, S, aligned, split)
    shard, pos, val = flip_list(k, m, S, positions, data)
    n, obj = placement(shard.size, 1000 * k + m + seed)
    n_res = min(n, max(1, (CAP - 64) // lay.obj_bytes))
    resident = sum(off + n_res * pitch + lay.pad for _, _, off, pitch in lay.parts)
    assert resident <= CAP or n_res == 1
    bufs = replicate(codeword(k, m, S, 7 * k + m + S), lay, n_res)
    run = make_run(bufs, lay, n_res)
    c0 = counters()
    calls = 0
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    for o0 in range(0, n, n_res):
        o1 = min(n, o0 + n_res)
        sel = (obj >= o0) & (obj < o1)
        xor_flips(bufs, lay, obj[sel] - o0, shard[sel], pos[sel], val[sel])
        run(o1 - o0, flags[o0:])
        calls += 1
        xor_flips(bufs, lay, obj[sel] - o0, shard[sel], pos[sel], val[sel])  # the clean replica again
    torch.cuda.synchronize()
    got = flags.cpu().numpy()
    want = np.zeros(n, np.int32)
    want[obj] = 1
    if not np.array_equal(got, want):
        missed = np.nonzero(got[obj] != 1)[0]
        false = np.nonzero((got != 0) & (want == 0))[0]
        other = np.nonzero((got != want) & (got != 0) & (want != 0))[0]
        pytest.fail(f"{label} {k}+{m} S={S}: {missed.size} of {obj.size} flips missed, first (shard, position): "
                    f"{sorted(zip(shard[missed].tolist(), pos[missed].tolist()))[:12]}; "
                    f"{false.size} clean objects flagged: {false[:12].tolist()}; other values at {other[:6].tolist()}")
    # the all-clean replica
    clean = torch.zeros(n_res, dtype=torch.int32, device="cuda")
    run(n_res, clean)
    calls += 1
    torch.cuda.synchronize()
    assert not clean.any().item(), (label, "clean replica flagged", torch.nonzero(clean)[:12].flatten().tolist())
    if fp:
        # every byte that belongs to no shard inverted: still clean, and nothing written
        assert not aligned
        want_rows = []
        for (a, b, off, pitch), t in zip(lay.parts, bufs):
            w = (b - a) * S
            rows = t[off:off + n_res * pitch].view(n_res, pitch)
            rows[:, w:] ^= 0xFF
            t[:off] ^= 0xFF
            t[off + n_res * pitch:] ^= 0xFF
            want_rows.append(rows[0].clone())
        run(n_res, clean)
        calls += 1
        torch.cuda.synchronize()
        assert not clean.any().item(), (label, "slack bytes were compared", torch.nonzero(clean)[:12].flatten().tolist())
        for (a, b, off, pitch), t, row in zip(lay.parts, bufs, want_rows):
            assert (row[(b - a) * S:] == (FILL ^ 0xFF)).all().item()
            assert (t[:off] == (FILL ^ 0xFF)).all().item() and (t[off + n_res * pitch:] == (FILL ^ 0xFF)).all().item()
            rows = t[off:off + n_res * pitch].view(n_res, pitch)
            step = max(1, (64 << 20) // pitch)
            for i in range(0, n_res, step):
                assert (rows[i:i + step] == row).all().item(), (label, "buffer written", i)
    delta = changed(c0, counters())
    if not quiet:
        print(f"SWEEP {label} {k}+{m} S={S} n={n} flips={obj.size} resident={resident} calls={calls} {delta}")
    return delta, calls


# ---- 2. strided batches ------------------------------------------------------

# (id, route, odd family, k, m, S, 16-B aligned, slack-inversion check)
BATCH_CASES = [
    # packed: S % 16 == 0 below max(verify_tile_bytes(k), 2048)
    ("packed-4+2-under-limit", "packed", None, 4, 2, 4096 - 16, True, False),
    ("packed-8+3-under-limit", "packed", None, 8, 3, 2048 - 16, True, False),
    ("packed-4+2-S16", "packed", None, 4, 2, 16, True, False),
    ("packed-4+2-S32", "packed", None, 4, 2, 32, True, False),
    ("packed-8+3-S16", "packed", None, 8, 3, 16, True, False),
    ("packed-8+3-S32", "packed", None, 8, 3, 32, True, False),
    # pipe: verify_tile_bytes(k) = 4096 (k <= 4, U = 4), 1024 above
    ("pipe-4+2", "pipe", None, 4, 2, 2 * 4096 + 48, True, False),
    ("pipe-8+3", "pipe", None, 8, 3, 2 * 1024 + 48, True, False),
    ("pipe-8+4", "pipe", None, 8, 4, 2 * 1024 + 48, True, False),
    # gf_odd, k <= 4: HBEC_ODD_U_VERIFY = 4 chained windows, (64 * 4 - 1) * 16
    ("odd-chained-4+2", "odd", "strided", 4, 2, 2 * 4080 + 37, False, True),
    ("odd-chained-2+1", "odd", "strided", 2, 1, 2 * 4080 + 37, False, False),
    ("odd-chained-3+2", "odd", "strided", 3, 2, 2 * 4080 + 37, False, False),
    # gf_odd, 5 <= k <= 8: one 63-column window with register tables; the
    # shapes with a compiled schedule: bit-plane, (64 * 2 - 1) * 16
    ("odd-regs-7+2", "odd", "strided", 7, 2, 2 * 1008 + 37, False, True),
    ("odd-regs-5+4", "odd", "strided", 5, 4, 2 * 1008 + 37, False, False),
    ("odd-bitplane-8+3", "odd", "bitplane", 8, 3, 2 * 2032 + 37, False, True),
    ("odd-bitplane-6+3", "odd", "bitplane", 6, 3, 2 * 2032 + 37, False, False),
    # 9 <= k <= 12 with 3-4 rows: LDS-table records (one window), or bit-plane
    ("odd-ldsrec-11+4", "odd", "records", 11, 4, 2 * 1008 + 37, False, True),
    ("odd-ldsrec-9+4", "odd", "records", 9, 4, 2 * 1008 + 37, False, False),
    ("odd-bitplane-10+4", "odd", "bitplane", 10, 4, 2 * 2032 + 37, False, False),
    ("odd-bitplane-12+4", "odd", "bitplane", 12, 4, 2 * 2032 + 37, False, False),
    # 9 <= k <= 12 with m <= 2: bit-plane where compiled (10+2), else gf_verify_wide (9+1)
    ("odd-bitplane-10+2", "odd", "bitplane", 10, 2, 2 * 2032 + 37, False, False),
    ("wide-9+1", "wide", None, 9, 1, 2 * 1984 + 37, False, False),
    # gf_wide<R, false> + gf_verify_wide_tail: kWideTile = 2 * 992
    ("wide-17+3", "wide", None, 17, 3, 2 * 1984 + 37, False, True),
    ("wide-20+4", "wide", None, 20, 4, 2 * 1984 + 37, False, False),
    ("wide-32+8", "wide", None, 32, 8, 2 * 1984 + 37, False, False),
    ("wide-9+6", "wide", None, 9, 6, 2 * 1984 + 37, False, False),
    ("wide-12+9-two-passes", "wide", None, 12, 9, 2 * 1984 + 37, False, False),
]


@pytest.mark.parametrize("label,route,family,k,m,S,aligned,fp", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_batch_every_row_and_position(label, route, family, k, m, S, aligned, fp):
    enc = RS.New(k, m)
    delta, calls = sweep(label, k, m, S, aligned, lambda bufs, lay, n: batch_run(enc, bufs, lay), fp=fp)
    expect_route(delta, calls, route, family)


@pytest.mark.parametrize("part", range(6))
def test_batch_aligned_to_records_8_4(part):
    """8+4 at the smallest S the aligned-to-records route takes.  Objects are
    590 KB, so this case alone samples: the first 8192 and last 8192 positions
    and every 7th between them, cut into 6 parts of about 10 GB of objects."""
    k, m, S = 8, 4, REC_ROUTE_MIN_S + 16
    P = np.concatenate([np.arange(8192), np.arange(8192, S - 8192, 7), np.arange(S - 8192, S)])
    assert np.unique(P).size == P.size
    enc = RS.New(k, m)
    delta, calls = sweep(f"aligned-to-records-part{part}", k, m, S, True,
                         lambda bufs, lay, n: batch_run(enc, bufs, lay), positions=np.array_split(P, 6)[part], seed=part)
    expect_route(delta, calls, "records", "bitplane")


def test_batch_wide_17_3_every_short_length():
    """S = 1..80: shards only gf_verify_wide_tail sees (S < 32), and the first main columns."""
    k, m = 17, 3
    enc = RS.New(k, m)
    for S in range(1, 81):
        delta, calls = sweep("wide-short", k, m, S, False, lambda bufs, lay, n: batch_run(enc, bufs, lay), seed=S,
                             quiet=S != 80)
        expect_route(delta, calls, "wide")


HANDOFF = [("odd", "strided", 4, 2, 4080), ("odd", "bitplane", 8, 3, 2032), ("wide", None, 20, 4, 1984)]


@pytest.mark.parametrize("route,family,k,m,tile", HANDOFF, ids=[f"{c[2]}+{c[3]}" for c in HANDOFF])
def test_batch_main_tail_handoff_at_every_length(route, family, k, m, tile):
    """Every S within 40 bytes of one and of two tiles, at any alignment: each
    of the last 34 positions of each parity row flipped, one object per flip."""
    enc = RS.New(k, m)
    for S in list(range(tile - 40, tile + 41)) + list(range(2 * tile - 40, 2 * tile + 41)):
        delta, calls = sweep("handoff", k, m, S, False, lambda bufs, lay, n: batch_run(enc, bufs, lay),
                             positions=np.arange(S - 34, S), data=False, seed=S, quiet=S != 2 * tile + 40)
        expect_route(delta, calls, route, family)


# ---- 3. plans ----------------------------------------------------------------

def aligned_tile(k, m):
    return B.StripePlan(RS.New(k, m), stripes=[]).info()["tile_bytes"]


@pytest.mark.parametrize("layout", ["stripes", "objects"])
@pytest.mark.parametrize("k,m,aligned", [(4, 2, True), (8, 3, True), (4, 2, False), (8, 3, False), (10, 4, False),
                                         (12, 4, False)])
def test_plan_of_equal_stripes_every_row_and_position(k, m, aligned, layout):
    """Aligned (S % 16 == 0, k <= 8): gf_verify_tiles alone, one launch per
    call; odd offsets: gf_verify_recs and its tail, two launches per call."""
    enc = RS.New(k, m)
    S = 2 * aligned_tile(k, m) + 48 if aligned else 2 * B.verify_plan_tile_bytes(k) + 37
    made = []

    def make(bufs, lay, n):
        made.append(plan_run(enc, bufs, lay, n, layout))
        return made[-1]

    delta, calls = sweep(f"plan-{layout}-{'aligned' if aligned else 'odd'}", k, m, S, aligned, make,
                         split=layout == "objects", fp=not aligned and (k, m) in ((4, 2), (10, 4)))
    info = made[0].plan.info()
    if aligned:
        assert info["n_tiles"] > 0 and info["n_fallback"] == 0, info
    # no stripe took the per-stripe route (nor any hbec_verify_batch), and none of an aligned plan the records
    assert delta == {"plan_launches": (1 if aligned else 2) * calls}, (delta, calls, info)


def every_length_layout(k, m, max_s, D=34):
    """One buffer with D stripes of every shard length 1..max_s, each at an odd
    address (odd block starts, even pitch of at least 5 slack bytes).  Returns
    (total bytes, [(S, pitch, start)] per length, and per stripe: base, S,
    flipped?, parity row, position)."""
    L = k + m
    lengths = np.arange(1, max_s + 1, dtype=np.int64)
    pitch = L * lengths + 5
    pitch += pitch % 2
    start = 1 + np.concatenate([[0], np.cumsum(D * pitch)[:-1]])
    total = int(start[-1] + D * pitch[-1]) + 11
    d = np.tile(np.arange(D, dtype=np.int64), lengths.size)
    Sx, px, sx = (np.repeat(a, D) for a in (lengths, pitch, start))
    base = sx + d * px
    assert np.all(base % 2 == 1)
    return total, list(zip(lengths.tolist(), pitch.tolist(), start.tolist())), base, Sx, d < Sx, d % m, Sx - 1 - d


@pytest.mark.parametrize("k,m", [(4, 2), (10, 4)])
def test_plan_of_every_length_main_tail_seam(k, m):
    """One plan with every shard length 1 .. 2 T + 64 at odd offsets, 34 stripes
    per length: stripe d of length S is flipped at S - 1 - d of parity row
    d % m (stripes beyond S are controls), the main/tail seam of every length in
    one call."""
    T = B.verify_plan_tile_bytes(k)
    L = k + m
    total, blocks, base, Sx, bad, frow, fpos = every_length_layout(k, m, 2 * T + 64)
    assert total <= CAP
    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
    buf.fill_(FILL)
    for S, p, st in blocks:
        cw = np.full(p, FILL, np.uint8)
        cw[:L * S] = codeword(k, m, S, S)
        buf[st:st + 34 * p].view(34, p).copy_(torch.from_numpy(cw).cuda())
    idx = (base + (k + frow) * Sx + fpos)[bad]
    val = (1 << ((fpos + fpos // 8 + frow) % 8)).astype(np.uint8)[bad]
    enc = RS.New(k, m)
    plan = B.StripePlan(enc, stripes=[(buf.data_ptr() + int(b), int(s)) for b, s in zip(base, Sx)])
    flags = torch.zeros(base.size, dtype=torch.int32, device="cuda")
    c0 = counters()
    plan.verify(flags)
    torch.cuda.synchronize()
    assert not flags.any().item(), ("clean plan flagged", torch.nonzero(flags)[:12].flatten().tolist())
    tidx = torch.from_numpy(idx).cuda()
    buf[tidx] = buf[tidx] ^ torch.from_numpy(val).cuda()
    plan.verify(flags)
    torch.cuda.synchronize()
    delta = changed(c0, counters())
    got = flags.cpu().numpy()
    want = bad.astype(np.int32)
    miss = np.nonzero(got != want)[0]
    assert miss.size == 0, (f"{miss.size} stripes wrong, first (S, row, position, got): "
                            f"{[(int(Sx[i]), int(frow[i]), int(fpos[i]), int(got[i])) for i in miss[:12]]}")
    assert delta == {"plan_launches": 4}, delta  # gf_verify_recs + its tail, twice
    print(f"SWEEP plan-every-length {k}+{m} S=1..{2 * T + 64} n={base.size} flips={int(bad.sum())} resident={total} {delta}")


# ---- 4. host stripes ---------------------------------------------------------

def host_sweep(k, m, S, shards_and_positions, buf):
    """Stripes at offset 3 with an odd pitch in `buf` (a numpy uint8 array, filled
    here): one stripe per (shard, position), controls every 61st.  Returns
    (stripes, want, (shard, position, stripe) of every flip, the stripe rows)."""
    L = k + m
    shard, pos, val = shards_and_positions
    n, obj = placement(shard.size, 31 * k + m)
    pitch = L * S + 5 + (L * S) % 2
    assert buf.size >= 3 + n * pitch
    buf[:] = FILL
    rows = buf[3:3 + n * pitch].reshape(n, pitch)
    rows[:, :L * S] = codeword(k, m, S, 5 * k + m + S)
    rows[obj, shard * S + pos] ^= val
    want = np.zeros(n, bool)
    want[obj] = True
    return [rows[o, :L * S] for o in range(n)], want, (shard, pos, obj), rows


def host_flips(k, m, S):
    """Every position of the last parity row and of a rotating data shard."""
    P = np.arange(S, dtype=np.int64)
    shard = np.concatenate([np.full(S, k + m - 1, np.int64), P % k])
    pos = np.tile(P, 2)
    r = np.repeat(np.array([m - 1, m], dtype=np.int64), S)
    return shard, pos, (1 << ((pos + pos // 8 + r) % 8)).astype(np.uint8)


def report(got, want, where, label):
    shard, pos, obj = where
    if not np.array_equal(got, want):
        missed = np.nonzero(~got[obj])[0]
        false = np.nonzero(got & ~want)[0]
        pytest.fail(f"{label}: {missed.size} flips missed, first (shard, position): "
                    f"{sorted(zip(shard[missed].tolist(), pos[missed].tolist()))[:12]}; "
                    f"clean stripes flagged: {false[:12].tolist()}")


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_host_stripes_every_position(k, m, pinned):
    """The staging copy (pageable) and the in-place reads over PCIe (pinned)."""
    S = 2 * B.verify_plan_tile_bytes(k) + 37
    flips = host_flips(k, m, S)
    n = placement(flips[0].size, 0)[0]
    size = 3 + n * ((k + m) * S + 6) + 11
    hb = RS.HostBuffer(size) if pinned else None
    buf = hb.array if pinned else np.empty(size, np.uint8)
    if pinned:
        assert RS.host_device_addr(buf) != 0
    stripes, want, where, rows = host_sweep(k, m, S, flips, buf)
    enc = RS.New(k, m)
    keep = buf.copy()
    c0 = counters()
    got = enc.VerifyStripes(stripes)
    delta = changed(c0, counters())
    report(got, want, where, f"host {k}+{m} S={S} pinned={pinned}")
    assert np.array_equal(buf, keep)  # read-only
    assert set(delta) == {"plan_launches"}, delta
    # repaired: all clean
    shard, pos, obj = where
    rows[obj, shard * S + pos] ^= flips[2]
    assert not enc.VerifyStripes(stripes).any()
    print(f"SWEEP host-{'pinned' if pinned else 'pageable'} {k}+{m} S={S} n={n} bytes={size} {delta}")
    del stripes, rows, buf, keep
    if hb is not None:
        hb.free()


def _child():
    """HBEC_HOST_SLOT_MB=1, 4+2: stripes wider than a slot are cut into column
    pieces of W bytes per shard.  S = W + 2 T + 37 (a full piece and one of two
    tiles and a ragged third); every position within 48 bytes of the piece
    boundary, in both parity rows and one data shard, one stripe per flip, with
    clean 1000-byte-shard stripes (which fit a slot) after every third."""
    k, m = 4, 2
    L = k + m
    slot = int(os.environ["HBEC_HOST_SLOT_MB"]) << 20
    W = (slot // L) // 16 * 16  # the piece width (test_gpu_verify_host.py's expression)
    S = W + 2 * B.verify_plan_tile_bytes(k) + 37
    assert L * S > slot
    bounds = list(range(W, S, W))
    P = np.unique(np.concatenate([np.arange(max(0, b - 48), min(S, b + 48)) for b in bounds]))
    flips = [(k + r, int(p), 1 << ((int(p) + int(p) // 8 + r) % 8)) for r in range(m) for p in P]
    flips += [(int(p) % k, int(p), 1 << ((int(p) + int(p) // 8 + m) % 8)) for p in P]
    order = np.random.default_rng(42).permutation(len(flips))
    big = codeword(k, m, S, 1)
    small = codeword(k, m, 1000, 2)
    enc = RS.New(k, m)
    stripes, want, what = [], [], []
    for q, i in enumerate(order):
        sh, p, v = flips[i]
        if q % CONTROL_EVERY == CONTROL_EVERY - 1:
            stripes.append(big.copy())  # a clean wide stripe
            want.append(False)
            what.append(None)
        s = big.copy()
        s[sh * S + p] ^= v
        stripes.append(s)
        want.append(True)
        what.append((sh, p))
        if q % 3 == 2:
            stripes.append(small.copy())
            want.append(False)
            what.append(None)
    got = enc.VerifyStripes(stripes).tolist()
    missed = [w for g, t, w in zip(got, want, what) if t and not g]
    false = [i for i, (g, t) in enumerate(zip(got, want)) if g and not t]
    res = {"pieces": -(-S // W), "bounds": bounds, "n": len(stripes), "flips": len(flips), "missed": missed[:12],
           "n_missed": len(missed), "false": false[:12],
           "clean": enc.VerifyStripes([big.copy(), small.copy(), big.copy()]).tolist()}
    print(json.dumps(res))


def test_host_column_piece_seams():
    env = dict(os.environ, HBEC_HOST_SLOT_MB="1")
    p = subprocess.run([sys.executable, str(Path(__file__).resolve())], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print("SWEEP host-column-pieces 4+2", {f: res[f] for f in ("pieces", "bounds", "n", "flips")})
    assert res["pieces"] >= 2 and res["flips"] == 3 * 96 * len(res["bounds"])
    assert res["n_missed"] == 0 and res["false"] == [], res
    assert res["clean"] == [False, False, False]


if __name__ == "__main__":
    _child()
