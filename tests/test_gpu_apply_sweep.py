"""Byte-exact sweep of the kernels that write data: encode, reconstruct and
the generic apply, as plans, mixed plans and strided batches, at every shard
length 1..SMAX (apply_sweep_layout.SMAX = 2 x 2016 + 368 = 4400) and every
alignment class.

A wrong byte from these kernels is silent data loss.  What varies inside them
(input shift (in + c0) mod 4, output delta (-(out + c0)) mod 16, the clamp of
the last input load, each output's guard band, the tile count per shard) is a
function of (S mod 16, input bases mod 16, output bases mod 16), so the
layouts walk that triple (tests/apply_sweep_layout.py; its coverage is
asserted in tests/test_apply_sweep_layout.py).  Every expected byte is the
oracle's (coracle build_matrix / apply); after a reconstruct the expected
image is the oracle codeword itself.  Whole buffers are compared: slack
bytes, gaps between entries and untouched shards hold a sentinel, shards an
operation must write are garbled with a second one first.  No tolerance, no
sampling.

Plans: one plan per (shape, layout) with every length in it; plan.encode(),
three plan.reconstruct patterns, and plan.reconstruct_mixed with a mask per
entry cycling through every pattern of 1..m losses.  Routes are proven from
plan.info(), hbec_odd_path_stats / hbec_odd_edge_stats and
hbec_mixed_plan_stats.  As the code routes them (plan.cpp
launch_unaligned_passes): with gf_odd enabled every plan pass over unaligned
entries is the record kernel over the plan's tile lists, bit-plane where
gen_xor.USE[(k, m)][1], in passes of <= 12 inputs, the later ones
accumulating - 16+4 is a 12-input and a 4-input accumulate pass, 24+4 two
12-input passes; gf_apply_unaligned_plan only codes shards of 2^31 bytes or
more (tests/test_gpu_large.py).  The record kernels' fused guard band is
compiled out by default (tuning.h HBEC_ODD_EDGE_FUSE = 1: gf_odd only), so
every plan pass has its gf_odd_edges_plan launch.

Strided batches (hbec_encode_batch / hbec_reconstruct_batch /
hbec_apply_batch): 16 objects per call at a stride = 1 mod 16, so the objects
rotate the common base through every residue and no call is 16-B aligned.
Routes from hbec_apply_route_stats and the odd counters.  12+2 codes from LDS
records (K R = 24, tuning.h HBEC_ODD_REC_BIGK_MINKR), so the strided K > 8
kernel is swept with 11+2.

gf_apply_unaligned and gf_mixed_plan tile by HBEC_UNALIGNED_U = 4 windows of
992 B (unaligned_tile.h, 3968 B), more than the 2016 B of the gf_odd family:
for those two kernels alone the sweep goes on from 4401 to 2 x 3968 + 368 =
8304 (16+4 strided batches; 4+2 and 12+4 mixed plans).
"""
import numpy as np
import pytest
import torch

from hummingbird_amd import batch as B
from hummingbird_amd import gen_xor
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO

import apply_sweep_layout as L
import route_rule as R

pytestmark = pytest.mark.gpu

SMAX = L.SMAX
MIN_MAIN = 160          # odd_impl.h kOddMinMain: shorter shards are coded by the edge kernels alone
ODD_MAX_K = 12          # kernels.h kOddMaxK: inputs per gf_odd pass
FUSE_FROM = 2016 + 96   # odd.hip odd_frame_tiles: two 2016-B tiles from S - 96 >= 2016
CAP = 4 << 30           # bytes resident per call (tests/test_gpu_verify_sweep.py)
CHUNK = 768 << 20       # bytes of views queued before one synchronise and compare
N_OBJ = 16
WIDE_TILE = 3968        # unaligned_tile.h: HBEC_UNALIGNED_U (4) windows of 992 B
TOP = 2 * WIDE_TILE + 368  # the last length of the two kernels that tile by it


def counters():
    c = {"ar_" + f: v for f, v in B.apply_route_stats().items()}
    c.update({"odd_" + f: v for f, v in B.odd_path_stats().items()})
    c.update({"mp_" + f: v for f, v in B.mixed_plan_stats().items()})
    return c


def changed(c0, c1):
    return {f: c1[f] - c0[f] for f in c0 if c1[f] != c0[f]}


def bp_plan(k, m):
    return gen_xor.USE.get((k, m), (False, False, False))[1]


# ---- 2. plans ------------------------------------------------------------------

PLAN_SHAPES = [(4, 2), (2, 4), (8, 2), (8, 3), (7, 3), (6, 3), (11, 4), (10, 4), (12, 4), (16, 4), (24, 4)]
PLAN_CASES = [(k, m, lay) for k, m in PLAN_SHAPES for lay in (("stripes", "objects") if k <= 12 else ("stripes",))]


def report(lay, bufs, want, what):
    got = [b.cpu().numpy() for b in bufs]
    bad = lay.mismatches(got, want)
    n_bad = sum(int((g != w).sum()) for g, w in zip(got, want))
    e = bad[0][1]
    where = (f"S={int(lay.S[e])} data base mod 16={int(lay.a[e]) % 16} parity base mod 16={int(lay.b[e]) % 16}"
             if e >= 0 else "before the first entry")
    pytest.fail(f"{lay.k}+{lay.m} {lay.layout} {what}: {n_bad} bytes differ; first at {where}; "
                f"(buffer, entry, shard, position, got, want): {bad}")


@pytest.mark.parametrize("k,m,layout", PLAN_CASES, ids=[f"{k}+{m}-{lay}" for k, m, lay in PLAN_CASES])
def test_plan_every_length_and_alignment(k, m, layout):
    lay = L.Layout(k, m, layout)
    assert sum(lay.sizes) <= CAP
    want = lay.expected()
    bufs = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in lay.sizes]
    addrs = [b.data_ptr() for b in bufs]
    assert all(a % 16 == 0 for a in addrs)  # so offsets mod 16 are address residues
    want_dev = [torch.from_numpy(w).cuda() for w in want]
    enc = RS.New(k, m)
    plan = B.StripePlan(enc, **{layout: lay.entries(addrs)})
    info = plan.info()
    if layout == "stripes":
        on_recs = [R.stripe_on_records(k, m, addrs[0] + int(a), int(s)) for a, s in zip(lay.a, lay.S)]
    else:
        on_recs = [R.object_on_records(k, m, addrs[0] + int(a), addrs[1] + int(b), int(s))
                   for a, b, s in zip(lay.a, lay.b, lay.S)]
    n_rec = sum(on_recs)
    assert info["n_fallback"] == n_rec and 0 < lay.n - n_rec < lay.n // 8, (info, n_rec)
    assert info["shard_bytes"] == int(lay.S.sum())
    col_passes = -(-k // ODD_MAX_K)
    log = {}

    def run(what, lost, call):
        init = lay.initial(want, lost)
        for b, i in zip(bufs, init):
            b.copy_(torch.from_numpy(i))
        torch.cuda.synchronize()
        c0 = counters()
        call()
        torch.cuda.synchronize()
        log[what] = changed(c0, counters())
        if not all(torch.equal(b, w) for b, w in zip(bufs, want_dev)):
            report(lay, bufs, want, what)
        return log[what]

    family = "odd_bitplane" if bp_plan(k, m) and k <= ODD_MAX_K else "odd_records"
    as_encode = {family: col_passes, "odd_edges": col_passes}
    # encode: every parity shard garbled first
    d = run("encode", list(range(k, k + m)), plan.encode)
    assert d == as_encode, d
    # reconstruct: one data shard; min(m, 4) shards, data and parity; all parity (the encode rows again)
    pats = L.single_patterns(k, m)
    for name, lost in zip(("rec-data", "rec-mixed", "rec-parity"), pats):
        present = [0 if i in lost else 1 for i in range(k + m)]
        d = run(name, lost, lambda: plan.reconstruct(present))
        if name == "rec-parity":
            assert d == as_encode, (name, d)
        else:
            assert set(d) <= {"odd_bitplane", "odd_records", "odd_edges"}, (name, d)
            assert d.get("odd_bitplane", 0) + d.get("odd_records", 0) == col_passes and d["odd_edges"] == col_passes, (name, d)
    # reconstruct_mixed: a mask per entry, every pattern of 1..m losses
    lost, which, P = L.mixed_losses(k, m, lay.n)
    assert set(lost.sum(1).tolist()) == set(range(1, m + 1))
    assert P > lay.n or set(which.tolist()) == set(range(P))
    d = dict(run("mixed", lost, lambda: plan.reconstruct_mixed(~lost)))
    if k <= ODD_MAX_K:
        assert d == {"mp_kernel_launches": 1}, d
    else:
        # k > 12: one single-pattern apply per entry (plan.cpp mp_other), aligned entries on the
        # 16-B kernels, the others on gf_apply_unaligned (k <= 16) or gf_wide
        assert d.pop("mp_per_stripe_calls") == lay.n and "mp_kernel_launches" not in d, d
        route = "ar_unaligned" if k <= 16 else "ar_wide"
        assert d.pop(route) == n_rec, (d, n_rec)
        assert d.pop("ar_vec", 0) + d.pop("ar_packed", 0) == (lay.n - n_rec) * -(-k // 16) and not d, d
    print(f"APPLY-SWEEP plan {k}+{m} {layout} entries={lay.n} resident={sum(lay.sizes)} records={n_rec} "
          f"tiles={info['n_tiles']} patterns={P} {log}")


@pytest.mark.parametrize("k,m", [(4, 2), (12, 4)])
def test_mixed_plan_second_tile_seam(k, m):
    """gf_mixed_plan's tile is 3968 B: every length from 4401 to 2 x 3968 + 368
    in one stripe plan, a mask per entry over every pattern of 1..m losses."""
    assert B.mixed_plan_tile_bytes() == WIDE_TILE
    lay = L.Layout(k, m, "stripes", smin=SMAX + 1, smax=TOP)
    assert lay.n == TOP - SMAX and sum(lay.sizes) <= CAP
    want = lay.expected()
    lost, which, P = L.mixed_losses(k, m, lay.n)
    assert set(lost.sum(1).tolist()) == set(range(1, m + 1)) and set(which.tolist()) == set(range(P))
    buf = torch.from_numpy(lay.initial(want, lost)[0]).cuda()
    assert buf.data_ptr() % 16 == 0
    plan = B.StripePlan(RS.New(k, m), stripes=lay.entries([buf.data_ptr()]))
    c0 = counters()
    plan.reconstruct_mixed(~lost)
    torch.cuda.synchronize()
    delta = changed(c0, counters())
    if not torch.equal(buf, torch.from_numpy(want[0]).cuda()):
        report(lay, [buf], want, "mixed")
    assert delta == {"mp_kernel_launches": 1}, delta
    print(f"APPLY-SWEEP plan-mixed {k}+{m} stripes S={SMAX + 1}..{TOP} entries={lay.n} resident={sum(lay.sizes)} "
          f"patterns={P} {delta}")


# ---- 3. strided views ---------------------------------------------------------

def stride_for(row_bytes):
    """The first stride >= row_bytes + 5 that is 1 mod 16."""
    t = row_bytes + L.GAP
    return t + (1 - t) % 16


def length_chunks(lengths, bytes_of):
    out, cur, tot = [], [], 0
    for S in lengths:
        b = bytes_of(S)
        if cur and tot + b > CHUNK:
            out.append(cur)
            cur, tot = [], 0
        cur.append(S)
        tot += b
    return out + ([cur] if cur else [])


STEP = TOP + 9  # pool columns between the objects of one length


def pool_dev(k, m):
    return torch.tensor(L.pool(k, m), device="cuda")


def first_col(S):
    return (S * 40503) % (L.POOL - N_OBJ * STEP)


class Region:
    """The 16 objects of one length in one buffer: object o's shard i at
    start + o stride + i S."""

    def __init__(self, start, stride, S, n_shards):
        self.start, self.stride, self.S, self.n = start, stride, S, n_shards

    def view(self, buf, i=None):
        """[16, S] of shard i, or [16, n, S] of all shards"""
        if i is None:
            return buf.as_strided((N_OBJ, self.n, self.S), (self.stride, self.S, 1), self.start)
        return buf.as_strided((N_OBJ, self.S), (self.stride, 1), self.start + i * self.S)


def place_regions(lengths, residue, n_shards, stride):
    regs, pos = {}, 0
    for S in lengths:
        pos = L._place(pos, residue(S))
        regs[S] = Region(pos, stride(S), S, n_shards)
        pos += N_OBJ * stride(S)
    return regs, pos + 11


def locate_view(regs, off):
    starts = sorted((r.start, S) for S, r in regs.items())
    i = int(np.searchsorted([s for s, _ in starts], off, side="right")) - 1
    if i < 0:
        return f"offset {off}, before the first region"
    S = starts[i][1]
    r = regs[S]
    o, w = divmod(off - r.start, r.stride)
    if o >= N_OBJ:
        return f"{off - r.start - N_OBJ * r.stride} bytes past the regions of S={S}"
    where = f"shard {w // S} position {w % S}" if w < r.n * S else f"slack byte {w - r.n * S}"
    return f"S={S} object {o} (base mod 16 = {(r.start + o * r.stride) % 16}) {where}"


def compare(label, bufs, wants, regs_of):
    for name in bufs:
        if torch.equal(bufs[name], wants[name]):
            continue
        g, w = bufs[name].cpu().numpy(), wants[name].cpu().numpy()
        bad = np.nonzero(g != w)[0]
        pytest.fail(f"{label}: {bad.size} bytes of buffer {name} differ; first: "
                    + "; ".join(f"{locate_view(regs_of[name], int(o))} got {int(g[o])} want {int(w[o])}" for o in bad[:8]))


def parts_of(k):
    """Cases per (shape, op): length ranges of about equal bytes."""
    return 1 if k <= 8 else (2 if k <= 12 else 4)


def part_lengths(part, parts, lo=1, hi=SMAX):
    edge = [lo + int(round((hi + 1 - lo) * np.sqrt(i / parts))) for i in range(parts + 1)]
    edge[-1] = hi + 1
    return list(range(edge[part], edge[part + 1]))


# (k, m, apply route, main-kernel family of an encode)
VIEW_SHAPES = [
    (4, 2, "odd", "strided"),      # fused guard band once a shard has 2 tiles
    (2, 4, "odd", "strided"),      # R = 4: separate edge launch
    (8, 2, "odd", "strided"),      # register tables
    (8, 3, "odd", "records"),      # table records
    (6, 3, "odd", "bitplane"),
    (11, 4, "odd", "records"),     # table records, tables in LDS
    (10, 4, "odd", "bitplane"),
    (11, 2, "odd", "strided"),     # strided, K > 8 (12+2 codes from records: K R = 24)
    (16, 4, "unaligned", None),    # gf_apply_unaligned
    (20, 4, "wide", None),         # gf_wide
]
VIEW_CASES = [(k, m, route, fam, p) for k, m, route, fam in VIEW_SHAPES for p in range(parts_of(k))]
VIEW_IDS = [f"{k}+{m}-part{p}" for k, m, _, _, p in VIEW_CASES]


def databuf_sweep(k, m, route, family, op, lengths):
    """hbec_encode_batch (op 'encode') or hbec_reconstruct_batch of the pattern
    S mod 3 over 16 objects per length: data and parity in separate buffers,
    shards S apart, every view at one stride = 1 mod 16, the data base at
    residue 0 and the parity base at (S >> 4) & 15."""
    enc = RS.New(k, m)
    cw = pool_dev(k, m)
    pats = L.single_patterns(k, m)
    stride = lambda S: stride_for(max(k, m) * S)  # noqa: E731
    total = {}
    calls = n_main = n_fused = 0
    for chunk in length_chunks(lengths, lambda S: 2 * N_OBJ * stride(S)):
        dreg, dsize = place_regions(chunk, lambda S: 0, k, stride)
        preg, psize = place_regions(chunk, lambda S: (S >> 4) & 15, m, stride)
        assert 2 * (dsize + psize) <= CAP
        want = {"data": torch.full((dsize,), L.FILL, dtype=torch.uint8, device="cuda"),
                "parity": torch.full((psize,), L.FILL, dtype=torch.uint8, device="cuda")}
        for S in chunk:
            src = cw.as_strided((N_OBJ, k + m, S), (STEP, L.POOL, 1), first_col(S))
            dreg[S].view(want["data"]).copy_(src[:, :k])
            preg[S].view(want["parity"]).copy_(src[:, k:])
        bufs = {n: w.clone() for n, w in want.items()}
        assert bufs["data"].data_ptr() % 16 == 0 and bufs["parity"].data_ptr() % 16 == 0
        lost_of = {}
        for S in chunk:
            lost_of[S] = list(range(k, k + m)) if op == "encode" else pats[S % 3]
            for i in lost_of[S]:
                (dreg[S].view(bufs["data"], i) if i < k else preg[S].view(bufs["parity"], i - k)).fill_(L.GARBLE)
        d0, p0 = bufs["data"].data_ptr(), bufs["parity"].data_ptr()
        c0 = counters()
        for S in chunk:
            views = [(d0 + dreg[S].start + j * S, stride(S)) for j in range(k)]
            views += [(p0 + preg[S].start + r * S, stride(S)) for r in range(m)]
            assert views[k][0] % 16 == (S >> 4) & 15 and views[0][0] % 16 == 0 and stride(S) % 16 == 1
            if op == "encode":
                B.encode_views(enc, views, N_OBJ, S)
            else:
                B.reconstruct_views(enc, views, [0 if i in lost_of[S] else 1 for i in range(k + m)], N_OBJ, S)
        torch.cuda.synchronize()
        for f, v in changed(c0, counters()).items():
            total[f] = total.get(f, 0) + v
        compare(f"databuf {op} {k}+{m}", bufs, want, {"data": dreg, "parity": preg})
        calls += len(chunk)
        n_main += sum(S > MIN_MAIN for S in chunk)
        n_fused += sum(S >= FUSE_FROM for S in chunk)
    # the route: one pass per call (<= 4 rows from <= 16 inputs; gf_wide one count per call)
    routes = {f: v for f, v in total.items() if f.startswith("ar_")}
    assert routes == {"ar_" + route: calls}, (routes, calls)
    odd = {f: v for f, v in total.items() if f.startswith("odd_")}
    if route != "odd":
        assert not odd, odd
    else:
        mains = {f: odd.get("odd_" + f, 0) for f in ("bitplane", "records", "strided")}
        assert sum(mains.values()) == n_main, (odd, n_main)
        if op == "encode":
            assert mains[family] == n_main, (odd, family)
            # the guard band: inside gf_odd for K <= 4, R <= 3 from two tiles per shard, else its own launch
            fused = n_fused if (k, m) == (4, 2) else 0
            assert odd.get("odd_fused", 0) == fused and odd.get("odd_edges", 0) == calls - fused, (odd, calls, fused)
        else:
            assert odd.get("odd_fused", 0) + odd.get("odd_edges", 0) == calls, (odd, calls)
    assert not [f for f in total if f.startswith("mp_")]
    return calls, total


@pytest.mark.parametrize("k,m,route,family,part", VIEW_CASES, ids=VIEW_IDS)
def test_databuf_encode_every_length(k, m, route, family, part):
    lengths = part_lengths(part, parts_of(k))
    calls, total = databuf_sweep(k, m, route, family, "encode", lengths)
    print(f"APPLY-SWEEP databuf-encode {k}+{m} S={lengths[0]}..{lengths[-1]} calls={calls} {total}")


@pytest.mark.parametrize("k,m,route,family,part", VIEW_CASES, ids=VIEW_IDS)
def test_databuf_reconstruct_every_length(k, m, route, family, part):
    lengths = part_lengths(part, parts_of(k))
    calls, total = databuf_sweep(k, m, route, family, "reconstruct", lengths)
    print(f"APPLY-SWEEP databuf-reconstruct {k}+{m} S={lengths[0]}..{lengths[-1]} calls={calls} {total}")


@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("op", ["encode", "reconstruct"])
def test_databuf_unaligned_second_tile_seam(op, part):
    """gf_apply_unaligned's tile is 3968 B: 16+4 from 4401 to 2 x 3968 + 368."""
    lengths = part_lengths(part, 4, SMAX + 1, TOP)
    calls, total = databuf_sweep(16, 4, "unaligned", None, op, lengths)
    print(f"APPLY-SWEEP databuf-{op} 16+4 S={lengths[0]}..{lengths[-1]} calls={calls} {total}")


SCATTER_LENGTHS = (list(range(145, 209)) + list(range(960, 1089)) + list(range(1960, 2101))
                   + list(range(3990, 4121)))


SCATTER_CASES = [(4, "odd"), (2, "odd"), (8, "odd"), (6, "odd"), (11, "odd"), (10, "odd"), (12, "odd"),
                 (16, "unaligned"), (20, "wide")]


@pytest.mark.parametrize("k,route", SCATTER_CASES, ids=[f"{c[0]}-inputs" for c in SCATTER_CASES])
def test_scattered_apply(k, route):
    """hbec_apply_batch with every view in a buffer of its own, view v at base
    residue (7 v + 3 S) & 15 (inputs differ from each other mod 4 whatever S
    is), k inputs, 1 + S % 4 output rows, random coefficients with about 15 %
    zeros and 15 % ones."""
    m = 4
    cw = pool_dev(k, m)
    host = L.pool(k, m)
    stride = lambda S: stride_for(S)  # noqa: E731
    total = {}
    calls = 0
    n_views = k + 4
    for chunk in length_chunks(SCATTER_LENGTHS, lambda S: 2 * n_views * N_OBJ * stride(S)):
        regs, want = {}, {}
        for v in range(n_views):
            regs[v], size = place_regions(chunk, lambda S, v=v: (7 * v + 3 * S) & 15, 1, stride)
            want[v] = torch.full((size,), L.FILL, dtype=torch.uint8, device="cuda")
        coeffs = {}
        for S in chunk:
            rows, c = 1 + S % 4, first_col(S)
            rng = np.random.default_rng(1000 * k + S)
            co = rng.integers(0, 256, (rows, k), dtype=np.uint8)
            special = rng.random((rows, k))
            co[special < 0.15] = 0
            co[(special >= 0.15) & (special < 0.3)] = 1
            coeffs[S] = co
            res = CO.apply(co, [host[j, c:c + N_OBJ * S] for j in range(k)])
            for j in range(k):
                regs[j][S].view(want[j], 0).copy_(cw.as_strided((N_OBJ, S), (S, 1), j * L.POOL + c))
            for r in range(rows):
                regs[k + r][S].view(want[k + r], 0).copy_(torch.from_numpy(res[r].reshape(N_OBJ, S)).cuda())
        bufs = {v: w.clone() for v, w in want.items()}
        for S in chunk:
            for r in range(1 + S % 4):
                regs[k + r][S].view(bufs[k + r], 0).fill_(L.GARBLE)
        base = {v: b.data_ptr() for v, b in bufs.items()}
        assert all(a % 16 == 0 for a in base.values())
        c0 = counters()
        for S in chunk:
            rows = 1 + S % 4
            iv = [(base[j] + regs[j][S].start, stride(S)) for j in range(k)]
            ov = [(base[k + r] + regs[k + r][S].start, stride(S)) for r in range(rows)]
            assert all(a % 16 == (7 * v + 3 * S) & 15 for v, (a, _) in enumerate(iv))
            B.apply_views(rows, k, coeffs[S].tolist(), iv, ov, N_OBJ, S)
        torch.cuda.synchronize()
        for f, v in changed(c0, counters()).items():
            total[f] = total.get(f, 0) + v
        compare(f"scattered apply {k} inputs", bufs, want, regs)
        calls += len(chunk)
    assert calls == len(SCATTER_LENGTHS) == 465
    routes = {f: v for f, v in total.items() if f.startswith("ar_")}
    assert routes == {"ar_" + route: calls}, (routes, calls)
    odd = {f: v for f, v in total.items() if f.startswith("odd_")}
    if route != "odd":
        assert not odd, odd
    else:
        n_main = sum(S > MIN_MAIN for S in SCATTER_LENGTHS)
        assert sum(odd.get("odd_" + f, 0) for f in ("bitplane", "records", "strided")) == n_main, (odd, n_main)
        assert odd.get("odd_fused", 0) + odd.get("odd_edges", 0) == calls, (odd, calls)
    print(f"APPLY-SWEEP scattered-apply {k} inputs calls={calls} {total}")
