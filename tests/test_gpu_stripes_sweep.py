"""Byte-exact sweep of the tiled stripes kernel gf_apply_stripes<K, R, SPLIT,
ACC> of csrc/stripes.hip as stripe plans and object plans run it, one case per
plan (tests/stripes_sweep_cases.py; what its cases cover is asserted in
tests/test_stripes_sweep_cases.py).  The mirrored variants only run from the
host path: tests/test_gpu_host_seams.py.

The kernel codes every 16-B-aligned entry of a plan, every chunk of the host
staging ring and every pinned stripe, and a wrong byte from it is silent data
loss.  What varies inside it is a function of each tile's `valid` bytes (below
a tile: loads clamped to valid - 16, stores masked per 1 KiB window), of the
tile's place in the pipelined loop (prologue, loop body with the record
fetched two ahead, epilogue, stand-in tiles of the last row), of the per-shard
base selection of an object plan, and of the read-back of an accumulate pass.
Plan launches are sized CUs x 1 block x 4 waves, so on a whole chip the loop
body needs more than a thousand tiles to run once: every call here runs under
set_stripes_grid_cap(1), one block of 4 waves, where a plan of a few hundred
tiles walks the loop hundreds of times; encode() runs again under a cap of 3
blocks and on the default grid.

One plan per (k, layout) holds every shard length 16, 32, ..., 2 T + 368, each
entry 16-B aligned with 48 sentinel bytes after it, in several entry orders
(ascending; a seeded shuffle in which a wave's consecutive tiles differ in
`valid`; rotations that bring every `valid` value to the first and the last
iteration), with up to three 16-byte fillers so that n_tiles % 4 is what the
cases module assigned.  For k = 5..12 two entries sit at the record-route
threshold: 16 bytes below it (tiled) and on it (record kernels).

Every call: hbec_stripes_kernel_stats gains exactly the passes the restated
rule predicts, variant by variant; the odd-shard and apply-route counters move
only for the one entry on records.  The whole buffer is compared, shards,
sentinel gaps and fillers: after encode() with the oracle image (coracle
build_matrix / apply), after a reconstruct with the codeword; lost shards are
garbled with a second sentinel first.  No tolerance, no sampling of lengths.
"""
import numpy as np
import pytest
import torch

from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO

import route_rule as R
import stripes_sweep_cases as S

pytestmark = pytest.mark.gpu

FILL, GARBLE = 0xA7, 0x5C
CAPS = (1, 3, 0)  # encode(); every reconstruct runs under the first


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


@pytest.fixture(autouse=True)
def _hooks():
    yield
    B.set_stripes_grid_cap(0)


def counters():
    c = {"sk_" + f: v for f, v in B.stripes_kernel_stats().items()}
    c.update({"ar_" + f: v for f, v in B.apply_route_stats().items()})
    c.update({"odd_" + f: v for f, v in B.odd_path_stats().items()})
    return c


def changed(c0, c1):
    return {f: c1[f] - c0[f] for f in c0 if c1[f] != c0[f]}


class Layout:
    """Where the entries of one order lie.  Stripes: one buffer, entry e's k+m
    shards back to back at off[0][e].  Objects: a data buffer (k shards per
    entry) and a parity buffer (m shards).  Every entry is followed by GAP
    sentinel bytes; the entry on the record route starts 16 bytes into a 128-B
    line, so that it is no whole-line entry whatever its length."""

    def __init__(self, p, order):
        self.p, self.order = p, order
        self.S = list(order.entries)
        k, m = p.k, p.m
        self.parts = [(0, k + m)] if p.layout == "stripes" else [(0, k), (k, k + m)]
        self.off = [[] for _ in self.parts]
        pos = [0 for _ in self.parts]
        for s in self.S:
            for b, (lo, hi) in enumerate(self.parts):
                if S.on_records(k, s):
                    pos[b] += (16 - pos[b]) % 128
                self.off[b].append(pos[b])
                pos[b] += (hi - lo) * s + S.GAP
        self.sizes = pos
        self.col = np.concatenate([[0], np.cumsum(self.S)]).astype(np.int64)

    def images(self, cw):
        """(expected bytes, shard index of every byte or -1) per buffer"""
        want = [np.full(n, FILL, np.uint8) for n in self.sizes]
        sid = [np.full(n, -1, np.int8) for n in self.sizes]
        for e, s in enumerate(self.S):
            c = int(self.col[e])
            for b, (lo, hi) in enumerate(self.parts):
                o = self.off[b][e]
                want[b][o:o + (hi - lo) * s].reshape(hi - lo, s)[:] = cw[lo:hi, c:c + s]
                sid[b][o:o + (hi - lo) * s].reshape(hi - lo, s)[:] = np.arange(lo, hi, dtype=np.int8)[:, None]
        return want, sid

    def entries(self, addrs):
        if self.p.layout == "stripes":
            return [(addrs[0] + o, s) for o, s in zip(self.off[0], self.S)]
        return [(addrs[0] + a, addrs[1] + b, s) for a, b, s in zip(self.off[0], self.off[1], self.S)]

    def where(self, b, off):
        """the (S, shard, position) of byte `off` of buffer b"""
        e = int(np.searchsorted(self.off[b], off, side="right")) - 1
        s = self.S[e]
        lo, hi = self.parts[b]
        w = off - self.off[b][e]
        if w >= (hi - lo) * s:
            return f"sentinel byte {w - (hi - lo) * s} after entry {e} (S={s})"
        return f"entry {e} S={s} shard {lo + w // s} position {w % s}"


@pytest.fixture(scope="module")
def codewords():
    """k+m rows of codeword columns per plan, computed once: [k+m, columns]"""
    cache = {}

    def get(p):
        if p not in cache:
            n = max(sum(o.entries) for o in S.orders(p))
            rng = np.random.default_rng(1000 * p.k + 10 * p.m + (p.layout == "objects"))
            data = rng.integers(0, 256, (p.k, n), dtype=np.uint8)
            par = CO.apply(CO.build_matrix(p.k, p.m)[p.k:], list(data))
            cache[p] = np.concatenate([data, np.stack(par)])
        return cache[p]

    return get


def fail_at(p, lay, what, bufs, want):
    for b, (g, w) in enumerate(zip(bufs, want)):
        g = g.cpu().numpy()
        bad = np.flatnonzero(g != w)
        if bad.size:
            o = int(bad[0])
            pytest.fail(f"{p.k}+{p.m} {p.layout} order {lay.order.name} {what}: {bad.size} bytes of buffer {b} differ; "
                        f"first at {lay.where(b, o)}: got {int(g[o])} want {int(w[o])}")


@pytest.mark.parametrize("p", S.PLANS, ids=[S.plan_id(p) for p in S.PLANS])
def test_every_length_of_the_plan(p, codewords):
    k, m = p.k, p.m
    T = S.tile_bytes(k)
    enc = RS.New(k, m)
    cw = codewords(p)
    log = []
    for order in S.orders(p):
        lay = Layout(p, order)
        want, sid = lay.images(cw)
        want_dev = [torch.from_numpy(w).cuda() for w in want]
        sid_dev = [torch.from_numpy(s).cuda() for s in sid]
        bufs = [torch.empty(n, dtype=torch.uint8, device="cuda") for n in lay.sizes]
        addrs = [b.data_ptr() for b in bufs]
        assert all(a % 128 == 0 for a in addrs)  # so offsets mod 128 are address residues
        plan = B.StripePlan(enc, **{p.layout: lay.entries(addrs)})
        info = plan.info()
        if p.layout == "stripes":
            on_recs = [R.stripe_on_records(k, m, a, s) for a, s in lay.entries(addrs)]
        else:
            on_recs = [R.object_on_records(k, m, a, b, s) for a, b, s in lay.entries(addrs)]
        assert on_recs == [S.on_records(k, s) for s in lay.S]
        assert info["tile_bytes"] == T and info["n_tiles"] == S.n_tiles(p, order), (order.name, info)
        assert info["n_fallback"] == sum(on_recs) == S.n_records(p, order) == (1 if S.boundary(p) else 0)
        assert info["shard_bytes"] == sum(lay.S)
        n_rec = sum(on_recs)
        for name, lost in S.lost_patterns(p):
            if order.rotation and name != "encode":
                continue
            present = [0 if i in lost else 1 for i in range(k + m)]
            call = plan.encode if name == "encode" else (lambda: plan.reconstruct(present))
            for cap in (CAPS if name == "encode" and not order.rotation else CAPS[:1]):
                for b, w, s in zip(bufs, want_dev, sid_dev):
                    gone = torch.zeros_like(s, dtype=torch.bool)
                    for i in lost:
                        gone |= s == i
                    b.copy_(torch.where(gone, torch.full_like(w, GARBLE), w))
                B.set_stripes_grid_cap(cap)
                torch.cuda.synchronize()
                c0 = counters()
                call()
                torch.cuda.synchronize()
                d = changed(c0, counters())
                what = f"{name} lost={list(lost)} cap={cap}"
                sk = {f[3:]: v for f, v in d.items() if f.startswith("sk_")}
                assert sk == {v: n for v, n in S.op_launches(p, lost).items() if n}, (what, d)
                rest = {f: v for f, v in d.items() if not f.startswith("sk_")}
                if n_rec == 0:
                    assert not rest, (what, d)
                else:
                    # the one entry on records: one main record pass per 12 inputs and row pass, and its guard band
                    assert set(rest) <= {"odd_bitplane", "odd_records", "odd_strided", "odd_edges", "odd_fused"}, (what, d)
                    mains = sum(rest.get(f, 0) for f in ("odd_bitplane", "odd_records", "odd_strided"))
                    assert mains == -(-len(lost) // 4) * -(-k // 12), (what, d)
                if not all(torch.equal(b, w) for b, w in zip(bufs, want_dev)):
                    fail_at(p, lay, what, bufs, want)
                log.append((order.name, name, cap, sk))
        # the expected image is not the garbled start: the oracle's parity is in it
        assert (want[-1][lay.off[-1][0]:lay.off[-1][0] + 16] != GARBLE).any()
        del plan
    o0 = S.orders(p)[0]
    print(f"STRIPES-SWEEP {S.plan_id(p)} T={T} entries={len(o0.entries)} n_tiles={S.n_tiles(p, o0)} "
          f"orders={len(S.orders(p))} calls={len(log)} resident={sum(Layout(p, o0).sizes)} "
          f"launches={ {n: S.op_launches(p, l) for n, l in S.lost_patterns(p)} }")
