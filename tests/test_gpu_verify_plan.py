"""hbec_verify_plan: Encoder.Verify of a whole plan (stripes or objects of any
sizes at any alignment) in a fixed number of launches, one flag per stripe.

Codewords come from the oracle (oracle.coracle build_matrix / apply).  The
stripes sit in one buffer (objects: a data and a parity buffer) with a few
bytes of slack before, between and after them; stripes whose S is a multiple
of 16 alternate between 16-B-aligned offsets (the plan's tile records,
gf_verify_tiles) and odd ones (gf_verify_recs), all others are at odd offsets.
Every parity coefficient of the codec's matrix is non-zero (MDS), so a flip of
any single data or parity byte must be flagged, and nothing else may be.
"""
import functools

import numpy as np
import pytest
import torch

from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO

pytestmark = pytest.mark.gpu

SHAPES = [(4, 2), (8, 3), (10, 4), (12, 4)]
LAYOUTS = ["stripes", "objects"]


def tile_sizes(k, m):
    """(T, A): the any-alignment kernel's tile and the plan's aligned tile."""
    enc = RS.New(k, m)
    return B.verify_plan_tile_bytes(k), B.StripePlan(enc, stripes=[]).info()["tile_bytes"]


def size_set(k, m, seed, n_random=40, zeros=6):
    T, A = tile_sizes(k, m)
    rng = np.random.default_rng(seed)
    sizes = [1, 3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, T - 1, T, T + 1, 2 * T - 1, 2 * T + 17, A, A + 16, 3 * A]
    sizes += [int(x) for x in rng.integers(1, 300_000, n_random)]
    sizes += [A, 3 * A, 4096, 2 * A + 16]  # more aligned ones, so both placements occur
    order = rng.permutation(len(sizes))
    sizes = [sizes[i] for i in order]
    for z in range(zeros):  # zero-length stripes scattered through the array (first and last too)
        sizes.insert(0 if z == 0 else (len(sizes) if z == 1 else int(rng.integers(1, len(sizes)))), 0)
    return sizes


class Case:
    """Clean codewords of `sizes` (host), and where every shard lives:
    shards[i] = [(buffer, offset)] * (k+m); slack = [(buffer, lo, hi)]."""

    def __init__(self, k, m, layout, sizes, seed):
        self.k, self.m, self.layout, self.sizes = k, m, layout, sizes
        rng = np.random.default_rng(seed)
        rows = CO.build_matrix(k, m)[k:]
        n_buf = 1 if layout == "stripes" else 2
        per = [(k + m,)] if layout == "stripes" else [(k,), (m,)]
        pos = [0] * n_buf
        self.shards, self.base, self.slack = [], [], []
        aligned_turn = 0
        for s in sizes:
            where, bases = [], []
            for b in range(n_buf):
                lo = pos[b]
                off = lo + 1 + int(rng.integers(0, 13))
                if s and s % 16 == 0 and aligned_turn % 2 == 0:
                    off = (off + 15) & ~15
                elif off % 16 == 0:
                    off += 5
                self.slack.append((b, lo, off))
                bases.append(off)
                where += [(b, off + j * s) for j in range(per[b][0])]
                pos[b] = off + per[b][0] * s
            if s and s % 16 == 0:
                aligned_turn += 1
            self.shards.append(where)
            self.base.append(bases)
        self.bufs = []
        for b in range(n_buf):
            self.slack.append((b, pos[b], pos[b] + 11))
            self.bufs.append(rng.integers(0, 256, pos[b] + 11, dtype=np.uint8))
        for s, where in zip(sizes, self.shards):
            if s == 0:
                continue
            data = [self.bufs[b][o:o + s] for b, o in where[:k]]
            for (b, o), p in zip(where[k:], CO.apply(rows, data)):
                self.bufs[b][o:o + s] = p

    def upload(self, bufs=None):
        return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (bufs or self.bufs)]

    def plan(self, enc, tensors):
        if self.layout == "stripes":
            return B.StripePlan(enc, stripes=[(tensors[0].data_ptr() + b[0], s) for b, s in zip(self.base, self.sizes)])
        return B.StripePlan(enc, objects=[(tensors[0].data_ptr() + b[0], tensors[1].data_ptr() + b[1], s)
                                          for b, s in zip(self.base, self.sizes)])

    def corrupt(self, picks):
        """Copies of the buffers with byte `pos` of shard `i` of stripe `e` flipped for (e, i, pos) in picks."""
        bufs = [x.copy() for x in self.bufs]
        for e, i, p in picks:
            b, o = self.shards[e][i]
            bufs[b][o + p] ^= 0x5A
        return bufs


@functools.lru_cache(maxsize=None)
def case(k, m, layout):
    return Case(k, m, layout, size_set(k, m, 100 * k + m), 7 * k + m + len(layout))


def run(plan, n, stream=None, init=0):
    flags = torch.full((n,), init, dtype=torch.int32, device="cuda")
    plan.verify(flags, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    return flags.cpu().numpy()


def single_byte_picks(c):
    """About a third of the stripes, one byte each: the shard index cycles over
    0..k+m-1, the position over the edge cases, clipped to the shard."""
    T = B.verify_plan_tile_bytes(c.k)
    live = [e for e, s in enumerate(c.sizes) if s]
    picks = []
    for q, e in enumerate(live[::3]):
        s = c.sizes[e]
        cand = [0, 1, 15, 16, s - 17, s - 16, s - 1, T - 1, T, T + 1, s // 2]
        picks.append((e, q % (c.k + c.m), min(max(cand[q % len(cand)], 0), s - 1)))
    return picks


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", SHAPES)
def test_clean_plan_flags_nothing(k, m, layout):
    c = case(k, m, layout)
    t = c.upload()
    plan = c.plan(RS.New(k, m), t)
    info = plan.info()
    if k <= 8:
        assert info["n_tiles"] > 0  # both kernels run
    flags = run(plan, len(c.sizes))
    assert not flags.any(), np.nonzero(flags)[0]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", SHAPES)
def test_exact_flags_for_single_byte_flips(k, m, layout):
    c = case(k, m, layout)
    picks = single_byte_picks(c)
    assert len(picks) >= (len(c.sizes) - 6) // 3
    t = c.upload(c.corrupt(picks))
    plan = c.plan(RS.New(k, m), t)
    flags = run(plan, len(c.sizes))
    want = np.zeros(len(c.sizes), np.int32)
    want[[e for e, _, _ in picks]] = 1
    assert np.array_equal(flags, want), (np.nonzero(flags != want)[0], [p for p in picks if flags[p[0]] != 1])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", SHAPES)
def test_two_flips_in_different_tiles_flag_once(k, m, layout):
    c = case(k, m, layout)
    T, A = tile_sizes(k, m)
    big = [e for e, s in enumerate(c.sizes) if s >= 2 * max(T, A) + 16]
    picks = []
    for q, e in enumerate(big[:12]):
        s = c.sizes[e]
        picks += [(e, q % (k + m), 0), (e, (q + k) % (k + m), s - 1)]
    t = c.upload(c.corrupt(picks))
    flags = run(c.plan(RS.New(k, m), t), len(c.sizes))
    want = np.zeros(len(c.sizes), np.int32)
    want[[e for e, _, _ in picks]] = 1
    assert np.array_equal(flags, want)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_flags_are_ored_not_stored(layout):
    k, m = 8, 3
    c = case(k, m, layout)
    picks = single_byte_picks(c)
    enc = RS.New(k, m)
    t = c.upload(c.corrupt(picks))
    plan = c.plan(enc, t)
    flags = torch.full((len(c.sizes),), 2, dtype=torch.int32, device="cuda")  # a caller's bit 1
    plan.verify(flags)
    torch.cuda.synchronize()
    want = np.full(len(c.sizes), 2, np.int32)
    want[[e for e, _, _ in picks]] = 3
    assert np.array_equal(flags.cpu().numpy(), want)
    # repaired in place: a second call leaves the earlier flags as they were
    for x, clean in zip(t, c.bufs):
        x.copy_(torch.from_numpy(clean))
    plan.verify(flags)
    torch.cuda.synchronize()
    assert np.array_equal(flags.cpu().numpy(), want)
    assert not run(plan, len(c.sizes)).any()


@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (10, 4)])
@pytest.mark.parametrize("which", ["T+5", "4096"])
def test_agrees_with_uniform_verify(k, m, which):
    S = B.verify_plan_tile_bytes(k) + 5 if which == "T+5" else 4096
    n = 64
    rng = np.random.default_rng(S + k)
    rows = CO.build_matrix(k, m)[k:]
    buf = rng.integers(0, 256, (n, (k + m) * S), dtype=np.uint8)
    for o in range(n):
        par = CO.apply(rows, [buf[o, j * S:(j + 1) * S] for j in range(k)])
        for r in range(m):
            buf[o, (k + r) * S:(k + r + 1) * S] = par[r]
    bad = sorted(rng.choice(n, 20, replace=False).tolist())
    for q, o in enumerate(bad):
        buf[o, (q % (k + m)) * S + int(rng.integers(0, S))] ^= 0x01
    t = torch.from_numpy(buf).cuda()
    enc = RS.New(k, m)
    plan = B.StripePlan(enc, stripes=[(t.data_ptr() + o * (k + m) * S, S) for o in range(n)])
    got = run(plan, n)
    ref = torch.zeros(n, dtype=torch.int32, device="cuda")
    B.verify_views(enc, B.shard_views(t, k + m, S), n, S, ref)
    torch.cuda.synchronize()
    assert np.array_equal(got, ref.cpu().numpy())
    assert np.nonzero(got)[0].tolist() == bad


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (10, 4)])
def test_bytes_outside_the_stripes_are_ignored_and_nothing_is_written(k, m, layout):
    c = case(k, m, layout)
    picks = single_byte_picks(c)
    bufs = c.corrupt(picks)
    rng = np.random.default_rng(5)
    for b, lo, hi in c.slack:  # other garbage in every gap of both regions
        bufs[b][lo:hi] = rng.integers(0, 256, hi - lo, dtype=np.uint8)
    t = c.upload(bufs)
    keep = [x.clone() for x in t]
    flags = run(c.plan(RS.New(k, m), t), len(c.sizes))
    want = np.zeros(len(c.sizes), np.int32)
    want[[e for e, _, _ in picks]] = 1
    assert np.array_equal(flags, want)
    for x, y in zip(t, keep):
        assert torch.equal(x, y)


def test_side_stream():
    k, m = 8, 3
    c = case(k, m, "stripes")
    picks = single_byte_picks(c)
    t = c.upload(c.corrupt(picks))
    plan = c.plan(RS.New(k, m), t)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        flags = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
        plan.verify(flags, stream=side)
    side.synchronize()
    want = np.zeros(len(c.sizes), np.int32)
    want[[e for e, _, _ in picks]] = 1
    assert np.array_equal(flags.cpu().numpy(), want)


def test_other_route_16_4_is_exact_and_counted():
    k, m = 16, 4
    sizes = [1, 17, 0, 64, 4096, 1985, 33, 100_001, 5000, 0, 16, 2048, 777, 31, 65_536, 12_345, 3, 129, 1024, 40_000,
             63, 255, 9_999, 2]
    c = Case(k, m, "stripes", sizes, 11)
    live = [e for e, s in enumerate(sizes) if s]
    picks = [(e, (3 * q) % (k + m), (c.sizes[e] - 1) * (q % 2)) for q, e in enumerate(live[::2])]
    t = c.upload(c.corrupt(picks))
    plan = c.plan(RS.New(k, m), t)
    s0 = B.verify_plan_stats()
    flags = run(plan, len(sizes))
    s1 = B.verify_plan_stats()
    want = np.zeros(len(sizes), np.int32)
    want[[e for e, _, _ in picks]] = 1
    assert np.array_equal(flags, want)
    assert s1["per_stripe_calls"] - s0["per_stripe_calls"] == len(live)
    assert s1["plan_launches"] == s0["plan_launches"]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_launch_count_does_not_depend_on_the_number_of_stripes(layout):
    k, m = 8, 3
    c1 = case(k, m, layout)
    c2 = Case(k, m, layout, c1.sizes + c1.sizes, 99)
    enc = RS.New(k, m)
    deltas = []
    for c in (c1, c2):
        t = c.upload()
        plan = c.plan(enc, t)
        s0 = B.verify_plan_stats()
        assert not run(plan, len(c.sizes)).any()
        s1 = B.verify_plan_stats()
        assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
        deltas.append(s1["plan_launches"] - s0["plan_launches"])
    assert deltas[0] == deltas[1] and 1 <= deltas[0] <= 3, deltas


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4)])
def test_encode_reconstruct_and_verify_share_one_plan(k, m, layout):
    c = case(k, m, layout)
    rng = np.random.default_rng(k)
    bufs = [x.copy() for x in c.bufs]
    # every parity shard wrong in every byte (an error of weight m <= the code's
    # distance - 1 is never a codeword: each stripe must be flagged); encode rewrites it
    for s, where in zip(c.sizes, c.shards):
        for b, o in where[k:]:
            bufs[b][o:o + s] ^= 0xEE
    t = c.upload(bufs)
    plan = c.plan(RS.New(k, m), t)
    assert run(plan, len(c.sizes)).astype(bool).tolist() == [s > 0 for s in c.sizes]
    plan.encode()
    assert not run(plan, len(c.sizes)).any()
    for x, clean in zip(t, c.bufs):
        assert np.array_equal(x.cpu().numpy(), clean)
    lost = sorted(rng.choice(k + m, size=m, replace=False).tolist())
    for s, where in zip(c.sizes, c.shards):
        for i in lost:
            b, o = where[i]
            t[b][o:o + s] ^= 0x3C
    assert run(plan, len(c.sizes)).astype(bool).tolist() == [s > 0 for s in c.sizes]
    plan.reconstruct([0 if i in lost else 1 for i in range(k + m)])
    assert not run(plan, len(c.sizes)).any()
    for x, clean in zip(t, c.bufs):
        assert np.array_equal(x.cpu().numpy(), clean)
