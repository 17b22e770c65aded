"""hbec_reconstruct_plan_mixed: reconstruct over a plan (stripes or objects of
any sizes at any alignment) with an erasure pattern per stripe, in one call.

Codewords come from the oracle (oracle.coracle build_matrix / apply).  The
stripes sit in one buffer (objects: a data and a parity buffer) with a few
random slack bytes before, between and after them; stripes whose S is a
multiple of 16 alternate between 16-B-aligned and odd offsets, all others are
at odd offsets.  Every case garbles the shards its masks call missing, makes
one call and compares the WHOLE buffers, slack included, with what they must
hold: the clean codeword in every rebuilt shard and the input everywhere else.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO

pytestmark = pytest.mark.gpu

LAYOUTS = ["stripes", "objects"]
W = 992  # one 64-lane window of the kernel (unaligned_tile.h)
U32P = C.POINTER(C.c_uint32)


def size_set(seed, n_random=20):
    """The smallest sizes at which the tile logic can go wrong, ~20 random
    ones, and 5 zero-length entries (first, last, interior)."""
    T = B.mixed_plan_tile_bytes()
    rng = np.random.default_rng(seed)
    sizes = [1, 3, 15, 16, 17, 31, 33, 63, 64, 65, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 17]
    sizes += [int(x) for x in rng.integers(1, 40_001, n_random)]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    for z in range(3):
        sizes.insert(int(rng.integers(1, len(sizes))), 0)
    return [0] + sizes + [0]


def sizes_for(n_live, seed):
    """size_set repeated until it has at least n_live non-empty entries."""
    sizes = []
    while sum(1 for s in sizes if s) < n_live:
        sizes += size_set(seed + len(sizes))
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
        self.live = [e for e, s in enumerate(sizes) if s]

    def upload(self, bufs=None):
        return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (bufs or self.bufs)]

    def plan(self, enc, tensors):
        if self.layout == "stripes":
            return B.StripePlan(enc, stripes=[(tensors[0].data_ptr() + b[0], s) for b, s in zip(self.base, self.sizes)])
        return B.StripePlan(enc, objects=[(tensors[0].data_ptr() + b[0], tensors[1].data_ptr() + b[1], s)
                                          for b, s in zip(self.base, self.sizes)])

    def garble(self, present, data_only=False, extra=False, wrong_full=False, seed=1):
        """(input, expected) buffers for one call with mask rows `present`.
        Input: random bytes in every missing shard; with `extra` also in the
        present shards beyond the first k (never read); with `wrong_full` in
        one shard of every all-present stripe (must stay as it is).
        Expected: the input with every rebuilt shard clean."""
        k, n = self.k, self.k + self.m
        rng = np.random.default_rng(seed)
        inp = [x.copy() for x in self.bufs]
        outs = {}
        for e in self.live:
            s, where = self.sizes[e], self.shards[e]
            missing = [i for i in range(n) if not present[e][i]]
            here = [i for i in range(n) if present[e][i]]
            g = list(missing) + (here[k:] if extra else [])
            if wrong_full and not missing:
                g.append(e % n)
            for i in g:
                b, o = where[i]
                inp[b][o:o + s] = rng.integers(0, 256, s, dtype=np.uint8)
            outs[e] = [i for i in missing if i < k or not data_only]
        want = [x.copy() for x in inp]
        for e, o_list in outs.items():
            s = self.sizes[e]
            for i in o_list:
                b, o = self.shards[e][i]
                want[b][o:o + s] = self.bufs[b][o:o + s]
        return inp, want


@functools.lru_cache(maxsize=None)
def case(k, m, layout, n_live=1):
    return Case(k, m, layout, sizes_for(n_live, 100 * k + m), 7 * k + m + len(layout))


def masks_with_missing(n, counts):
    out = []
    for c in counts:
        for lost in itertools.combinations(range(n), c):
            out.append([0 if i in lost else 1 for i in range(n)])
    return out


def spread(c, masks, seed, shuffle=True, full_every=0):
    """One mask row per entry: `masks` cycled over the live stripes (shuffled),
    every full_every-th live stripe all present; zero-length entries get masks too."""
    rng = np.random.default_rng(seed)
    order = [q % len(masks) for q in range(len(c.live))]
    if shuffle:
        rng.shuffle(order)
    present = np.ones((len(c.sizes), c.k + c.m), np.uint8)
    for q, e in enumerate(c.live):
        if full_every and q % full_every == full_every - 1:
            continue
        present[e] = masks[order[q]]
    for e, s in enumerate(c.sizes):
        if s == 0 and e % 2:
            present[e] = masks[e % len(masks)]
    return present


def check_equal(tensors, want):
    for b, (t, w) in enumerate(zip(tensors, want)):
        got = t.cpu().numpy()
        if not np.array_equal(got, w):
            bad = np.nonzero(got != w)[0]
            raise AssertionError(f"buffer {b}: {bad.size} bytes differ, first at {bad[:8].tolist()}")


def run_case(c, present, data_only=False, extra=False, wrong_full=False, stream=None):
    enc = RS.New(c.k, c.m)
    inp, want = c.garble(present, data_only=data_only, extra=extra, wrong_full=wrong_full)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    torch.cuda.synchronize()
    plan.reconstruct_mixed(present, data_only=data_only, stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    check_equal(t, want)
    return plan, t


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_4_2_mask(layout):
    c = case(4, 2, layout)
    masks = masks_with_missing(6, [1, 2])
    assert len(masks) == 21 and len(c.live) >= 21
    run_case(c, spread(c, masks, 1, full_every=9), wrong_full=True)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_8_3_mask(layout):
    masks = masks_with_missing(11, [1, 2, 3])
    assert len(masks) == 231
    c = case(8, 3, layout, len(masks))
    assert len(c.live) >= len(masks)
    run_case(c, spread(c, masks, 2, full_every=40), wrong_full=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(10, 4), (12, 4)])
def test_sampled_masks_k_above_8_run_on_the_kernel(k, m, layout):
    rng = np.random.default_rng(k)
    masks = []
    for q in range(200):
        lost = rng.choice(k + m, size=1 + q % 4, replace=False)
        masks.append([0 if i in lost else 1 for i in range(k + m)])
    c = case(k, m, layout, 200)
    s0 = B.mixed_plan_stats()
    run_case(c, spread(c, masks, 3, full_every=50), wrong_full=True)
    s1 = B.mixed_plan_stats()
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    assert 1 <= s1["kernel_launches"] - s0["kernel_launches"] <= 4


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_data_only_leaves_missing_parity_as_it_was(k, m, layout):
    c = case(k, m, layout)
    masks = masks_with_missing(k + m, range(1, m + 1))
    present = spread(c, masks, 4)
    assert any(not present[e][k:].all() and present[e][:k].all() for e in c.live)  # parity-only losses occur
    run_case(c, present, data_only=True)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4)])
def test_present_shards_beyond_the_first_k_are_not_read(k, m, layout):
    c = case(k, m, layout)
    masks = masks_with_missing(k + m, range(1, m))  # at least one spare survivor
    run_case(c, spread(c, masks, 5), extra=True)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_same_bytes_as_single_pattern_reconstruct(layout):
    k, m = 8, 3
    c = case(k, m, layout)
    enc = RS.New(k, m)
    for mask in ([0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], [1, 1, 0, 1, 1, 1, 1, 0, 1, 0, 1], [1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1]):
        present = np.tile(np.array(mask, np.uint8), (len(c.sizes), 1))
        inp, want = c.garble(present)
        t1, t2 = c.upload(inp), c.upload(inp)
        c.plan(enc, t1).reconstruct_mixed(present)
        c.plan(enc, t2).reconstruct(mask)
        torch.cuda.synchronize()
        for a, b in zip(t1, t2):
            assert torch.equal(a, b)
        check_equal(t1, want)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_launch_boundaries_anywhere_in_the_tile_list(layout):
    k, m = 8, 3
    c = case(k, m, layout)
    present = spread(c, masks_with_missing(k + m, [1, 2, 3]), 6)
    T = B.mixed_plan_tile_bytes()
    n_tiles = sum(-(-s // T) for s in c.sizes)
    chunks = -(-n_tiles // 3)
    assert chunks > 10
    B.set_mixed_plan_chunk_tiles(3)
    try:
        s0 = B.mixed_plan_stats()
        run_case(c, present)
        s1 = B.mixed_plan_stats()
    finally:
        B.set_mixed_plan_chunk_tiles(0)
    d = s1["kernel_launches"] - s0["kernel_launches"]
    assert chunks <= d <= 4 * chunks, (d, chunks)


def test_side_stream():
    c = case(8, 3, "stripes")
    present = spread(c, masks_with_missing(11, [1, 2, 3]), 7)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        run_case(c, present, stream=side)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_calls_with_different_patterns_on_one_plan(layout):
    k, m = 4, 2
    c = case(k, m, layout)
    enc = RS.New(k, m)
    masks = masks_with_missing(6, [1, 2])
    t = c.upload()
    plan = c.plan(enc, t)
    for seed in (8, 9):
        present = spread(c, masks, seed)
        inp, want = c.garble(present, seed=seed)
        for x, h in zip(t, inp):
            x.copy_(torch.from_numpy(h))
        plan.reconstruct_mixed(present)
        torch.cuda.synchronize()
        check_equal(t, want)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (12, 4)])
def test_encode_verify_and_mixed_reconstruct_share_one_plan(k, m, layout):
    c = case(k, m, layout)
    enc = RS.New(k, m)
    n = len(c.sizes)
    # parity wrong everywhere: encode rewrites it
    bufs = [x.copy() for x in c.bufs]
    for e in c.live:
        for b, o in c.shards[e][k:]:
            bufs[b][o:o + c.sizes[e]] ^= 0xEE
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    plan.encode()
    torch.cuda.synchronize()
    check_equal(t, c.bufs)
    # corrupted, then declared erased: the repair makes every stripe verify
    present = spread(c, masks_with_missing(k + m, range(1, m + 1)), 10)
    for e in c.live:
        for i in range(k + m):
            if not present[e][i]:
                b, o = c.shards[e][i]
                t[b][o:o + c.sizes[e]] ^= 0x3C
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.verify(flags)
    torch.cuda.synchronize()
    assert flags.cpu().numpy().astype(bool).tolist() == [s > 0 for s in c.sizes]
    plan.reconstruct_mixed(present)
    flags.zero_()
    plan.verify(flags)
    torch.cuda.synchronize()
    assert not flags.cpu().numpy().any()
    check_equal(t, c.bufs)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernel_route_launches_do_not_depend_on_stripes_or_patterns(layout):
    k, m = 8, 3
    c = case(k, m, layout, 60)
    assert len(c.live) >= 60
    rng = np.random.default_rng(11)
    masks = masks_with_missing(k + m, [1, 2, 3])
    present = np.array([masks[int(rng.integers(len(masks)))] for _ in c.sizes], np.uint8)
    s0 = B.mixed_plan_stats()
    run_case(c, present)
    s1 = B.mixed_plan_stats()
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    assert 1 <= s1["kernel_launches"] - s0["kernel_launches"] <= 4  # one chunk


def test_other_route_16_4_is_exact_and_counted():
    k, m = 16, 4
    sizes = [0, 17, 4096, 1985, 0, 100_001, 33, 64, 0]
    c = Case(k, m, "stripes", sizes, 12)
    assert len(c.live) == 6
    rng = np.random.default_rng(13)
    present = np.ones((len(sizes), k + m), np.uint8)
    for q, e in enumerate(c.live):
        present[e][rng.choice(k + m, size=1 + q % 4, replace=False)] = 0
    s0 = B.mixed_plan_stats()
    run_case(c, present)
    s1 = B.mixed_plan_stats()
    assert s1["per_stripe_calls"] - s0["per_stripe_calls"] == 6
    assert s1["kernel_launches"] == s0["kernel_launches"]


def test_nothing_to_rebuild_launches_nothing():
    c = case(4, 2, "stripes")
    s0 = B.mixed_plan_stats()
    run_case(c, np.ones((len(c.sizes), 6), np.uint8))
    present = np.ones((len(c.sizes), 6), np.uint8)
    present[:, 4] = 0  # parity only, with data_only
    run_case(c, present, data_only=True)
    assert B.mixed_plan_stats() == s0


@pytest.mark.parametrize("layout", LAYOUTS)
def test_errors_leave_live_buffers_unchanged(layout):
    k, m = 4, 2
    c = case(k, m, layout)
    enc = RS.New(k, m)
    n = len(c.sizes)
    present = spread(c, masks_with_missing(6, [1, 2]), 14)
    inp, _ = c.garble(present)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    pats, idx = np.unique(present, axis=0, return_inverse=True)
    pats = np.ascontiguousarray(pats, np.uint8)
    idx = np.ascontiguousarray(idx.reshape(-1), np.uint32)

    def call(p, i, n_patterns=None, e=enc):
        return N.lib().hbec_reconstruct_plan_mixed(e.handle, plan._h, p.ctypes.data_as(N._U8P),
                                                   p.shape[0] if n_patterns is None else n_patterns,
                                                   i.ctypes.data_as(U32P), 0, None)

    s0 = B.mixed_plan_stats()
    bad = idx.copy()
    bad[n - 1] = pats.shape[0]  # the last entry is zero-length: checked all the same
    assert c.sizes[n - 1] == 0
    assert call(pats, bad) == N.ERR_INVALID_ARG and "index" in N.last_error()
    few = np.vstack([pats, np.array([[1, 1, 1, 0, 0, 0]], np.uint8)])  # listed, unused
    assert call(few, idx) == N.ERR_TOO_FEW_SHARDS
    assert call(pats, idx, n_patterns=0) == N.ERR_INVALID_ARG
    assert call(pats, idx, e=RS.New(8, 3)) == N.ERR_INVALID_ARG
    with pytest.raises(ValueError):
        plan.reconstruct_mixed(present[:-1])
    with pytest.raises(ValueError):
        plan.reconstruct_mixed(present[:, :-1])
    torch.cuda.synchronize()
    assert B.mixed_plan_stats() == s0
    check_equal(t, inp)
