"""Byte-exact sweep of gf_apply_mixed<K, R> (csrc/mixed.hip, behind
hbec_reconstruct_batch_mixed): all 32 compiled instances, K = 1..8 x R = 1..4,
at every shard length of up to two tiles and a ragged third, on looping
launches of both walks, and across launch boundaries.

Every case is k + 4 (RS.New(k, 4)), so one call launches the four R instances
of that K.  Only shapes the kernel takes: 16-B-aligned bases and pitch,
S % 16 == 0; every call asserts from hbec_mixed_stats that the run route was
not taken, and from hbec_mixed_walk_stats how the launches walked.

Data: one pool of NP oracle codewords per k at the longest length
(coracle build_matrix / apply), uploaded once.  The batch of length s is packed
on the device from the first s bytes of every pool shard - a prefix of a
codeword is a codeword, asserted on the host against coracle.apply at two
lengths.  Layout as tests/test_gpu_mixed.py Batch: shards back to back, 48
slack bytes after each object, 64 after the last, slack bytes random, a clone
kept.  Missing shards are overwritten with GONE; after the call the WHOLE
buffer must equal the clone: the rebuilt bytes are the oracle's, and nothing
else was written, not one byte past a shard.  No tolerance, no sampling of
lengths.

1. every S = 16, 32, .. 2 T + 64 (T = batch.mixed_tile_bytes(k): 4096, 2048,
   then 1024): with stripes_u(1) = 4 and stripes_u(2) = 2 the u > 0 iterations
   of load_mixed_tile / store_mixed_tile_ (the u * 1024 offsets, the clamp to
   valid - 16, off < live over several windows) run at every fill.  Masks:
   every mask with <= 2 missing, and masks with 3 and 4 missing in which every
   shard is an output and a survivor at every slot it can take (asserted).
2. the seam lengths on launches with more tiles than resident waves, so the
   pipelined loop (prefetch, resolve two tiles ahead, the table reload when
   the record changes) runs: many patterns shuffled - a contiguous run per
   wave, records changing inside runs (asserted from the entry counts) - and
   one mask per output count over >= 16 x CUs tiles per slice - grid-stride.
   hbec.cpp mixed_contiguous picks the walks as predicted here:
   waves x records x 4 > tiles.
3. launches split at whole objects in the middle of the list
   (hbec_set_mixed_chunk_tiles with an odd, small count).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO

from test_gpu_mixed import GONE, masks_upto

pytestmark = pytest.mark.gpu

M = 4
NP = 64      # codewords in a pool; object o of a batch holds codeword o % NP
SLACK = 48   # bytes after each object
TAIL = 64    # bytes after the last object
WPB = 4      # kernels.h kBlockThreads / 64: waves per block, one block per CU
KS = list(range(1, 9))
NOISE = 512 << 20  # random bytes kept on the device; every batch starts as a prefix of them


def tile(k):
    return B.mixed_tile_bytes(k)


def smax(k):
    return 2 * tile(k) + 64


@functools.lru_cache(maxsize=None)
def pool(k):
    """[NP, k + M, smax] oracle codewords on the device."""
    S, T = smax(k), tile(k)
    data = np.random.default_rng(9000 + k).integers(0, 256, (NP, k, S), dtype=np.uint8)
    rows = CO.build_matrix(k, M)[k:]
    par = CO.apply(rows, [data[:, j, :].reshape(-1) for j in range(k)])
    cw = np.concatenate([data, np.stack([p.reshape(NP, S) for p in par], axis=1)], axis=1)
    for s in (16, T + 16):  # a prefix of a codeword is a codeword
        pre = CO.apply(rows, [np.ascontiguousarray(data[:, j, :s]).reshape(-1) for j in range(k)])
        for r in range(M):
            assert np.array_equal(pre[r].reshape(NP, s), cw[:, k + r, :s])
    return torch.from_numpy(np.ascontiguousarray(cw)).cuda()


@functools.lru_cache(maxsize=None)
def noise(n):
    """n random bytes on the device (the slack of every batch is a prefix of these)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


class Packed:
    """n objects of k + M shards of s bytes, packed on the device from the pool."""

    def __init__(self, k, n, s, fill):
        L = k + M
        self.k, self.n, self.s = k, n, s
        self.pitch = L * s + SLACK
        total = n * self.pitch + TAIL
        assert fill.numel() >= total
        self.buf = fill[:total].clone()
        assert self.buf.data_ptr() % 16 == 0 and self.pitch % 16 == 0 and s % 16 == 0
        idx = torch.arange(n, device="cuda") % NP
        self.shards().copy_(pool(k)[:, :, :s][idx])
        self.keep = self.buf.clone()
        self.views = [(self.buf.data_ptr() + i * s, self.pitch) for i in range(L)]

    def shards(self):
        L = self.k + M
        return self.buf[:self.n * self.pitch].view(self.n, self.pitch)[:, :L * self.s].view(self.n, L, self.s)

    def erase(self, gone):
        self.shards()[gone] = GONE

    def first_difference(self, present):
        bad = torch.nonzero(self.buf != self.keep).flatten()
        if bad.numel() == 0:
            return None
        at = int(bad[0])
        o, r = divmod(at, self.pitch)
        where = (f"shard {r // self.s} position {r % self.s}" if o < self.n and r < (self.k + M) * self.s
                 else f"slack byte {r}")
        mask = present[o].tolist() if o < self.n else None
        return (f"{int(bad.numel())} bytes differ; first: object {o} {where}, mask {mask}, "
                f"got {int(self.buf[at])} want {int(self.keep[at])}")


def run(enc, b, present):
    """One call; the counter changes.  Asserts the mixed route and that every
    launch was counted under one walk."""
    s0, w0 = B.mixed_stats(), B.mixed_walk_stats()
    B.reconstruct_views_mixed(enc, b.views, present, b.n, b.s)
    torch.cuda.synchronize()
    s1, w1 = B.mixed_stats(), B.mixed_walk_stats()
    d = {f: s1[f] - s0[f] for f in s0}
    d.update({f: w1[f] - w0[f] for f in w0})
    assert d["runs"] == 0 and d["mixed"] >= 1, d
    assert d["contiguous"] + d["grid_stride"] == d["mixed"] and d["looping"] <= d["mixed"], d
    return d


def check(enc, b, present, what):
    gone = torch.from_numpy(present == 0).cuda()
    b.erase(gone)
    d = run(enc, b, present)
    if not torch.equal(b.buf, b.keep):
        pytest.fail(f"{b.k}+{M} S={b.s} n={b.n} {what} {d}: {b.first_difference(present)}")
    return d


# ---- masks -------------------------------------------------------------------

def mask_of(n, missing):
    return tuple(0 if i in missing else 1 for i in range(n))


def slots_possible(k, e):
    """(shard i, survivor slot j) pairs that occur under some mask with e
    missing: i - j shards missing before i, the other e - (i - j) after it."""
    n = k + M
    return {(i, j) for i in range(n) for j in range(k) if 0 <= i - j <= e and e - (i - j) <= n - 1 - i}


def sampled_masks(k, seed):
    """Masks with 3 and 4 missing: per count, every shard as an output and at
    every survivor slot it can take."""
    n = k + M
    rng = np.random.default_rng(seed)
    out = set()
    for e in (3, 4):
        for i in range(n):
            others = rng.choice([x for x in range(n) if x != i], e - 1, replace=False)
            out.add(mask_of(n, {i, *others.tolist()}))
        for i, j in sorted(slots_possible(k, e)):
            d = i - j
            before = rng.choice(i, d, replace=False).tolist() if d else []
            after = rng.choice(np.arange(i + 1, n), e - d, replace=False).tolist() if e - d else []
            out.add(mask_of(n, set(before) | set(after)))
    return np.array(sorted(out), dtype=np.uint8)


def survivor_slots(masks, k):
    return {(int(i), j) for row in masks for j, i in enumerate(np.flatnonzero(row)[:k])}


def outputs(masks):
    return {int(i) for row in masks for i in np.flatnonzero(row == 0)}


@functools.lru_cache(maxsize=None)
def sweep_masks(k):
    """The object masks of one A1-sized call, shuffled: a few hundred objects."""
    n = k + M
    few = masks_upto(k, M, 2)
    assert len(few) == 1 + n + n * (n - 1) // 2
    many = sampled_masks(k, 40 + k)
    for e in (3, 4):
        sub = many[many.sum(axis=1) == n - e]
        assert outputs(sub) == set(range(n)), (k, e)
        assert survivor_slots(sub, k) == slots_possible(k, e), (k, e)
    masks = np.concatenate([few, many])
    present = np.concatenate([masks] * -(-256 // len(masks)) + [np.ones((8, n), np.uint8)])
    np.random.default_rng(k).shuffle(present, axis=0)
    lost = n - present.sum(axis=1)
    assert set(lost.tolist()) == {0, 1, 2, 3, 4}  # untouched objects and all four R instances
    assert (lost == 0).sum() >= 9 and 256 <= len(present) < 600
    return present


def exactly(n, e):
    return np.array([mask_of(n, set(c)) for c in itertools.combinations(range(n), e)], dtype=np.uint8)


# ---- 1. every length ----------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_every_length(k):
    T = tile(k)
    lengths = list(range(16, smax(k) + 1, 16))
    assert len(lengths) == {1: 516, 2: 260}.get(k, 132)
    enc = RS.New(k, M)
    base = sweep_masks(k)
    n = len(base)
    fill = noise(NOISE)
    launches = 0
    for s in lengths:
        present = np.roll(base, s // 16, axis=0)  # the masks move over the pool's codewords
        b = Packed(k, n, s, fill[s:])
        d = check(enc, b, present, "every-length")
        assert d["mixed"] == 4, d  # one launch per output count
        launches += d["mixed"]
    print(f"SWEEP mixed-every-length {k}+{M} S=16..{smax(k)} step 16 ({len(lengths)} lengths) T={T} objects={n} "
          f"masks={len(np.unique(base, axis=0))} resident={2 * (n * ((k + M) * smax(k) + SLACK) + TAIL)} "
          f"launches={launches}")


# ---- 2. looping launches, both walks --------------------------------------------

def seams(k):
    T = tile(k)
    return [16, 32, T - 16, T, T + 16, 2 * T - 16, 2 * T, 2 * T + 16, 2 * T + 64]


def runs_cross_records(present, k, tpo, iters):
    """Per output count: does a record boundary of the sorted entry list fall
    inside a wave's contiguous run of `iters` tiles?  Records are in pattern
    order (np.unique's, hbec.cpp mixed_fast)."""
    n = k + M
    pats, inv = np.unique(present, axis=0, return_inverse=True)
    uses = np.bincount(inv.reshape(-1), minlength=len(pats))
    ok = []
    for r in range(1, M + 1):
        sel = uses[(n - pats.sum(axis=1)) == r]
        assert len(sel) >= 2
        bounds = np.cumsum(sel * tpo)[:-1]
        ok.append(bool((bounds % iters != 0).any()))
    return all(ok)


def many_patterns(k, tpo, waves, seed):
    """Shuffled objects over many masks whose four slices each have more tiles
    than `waves`; returns (present, iters per launch)."""
    n = k + M
    rng = np.random.default_rng(seed)
    for iters in (3, 4, 5):
        ents = (iters - 1) * waves // tpo + 3  # tiles in ((iters - 1) waves, iters waves]
        assert (iters - 1) * waves < ents * tpo <= iters * waves
        rows = []
        for r in range(1, M + 1):
            masks = exactly(n, r)
            if len(masks) > 64:
                masks = masks[np.sort(rng.choice(len(masks), 64, replace=False))]
            rows.append(masks[np.arange(ents) % len(masks)])
        present = np.concatenate(rows)
        rng.shuffle(present, axis=0)
        if runs_cross_records(present, k, tpo, iters):
            return present, iters
    raise AssertionError("no batch size whose runs cross a record")


def one_pattern_per_count(k, tpo, cus, seed):
    """One mask per output count, each slice of at least 16 x CUs tiles."""
    n = k + M
    rng = np.random.default_rng(seed)
    ents = -(-16 * cus // tpo) + 3
    rows = []
    for r in range(1, M + 1):
        masks = exactly(n, r)
        rows.append(np.repeat(masks[rng.integers(len(masks))][None, :], ents, axis=0))
    present = np.concatenate(rows)
    rng.shuffle(present, axis=0)
    return present, ents * tpo


@pytest.mark.parametrize("k", KS)
def test_looping_launches_on_both_walks(k):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = WPB * cus
    T = tile(k)
    enc = RS.New(k, M)
    fill = noise(NOISE)
    walks = {"contiguous": 0, "grid_stride": 0}
    log = []
    for s in seams(k):
        tpo = -(-s // T)
        # many patterns: waves x records x 4 > tiles, a contiguous run per wave
        present, iters = many_patterns(k, tpo, waves, seed=1000 * k + s)
        b = Packed(k, len(present), s, fill)
        d = check(enc, b, present, "looping-contiguous")
        assert d == {"mixed": 4, "runs": 0, "contiguous": 4, "grid_stride": 0, "looping": 4}, (s, d)
        walks["contiguous"] += d["contiguous"]
        log.append((s, b.n, iters))
        del b
        # one record per slice over >= 4 tiles per wave: grid-stride
        present, tiles = one_pattern_per_count(k, tpo, cus, seed=2000 * k + s)
        assert tiles >= 16 * cus and tiles > waves
        b = Packed(k, len(present), s, fill)
        d = check(enc, b, present, "looping-grid-stride")
        assert d == {"mixed": 4, "runs": 0, "contiguous": 0, "grid_stride": 4, "looping": 4}, (s, d)
        walks["grid_stride"] += d["grid_stride"]
        log.append((s, b.n, -(-tiles // waves)))
        del b
    assert walks == {"contiguous": 36, "grid_stride": 36}  # every R of this K looped on both walks
    print(f"SWEEP mixed-looping {k}+{M} CUs={cus} (S, objects, tiles per wave) contiguous / grid-stride: {log} "
          f"resident<={2 * max(n * ((k + M) * s + SLACK) + TAIL for s, n, _ in log)}")


# ---- 3. launch boundaries ---------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_launch_boundaries_inside_the_list(k):
    T = tile(k)
    enc = RS.New(k, M)
    present = sweep_masks(k)
    n = len(present)
    lost = (k + M) - present.sum(axis=1)
    fill = noise(NOISE)
    log = []
    for s, chunk in ((32, 5), (T + 16, 7), (2 * T + 64, 7)):
        tpo = -(-s // T)
        per_launch = max(1, chunk // tpo)  # whole objects per launch
        want = sum(-(-int((lost == r).sum()) // per_launch) for r in range(1, M + 1))
        b = Packed(k, n, s, fill)
        try:
            B.set_mixed_chunk_tiles(chunk)
            d = check(enc, b, present, f"chunk-{chunk}")
        finally:
            B.set_mixed_chunk_tiles(0)
        assert d["mixed"] == want and want > 40, (s, d, want)
        log.append((s, chunk, per_launch, d["mixed"]))
    print(f"SWEEP mixed-launch-boundaries {k}+{M} objects={n} (S, chunk tiles, objects per launch, launches): {log}")
