"""Plans whose entries name every shard (hbec_plan_shards): every plan call on
shards that are not one buffer's slots.

Placement.  Every shard of every entry sits at an offset of its own in one of
three device tensors picked per shard, the (entry, shard) pairs shuffled, so the
shards of an entry are not in index order in memory and the entries are
interleaved; 1..13 sentinel bytes lie around every shard.  Across the shards of
an entry the address residues mod 16 differ, which no stripe can do; one group of
entries has every residue 0 and one has its data aligned and its parity odd.

Codewords come from oracle.coracle, digests from hashlib.  After each call the
WHOLE buffers are compared with what the contract says they hold, slack
included, so a byte written outside a rebuilt shard shows."""
import hashlib
import itertools

import numpy as np
import pytest
import torch

from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import ecutils as E
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

W = 992  # one 64-lane window of the kernels (unaligned_tile.h)
SENT = 0x5A
FAST = [(4, 2), (8, 3), (12, 4)]
IDS = ["4+2", "8+3", "12+4"]


def tile():
    return B.mixed_plan_tile_bytes()


def sizes_for(reps=1):
    T = tile()
    mid = [1, 3, 15, 16, 17, 31, 33, 63, 64, 65, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 17]
    assert T == 4 * W
    return [0] + (mid[:8] + [0] + mid[8:]) * reps + [0]  # zero-length first, interior and last


def patterns(k, m):
    """Every mask with 0..m shards missing, the counts taken in turn (1, 2, .. m, 0):
    entry e takes pattern e mod P, so neighbours differ in how many shards they
    rebuild, and the all-present mask falls on a live entry, not on the empty first one."""
    n = k + m
    by = [[tuple(0 if i in lost else 1 for i in range(n)) for lost in itertools.combinations(range(n), c)]
          for c in range(m + 1)]
    out, at = [], [0] * (m + 1)
    while any(at[c] < len(by[c]) for c in range(m + 1)):
        for c in list(range(1, m + 1)) + [0]:
            if at[c] < len(by[c]):
                out.append(by[c][at[c]])
                at[c] += 1
    return out


def masks_for(k, m, n_entries):
    p = patterns(k, m)
    return np.array([p[e % len(p)] for e in range(n_entries)], np.uint8)


class Lay:
    """Codewords of the given shard lengths, scattered.  at[e][j] = (buffer, offset)."""

    def __init__(self, k, m, sizes, seed):
        self.k, self.m, self.n, self.sizes = k, m, k + m, list(sizes)
        rng = np.random.default_rng(seed)
        self.mat = CO.build_matrix(k, m)
        self.code = []
        for s in self.sizes:
            data = [rng.integers(0, 256, s, dtype=np.uint8) for _ in range(k)]
            par = CO.apply(self.mat[k:], data) if s and m else [np.zeros(s, np.uint8) for _ in range(m)]
            self.code.append(data + [np.asarray(p, np.uint8) for p in par])
        self.live = [e for e, s in enumerate(self.sizes) if s]
        # residue groups by position among the live entries: 0 all aligned, 1 data aligned and parity odd
        self.group = {e: (i % 5 if i % 5 < 2 else 2) for i, e in enumerate(self.live)}
        pairs = [(e, j) for e in self.live for j in range(self.n)]
        order = rng.permutation(len(pairs))
        fill = [0, 0, 0]
        self.at = {e: [None] * self.n for e in range(len(self.sizes))}
        for q in order:
            e, j = pairs[q]
            b = int(rng.integers(0, 3))
            g = self.group[e]
            res = 0 if g == 0 else ((0 if j < k else 1 + 2 * ((j - k) % 7)) if g == 1 else (3 * j + e) % 16)
            off = fill[b] + 1 + int(rng.integers(0, 13))
            off += (res - off) % 16
            self.at[e][j] = (b, off)
            fill[b] = off + self.sizes[e]
        for e in range(len(self.sizes)):  # zero-length entries: pointers that are never followed
            if not self.sizes[e]:
                self.at[e] = [(0, 0)] * self.n
        self.lens = [f + 13 for f in fill]

    def clean(self):
        bufs = [np.full(n, SENT, np.uint8) for n in self.lens]
        for e in self.live:
            for j, (b, o) in enumerate(self.at[e]):
                bufs[b][o:o + self.sizes[e]] = self.code[e][j]
        return bufs

    def put(self, bufs, e, j, data):
        b, o = self.at[e][j]
        bufs[b][o:o + self.sizes[e]] = data

    def get(self, bufs, e, j):
        b, o = self.at[e][j]
        return bufs[b][o:o + self.sizes[e]]

    def upload(self, bufs):
        return [torch.from_numpy(x.copy()).cuda() for x in bufs]

    def plan(self, enc, t):
        assert all(x.data_ptr() % 16 == 0 for x in t)  # an offset's residue is its address's
        return B.StripePlan(enc, shards=[([t[b].data_ptr() + o for b, o in self.at[e]], s)
                                         for e, s in enumerate(self.sizes)])

    def check_placement(self):
        k, n = self.k, self.n
        groups = set(self.group.values())
        assert groups == {0, 1, 2}
        out_of_order = spread = False
        for e in self.live:
            res = [o % 16 for _, o in self.at[e]]
            if self.group[e] == 0:
                assert set(res) == {0}
            elif self.group[e] == 1:
                assert set(res[:k]) == {0} and all(r % 2 == 1 for r in res[k:])
            else:
                assert len(set(res)) >= min(n, 4)  # a stripe has one residue pattern; here they differ
            spread = spread or len({b for b, _ in self.at[e]}) > 1
            keys = [(b, o) for b, o in self.at[e]]
            out_of_order = out_of_order or keys != sorted(keys)
        assert spread and out_of_order
        # interleaved: between two shards of one entry lies a shard of another
        flat = sorted((b, o, e) for e in self.live for b, o in self.at[e])
        runs = sum(1 for x, y in zip(flat, flat[1:]) if x[2] != y[2])
        assert runs > len(self.live) * 2
        # slack of 1..13 bytes (and up to 15 more to reach the residue) around every shard, no overlap
        for x, y in zip(flat, flat[1:]):
            if x[0] == y[0]:
                assert y[1] - (x[1] + self.sizes[x[2]]) >= 1


def dev32(n, fill=0):
    return torch.full((max(1, n),), fill, dtype=torch.int32, device="cuda")


def host32(t, n):
    return t.cpu().numpy().view(np.uint32)[:n].copy()


def check_equal(t, want):
    torch.cuda.synchronize()
    for b, w in enumerate(want):
        got = t[b].cpu().numpy()
        assert np.array_equal(got, w), (b, np.flatnonzero(got != w)[:6])


def garble(lay, bufs, present, rng):
    for e in lay.live:
        for j in range(lay.n):
            if not present[e][j]:
                lay.put(bufs, e, j, rng.integers(0, 256, lay.sizes[e], dtype=np.uint8))


def rebuilt(present_row, k, data_only):
    n_present = int(np.sum(present_row))
    if n_present == len(present_row) or (data_only and all(present_row[:k])):
        return []
    return [j for j, p in enumerate(present_row) if not p and (j < k or not data_only)]


def delta(fn, call):
    a = fn()
    call()
    torch.cuda.synchronize()
    b = fn()
    return {x: b[x] - a[x] for x in a}


# ---- 1. reconstruct_mixed and repair_mixed ----

@pytest.mark.parametrize("data_only", [False, True], ids=["all", "data_only"])
@pytest.mark.parametrize("k,m", FAST, ids=IDS)
def test_reconstruct_mixed_rebuilds_exactly_the_missing_shards(k, m, data_only):
    lay = Lay(k, m, sizes_for(3), seed=10 * k + m)
    lay.check_placement()
    present = masks_for(k, m, len(lay.sizes))
    lost_counts = {int((1 - present[e]).sum()) for e in lay.live}
    assert lost_counts == set(range(m + 1))  # every output count and the all-present case
    assert {s for s in lay.sizes} >= set(sizes_for())
    rng = np.random.default_rng(1)
    start = lay.clean()
    garble(lay, start, present, rng)
    want = [x.copy() for x in start]
    for e in lay.live:
        for j in rebuilt(present[e], k, data_only):
            lay.put(want, e, j, lay.code[e][j])
    enc = RS.New(k, m)
    t = lay.upload(start)
    plan = lay.plan(enc, t)
    assert plan.info() == {"n_tiles": 0, "tile_bytes": 0, "n_fallback": 0, "shard_bytes": sum(lay.sizes)}
    d = delta(B.mixed_plan_stats, lambda: plan.reconstruct_mixed(present, data_only=data_only))
    assert d == {"kernel_launches": 1, "per_stripe_calls": 0}
    check_equal(t, want)


@pytest.mark.parametrize("data_only", [False, True], ids=["all", "data_only"])
@pytest.mark.parametrize("k,m", FAST, ids=IDS)
def test_repair_mixed_rebuilds_and_flags_exactly(k, m, data_only):
    lay = Lay(k, m, sizes_for(3), seed=20 * k + m)
    n = k + m
    present = masks_for(k, m, len(lay.sizes))
    rng = np.random.default_rng(2)
    start = lay.clean()
    garble(lay, start, present, rng)
    want_flags = np.zeros(len(lay.sizes), np.uint32)
    flipped = 0
    for i, e in enumerate(lay.live):
        here = [j for j in range(n) if present[e][j]]
        if len(here) == k:
            want_flags[e] = 2  # nothing to check
        elif i % 2 == 0:  # one flipped bit in one surplus shard: the rebuilt shards do not depend on it
            j = here[k + (i // 2) % (len(here) - k)]
            x = lay.get(start, e, j).copy()
            x[(7 * i) % x.size] ^= 1 << (i % 8)
            lay.put(start, e, j, x)
            want_flags[e] = 1
            flipped += 1
    assert flipped > 5 and 2 in want_flags and 0 in want_flags[lay.live]
    want = [x.copy() for x in start]
    for e in lay.live:
        for j in rebuilt(present[e], k, data_only):
            lay.put(want, e, j, lay.code[e][j])
    enc = RS.New(k, m)
    t = lay.upload(start)
    plan = lay.plan(enc, t)
    flags = dev32(len(lay.sizes))
    d = delta(B.repair_plan_stats, lambda: plan.repair_mixed(present, flags, data_only=data_only))
    assert d == {"kernel_launches": 1, "per_stripe_calls": 0}
    check_equal(t, want)
    assert host32(flags, len(lay.sizes)).tolist() == want_flags.tolist()


# ---- 2. verify and verify_mixed ----

def flip_positions(S):
    T = tile()
    return [0, W - 1, W, T - 1, T, S - 1]


@pytest.mark.parametrize("k,m", FAST, ids=IDS)
def test_verify_flags_exactly_the_flipped_entries(k, m):
    T = tile()
    S = 2 * T + 17
    # entries 1..12 carry one flip each: six positions, in a data shard then in a parity shard
    sizes = [0] + [S if i % 2 == 0 else 33 + i for i in range(26)] + [0]
    lay = Lay(k, m, sizes, seed=30 * k + m)
    big = [e for e in lay.live if lay.sizes[e] == S]
    assert len(big) >= 13
    bufs = lay.clean()
    want = np.zeros(len(sizes), np.uint32)
    for i, pos in enumerate(flip_positions(S) * 2):
        e, j = big[i], ((i * 5) % k if i < 6 else k + i % m)
        x = lay.get(bufs, e, j).copy()
        x[pos] ^= 0x10
        lay.put(bufs, e, j, x)
        want[e] = 1
    enc = RS.New(k, m)
    t = lay.upload(bufs)
    plan = lay.plan(enc, t)
    flags = dev32(len(sizes))
    d = delta(B.verify_mixed_plan_stats, lambda: plan.verify(flags))
    assert d == {"kernel_launches": 1, "per_stripe_calls": 0}  # the mixed Verify kernel, every shard present
    assert host32(flags, len(sizes)).tolist() == want.tolist()  # bit 0 only, never bit 1
    check_equal(t, bufs)  # read-only


@pytest.mark.parametrize("k,m", FAST, ids=IDS)
def test_verify_mixed_flags_flips_and_says_where_nothing_is_checked(k, m):
    n = k + m
    S = 2 * tile() + 17
    sizes = [0] + [S if i % 3 else 17 + i for i in range(120)] + [0]
    lay = Lay(k, m, sizes, seed=40 * k + m)
    present = masks_for(k, m, len(sizes))
    # the flipped entries have a surplus shard to notice it with; the second six a present parity shard
    surplus = [e for e in lay.live if lay.sizes[e] == S and int(present[e].sum()) > k]
    with_par = [e for e in surplus if present[e][k:].any()]
    big = [e for e in surplus if e not in with_par[:6]][:6] + with_par[:6]
    assert len(big) == 12 and len(set(big)) == 12
    bufs = lay.clean()
    garble(lay, bufs, present, np.random.default_rng(3))
    want = np.zeros(len(sizes), np.uint32)
    for e in lay.live:
        if int(present[e].sum()) == k:
            want[e] = 2
    used = 0
    for i, pos in enumerate(flip_positions(S) * 2):
        e = big[i]
        here = [j for j in range(n) if present[e][j]]
        data, par = [j for j in here if j < k], [j for j in here if j >= k]
        j = data[i % len(data)] if i < 6 else par[i % len(par)]
        x = lay.get(bufs, e, j).copy()
        x[pos] ^= 0x01
        lay.put(bufs, e, j, x)
        want[e] |= 1  # a flipped survivor disagrees with the surplus shards, a flipped surplus shard with them
        used += 1
    assert used == 12 and 2 in want
    enc = RS.New(k, m)
    t = lay.upload(bufs)
    plan = lay.plan(enc, t)
    flags = dev32(len(sizes))
    d = delta(B.verify_mixed_plan_stats, lambda: plan.verify_mixed(present, flags))
    assert d == {"kernel_launches": 1, "per_stripe_calls": 0}
    assert host32(flags, len(sizes)).tolist() == want.tolist()
    check_equal(t, bufs)


# ---- 3. encode and reconstruct with one mask ----

@pytest.mark.parametrize("k,m", FAST, ids=IDS)
def test_encode_and_uniform_reconstruct_run_the_mixed_kernel(k, m):
    n = k + m
    lay = Lay(k, m, sizes_for(1), seed=50 * k + m)
    clean = lay.clean()
    start = [x.copy() for x in clean]
    for e in lay.live:
        for j in range(k, n):
            lay.put(start, e, j, np.zeros(lay.sizes[e], np.uint8))
    enc = RS.New(k, m)
    t = lay.upload(start)
    plan = lay.plan(enc, t)
    d = delta(B.mixed_plan_stats, plan.encode)
    assert d == {"kernel_launches": 1, "per_stripe_calls": 0}
    check_equal(t, clean)  # the oracle's parity
    # one mask for all: a data shard and a parity shard lost
    mask = [1] * n
    mask[1] = mask[n - 1] = 0
    for data_only in (True, False):
        start = [x.copy() for x in clean]
        garble(lay, start, [mask] * len(lay.sizes), np.random.default_rng(4))
        want = [x.copy() for x in start]
        for e in lay.live:
            for j in rebuilt(mask, k, data_only):
                lay.put(want, e, j, lay.code[e][j])
        t = lay.upload(start)
        plan = lay.plan(enc, t)
        d = delta(B.mixed_plan_stats, lambda: plan.reconstruct(mask, data_only=data_only))
        assert d == {"kernel_launches": 1, "per_stripe_calls": 0}
        check_equal(t, want)


def test_13_2_takes_the_per_stripe_route():
    k, m, n = 13, 2, 15
    T = tile()
    sizes = [0, 1, 17, W + 1, 0, T - 1, T + 1, 2 * T + 17, 0]
    lay = Lay(k, m, sizes, seed=132)
    assert len(lay.live) == 6
    enc = RS.New(k, m)
    clean = lay.clean()
    start = [x.copy() for x in clean]
    for e in lay.live:
        for j in range(k, n):
            lay.put(start, e, j, np.zeros(lay.sizes[e], np.uint8))
    t = lay.upload(start)
    plan = lay.plan(enc, t)
    assert delta(B.mixed_plan_stats, plan.encode) == {"kernel_launches": 0, "per_stripe_calls": 6}
    check_equal(t, clean)
    # masks per entry: rebuilt, checked and flagged one stripe at a time
    present = masks_for(k, m, len(sizes))
    start = [x.copy() for x in clean]
    garble(lay, start, present, np.random.default_rng(5))
    want_flags = np.zeros(len(sizes), np.uint32)
    for i, e in enumerate(lay.live):
        here = [j for j in range(n) if present[e][j]]
        if len(here) == k:
            want_flags[e] = 2
        elif i % 2 == 0:
            x = lay.get(start, e, here[-1]).copy()
            x[-1] ^= 0x80
            lay.put(start, e, here[-1], x)
            want_flags[e] = 1
    want = [x.copy() for x in start]
    for e in lay.live:
        for j in rebuilt(present[e], k, False):
            lay.put(want, e, j, lay.code[e][j])
    t = lay.upload(start)
    plan = lay.plan(enc, t)
    flags = dev32(len(sizes))
    assert delta(B.repair_plan_stats, lambda: plan.repair_mixed(present, flags)) == {
        "kernel_launches": 0, "per_stripe_calls": 6}
    check_equal(t, want)
    assert host32(flags, len(sizes)).tolist() == want_flags.tolist()
    vflags = dev32(len(sizes))
    t = lay.upload(clean)
    plan = lay.plan(enc, t)
    assert delta(B.verify_mixed_plan_stats, lambda: plan.verify(vflags)) == {
        "kernel_launches": 0, "per_stripe_calls": 6}
    assert host32(vflags, len(sizes)).tolist() == [0] * len(sizes)
    # locate, hash and heal leave this route alone and say so
    where, healed = dev32(len(sizes)), dev32(len(sizes))
    plan.locate_mixed(None, where)
    plan.heal_mixed(None, where, healed)
    torch.cuda.synchronize()
    assert host32(where, len(sizes)).tolist() == [N.LOC_SKIPPED if s else 0 for s in sizes]
    assert host32(healed, len(sizes)).tolist() == [0] * len(sizes)
    check_equal(t, clean)


# ---- 4. the device sweep, and 5. the same bytes in a stripes plan ----

class Stripes:
    """The codewords of a Lay as databuf stripes in one buffer, 1..13 bytes between them."""

    def __init__(self, lay, seed):
        rng = np.random.default_rng(seed)
        self.lay, self.base, at = lay, {}, 0
        for e in lay.live:
            at += 1 + int(rng.integers(0, 13))
            self.base[e] = at
            at += lay.n * lay.sizes[e]
        self.len = at + 13

    def host(self, bufs):
        """The same shard bytes as the Lay's buffers hold."""
        out = np.full(self.len, SENT, np.uint8)
        for e in self.lay.live:
            s = self.lay.sizes[e]
            for j in range(self.lay.n):
                out[self.base[e] + j * s:self.base[e] + (j + 1) * s] = self.lay.get(bufs, e, j)
        return out

    def get(self, buf, e, j):
        s = self.lay.sizes[e]
        return buf[self.base[e] + j * s:self.base[e] + (j + 1) * s]

    def plan(self, enc, t):
        return B.StripePlan(enc, stripes=[(t.data_ptr() + self.base.get(e, 0), s)
                                          for e, s in enumerate(self.lay.sizes)])


def sweep_case(k, m, lost_n, seed):
    """Entries with `lost_n` shards lost; every other one has one corrupt present shard."""
    n = k + m
    lay = Lay(k, m, sizes_for(2), seed=seed)
    rng = np.random.default_rng(seed)
    present = np.ones((len(lay.sizes), n), np.uint8)
    bufs = lay.clean()
    hit = {}
    for i, e in enumerate(lay.live):
        lost = rng.choice(n, size=lost_n, replace=False)
        present[e, lost] = 0
        if i % 2 == 0:
            here = [j for j in range(n) if present[e][j]]
            j = here[i // 2 % len(here)]  # survivors and surplus shards in turn
            x = lay.get(bufs, e, j).copy()
            x[(11 * i) % x.size] ^= 1 << (i % 8)
            lay.put(bufs, e, j, x)
            hit[e] = j
    garble(lay, bufs, present, rng)
    return lay, present, bufs, hit


def run_locate_sweep(plan, present, ne):
    flags, where, healed = dev32(ne), dev32(ne), dev32(ne)
    plan.repair_mixed(present, flags)
    plan.locate_mixed(present, where, flags=flags)
    plan.heal_mixed(present, where, healed)  # one stream, nothing copied back in between
    torch.cuda.synchronize()
    return host32(flags, ne), host32(where, ne), host32(healed, ne)


@pytest.mark.parametrize("k,m,lost_n", [(4, 2, 0), (8, 3, 1)], ids=["4+2-all-present", "8+3-one-lost"])
def test_repair_locate_heal_sweep_and_its_stripes_twin(k, m, lost_n):
    lay, present, bufs, hit = sweep_case(k, m, lost_n, seed=60 * k + m)
    ne = len(lay.sizes)
    assert len(hit) >= 10 and any(j < k for j in hit.values()) and any(j >= k for j in hit.values())
    enc = RS.New(k, m)
    t = lay.upload(bufs)
    plan = lay.plan(enc, t)
    flags, where, healed = run_locate_sweep(plan, present, ne)
    check_equal(t, lay.clean())  # the named shard and the lost ones hold the codeword again
    assert flags.tolist() == [1 if e in hit else 0 for e in range(ne)]
    named = B.locate_decode(k, m, present, where)
    assert [int(named[e]) for e in sorted(hit)] == [hit[e] for e in sorted(hit)]
    # m - lost_n - 1 = 1 surplus shard is left to check after the named one is dropped, and it agrees
    assert healed.tolist() == [N.HEAL_DONE if e in hit else 0 for e in range(ne)]
    # 5. differential: the same bytes as databuf stripes give the same words and the same shards
    st = Stripes(lay, seed=9)
    ts = torch.from_numpy(st.host(bufs)).cuda()
    f2, w2, h2 = run_locate_sweep(st.plan(enc, ts), present, ne)
    assert f2.tolist() == flags.tolist() and w2.tolist() == where.tolist() and h2.tolist() == healed.tolist()
    got_s = ts.cpu().numpy()
    got = [x.cpu().numpy() for x in t]
    for e in lay.live:
        for j in range(k + m):
            assert np.array_equal(st.get(got_s, e, j), lay.get(got, e, j)), (e, j)


def md5s(lay, bufs):
    out = np.zeros((len(lay.sizes), lay.n, 16), np.uint8)
    for e in lay.live:
        for j in range(lay.n):
            out[e, j] = np.frombuffer(hashlib.md5(lay.get(bufs, e, j).tobytes()).digest(), np.uint8)
    return out


def run_hash_sweep(plan, present, expected, ne, n):
    flags, bad, where, healed = dev32(ne), dev32(ne), dev32(ne), dev32(ne)
    dig = torch.full((ne * n * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    exp = torch.from_numpy(expected.reshape(-1).copy()).cuda()
    plan.repair_mixed(present, flags)
    plan.hash_mixed(present, digests=dig, expected=exp, bad=bad, where=where, filter=flags)
    plan.heal_mixed(present, where, healed)
    torch.cuda.synchronize()
    return host32(flags, ne), host32(bad, ne), host32(where, ne), host32(healed, ne), dig.cpu().numpy()


@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)], ids=["4+2", "8+3"])
def test_hash_sweep_with_one_surplus_shard_and_its_stripes_twin(k, m):
    """k + 1 present: Verify can say an entry is inconsistent, only the stored hashes say which shard."""
    n = k + m
    lay, present, bufs, hit = sweep_case(k, m, m - 1, seed=70 * k + m)
    ne = len(lay.sizes)
    expected = md5s(lay, lay.clean())
    enc = RS.New(k, m)
    t = lay.upload(bufs)
    flags, bad, where, healed, dig = run_hash_sweep(lay.plan(enc, t), present, expected, ne, n)
    check_equal(t, lay.clean())
    assert flags.tolist() == [1 if e in hit else 0 for e in range(ne)]
    assert bad.tolist() == [1 << hit[e] if e in hit else 0 for e in range(ne)]
    named = B.locate_decode(k, m, present, where)
    assert [int(named[e]) for e in sorted(hit)] == [hit[e] for e in sorted(hit)]
    assert healed.tolist() == [N.HEAL_DONE | 2 if e in hit else 0 for e in range(ne)]  # k left: nothing to check
    # the digests written are those of the flagged entries' present shards, as they were read
    seen = md5s(lay, bufs)
    dig = dig.reshape(ne, n, 16)
    for e in range(ne):
        for j in range(n):
            want = seen[e, j] if e in hit and present[e][j] else np.full(16, 0xA5, np.uint8)
            assert np.array_equal(dig[e, j], want), (e, j)
    st = Stripes(lay, seed=10)
    ts = torch.from_numpy(st.host(bufs)).cuda()
    f2, b2, w2, h2, d2 = run_hash_sweep(st.plan(enc, ts), present, expected, ne, n)
    assert (f2.tolist(), b2.tolist(), w2.tolist(), h2.tolist()) == (flags.tolist(), bad.tolist(), where.tolist(),
                                                                   healed.tolist())
    assert np.array_equal(d2.reshape(ne, n, 16), dig)
    got_s, got = ts.cpu().numpy(), [x.cpu().numpy() for x in t]
    for e in lay.live:
        for j in range(n):
            assert np.array_equal(st.get(got_s, e, j), lay.get(got, e, j)), (e, j)


# ---- 6. digests ----

@pytest.mark.parametrize("k,m", FAST + [(13, 2)], ids=IDS + ["13+2"])
def test_hash_mixed_digests_match_hashlib(k, m):
    n = k + m
    lay = Lay(k, m, sizes_for(1) + [5 * 64 * 4 + 3, 64, 128, 55, 56, 57], seed=80 * k + m)
    bufs = lay.clean()
    ne = len(lay.sizes)
    enc = RS.New(k, m)
    t = lay.upload(bufs)
    plan = lay.plan(enc, t)
    dig = torch.full((ne * n * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    d = delta(B.hash_plan_stats, lambda: plan.hash_mixed(None, digests=dig))
    assert d == {"kernel_launches": 1, "chains": len(lay.live) * n}
    want = md5s(lay, bufs)
    for e in range(ne):
        if not lay.sizes[e]:
            want[e] = 0xA5
    assert np.array_equal(dig.cpu().numpy().reshape(ne, n, 16), want)
    check_equal(t, bufs)


# ---- 7. the stabilisation layout ----

@pytest.mark.parametrize("k,m,chunk,L", [(4, 2, 1000, 3 * 4 * 1000 + 2777), (8, 3, 512, 2 * 8 * 512 + 13),
                                         (4, 2, 4096, 2 * 4 * 4096)],
                         ids=["4+2", "8+3", "4+2-whole-stripes"])
def test_stabilisation_layout_encodes_into_parity_files(k, m, chunk, L):
    """Data shards read out of the contiguous object (zero-padded to a multiple of k, the
    caller's pad bytes), parity written into m parity files at pfile_r + t chunk."""
    n = k + m
    obj = O.object_bytes(5, L).tobytes()
    files = O.ec_split(k, m, obj, chunk)
    hashes = O.ec_split_hashes(k, m, obj, chunk)
    nt = E.ec_stripe_count(L, k, chunk)
    S = [E.ec_stripe_shard_length(L, k, chunk, t) for t in range(nt)]
    assert sum(S) == len(files[0]) and nt == (L + k * chunk - 1) // (k * chunk)
    lead = 3  # the object at an odd address
    padded = (nt - 1) * k * chunk + k * S[-1]
    assert L <= padded < L + k
    hobj = np.full(lead + padded + 7, SENT, np.uint8)
    hobj[lead:lead + L] = np.frombuffer(obj, np.uint8)
    hobj[lead + L:lead + padded] = 0
    hpar = [np.full(5 + r + len(files[0]) + 7, SENT, np.uint8) for r in range(m)]
    tobj = torch.from_numpy(hobj.copy()).cuda()
    tpar = [torch.from_numpy(p.copy()).cuda() for p in hpar]
    shards = []
    for t in range(nt):
        row = [tobj.data_ptr() + lead + t * k * chunk + j * S[t] for j in range(k)]
        row += [tpar[r].data_ptr() + 5 + r + t * chunk for r in range(m)]
        shards.append((row, S[t]))
    enc = RS.New(k, m)
    plan = B.StripePlan(enc, shards=shards)
    plan.encode()
    dig = torch.full((n * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.hash_files(np.array([0, nt], np.uint32), None, digests=dig)
    torch.cuda.synchronize()
    assert np.array_equal(tobj.cpu().numpy(), hobj)  # the object is only read
    for r in range(m):
        want = hpar[r].copy()
        want[5 + r:5 + r + len(files[0])] = np.frombuffer(files[k + r], np.uint8)
        assert np.array_equal(tpar[r].cpu().numpy(), want), r
    got = dig.cpu().numpy().reshape(n, 16)
    assert [got[j].tobytes().hex() for j in range(n)] == hashes


# ---- hash_files over scattered entries ----

@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)], ids=["4+2", "8+3"])
def test_hash_files_walks_scattered_entries_and_skips_empty_ones(k, m):
    """A shard file is shard j of each of an object's entries back to back; here every
    piece lies somewhere else, and zero-length entries (which have no address row) sit
    first, between and last in the objects."""
    n = k + m
    T = tile()
    sizes = [0, 70, 0, 130, 64, 0, 5, 0, T + 1, 63, 1, 0, 0, 2 * T + 17, 33]
    starts = np.array([0, 3, 6, 8, 11, 13, 15], np.uint32)
    lay = Lay(k, m, sizes, seed=90 * k + m)
    bufs = lay.clean()
    enc = RS.New(k, m)
    t = lay.upload(bufs)
    plan = lay.plan(enc, t)
    no = len(starts) - 1
    dig = torch.full((no * n * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.hash_files(starts, None, digests=dig)
    torch.cuda.synchronize()
    got = dig.cpu().numpy().reshape(no, n, 16)
    for g in range(no):
        ents = [e for e in range(starts[g], starts[g + 1]) if sizes[e]]
        for j in range(n):
            body = b"".join(lay.get(bufs, e, j).tobytes() for e in ents)
            want = hashlib.md5(body).digest() if ents else bytes([0xA5] * 16)
            assert got[g, j].tobytes() == want, (g, j)
    assert not [e for e in range(starts[4], starts[5]) if sizes[e]]  # an object of empty entries only
    check_equal(t, bufs)
