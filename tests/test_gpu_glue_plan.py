"""hbec_glue_plan_mixed on the device: the object bytes of every entry of a plan
from its shards, degraded or not, in one call, on all four kinds of plan.

Nothing expected comes from the product.  Entry e's object is
oracle.object_bytes, its codeword coracle's, and what the call must write is the
object's own bytes, which must also be oracle.ec_glue of the surviving shards.

The common discipline (class Glue, shared with the files and sweep tests): whole
buffers are compared, the destinations with 0xC3 sentinels around and between
them; every shard buffer must come back bit-identical to its input; the shards
a mask calls missing hold random bytes, and so do the present shards beyond the
entry's first k present, which must never be read."""
import itertools

import numpy as np
import pytest
import torch

import test_glue_host as GH
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SENT = 0xC3
W = 992
KINDS = ["stripes", "objects", "shards", "files"]
SHAPES = [(4, 2), (8, 3), (12, 4)]


def tile():
    return B.glue_plan_tile_bytes()


def sizes_for():
    T = tile()
    assert T == 3968 == 4 * W
    rng = np.random.default_rng(20240611)
    rand = [int(s) + (1 if s % 16 == 0 else 0) for s in rng.integers(1, 40001, 20)]
    mid = [1, 3, 15, 16, 17, 31, 33, 63, 64, 65, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 17]
    return [0] + mid[:8] + [0] + mid[8:] + rand + [0]  # zero-length first, interior and last


def masks_by_kind(k, m):
    """Every mask with 0..m shards missing, arranged so that the healthy mask, the
    masks that lost data alone, parity alone and both come up in turn."""
    n = k + m
    cats = {"healthy": [], "data": [], "parity": [], "mixed": []}
    per_count = [list(itertools.combinations(range(n), c)) for c in range(m + 1)]
    for pos in range(max(len(p) for p in per_count)):
        for c in range(m + 1):
            if pos < len(per_count[c]):
                lost = per_count[c][pos]
                d, p = any(i < k for i in lost), any(i >= k for i in lost)
                cats["mixed" if d and p else "data" if d else "parity" if p else "healthy"].append(
                    tuple(0 if i in lost else 1 for i in range(n)))
    out = []
    order = [cats["data"], cats["healthy"], cats["mixed"], cats["parity"]]
    for pos in range(max(len(c) for c in order)):
        out += [c[pos] for c in order if pos < len(c)]
    assert len(out) == len(set(out)) == sum(len(p) for p in per_count)
    return out


def masks_for(k, m, n_entries):
    p = masks_by_kind(k, m)
    return np.array([p[e % len(p)] for e in range(n_entries)], np.uint8)


def first_k(mask, k):
    return [j for j, x in enumerate(mask) if x][:k]


class Glue:
    """Entries of the given shard lengths and masks on a plan of one kind, and the
    common discipline of every glue test.  at[e][j] = (buffer, offset) of shard j."""

    def __init__(self, k, m, kind, sizes, masks, seed):
        self.k, self.m, self.n, self.kind = k, m, k + m, kind
        if kind == "files":  # an object of no bytes has no entry
            keep = [e for e, s in enumerate(sizes) if s]
            sizes, masks = [sizes[e] for e in keep], np.asarray(masks)[keep]
        self.sizes, self.masks = [int(s) for s in sizes], np.asarray(masks, np.uint8)
        self.live = [e for e, s in enumerate(self.sizes) if s]
        rng = np.random.default_rng(seed)
        mat = CO.build_matrix(k, m)
        self.objs, self.stored = [], []
        for e, s in enumerate(self.sizes):
            obj = np.asarray(O.object_bytes(seed * 100003 + e, k * s), np.uint8)
            data = [obj[j * s:(j + 1) * s] for j in range(k)]
            par = [np.asarray(p, np.uint8) for p in CO.apply(mat[k:], data)] if s and m else \
                [np.zeros(s, np.uint8) for _ in range(m)]
            code = data + par
            if s:  # the reference's ecGlue of the surviving shards is the object
                files = [code[j].tobytes() if self.masks[e][j] else None for j in range(self.n)]
                assert O.ec_glue(k, m, files, s, k * s) == obj.tobytes(), e
            read = first_k(self.masks[e], k)
            self.objs.append(obj)
            self.stored.append([code[j] if j in read else rng.integers(0, 256, s, dtype=np.uint8)
                                for j in range(self.n)])
        self._place(rng)

    def _place(self, rng):
        k, n = self.k, self.n
        self.at = {e: [(0, 0)] * n for e in range(len(self.sizes))}  # zero-length: never followed
        if self.kind == "stripes":
            at = 0
            for i, e in enumerate(self.live):
                base = at + 1 + (5 * i) % 16
                self.at[e] = [(0, base + j * self.sizes[e]) for j in range(n)]
                at = base + n * self.sizes[e]
            self.lens = [at + 9]
        elif self.kind == "objects":
            a = b = 0
            for i, e in enumerate(self.live):
                da, pb = a + 1 + (3 * i) % 16, b + 1 + (7 * i) % 16
                self.at[e] = [(0, da + j * self.sizes[e]) for j in range(k)] + \
                    [(1, pb + j * self.sizes[e]) for j in range(self.m)]
                a, b = da + k * self.sizes[e], pb + self.m * self.sizes[e]
            self.lens = [a + 9, b + 9]
        else:  # every shard on its own, over three buffers, residues differing within an entry
            fill = [0, 0, 0]
            pairs = [(e, j) for e in self.live for j in range(n)]
            for q in rng.permutation(len(pairs)):
                e, j = pairs[q]
                b = int(rng.integers(0, 3))
                off = fill[b] + 1 + int(rng.integers(0, 13))
                off += ((3 * j + e) % 16 - off) % 16
                self.at[e][j] = (b, off)
                fill[b] = off + self.sizes[e]
            self.lens = [f + 13 for f in fill]

    def shard_bufs(self):
        bufs = [np.full(x, SENT, np.uint8) for x in self.lens]
        for e in self.live:
            for j, (b, o) in enumerate(self.at[e]):
                bufs[b][o:o + self.sizes[e]] = self.stored[e][j]
        return bufs

    def plan(self, enc, t):
        assert all(x.data_ptr() % 16 == 0 for x in t)  # an offset's residue is its address's
        addr = {e: [t[b].data_ptr() + o for b, o in self.at[e]] for e in range(len(self.sizes))}
        if self.kind == "stripes":
            return B.StripePlan(enc, stripes=[(addr[e][0], s) for e, s in enumerate(self.sizes)])
        if self.kind == "objects":
            return B.StripePlan(enc, objects=[(addr[e][0], addr[e][self.k] if self.m else 0, s)
                                              for e, s in enumerate(self.sizes)])
        if self.kind == "shards":
            return B.StripePlan(enc, shards=[(addr[e], s) for e, s in enumerate(self.sizes)])
        plan = B.StripePlan(enc, files=[(addr[e], self.k * s) for e, s in enumerate(self.sizes)],
                            chunk_size=max(self.sizes))
        assert plan.object_start.tolist() == list(range(len(self.sizes) + 1))  # one stripe each
        return plan

    def dst_layout(self, lens, residues):
        """Destinations back to back in one arena, 1..16 sentinel bytes between two."""
        offs, at = [], 0
        for ln, r in zip(lens, residues):
            o = at + 1
            o += (r - o) % 16
            offs.append(o)
            at = o + ln
        return offs, at + 11

    def expect(self, lens, offs, total):
        want = np.full(total, SENT, np.uint8)
        for e, (ln, o) in enumerate(zip(lens, offs)):
            want[o:o + ln] = self.objs[e][:ln]
        return want

    def run(self, enc, lens, residues, call=None):
        """One call on fresh buffers; asserts the discipline and returns the arena's bytes."""
        offs, total = self.dst_layout(lens, residues)
        host = self.shard_bufs()
        t = [torch.from_numpy(x.copy()).cuda() for x in host]
        dst = torch.full((total,), SENT, dtype=torch.uint8, device="cuda")
        plan = self.plan(enc, t)
        dsts = [dst.data_ptr() + o for o in offs]
        torch.cuda.synchronize()  # the fills are done before a call on any stream
        if call is None:
            plan.glue_mixed(self.masks, dsts, lens)
        else:
            call(plan, dsts)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        want = self.expect(lens, offs, total)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (self.kind, bad[:6], [(e, o, ln) for e, (o, ln) in enumerate(zip(offs, lens))
                                                    if o - 16 <= bad[0] <= o + ln + 16])
        for b, (x, h) in enumerate(zip(t, host)):
            assert np.array_equal(x.cpu().numpy(), h), ("a shard buffer was written", self.kind, b)
        return got


def residues_for(sizes):
    """0..15 in turn, and residue 0 on a length that is a multiple of 16 and on one that is not."""
    live = [e for e, s in enumerate(sizes) if s]
    res = [(i + 1) % 16 for i in range(len(sizes))]
    res[next(e for e in live if sizes[e] % 16 == 0)] = 0
    res[next(e for e in live if sizes[e] % 16 and sizes[e] > 16)] = 0
    assert set(res) == set(range(16))
    return res


def trunc_lens(k, sizes):
    """ecGlue's cut: k S - pad, pad in 0..k-1 in turn (positive for every S >= 1)."""
    out, i = [], 0
    for s in sizes:
        out.append(k * s - (i % k) if s else 0)
        i += 1 if s else 0
    assert all(ln > 0 for ln, s in zip(out, sizes) if s)
    return out


def prefix_lens(k, sizes):
    out, i = [], 0
    for s in sizes:
        out.append([0, 1, s - 1, s, s + 1, (k - 1) * s + 1][i % 6] if s else 0)
        i += 1 if s else 0
    return out


_CACHE = {}


def glue_of(k, m, kind):
    key = (k, m, kind)
    if key not in _CACHE:
        sizes = sizes_for()
        _CACHE[key] = Glue(k, m, kind, sizes, masks_for(k, m, len(sizes)), seed=17 * k + m)
    return _CACHE[key]


def test_masks_cover_every_kind_of_loss():
    for k, m in SHAPES:
        n_live = len([s for s in sizes_for() if s])
        masks = masks_for(k, m, len(sizes_for()))
        kinds = set()
        for e, s in enumerate(sizes_for()):
            if s:
                d, p = (masks[e][:k] == 0).any(), (masks[e][k:] == 0).any()
                kinds.add((bool(d), bool(p)))
                assert masks[e].sum() >= k
        assert kinds == {(False, False), (True, False), (False, True), (True, True)}, (k, m)
        assert n_live >= 37


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,m", SHAPES, ids=["4+2", "8+3", "12+4"])
def test_glue_every_kind_of_plan(k, m, kind):
    enc = RS.New(k, m)
    g = glue_of(k, m, kind)
    res = residues_for(g.sizes)
    s0 = B.glue_plan_stats()
    g.run(enc, trunc_lens(k, g.sizes), res)
    s1 = B.glue_plan_stats()
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1  # whatever the entries, masks or lengths
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    # prefixes: a ranged GET that ends inside the stripe, at other residues
    g.run(enc, prefix_lens(k, g.sizes), res[5:] + res[:5])
    s2 = B.glue_plan_stats()
    assert s2["kernel_launches"] - s1["kernel_launches"] == 1
    assert s2["per_stripe_calls"] == s0["per_stripe_calls"]


@pytest.mark.parametrize("kind", ["stripes", "shards"])
def test_launches_cut_by_the_hook_write_the_same_bytes(kind):
    k, m = 4, 2
    enc = RS.New(k, m)
    g = glue_of(k, m, kind)
    res, lens = residues_for(g.sizes), trunc_lens(k, g.sizes)
    one = g.run(enc, lens, res)
    n_tiles = sum((s + tile() - 1) // tile() for s in g.sizes)
    s0 = B.glue_plan_stats()
    B.set_glue_plan_chunk_tiles(3)
    try:
        cut = g.run(enc, lens, res)
    finally:
        B.set_glue_plan_chunk_tiles(0)
    assert B.glue_plan_stats()["kernel_launches"] - s0["kernel_launches"] == (n_tiles + 2) // 3 > 10
    assert np.array_equal(one, cut)


def test_other_streams_write_the_same_bytes():
    k, m = 8, 3
    enc = RS.New(k, m)
    g = glue_of(k, m, "objects")
    res, lens = residues_for(g.sizes), trunc_lens(k, g.sizes)
    one = g.run(enc, lens, res)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def on_stream(plan, dsts):
        plan.glue_mixed(g.masks, dsts, lens, stream=s1)
        s1.synchronize()

    assert np.array_equal(g.run(enc, lens, res, call=on_stream), one)

    # two calls back to back on two streams: the second's staging waits for the first's launches.
    # The first writes prefixes, the second the whole cut over them.
    pre = [min(ln, 5) for ln in lens]

    def two_streams(plan, dsts):
        plan.glue_mixed(g.masks, dsts, pre, stream=s1)
        plan.glue_mixed(g.masks, dsts, lens, stream=s2)
        s1.synchronize()
        s2.synchronize()

    assert np.array_equal(g.run(enc, lens, res, call=two_streams), one)


def test_13_plus_2_goes_entry_by_entry():
    k, m = 13, 2
    enc = RS.New(k, m)
    sizes = [0, 1, 17, 64, W + 1, 0, 4099, 333, 16, 2 * W, 5, 0]
    masks = masks_for(k, m, len(sizes))
    lost = {(bool((masks[e][:k] == 0).any()), bool((masks[e][k:] == 0).any())) for e, s in enumerate(sizes) if s}
    assert len(lost) == 4  # healthy, data alone, parity alone, both
    for kind in ("stripes", "shards"):
        g = Glue(k, m, kind, sizes, masks, seed=132)
        res = [(3 * e) % 16 for e in range(len(sizes))]
        for lens in (trunc_lens(k, sizes), prefix_lens(k, sizes)):
            # what the per-entry route costs, from the masks and lengths alone: a copy per present data
            # shard with a byte wanted, an apply per entry with a missing one wanted, a copy more if that is cut
            calls = 0
            for e, s in enumerate(sizes):
                valid = [max(0, min(s, lens[e] - j * s)) for j in range(k)]
                calls += sum(1 for j in range(k) if valid[j] and masks[e][j])
                lost = [valid[j] for j in range(k) if valid[j] and not masks[e][j]]
                calls += (1 if lost else 0) + sum(1 for v in lost if v < s)
            s0 = B.glue_plan_stats()
            g.run(enc, lens, res)
            s1 = B.glue_plan_stats()
            assert s1["kernel_launches"] == s0["kernel_launches"]
            assert s1["per_stripe_calls"] - s0["per_stripe_calls"] == calls > 0


@pytest.mark.parametrize("kind", ["stripes", "shards"])
def test_four_lost_data_shards_around_the_half_tile(kind):
    """With four data shards to rebuild the kernel codes a tile as two halves of
    T / 2 shard bytes: lengths and prefixes on both sides of every half's edge,
    four data shards lost in every entry (and, in turn, none to three beside them
    in a second call's masks)."""
    k, m = 12, 4
    enc = RS.New(k, m)
    T, H = tile(), tile() // 2
    sizes = [H - 1, H, H + 1, H + 17, T - 1, T, T + 1, T + H - 1, T + H, T + H + 1, 2 * T + H + 5, 1, 16]
    lost = [(0, 1, 2, 3), (8, 9, 10, 11), (0, 5, 6, 11), (1, 3, 7, 10)]
    four = np.array([[0 if j in lost[e % 4] else 1 for j in range(k + m)] for e in range(len(sizes))], np.uint8)
    g = Glue(k, m, kind, sizes, four, seed=124)
    res = [(11 * e + 2) % 16 for e in range(len(sizes))]
    s0 = B.glue_plan_stats()
    g.run(enc, trunc_lens(k, sizes), res)
    # prefixes that end just before, at and just behind the half's edge of the first data shard
    g.run(enc, [min(k * s, [H - 1, H, H + 1, s + H, T + 1][e % 5]) for e, s in enumerate(sizes)], res)
    assert B.glue_plan_stats()["kernel_launches"] - s0["kernel_launches"] == 2
    mixed = np.array([[0 if j in lost[e % 4][:e % 5] else 1 for j in range(k + m)] for e in range(len(sizes))],
                     np.uint8)
    Glue(k, m, kind, sizes, mixed, seed=125).run(enc, trunc_lens(k, sizes), res)


def test_destinations_that_touch_own_shards_pass():
    """A destination may end where one of the entry's shards begins and begin where
    another ends: ranges that touch do not overlap.  One byte further is refused."""
    k, m, S = 4, 2, 50
    enc = RS.New(k, m)
    obj = np.asarray(O.object_bytes(77, k * S), np.uint8)
    par = CO.apply(CO.build_matrix(k, m)[k:], [obj[j * S:(j + 1) * S] for j in range(k)])
    stripe = np.concatenate([obj] + [np.asarray(p, np.uint8) for p in par])
    # [9 sentinels][hole of k S][stripe of (k+m) S][hole of k S][9 sentinels]
    host = np.full(18 + 2 * k * S + (k + m) * S, SENT, np.uint8)
    base = 9 + k * S
    host[base:base + (k + m) * S] = stripe
    t = torch.from_numpy(host.copy()).cuda()
    plan = B.StripePlan(enc, stripes=[(t.data_ptr() + base, S)])
    mask = np.ones((1, k + m), np.uint8)
    for at in (9, base + (k + m) * S):
        plan.glue_mixed(mask, [t.data_ptr() + at], [k * S])
        torch.cuda.synchronize()
        host[at:at + k * S] = obj
        assert np.array_equal(t.cpu().numpy(), host)
    for at in (10, base + (k + m) * S - 1):
        with pytest.raises(RS.ErrInvalidArg, match="overlaps"):
            plan.glue_mixed(mask, [t.data_ptr() + at], [k * S])
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), host)


def test_destination_errors_with_a_device():
    """tests/test_glue_host.py's checks on entries with bytes in them, which need a
    device to build their plans on: here there is one."""
    assert GH.destination_errors() is True
