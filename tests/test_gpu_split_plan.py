"""hbec_split_plan on the device: the k+m shards of every entry of a plan from
its object bytes in one call (ecSplit for a batch), on all four kinds of plan.

Nothing expected comes from the product.  Entry e's piece is oracle.object_bytes,
the shards it must become are oracle.ec_split's (one stripe: chunk >= S), and
oracle.ec_glue of those shards must return the piece.

The common discipline (class Split, shared with the sweep test): whole arenas
are compared; the shard arenas start as random garbage where a shard lies and
0xC3 sentinels around and between the shards; the source arena holds 0xC3, a
non-zero byte, directly before and after every piece, so a pad that reads
through instead of zeroing fails; and the source arena must come back
bit-identical."""
import contextlib

import numpy as np
import pytest
import torch

import test_split_host as SH
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SENT = 0xC3
W = 992
KINDS = ["stripes", "objects", "shards", "files"]
SHAPES = [(4, 2), (8, 3), (12, 4), (4, 0)]
IDS = ["4+2", "8+3", "12+4", "4+0"]


def tile():
    return B.split_plan_tile_bytes()


def sizes_for():
    T = tile()
    assert T == 3968 == 4 * W
    rng = np.random.default_rng(20240712)
    rand = [int(s) + (1 if s % 16 == 0 else 0) for s in rng.integers(1, 40001, 6)]
    mid = [1, 3, 15, 16, 17, 31, 33, 63, 64, 65, W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 17]
    return [0] + mid[:8] + [0] + mid[8:] + rand + [0]  # zero-length first, interior and last


def pads_for(k, sizes, shift=0):
    """ecSplit's pad, 0..min(k-1, k S - 1) in turn over the entries with bytes."""
    out, i = [], shift
    for s in sizes:
        out.append(i % (min(k - 1, k * s - 1) + 1) if s else 0)
        i += 1 if s else 0
    return out


@contextlib.contextmanager
def one_matrix_per_shape():
    """The oracle builds its coding matrix anew for every ec_split and ec_glue,
    which is most of the time of a few thousand small entries: while a Split is
    built, the oracle's own build_matrix runs once per shape and hands out copies."""
    built, real = {}, O.build_matrix

    def build_matrix(data_shards, total_shards):
        key = (data_shards, total_shards)
        if key not in built:
            built[key] = real(data_shards, total_shards)
        return [list(row) for row in built[key]]

    O.build_matrix = build_matrix
    try:
        yield
    finally:
        O.build_matrix = real


class Split:
    """Entries of the given shard lengths and pads on a plan of one kind, and the
    common discipline of every split test.  at[e][j] = (buffer, offset) of shard j.
    skip: entries whose length is given as 0, which must stay as they were."""

    def __init__(self, k, m, kind, sizes, pads, seed, skip=()):
        self.k, self.m, self.n, self.kind = k, m, k + m, kind
        if kind == "files":  # an object of no bytes has no entry
            keep = [e for e, s in enumerate(sizes) if s]
            skip = [keep.index(e) for e in skip if e in keep]
            sizes, pads = [sizes[e] for e in keep], [pads[e] for e in keep]
        self.sizes, self.skip = [int(s) for s in sizes], set(skip)
        self.live = [e for e, s in enumerate(self.sizes) if s]
        self.lens = [k * s - int(p) if s else 0 for s, p in zip(self.sizes, pads)]
        assert all(k * s - k < ln <= k * s for s, ln in zip(self.sizes, self.lens) if s)
        rng = np.random.default_rng(seed)
        self.pieces, self.want, self.before = [], [], []
        with one_matrix_per_shape():
            for e, (s, ln) in enumerate(zip(self.sizes, self.lens)):
                piece = np.asarray(O.object_bytes(seed * 100003 + e, ln), np.uint8)
                files = O.ec_split(k, m, piece.tobytes(), max(s, 1)) if s else [b""] * self.n
                assert [len(f) for f in files] == [s] * self.n, e
                if s:  # the reference's ecGlue of the shards is the piece
                    assert O.ec_glue(k, m, list(files), s, ln) == piece.tobytes(), e
                self.pieces.append(piece)
                self.want.append([np.frombuffer(f, np.uint8) for f in files])
                self.before.append([rng.integers(0, 256, s, dtype=np.uint8) for _ in range(self.n)])
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
            self.buf_lens = [at + 9]
        elif self.kind == "objects":
            a = b = 0
            for i, e in enumerate(self.live):
                da, pb = a + 1 + (3 * i) % 16, b + 1 + (7 * i) % 16
                self.at[e] = [(0, da + j * self.sizes[e]) for j in range(k)] + \
                    [(1, pb + j * self.sizes[e]) for j in range(self.m)]
                a, b = da + k * self.sizes[e], pb + self.m * self.sizes[e]
            self.buf_lens = [a + 9, b + 9]
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
            self.buf_lens = [f + 13 for f in fill]

    def shard_bufs(self, after):
        """The shard arenas before the call, or what they must hold after it."""
        bufs = [np.full(x, SENT, np.uint8) for x in self.buf_lens]
        for e in self.live:
            new = after and e not in self.skip
            for j, (b, o) in enumerate(self.at[e]):
                bufs[b][o:o + self.sizes[e]] = self.want[e][j] if new else self.before[e][j]
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
        # one stripe each: the content length is the piece's, the chunk no shorter than any shard
        plan = B.StripePlan(enc, files=[(addr[e], ln) for e, ln in enumerate(self.lens)], chunk_size=max(self.sizes))
        assert plan.object_start.tolist() == list(range(len(self.sizes) + 1))
        return plan

    def src_arena(self, residues, garbage=None):
        """The pieces in one arena, 1..16 sentinel bytes between two; with `garbage`
        (a generator) other bytes of the same lengths in their places."""
        offs, at = [], 0
        for ln, r in zip(self.lens, residues):
            o = at + 1
            o += (r - o) % 16
            offs.append(o)
            at = o + ln
        arena = np.full(at + 11, SENT, np.uint8)
        for e, o in enumerate(offs):
            arena[o:o + self.lens[e]] = self.pieces[e] if garbage is None else \
                garbage.integers(0, 256, self.lens[e], dtype=np.uint8)
        return offs, arena

    def run(self, enc, residues, call=None, then=None):
        """One call on fresh buffers; asserts the discipline and returns the shard arenas' bytes.
        call(plan, srcs, lens) replaces the plain call; then(plan, srcs, t) runs after the checks."""
        offs, arena = self.src_arena(residues)
        host = self.shard_bufs(after=False)
        t = [torch.from_numpy(x.copy()).cuda() for x in host]
        src = torch.from_numpy(arena.copy()).cuda()
        assert src.data_ptr() % 16 == 0
        plan = self.plan(enc, t)
        srcs = [src.data_ptr() + o for o in offs]
        lens = [0 if e in self.skip else ln for e, ln in enumerate(self.lens)]
        torch.cuda.synchronize()  # the fills are done before a call on any stream
        if call is None:
            plan.split(srcs, lens)
        else:
            call(plan, srcs, lens)
        torch.cuda.synchronize()
        got = [x.cpu().numpy() for x in t]
        for b, (g, w) in enumerate(zip(got, self.shard_bufs(after=True))):
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, (self.kind, b, bad[:6], [(e, j, o, self.sizes[e], self.lens[e])
                                                           for e in self.live for j, (bb, o) in enumerate(self.at[e])
                                                           if bb == b and o - 16 <= bad[0] <= o + self.sizes[e] + 16])
        assert np.array_equal(src.cpu().numpy(), arena), ("the source arena was written", self.kind)
        if then is not None:
            then(plan, srcs, t)
        return got


def residues_for(sizes, shift=0):
    """0..15 in turn over the pieces with bytes."""
    res, i = [], shift
    for s in sizes:
        res.append(i % 16)
        i += 1 if s else 0
    assert {r for r, s in zip(res, sizes) if s} == set(range(16))
    return res


_CACHE = {}


def split_of(k, m, kind):
    key = (k, m, kind)
    if key not in _CACHE:
        sizes = sizes_for()
        _CACHE[key] = Split(k, m, kind, sizes, pads_for(k, sizes), seed=19 * k + m)
    return _CACHE[key]


def test_whole_trailing_shards_are_pad():
    """S = 1 with a piece of one byte: every data shard but the first is ecSplit's pad."""
    for k in (4, 8, 12):
        assert O.ec_shard_length(1, k) == 1
        files = O.ec_split(k, 2, b"\x5a", 1)
        assert files[0] == b"\x5a" and files[1:k] == [b"\x00"] * (k - 1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,m", SHAPES, ids=IDS)
def test_split_every_kind_of_plan(k, m, kind):
    enc = RS.New(k, m)
    g = split_of(k, m, kind)
    s0 = B.split_plan_stats()
    g.run(enc, residues_for(g.sizes))
    s1 = B.split_plan_stats()
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1  # whatever the entries or lengths
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]


@pytest.mark.parametrize("kind", ["stripes", "shards"])
@pytest.mark.parametrize("k,m", SHAPES, ids=IDS)
def test_every_legal_length(k, m, kind):
    """len = k S - pad for every pad in 0..min(k-1, k S - 1), S = 1 with len = 1
    among them; each piece at its own residue, 0..15 in turn."""
    T = tile()
    H = T // 2  # the 12+4 tile is coded in two halves
    shard_lens = [1, 2, 3, 15, 16, 17, 33, W - 1, W + 1, H - 1, H, H + 1, T - 1, T + 1, T + H, T + H + 1]
    sizes, pads = [], []
    for s in shard_lens:
        for pad in range(min(k - 1, k * s - 1) + 1):
            sizes.append(s)
            pads.append(pad)
    assert (1, k - 1) in set(zip(sizes, pads))  # one byte: k - 1 data shards of pad
    g = Split(k, m, kind, sizes, pads, seed=23 * k + m)
    assert 1 in g.lens
    s0 = B.split_plan_stats()
    g.run(RS.New(k, m), [(5 * e + 3) % 16 for e in range(len(sizes))])
    s1 = B.split_plan_stats()
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]


@pytest.mark.parametrize("kind", ["stripes", "shards"])
def test_launches_cut_by_the_hook_write_the_same_bytes(kind):
    k, m = 4, 2
    enc = RS.New(k, m)
    g = split_of(k, m, kind)
    res = residues_for(g.sizes)
    one = g.run(enc, res)
    n_tiles = sum((s + tile() - 1) // tile() for s in g.sizes)
    s0 = B.split_plan_stats()
    B.set_split_plan_chunk_tiles(3)
    try:
        cut = g.run(enc, res)
    finally:
        B.set_split_plan_chunk_tiles(0)
    assert B.split_plan_stats()["kernel_launches"] - s0["kernel_launches"] == (n_tiles + 2) // 3 > 10
    assert all(np.array_equal(a, b) for a, b in zip(one, cut))


def test_other_streams_write_the_same_bytes():
    k, m = 8, 3
    enc = RS.New(k, m)
    g = split_of(k, m, "objects")
    res = residues_for(g.sizes, shift=5)
    one = g.run(enc, res)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def on_stream(plan, srcs, lens):
        plan.split(srcs, lens, stream=s1)
        s1.synchronize()

    assert all(np.array_equal(a, b) for a, b in zip(g.run(enc, res, call=on_stream), one))

    # two calls back to back on two streams: the second's staging waits for the first's launches.
    # The first splits other bytes of the same lengths, the second the pieces over them.
    offs, other = g.src_arena(res, garbage=np.random.default_rng(83))
    alt = torch.from_numpy(other).cuda()

    def two_streams(plan, srcs, lens):
        plan.split([alt.data_ptr() + o for o in offs], lens, stream=s1)
        plan.split(srcs, lens, stream=s2)
        s1.synchronize()
        s2.synchronize()

    assert all(np.array_equal(a, b) for a, b in zip(g.run(enc, res, call=two_streams), one))
    assert np.array_equal(alt.cpu().numpy(), other)


def test_13_plus_2_goes_entry_by_entry():
    k, m = 13, 2
    enc = RS.New(k, m)
    sizes = [0, 1, 17, 64, W + 1, 0, 4099, 333, 16, 2 * W, 5, 1, 0]
    pads = [0, 12, 3, 0, 12, 0, 7, 1, 0, 5, 11, 0, 0]
    for kind in ("stripes", "shards"):
        g = Split(k, m, kind, sizes, pads, seed=132)
        # what the per-entry route costs, from the lengths alone: a copy per data shard with a byte
        # of the piece, a memset per data shard the pad reaches, an apply per entry
        calls = 0
        for s, ln in zip(g.sizes, g.lens):
            if s:
                valid = [max(0, min(s, ln - j * s)) for j in range(k)]
                calls += sum(1 for v in valid if v) + sum(1 for v in valid if v < s) + 1
        s0 = B.split_plan_stats()
        g.run(enc, [(3 * e) % 16 for e in range(len(sizes))])
        s1 = B.split_plan_stats()
        assert s1["kernel_launches"] == s0["kernel_launches"]
        assert s1["per_stripe_calls"] - s0["per_stripe_calls"] == calls > 0


@pytest.mark.parametrize("kind", KINDS)
def test_entries_given_no_bytes_stay_as_they_were(kind):
    k, m = 4, 2
    sizes = sizes_for()
    live = [e for e, s in enumerate(sizes) if s]
    skip = live[::3]
    g = Split(k, m, kind, sizes, pads_for(k, sizes, shift=2), seed=61, skip=skip)
    assert g.skip and len(g.skip) < len(g.live)
    s0 = B.split_plan_stats()
    g.run(RS.New(k, m), residues_for(g.sizes, shift=9))
    assert B.split_plan_stats()["kernel_launches"] - s0["kernel_launches"] == 1
    # nothing given at all: nothing launched
    g = Split(k, m, kind, sizes, pads_for(k, sizes), seed=62, skip=live)
    s0 = B.split_plan_stats()
    g.run(RS.New(k, m), residues_for(g.sizes))
    assert B.split_plan_stats() == s0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,m", SHAPES, ids=IDS)
def test_split_then_glue_with_shards_lost_returns_the_sources(k, m, kind):
    """split -> (lose shards) -> glue on one plan: the shards a mask calls missing
    are overwritten with garbage after the split, and glue_mixed must return the
    pieces all the same."""
    enc = RS.New(k, m)
    g = split_of(k, m, kind)
    n = k + m
    ne = len(g.sizes)
    rng = np.random.default_rng(5 * k + m)
    masks = np.ones((ne, n), np.uint8)
    for e in range(ne):
        masks[e, rng.choice(n, size=e % (m + 1), replace=False)] = 0
    assert m == 0 or (masks[:, :k] == 0).any()

    def glue_back(plan, srcs, t):
        for e in g.live:
            for j, (b, o) in enumerate(g.at[e]):
                if not masks[e, j]:
                    t[b][o:o + g.sizes[e]] = torch.from_numpy(rng.integers(0, 256, g.sizes[e], dtype=np.uint8)).cuda()
        offs, arena = g.src_arena(residues_for(g.sizes, shift=7))
        out = torch.full((arena.size,), SENT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        plan.glue_mixed(masks, [out.data_ptr() + o for o in offs], g.lens)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), arena)

    g.run(enc, residues_for(g.sizes), then=glue_back)


@pytest.mark.parametrize("k,m", SHAPES[:3], ids=IDS[:3])
def test_split_then_verify_finds_nothing_on_a_stripes_plan(k, m):
    g = split_of(k, m, "stripes")

    def verify(plan, srcs, t):
        flags = torch.zeros(len(g.sizes), dtype=torch.int32, device="cuda")
        plan.verify(flags)
        torch.cuda.synchronize()
        assert not flags.cpu().numpy().any()
        # and it does find a parity byte changed afterwards
        e = g.live[-1]
        b, o = g.at[e][k]
        t[b][o] ^= 1
        plan.verify(flags)
        torch.cuda.synchronize()
        assert np.flatnonzero(flags.cpu().numpy()).tolist() == [e]

    g.run(RS.New(k, m), residues_for(g.sizes), then=verify)


def test_sources_that_touch_own_shards_pass():
    """A source may end where one of the entry's shards begins and begin where
    another ends: ranges that touch do not overlap.  One byte further is refused."""
    k, m, S = 4, 2, 50
    enc = RS.New(k, m)
    ln = k * S - 3
    piece = np.asarray(O.object_bytes(78, ln), np.uint8)
    want = np.concatenate([np.frombuffer(f, np.uint8) for f in O.ec_split(k, m, piece.tobytes(), S)])
    # [9 sentinels][piece][3 sentinels][stripe of (k+m) S][piece][3 + 9 sentinels]
    host = np.full(18 + 2 * k * S + (k + m) * S, SENT, np.uint8)
    base = 9 + k * S
    below, above = base - ln, base + (k + m) * S
    host[below:base] = piece
    host[above:above + ln] = piece
    for at in (below, above):
        t = torch.from_numpy(host.copy()).cuda()
        plan = B.StripePlan(enc, stripes=[(t.data_ptr() + base, S)])
        plan.split([t.data_ptr() + at], [ln])
        torch.cuda.synchronize()
        after = host.copy()
        after[base:base + (k + m) * S] = want
        assert np.array_equal(t.cpu().numpy(), after)
        for off in (below + 1, above - 1):
            with pytest.raises(RS.ErrInvalidArg, match="overlaps"):
                plan.split([t.data_ptr() + off], [ln])
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), after)


def test_source_errors_with_a_device():
    """tests/test_split_host.py's checks on entries with bytes in them, which need a
    device to build their plans on: here there is one."""
    assert SH.source_errors() is True
