"""Cases of the plan hash sweep (tests/test_gpu_hash_sweep.py) and a model of the
schedule of md5_plan and md5_files (hashplan_kernel.inc, hashfiles_kernel.inc)
and of their `_rows` copies.  Plain Python, no torch, no numpy;
tests/test_hash_sweep_cases.py asserts what these inputs cover on a machine
without a GPU.

The model restates where the blocks of a chain fall, not the arithmetic.  A chain
is its non-empty segments (address, length) in order:

  nb = total // 64 whole blocks and rv = total % 64 tail bytes;
  block i is INSIDE when the segment holding stream byte 64 i has at least 64
  bytes left from there (its shift is its first byte's address & 3), otherwise
  CUT, spanning some number of segments, the first boundary 1..63 bytes in;
  the kernels load blocks in two ping-ponged groups of D, so block i sits in
  slot i % 2D of trip i // 2D;
  the tail lies in 0, 1, 2 or more segments.

The wave composition of a call is the host's (hashplan.h hash_order /
hash_chains, hashfiles.h files_chains): entries, or objects by their total,
longest first and stable; the selected shards of each in index order; every 64
consecutive chains one wave.  From it come the `chains` and `segments` a call
adds to its counters.

Every placement is an offset into a buffer whose device address is a multiple of
64, so an offset's residue is the address's.  A call is placed for each of the
three plan kinds: `stripes` (one base per entry, shards back to back), `objects`
(data and parity regions apart: both address rules) and `shards` (every shard at
an offset of its own, 1..13 slack bytes around it, the (entry, shard) pairs
shuffled over three buffers: the `_rows` kernels).  Entry e's residue `res`
mod 16 is that of its base, of its data region (the parity region: res + 8) or
of its shard 0 (shard j: res + 5 j).
"""
import random
import re
from bisect import bisect_right
from functools import lru_cache
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
D = int(re.search(r"#define HBEC_MD5_DEPTH_LIST (\d+)", (ROOT / "hummingbird_amd/csrc/tuning.h").read_text()).group(1))
SENT = 0xA5                       # digest slots nothing may write
SLACK = 0x5A                      # bytes around the shards of a `shards` placement
KINDS = ("stripes", "objects", "shards")
SHAPES = ((4, 2), (8, 3))
SLOTS = 2 * D                     # blocks in flight: two groups of D
LONG = 4 * D + 1                  # blocks after which both groups have been reloaded twice
P_MAX = 64 * (4 * D + 2) + 63     # the longest P1 shard
P1_EXTRA = 5
TAILS = (0, 1, 55, 56, 57, 63)


# ---- the schedule of one chain ------------------------------------------------------------
class Sched:
    """nb, rv, blocks [(kind, ...)] and the tail's span of a chain of non-empty segments.
    blocks[i] = ("in", shift, segment) or ("cut", span, first boundary offset, length of
    the segment behind that boundary)."""

    def __init__(self, segs):
        assert all(n > 0 for _, n in segs)
        self.segs = list(segs)
        starts, pos = [], 0
        for _, n in segs:
            starts.append(pos)
            pos += n
        self.total = pos
        self.nb, self.rv = divmod(pos, 64)
        self.blocks = []
        for i in range(self.nb):
            s = bisect_right(starts, 64 * i) - 1
            off = 64 * i - starts[s]
            left = segs[s][1] - off
            if left >= 64:
                self.blocks.append(("in", (segs[s][0] + off) & 3, s))
            else:
                last = bisect_right(starts, 64 * i + 63) - 1
                self.blocks.append(("cut", last - s + 1, left, segs[s + 1][1]))
        self.tail_span = 0
        if self.rv:
            self.tail_span = len(segs) - (bisect_right(starts, 64 * self.nb) - 1)

    def first_cut(self):
        return next((i for i, b in enumerate(self.blocks) if b[0] == "cut"), None)

    def state(self, i):
        """what a lane does at block index i: "in", "cut" or "past" its end"""
        return self.blocks[i][0] if i < self.nb else "past"


def slot_trip(i):
    return i % SLOTS, min(i // SLOTS, 2)


# ---- a call ---------------------------------------------------------------------------------
class Call:
    """One hash_mixed call (objs None) or one hash_files call (objs: the objects, each a
    list of piece lengths; a piece may be (length, res)).  sizes: shard length of every
    entry; res: residue mod 16 of every entry (default: its index); select: rows of n
    flags per entry / per object, or None for every shard; flt: a filter word per entry
    (examined: flt & fbits), or None."""

    def __init__(self, name, k, m, sizes=None, objs=None, res=None, select=None, flt=None, fbits=1):
        self.name, self.k, self.m, self.n = name, k, m, k + m
        self.files = objs is not None
        if self.files:
            flat = [p if isinstance(p, tuple) else (p, None) for o in objs for p in o]
            sizes = [p[0] for p in flat]
            res = [(e if r is None else r) % 16 for e, (_, r) in enumerate(flat)]
            self.objs = [[p[0] if isinstance(p, tuple) else p for p in o] for o in objs]
            self.starts = [0]
            for o in objs:
                self.starts.append(self.starts[-1] + len(o))
        else:
            self.objs, self.starts = None, None
        self.sizes = list(sizes)
        self.res = [e % 16 for e in range(len(self.sizes))] if res is None else [r % 16 for r in res]
        self.n_rows = len(self.objs) if self.files else len(self.sizes)
        self.select = None if select is None else [tuple(1 if x else 0 for x in row) for row in select]
        assert self.select is None or (len(self.select) == self.n_rows and all(len(r) == self.n for r in self.select))
        self.flt, self.fbits = (None if flt is None else list(flt)), fbits
        assert self.flt is None or len(self.flt) == len(self.sizes)
        self._place = {}

    # -- the host's chain list --
    def row(self, r):
        return (1,) * self.n if self.select is None else self.select[r]

    def entries_of(self, r):
        """the entries a chain of row r walks"""
        return range(self.starts[r], self.starts[r + 1]) if self.files else (r,)

    def total(self, r):
        return sum(self.sizes[e] for e in self.entries_of(r))

    def chains(self):
        """[(row, shard)]: rows with a byte, longest first (stable), selected shards in index order"""
        rows = sorted((r for r in range(self.n_rows) if self.total(r)), key=lambda r: -self.total(r))
        return [(r, j) for r in rows for j in range(self.n) if self.row(r)[j]]

    def waves(self):
        c = self.chains()
        return [c[w:w + 64] for w in range(0, len(c), 64)]

    def stats(self):
        """(chains, segments) the call adds to its counters; segments count for hash_files only"""
        c = self.chains()
        return len(c), sum(sum(1 for e in self.entries_of(r) if self.sizes[e]) for r, _ in c)

    def passes(self, e):
        return self.flt is None or bool(self.flt[e] & self.fbits)

    def examined(self, r):
        return any(self.passes(e) for e in self.entries_of(r))

    # -- where the bytes lie --
    def place(self, kind):
        """(at, buffer lengths): at[e][j] = (buffer, offset), None for a zero-length entry"""
        if kind not in self._place:
            self._place[kind] = place(kind, self.k, self.m, self.sizes, self.res)
        return self._place[kind]

    def segs(self, kind, r, j):
        """[(buffer, offset, length)] of chain (r, j): its non-empty entries in order"""
        at, _ = self.place(kind)
        return [at[e][j] + (self.sizes[e],) for e in self.entries_of(r) if self.sizes[e]]

    def sched(self, kind, r, j):
        return Sched([(o, n) for _, o, n in self.segs(kind, r, j)])

    def describe(self, kind, r, j):
        """for a failure message: lengths, shard, start residues, first cut block"""
        segs = self.segs(kind, r, j)
        what = f"pieces {self.objs[r]}" if self.files else f"length {self.sizes[r]}"
        return (f"{self.name} [{kind} {self.k}+{self.m}] {'object' if self.files else 'entry'} {r}: {what}, "
                f"shard {j}, start residues {[o % 16 for _, o, _ in segs]}, "
                f"first cut block {Sched([(o, n) for _, o, n in segs]).first_cut()}")


def place(kind, k, m, sizes, res):
    n = k + m
    at = [None] * len(sizes)
    if kind == "shards":
        rng = random.Random(len(sizes) * 31 + n)
        pairs = [(e, j) for e, s in enumerate(sizes) if s for j in range(n)]
        rng.shuffle(pairs)
        fill = [16, 16, 16]
        for e, s in enumerate(sizes):
            if s:
                at[e] = [None] * n
        for e, j in pairs:
            b = rng.randrange(3)
            off = fill[b] + 1 + rng.randrange(13)
            off += (res[e] + 5 * j - off) % 16
            at[e][j] = (b, off)
            fill[b] = off + sizes[e]
        return at, [f + 32 for f in fill]
    regions = [(0, k, 0), (k, n, 8)] if kind == "objects" else [(0, n, 0)]
    pos = [16] * len(regions)
    for e, s in enumerate(sizes):
        if not s:
            continue
        at[e] = []
        for b, (lo, hi, shift) in enumerate(regions):
            off = pos[b] + 3
            off += (res[e] + shift - off) % 16
            at[e] += [(b, off + i * s) for i in range(hi - lo)]
            pos[b] = off + (hi - lo) * s
    return at, [p + 32 for p in pos]


# ---- P1. md5_plan: every length at every start residue -------------------------------------
@lru_cache(maxsize=None)
def p1_call(k, m):
    """Sixteen entries of every length 0..P_MAX, one per residue, so zero-length entries
    lie among the others.  Chains go out longest first and 16 (k + m) (P_MAX - L) is a
    multiple of 64 wherever L + 1 is, so on their own these entries never put two block
    counts into one wave: P1_EXTRA more of the longest move every such edge into a wave."""
    sizes, res = [], []
    for r in range(16):
        for s in range(P_MAX + 1):
            sizes.append(s)
            res.append(r)
    return Call("P1", k, m, sizes + [P_MAX] * P1_EXTRA, res=res + list(range(P1_EXTRA)))


# ---- P2. md5_plan: what one wave mixes ------------------------------------------------------
@lru_cache(maxsize=None)
def p2_calls(k, m):
    n, calls = k + m, []

    def one_shard(count, at=0):
        return [[1 if j == (at + e) % n else 0 for j in range(n)] for e in range(count)]

    for nb_max in range(1, LONG + 1):
        sizes = [64 * b + t for b in range(nb_max + 1) for t in TAILS]   # (0, 0) is a zero-length entry
        flt = [0 if e % 5 == 2 else 1 + e % 3 for e in range(len(sizes))]
        calls.append(Call(f"P2.nb_max{nb_max}", k, m, sizes, select=one_shard(len(sizes), nb_max), flt=flt, fbits=3))
    sizes = [64 * (e % 7) + TAILS[e % 6] + 1 for e in range(64)]
    calls.append(Call("P2.full_wave", k, m, sizes, select=one_shard(64)))
    calls.append(Call("P2.nothing_examined", k, m, sizes[:40], select=one_shard(40), flt=[4] * 40, fbits=3))
    # two waves, the longer entries' wave without an examined lane
    sizes = [700 - e for e in range(64)] + [300 - 4 * e for e in range(40)]
    calls.append(Call("P2.dead_wave", k, m, sizes, select=one_shard(104), flt=[0] * 64 + [1] * 40))
    return calls


# ---- F. md5_files ---------------------------------------------------------------------------
NEXT = 64 * (2 * D + 1)           # the piece behind an F1 cut: the load cursor crosses first


@lru_cache(maxsize=None)
def f1_call(k, m):
    """A cut in block i = slot + 2D trip, its boundary o bytes in: [64 i + o, >= 2D + 1 blocks]"""
    objs = []
    for i in range(3 * SLOTS):
        for o in range(1, 64):
            objs.append([(64 * i + o, i + o), (NEXT + (7 * o + i) % 64, 3 * i + o)])
    return Call("F1", k, m, objs=objs)


def shift_pairs():
    return {(a, b) for a in range(4) for b in range(4)}


@lru_cache(maxsize=None)
def f2_call(k, m):
    """Shift a before a boundary and b behind it, the boundary o bytes into block 2 (a cut)
    or on its edge (o = 0).  The first inside block behind a cut starts 64 - o bytes into
    the second piece."""
    objs = []
    for o in (0, 1, 2, 3, 31, 62, 63):
        for a in range(4):
            for b in range(4):
                r1 = (b - (64 - o if o else 0)) % 4
                objs.append([(128 + o, a + 4 * (b % 2)), (NEXT + 64 - o, r1 + 4 * (a % 3))])
    return Call("F2", k, m, objs=objs)


@lru_cache(maxsize=None)
def f3_call(k, m):
    objs = []
    for span in range(2, 9):      # block 1 over `span` segments: 10 bytes, span - 2 pieces of 5, the rest
        objs.append([74] + [5] * (span - 2) + [54 - 5 * (span - 2) + 64 * 3 + span])
    objs += [[1] * 64, [70] + [1] * 64 + [200], [1] * 64 + [1] * 64]           # 64 one-byte pieces in a block
    objs += [[74, 0, 5, 0, 0, 49 + 128], [40, 0, 0, 30, 0, 100]]                # zero-length entries inside a span
    objs += [[0, 50, 61, 0], [0, 0, 77, 100, 0], [0, 200], [200, 0], [0, 0, 0], [0], []]   # first and last; no byte
    objs += [[63] * (LONG + 2), [37] * (2 * LONG + 2), [7, 3, 11, 5, 20] * 15]  # runs of cut blocks
    return Call("F3", k, m, objs=objs)


def split(total, parts, salt):
    """`parts` positive lengths that sum to total"""
    out, left = [], total
    for p in range(parts - 1):
        x = 1 + (salt * 7 + p * 13) % (left - (parts - 1 - p))
        out.append(x)
        left -= x
    return out + [left]


def f4_expected():
    """(rv, tail span 0/1/2/3+, what the last whole block is)"""
    want = {(0, 0, "in"), (0, 0, "cut")}
    for rv in range(1, 64):
        for span in range(1, min(rv, 3) + 1):
            want |= {(rv, span, "in"), (rv, span, "cut"), (rv, span, "none")}
    return want


@lru_cache(maxsize=None)
def f4_call(k, m):
    objs = [[64, 64], [94, 34]]
    for rv in range(1, 64):
        for span in range(1, min(rv, 3) + 1):
            parts = 3 + rv % 3 if span == 3 and rv >= 5 else span   # tails over 4 and 5 segments as well
            t = split(rv, parts, rv + span)
            objs.append([64, 64 + t[0]] + t[1:])              # last whole block inside
            objs.append([94, 34 + t[0]] + t[1:])              # last whole block cut
            objs.append([94, 20, 14 + t[0]] + t[1:])          # cut over three segments
    for rv in range(1, 64):                                   # totals under 64 from 1..5 pieces
        for parts in range(1, min(rv, 5) + 1):
            objs.append(split(rv, parts, rv * parts))
    return Call("F4", k, m, objs=objs)


@lru_cache(maxsize=None)
def f5_calls(k, m):
    n = k + m
    some = [1 if j in (0, 2, k, n - 1) else 0 for j in range(n)]
    one = [1 if j == k else 0 for j in range(n)]
    calls = []
    # at block 1: cut lanes, inside lanes and lanes past their end
    objs = [[100, 400], [256, 244], [70, 20]] * 3
    calls.append(Call("F5.mixed_at_a_block", k, m, objs=objs, select=[some] * len(objs)))
    # one cut lane: every other boundary lies on a block edge
    objs = [[128, 128], [192, 64, 70], [64, 64, 64, 64, 9]] * 3 + [[100, 156]]
    calls.append(Call("F5.one_cut_lane", k, m, objs=objs, select=[some] * 9 + [one]))
    # lanes without a whole block among lanes of 4D + 1 blocks and more
    objs = [[10, 20], [64 * LONG, 50], [1, 1, 1], [300, 300, 40], [63], [64 * LONG + 5, 64, 59]] * 2
    calls.append(Call("F5.short_among_long", k, m, objs=objs, select=[some] * len(objs)))
    # unexamined objects between examined ones; an object examined through one passing entry;
    # an object whose only passing entry is zero-length
    objs = [[100 + 9 * g, 50 + g, 200 - 7 * g] for g in range(12)] + [[90, 80, 70, 60], [33, 0, 71]]
    flt = []
    for g in range(12):
        flt += [0, 0, 0] if g % 3 == 1 else [2, 1, 3]
    flt += [0, 0, 2, 0] + [0, 1, 0]
    calls.append(Call("F5.filtered", k, m, objs=objs, select=[some] * len(objs), flt=flt, fbits=3))
    # a final partial wave
    objs = [[60 + 11 * g, 5 + g, 130 + g % 3] for g in range(12)]
    calls.append(Call("F5.partial_wave", k, m, objs=objs))
    return calls


# ---- F6. files= plans -----------------------------------------------------------------------
F6_CHUNKS = range(1, 201)
F6_STRIPES = (3, 4, 5)


def ec_stripes(length, k, chunk):
    """ecSplit's cut of an object: the shard length of every stripe"""
    full, out = k * chunk, []
    while length > 0:
        out.append(chunk if length >= full else -(-length // k))
        length -= full
    return out


def f6_lengths(k, chunk):
    """content lengths of 3, 4 and 5 stripes, the last one short (chunk 1 has no shorter shard)"""
    out = []
    for s in F6_STRIPES:
        last = 1 + (7 * chunk + s) % (chunk - 1) if chunk > 1 else 1
        out.append(k * chunk * (s - 1) + k * (last - 1) + 1 + s % k)
    return out


def f6_layout(k, m, chunk):
    """(content lengths, per object the stripes' shard lengths, offsets [g][j] of every
    file in one buffer, buffer length): files at residues that differ within an object"""
    n = k + m
    lengths = f6_lengths(k, chunk)
    cuts = [ec_stripes(x, k, chunk) for x in lengths]
    offs, pos = [], 16
    for g, c in enumerate(cuts):
        row = []
        for j in range(n):
            off = pos + 1
            off += (3 * g + 5 * j + chunk - off) % 16
            row.append(off)
            pos = off + sum(c)
        offs.append(row)
    return lengths, cuts, offs, pos + 32


# ---- L. the bit count's upper word ----------------------------------------------------------
L_PIECE = 64 << 20
L_OFFSETS = (0, 16, 5, 32, 48, 1, 64, 33)     # first byte of each 64 MiB piece in the buffer
L_LAST = 7                                    # the one-byte piece
L_TOTAL = len(L_OFFSETS) * L_PIECE + 1
L_BUFFER = max(L_OFFSETS) + 2 * L_PIECE + 64  # every 1+1 entry's two shards lie inside
L2_BASE = 5                                   # md5_plan: one shift for the whole chain
