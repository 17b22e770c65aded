"""Exhaustive sweep of gf_locate_mixed_plan<RMAX> (csrc/locate.hip, behind
plan.locate_mixed): one stripe per flip, all masks of a case in ONE call, the
whole `where` array compared with np.array_equal.  Nothing is sampled, nothing
is tolerated.

The kernel's tile is a copy of verify_mixed_tile, not a shared function (its
own compare mask, lane predicate and ballot), and its cold path
locate_classify<R> exists nowhere else: the select chain that picks dword d out
of acc[R][U][4], a second partial-word mask, the per-byte split of a dword, the
proportionality test, surv_bit for the slots of the s_hi word, the shuffle OR
and lane 0's one atomicOr.  A wrong word is the worst output the library has:
the caller clears the named shard and rebuilds it from the others.

Expected words follow from the oracle alone.  For a mask with R >= 2 checked
shards and one bad byte in present shard j the word is LOC_BAD | (present bits
& ~(1 << j)): asserted per mask on the host (single_candidate: for every
present shard j and every e in 1..255 the only column of [rows | I] that
e * column_j is a multiple of is j's; rows from oracle.lagrange.lagrange_row,
products from oracle.MUL, a few vectors repeated through
test_gpu_locate.candidates).  R = 1: LOC_BAD.  A control or a flip in a missing
shard: 0.  Exactly k present: LOC_NOTHING, flipped or not.  Several bad bytes
in one stripe: test_gpu_locate.oracle_where, which searches by brute force.

Every case makes three calls: the clean replica unfiltered, the flipped one
unfiltered, the flipped one filtered with the flags plan.verify_mixed writes
for the same buffer and masks (the words must be the unfiltered ones).  After
each the buffer is bit-identical to its clone and the deltas of
B.locate_plan_stats() are exact.  Layout, placement, controls (every 61st
stripe, cycling over the masks), garbage in every missing shard and the cap on
resident bytes are test_gpu_verify_sweep's and test_gpu_verify_mixed_sweep's.

  every byte     the six shapes of the vmixed sweep: every position of every
                 checked shard, and at position p the survivor in slot
                 (p + p // 16) % k, so every slot meets every byte of a lane's
                 column and every window.
  every tile     12+4, S = 992 + 37: four calls whose largest checked count is
                 1, 2, 3, 4, each with fully swept masks of every R <= RMAX.
  every value    S = 67: every present shard x every e in 1..255 x every byte
                 lane of a dword, the dword cycling through a column's four.
  one dword      four bad bytes of one shard in one dword; two shards at
                 neighbouring bytes of one dword; two shards in two lanes, two
                 windows, two tiles of one stripe; two shards at one position.
  every length   three stripes per S = 1 .. T + 992 + 64, flipped at S - 1 of
                 a shard whose successor in memory is garbage.
  chunked        the 4+2 case under hbec_set_locate_plan_chunk_tiles(3).
  other route    13+2: LOC_SKIPPED for every stripe, counted, nothing launched.
"""
import functools

import numpy as np
import pytest
import torch

from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import lagrange as LG
from oracle import oracle as O

import test_gpu_locate as L
import test_gpu_verify_mixed_sweep as VMS
import test_gpu_verify_sweep as VS
from test_gpu_verify_mixed_sweep import assert_any_flip_shows, lose, roles

pytestmark = pytest.mark.gpu

W = VMS.W  # one 64-lane window of the kernel: 62 columns of 16 bytes
BAD, SKIPPED, NOTHING = N.LOC_BAD, N.LOC_SKIPPED, N.LOC_NOTHING
ORACLE_NAME = -99  # Flips.names: whatever hbec_locate_decode reads from the oracle's word


def tile():
    t = B.locate_plan_tile_bytes()
    assert t == VMS.tile() == 4 * W
    return t


# ---- the oracle (host, numpy only) ---------------------------------------------

def present_bits(mask):
    return sum(1 << i for i, x in enumerate(mask) if x)


@functools.lru_cache(maxsize=None)
def single_candidate(k, m, mask):
    """A mask with R >= 2: e * column_j, for every present shard j and every e in
    1..255, is a multiple of column j and of no other column of [rows | I].  So
    one bad byte in j rules out every present shard but j."""
    surv, checked, _ = roles(k, m, mask)
    R = len(checked)
    assert R >= 2
    rows = [LG.lagrange_row(surv, c) for c in checked]
    cols = [(j, [int(rows[q][t]) for q in range(R)]) for t, j in enumerate(surv)]
    cols += [(j, [1 if q == p else 0 for q in range(R)]) for p, j in enumerate(checked)]
    mult = {j: O.MUL[1:][:, col] for j, col in cols}  # [255, R]: e * column_j for e = 1..255
    for j, _ in cols:
        for i, _ in cols:
            reached = (mult[j][:, None, :] == mult[i][None, :, :]).all(axis=2).any(axis=1)
            assert reached.all() if i == j else not reached.any(), (mask, j, i)
    # the same answer from the search the example-based tests use
    for j, col in cols[::max(1, len(cols) // 4)] + cols[-1:]:
        for e in (1, 0x53, 255):
            assert L.candidates(cols, [int(O.MUL[e, c]) for c in col]) == 1 << j, (mask, j, e)
    return True


class Masks:
    """The masks of one call: roles, counts of checked shards, present bits."""

    def __init__(self, k, m, masks):
        self.k, self.m = k, m
        self.masks = [tuple(x) for x in masks]
        self.arr = np.array(self.masks, np.uint8)
        self.R = np.array([len(roles(k, m, x)[1]) for x in self.masks], np.int64)
        self.bits = np.array([present_bits(x) for x in self.masks], np.int64)
        for x, r in zip(self.masks, self.R):
            if r:
                assert_any_flip_shows(k, m, x)
            if r >= 2:
                single_candidate(k, m, x)

    def words(self, q, shard):
        """The word of a stripe under mask q with one bad byte in `shard` (-1: none)."""
        q, shard = np.asarray(q, np.int64), np.asarray(shard, np.int64)
        hit = (shard >= 0) & (self.arr[q, np.maximum(shard, 0)] != 0)
        named = BAD | (self.bits[q] & ~(np.int64(1) << np.maximum(shard, 0)))
        w = np.where(self.R[q] == 0, NOTHING, np.where(~hit, 0, np.where(self.R[q] == 1, BAD, named)))
        return w.astype(np.uint32)

    def names(self, q, shard):
        """What hbec_locate_decode must say of those words (include/hbec.h)."""
        q, shard = np.asarray(q, np.int64), np.asarray(shard, np.int64)
        hit = (shard >= 0) & (self.arr[q, np.maximum(shard, 0)] != 0)
        return np.where(self.R[q] == 0, N.LOC_UNCHECKED,
                        np.where(~hit, N.LOC_CLEAN, np.where(self.R[q] == 1, N.LOC_AMBIGUOUS, shard)))


class Stripes:
    """What test_gpu_locate.oracle_where reads of a case: n equal stripes in buffer 0."""

    def __init__(self, k, m, S, n, off, pitch):
        self.k, self.m = k, m
        self.sizes = [S] * n
        self.live = list(range(n))
        self.shards = [[(0, off + e * pitch + i * S) for i in range(k + m)] for e in range(n)]


class Flips:
    """F flipped stripes: mask q[f] of stripe f, and the bytes changed: `stripe`
    (0..F-1, ascending), shard, position, xor value of each.  names: what the word
    of stripe f must decode to (None: one change per stripe, from the masks)."""

    def __init__(self, q, shard, pos, val, stripe=None, names=None):
        self.q = np.asarray(q, np.int64)
        self.shard, self.pos = np.asarray(shard, np.int64), np.asarray(pos, np.int64)
        self.val = np.asarray(val, np.uint8)
        self.stripe = np.arange(self.q.size) if stripe is None else np.asarray(stripe, np.int64)
        self.names = None if names is None else np.asarray(names, np.int64)
        assert self.stripe.size == self.shard.size == self.pos.size == self.val.size
        assert np.all(self.val != 0) and np.all(np.diff(self.stripe) >= 0)
        assert np.array_equal(np.unique(self.stripe), np.arange(self.q.size))
        self.single = self.stripe.size == self.q.size
        assert self.single or self.names is not None
        self.first = np.searchsorted(self.stripe, np.arange(self.q.size))  # first change of stripe f


def slot(p, k):
    """The survivor slot flipped at position p.  Not p % k: at k = 4, 8 and 12
    that ties each slot to one byte lane of the dword."""
    return (p + p // 16) % k


def flip_set(k, m, S, masks):
    """Every flip of an every-byte case.  A mask with R checked shards: each at
    every position (role r), then the survivor in slot(p) at every position p
    (role R).  An exactly-k mask: 32 positions over the shard, in its missing
    shards in turn.  The flipped bit is the vmixed sweep's."""
    P = np.arange(S, dtype=np.int64)
    q_, sh_, pos_, val_ = [], [], [], []
    for q, mask in enumerate(masks):
        surv, checked, gone = roles(k, m, mask)
        if checked:
            at = slot(P, k)
            for t in range(k):  # every slot meets every byte of a column and every window
                assert set((P[at == t] % 16).tolist()) == set(range(16)), (mask, t)
                assert set((P[at == t] // W).tolist()) == set(range(-(-S // W))), (mask, t)
            shard = np.concatenate([np.full(S, c, np.int64) for c in checked] + [np.array(surv, np.int64)[at]])
            pos = np.tile(P, len(checked) + 1)
            role = np.repeat(np.arange(len(checked) + 1, dtype=np.int64), S)
        else:
            pos = np.unique(np.linspace(0, S - 1, 32).astype(np.int64))
            shard = np.array(gone, np.int64)[np.arange(pos.size) % len(gone)]
            role = np.zeros(pos.size, np.int64)
        q_.append(np.full(pos.size, q, np.int64))
        sh_.append(shard)
        pos_.append(pos)
        val_.append(VMS.bit(pos, role))
    return Flips(*(np.concatenate(x) for x in (q_, sh_, pos_, val_)))


def words_of(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32).copy()


def decode_all(k, m, marr, stripe_mask, words):
    """hbec_locate_decode of every word (once per distinct (mask, word))."""
    key = (stripe_mask.astype(np.int64) << 32) | words.astype(np.int64)
    u, inv = np.unique(key, return_inverse=True)
    return B.locate_decode(k, m, marr[u >> 32], u & 0xFFFFFFFF)[inv.reshape(-1)]


def stats_delta(s0):
    s1 = B.locate_plan_stats()
    return {f: s1[f] - s0[f] for f in s0}


def three_calls(label, head, plan, present, buf, flip_in, n, n_tiles, want_clean, want, flag_want, route, chunk,
                describe):
    """The calls of every case: clean unfiltered; flipped unfiltered; flipped
    filtered by verify_mixed's flags.  flip_in(): the clean buffer becomes the
    flipped one.  describe(stripes): failure text for wrong stripes.  Returns
    the counters of one call."""
    if route == "kernel":
        want_delta = {"kernel_launches": -(-n_tiles // chunk) if chunk else 1, "skipped_entries": 0}
    else:
        want_delta = {"kernel_launches": 0, "skipped_entries": n}
    keep = None

    def call(expect, what, flags=None):
        where = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s0 = B.locate_plan_stats()
        plan.locate_mixed(present, where, flags=flags)
        torch.cuda.synchronize()
        d = stats_delta(s0)
        got = words_of(where)
        if not np.array_equal(got, expect):
            bad = np.nonzero(got != expect)[0]
            pytest.fail(f"{head} {what}: {bad.size} of {n} stripes wrong, first {describe(bad[:8], got, expect)}")
        assert torch.equal(buf, keep), (label, what, "the buffer was written")
        assert d == want_delta, (label, what, d, want_delta)
        return got, d

    try:
        if chunk:
            B.set_locate_plan_chunk_tiles(chunk)
        keep = buf.clone()
        call(want_clean, "clean")
        flip_in()
        keep.copy_(buf)
        got, d = call(want, "flipped")
        vflags = torch.zeros(n, dtype=torch.int32, device="cuda")
        plan.verify_mixed(present, vflags)
        torch.cuda.synchronize()
        seen = vflags.cpu().numpy()
        assert np.array_equal(seen, flag_want), (label, "verify_mixed flags", np.nonzero(seen != flag_want)[0][:8])
        call(want, "filtered", flags=vflags)
        assert np.array_equal(vflags.cpu().numpy(), seen), (label, "the flags were written")
    finally:
        if chunk:
            B.set_locate_plan_chunk_tiles(0)
    return got, d


def sweep(label, k, m, S, masks, flips, want_r, route="kernel", chunk=0, oracle=False):
    """One case: one stripe per entry of `flips`, all masks in one call."""
    M = Masks(k, m, masks)
    assert set(M.R.tolist()) == set(want_r) | {0}, M.R  # every R named, and an exactly-k mask
    F = flips.q.size
    n, obj = VS.placement(F, 1000 * k + m)
    stripe_mask = np.empty(n, np.int64)
    stripe_mask[obj] = flips.q
    ctrl = np.setdiff1d(np.arange(n), obj)
    assert ctrl.size >= n // VS.CONTROL_EVERY and np.all((np.arange(n) % VS.CONTROL_EVERY != VS.CONTROL_EVERY - 1)
                                                         | np.isin(np.arange(n), ctrl))  # every 61st is a control
    stripe_mask[ctrl] = np.arange(ctrl.size) % len(masks)
    swept = int(np.sum(np.bincount(flips.q, minlength=len(masks)) >= S))
    if swept >= 2:  # fully swept masks interleaved: a wave's next tile is often another R and record
        assert (np.diff(stripe_mask) != 0).sum() >= n // 4
        if len(set(want_r)) >= 2:
            assert (np.diff(M.R[stripe_mask]) != 0).sum() >= n // 4
    present = M.arr[stripe_mask]
    exactly_k = M.R[stripe_mask] == 0
    assert exactly_k.any() and exactly_k[ctrl].any()
    flip_of = np.full(n, -1, np.int64)  # the first change of a stripe
    flip_of[obj] = flips.first

    lay = VS.Layout(k, m, S, aligned=False)
    (_, _, off, pitch), = lay.parts
    assert off == 3 and pitch % 2 == 1
    resident = 2 * (off + n * pitch + lay.pad)  # the buffer and the clone it is compared with
    assert resident <= VS.CAP, resident
    cw = VS.codeword(k, m, S, 7 * k + m + S)
    bufs = VS.replicate(cw, lay, n)
    buf = bufs[0]
    assert buf.data_ptr() % 16 == 0
    assert set(((off + obj * pitch) % 16).tolist()) == set(range(16))  # all 16 alignments are flipped
    # garbage in every missing shard: the codeword's bytes, every one changed
    rng = np.random.default_rng(31 * k + m)
    rows = buf[off:off + n * pitch].view(n, pitch)
    for q, mask in enumerate(M.masks):
        idx = torch.from_numpy(np.nonzero(stripe_mask == q)[0]).cuda()
        for g in roles(k, m, mask)[2]:
            junk = cw[g * S:(g + 1) * S] ^ rng.integers(1, 256, S, dtype=np.uint8)
            rows[idx, g * S:(g + 1) * S] = torch.from_numpy(junk).cuda()

    want_clean = M.words(stripe_mask, np.full(n, -1))
    names_want = M.names(stripe_mask, np.full(n, -1))
    if oracle:
        host = buf.cpu().numpy()
        at = off + obj[flips.stripe] * pitch + flips.shard * S + flips.pos
        assert np.unique(at).size == at.size
        host[at] ^= flips.val
        want = L.oracle_where(Stripes(k, m, S, n, off, pitch), [host], present)
        assert np.array_equal(want[ctrl], want_clean[ctrl])
        names_want[obj] = flips.names
        ask = names_want == ORACLE_NAME
        names_want[ask] = decode_all(k, m, M.arr, stripe_mask[ask], want[ask])
        # include/hbec.h: at r >= 3 two corrupt shards are never attributed to one
        assert np.all(names_want[ask & (M.R[stripe_mask] >= 3)] == N.LOC_MULTIPLE)
    else:
        assert flips.single
        one = np.full(n, -1, np.int64)
        one[obj] = flips.shard
        want = M.words(stripe_mask, one)
        names_want = M.names(stripe_mask, one) if flips.names is None else names_want
    flag_want = (np.where(want & BAD, 1, 0) | np.where(exactly_k, 2, 0)).astype(np.int32)
    if route != "kernel":
        # include/hbec.h: every non-empty entry of the other route gets LOC_SKIPPED, exactly-k ones too
        want_clean = np.full(n, SKIPPED, np.uint32)
        want = want_clean
        names_want = np.full(n, N.LOC_UNCHECKED, np.int64)

    def describe(stripes, got, expect):
        out = []
        for o in stripes:
            c = flip_of[o]
            what = ("control",) if c < 0 else (int(flips.shard[c]), int(flips.pos[c]), f"{int(flips.val[c]):#04x}")
            out.append((M.masks[stripe_mask[o]],) + what + (f"{int(got[o]):#010x}", f"{int(expect[o]):#010x}"))
        return f"(mask, shard, position, value, got, want): {out}"

    plan = B.StripePlan(RS.New(k, m), stripes=[(buf.data_ptr() + off + o * pitch, S) for o in range(n)])
    head = f"{label} {k}+{m} S={S}"
    got, d = three_calls(label, head, plan, present, buf,
                         lambda: VS.xor_flips(bufs, lay, obj[flips.stripe], flips.shard, flips.pos, flips.val),
                         n, n * -(-S // tile()), want_clean, want, flag_want, route, chunk, describe)
    names = decode_all(k, m, M.arr, stripe_mask, got)
    wrong = np.nonzero(names != names_want)[0]
    assert wrong.size == 0, (f"{head} decode: first (stripe, mask, word, got, want): "
                             f"{[(int(o), M.masks[stripe_mask[o]], hex(int(got[o])), int(names[o]), int(names_want[o])) for o in wrong[:8]]}")
    located = int(np.sum((names_want >= 0)))
    print(f"SWEEP locate-{label} {k}+{m} S={S} masks={len(masks)} R={sorted(set(M.R.tolist()))} stripes={n} "
          f"flips={F} bytes={flips.stripe.size} exactly_k={int(exactly_k.sum())} named={located} "
          f"resident={resident} per call {d}")


# ---- 1. every byte of every role ----------------------------------------------

CASES = VMS.CASES


@pytest.mark.parametrize("label,k,m,masks,want_r,exactly_k", CASES, ids=[c[0] for c in CASES])
def test_every_byte_of_every_role(label, k, m, masks, want_r, exactly_k):
    S = VMS.small_s(k, m)
    masks = masks + [exactly_k]
    sweep(label, k, m, S, masks, flip_set(k, m, S, masks), want_r)


# ---- 2. every tile instance inside every kernel instance ----------------------

TILES_K, TILES_M, TILES_S = 12, 4, W + 37
# R: [parity shards lost only; one data shard lost as well, so that slot 11 is a parity shard]
TILES_MASKS = {
    4: [lose(12, 4)],
    3: [lose(12, 4, 12), lose(12, 4, 5)],
    2: [lose(12, 4, 13, 15), lose(12, 4, 3, 14)],
    1: [lose(12, 4, 12, 14, 15), lose(12, 4, 7, 12, 13)],
}
TILES_EXACTLY_K = lose(12, 4, 0, 6, 12, 15)


def tiles_masks(rmax):
    return [x for r in range(1, rmax + 1) for x in TILES_MASKS[r]] + [TILES_EXACTLY_K]


@pytest.mark.parametrize("rmax", [1, 2, 3, 4])
def test_every_tile_instance_of_every_kernel_instance(rmax):
    k, m, S = TILES_K, TILES_M, TILES_S
    masks = tiles_masks(rmax)
    assert max(sum(x) for x in masks) - k == rmax
    sweep(f"rmax{rmax}", k, m, S, masks, flip_set(k, m, S, masks), set(range(1, rmax + 1)))


# ---- 3. every error value -----------------------------------------------------

# (id, k, m, the mask, its R, an exactly-k mask for the controls)
VALUE_CASES = [
    ("4+2", 4, 2, lose(4, 2), 2, lose(4, 2, 0, 5)),
    ("8+3-one-lost", 8, 3, lose(8, 3, 2), 2, lose(8, 3, 0, 4, 9)),
    ("8+3", 8, 3, lose(8, 3), 3, lose(8, 3, 0, 4, 9)),
    ("12+4", 12, 4, lose(12, 4), 4, lose(12, 4, 0, 6, 12, 15)),
]
VALUE_S = 67


def value_flips(k, m, mask):
    """Every present shard x every e in 1..255 x every byte lane b of a dword:
    `byte ^= e` at 16 lane + 4 d + b, the dword d and the lane cycling."""
    surv, checked, _ = roles(k, m, mask)
    j, e, b = (x.reshape(-1) for x in np.meshgrid(np.array(surv + checked, np.int64), np.arange(1, 256),
                                                  np.arange(4), indexing="ij"))
    d = (e + j) % 4
    lane = (e // 4 + b) % 4
    pos = 16 * lane + 4 * d + b
    assert pos.max() < VALUE_S and np.all(pos % 4 == b)
    for jj in surv + checked:
        for bb in range(4):
            sel = (j == jj) & (b == bb)
            assert set(((pos[sel] % 16) // 4).tolist()) == {0, 1, 2, 3} and set(e[sel].tolist()) == set(range(1, 256))
    return Flips(np.zeros(j.size, np.int64), j, pos, e.astype(np.uint8))


@pytest.mark.parametrize("label,k,m,mask,r,exactly_k", VALUE_CASES, ids=[c[0] for c in VALUE_CASES])
def test_every_error_value(label, k, m, mask, r, exactly_k):
    sweep("values-" + label, k, m, VALUE_S, [mask, exactly_k], value_flips(k, m, mask), {r})


# ---- 4. several bad bytes inside one dword ------------------------------------

def column(i, S):
    """The first byte of a lane's 16-byte column, varied with i over the lanes,
    windows and tiles a stripe of S bytes has.  Whole columns only."""
    T = tile()
    if S < W:
        return 16 * (i % (S // 16))
    assert T + 32 <= S < T + W
    if i % 5 == 4:
        return T + 16 * (i // 5 % 2)  # the second tile
    return (i % 5) * W + 16 * ((7 * i + 3) % 62)


def shard_pairs(k, m, mask):
    """(i, j), i != j: neighbours and opposites among the present shards, and the
    ends of both roles.  Survivor/survivor, survivor/checked (both orders) and
    checked/checked pairs all occur (asserted)."""
    surv, checked, _ = roles(k, m, mask)
    here = surv + checked
    pairs = [(here[a], here[(a + s) % len(here)]) for a in range(len(here)) for s in (1, len(here) // 2)]
    pairs += [(surv[0], checked[-1]), (checked[-1], surv[-1]), (checked[0], checked[1]), (checked[1], checked[0]),
              (surv[-1], surv[0])]
    pairs = list(dict.fromkeys(p for p in pairs if p[0] != p[1]))
    kinds = {(i in surv, j in surv) for i, j in pairs}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    return pairs


def dword_flips(k, m, mask, S):
    """(a) four bytes of one dword in one shard; (b) two shards at neighbouring
    bytes of one dword; (c) two shards in two lanes of a window, in two windows,
    in two tiles; (d) two shards at one position, at every byte lane: a syndrome
    that is a multiple of no column (r >= 3), or of any (r = 2: the oracle's
    word).  Positions are chosen by p % 16, the byte of the lane's column."""
    surv, checked, _ = roles(k, m, mask)
    rng = np.random.default_rng(17 * k + m + S)
    T = tile()
    stripe, shard, pos, val, names = [], [], [], [], []
    kinds = {}

    def add(changes, name, kind):
        f = len(names)
        for sh, p, v in changes:
            assert 0 <= p < S and 1 <= v <= 255
            stripe.append(f)
            shard.append(sh)
            pos.append(p)
            val.append(v)
        names.append(name)
        kinds[kind] = kinds.get(kind, 0) + 1

    i = 0
    for j in surv + checked:  # (a)
        for d in range(4):
            p = column(i, S) + 4 * d
            assert p % 16 == 4 * d
            vals = rng.choice(255, size=4, replace=False) + 1
            add([(j, p + b, int(vals[b])) for b in range(4)], j, "a")
            i += 1
    pairs = shard_pairs(k, m, mask)
    for a, c in [(a, c) for a in surv + checked for c in surv + checked if a != c]:  # (b): every ordered pair
        for b in range(3):
            p = column(i, S) + 4 * (i % 4) + b
            assert p % 4 == b and (p + 1) % 16 // 4 == p % 16 // 4
            add([(a, p, int(rng.integers(1, 256))), (c, p + 1, int(rng.integers(1, 256)))], N.LOC_MULTIPLE, "b")
            i += 1
    for a, c in pairs:  # (c)
        two = [("lanes", 16 * (i % 2), 16 * (2 + i // 2 % 2))] if S < W else [
            ("lanes", (i % 4) * W + 16 * (i % 30), (i % 4) * W + 16 * (i % 30 + (1, 16, 32)[i % 3])),
            ("windows", (i % 2) * W + 16 * (i % 62), (2 + i // 2 % 2) * W + 16 * ((5 * i) % 62)),
            ("tiles", (i % 4) * W + 16 * ((3 * i) % 62), T + 16 * (i % 2))]
        for kind, c1, c2 in two:
            p1, p2 = c1 + (5 * i) % 16, c2 + (11 * i + 3) % 16
            assert p1 // 16 != p2 // 16
            if kind == "lanes":
                assert p1 // W == p2 // W and p1 // T == p2 // T
            if kind == "windows":
                assert p1 // W != p2 // W and p1 // T == p2 // T
            if kind == "tiles":
                assert p1 // T != p2 // T
            add([(a, p1, int(rng.integers(1, 256))), (c, p2, int(rng.integers(1, 256)))], N.LOC_MULTIPLE, "c-" + kind)
            i += 1
    for a, c in pairs:  # (d)
        for b in range(4):
            p = column(i, S) + 4 * (i // 4 % 4) + b
            assert p % 4 == b
            add([(a, p, int(rng.integers(1, 256))), (c, p, int(rng.integers(1, 256)))], ORACLE_NAME, "d")
            i += 1
    assert set(kinds) == {"a", "b", "c-lanes", "d"} | (set() if S < W else {"c-windows", "c-tiles"}), kinds
    return Flips(np.zeros(len(names), np.int64), shard, pos, val, stripe=stripe, names=names), kinds


@pytest.mark.parametrize("big", [False, True], ids=["S67", "T+37"])
@pytest.mark.parametrize("label,k,m,mask,r,exactly_k", VALUE_CASES, ids=[c[0] for c in VALUE_CASES])
def test_several_bad_bytes_in_one_dword(label, k, m, mask, r, exactly_k, big):
    S = tile() + 37 if big else VALUE_S
    flips, kinds = dword_flips(k, m, mask, S)
    print(f"SWEEP locate-dword-{label} S={S} stripes per kind {kinds}")
    sweep("dword-" + label, k, m, S, [mask, exactly_k], flips, {r}, oracle=True)


# ---- 5. every length ----------------------------------------------------------

@pytest.mark.parametrize("k,m,lost_a,flip_a,lost_b,flip_b", [(8, 3, 10, 9, 3, 2), (4, 4, 7, 6, 2, 1)],
                         ids=["8+3", "4+4"])
def test_every_length(k, m, lost_a, flip_a, lost_b, flip_b):
    """Three stripes per length S = 1 .. T + 992 + 64: mask A flipped at S - 1
    of checked shard flip_a (the next shard in memory, lost_a, is garbage), a
    control (mask A for even S, B for odd), mask B flipped at S - 1 of survivor
    flip_b (the next shard, lost_b, is garbage).  A partial-word mask of the
    cold path one byte short leaves LOC_BAD alone; one byte long, the garbage
    byte at S rules everybody out."""
    L_ = k + m
    top = tile() + W + 64
    mask_a, mask_b = lose(k, m, lost_a), lose(k, m, lost_b)
    M = Masks(k, m, [mask_a, mask_b])
    assert flip_a in roles(k, m, mask_a)[1] and lost_a == flip_a + 1
    assert flip_b in roles(k, m, mask_b)[0] and lost_b == flip_b + 1
    assert np.all(M.R >= 2)
    cw = VS.codeword(k, m, top, 97 * k + m).reshape(L_, top)  # a prefix of a codeword is a codeword
    rng = np.random.default_rng(5 * k + m)
    n = 3 * top
    S = np.repeat(np.arange(1, top + 1, dtype=np.int64), 3)
    kind = np.tile(np.array([0, 1, 2]), top)
    use_b = (kind == 2) | ((kind == 1) & (S % 2 == 1))
    assert (np.diff(use_b.astype(np.int64)) != 0).sum() >= n // 4
    base = np.empty(n, np.int64)
    cur = 0
    for q in range(n):  # at least 5 slack bytes, then up to the alignment q % 16
        o = cur + 5
        o += (q - o) % 16
        base[q] = o
        cur = o + L_ * int(S[q])
    total = cur + 11
    assert 2 * total <= VS.CAP
    host = np.full(total, VS.FILL, np.uint8)
    for s in range(1, top + 1):
        row = np.ascontiguousarray(cw[:, :s]).reshape(-1)
        for q in range(3 * (s - 1), 3 * s):
            g = lost_b if use_b[q] else lost_a
            at = int(base[q])
            host[at:at + L_ * s] = row
            host[at + g * s:at + (g + 1) * s] ^= rng.integers(1, 256, s, dtype=np.uint8)  # garbage, every byte
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    for kd in (0, 2):
        assert set((base[kind == kd] % 16).tolist()) == set(range(16))  # all 16 alignments, both flips
    which = use_b.astype(np.int64)
    present = M.arr[which]
    fshard = np.where(kind == 0, flip_a, flip_b)
    flipped = kind != 1
    idx = torch.from_numpy((base + fshard * S + S - 1)[flipped]).cuda()
    bits = VMS.bit(S - 1, fshard)
    val = torch.from_numpy(bits[flipped]).cuda()
    want = M.words(which, np.where(flipped, fshard, -1))
    assert np.all(want[flipped] & BAD) and not want[~flipped].any()
    plan = B.StripePlan(RS.New(k, m), stripes=[(buf.data_ptr() + int(b), int(s)) for b, s in zip(base, S)])

    def flip_in():
        buf[idx] = buf[idx] ^ val

    def describe(stripes, got, expect):
        return (f"(S, kind, base mod 16, mask, shard, position, value, got, want): "
                f"{[(int(S[i]), int(kind[i]), int(base[i] % 16), M.masks[which[i]], int(fshard[i]), int(S[i] - 1), f'{int(bits[i]):#04x}', f'{int(got[i]):#010x}', f'{int(expect[i]):#010x}') for i in stripes]}")

    n_tiles = int(np.sum(-(-S // tile())))
    got, d = three_calls("every-length", f"every-length {k}+{m}", plan, present, buf, flip_in, n, n_tiles,
                         np.zeros(n, np.uint32), want, flipped.astype(np.int32), "kernel", 0, describe)
    names = decode_all(k, m, M.arr, which, got)
    assert np.array_equal(names, np.where(flipped, fshard, N.LOC_CLEAN))
    print(f"SWEEP locate-every-length {k}+{m} S=1..{top} R={sorted(set(M.R.tolist()))} stripes={n} "
          f"flips={int(flipped.sum())} resident={2 * total} per call {d}")


# ---- 6. chunked launches, 7. the other route ----------------------------------

def test_chunked_launches_4_2():
    label, k, m, masks, want_r, exactly_k = CASES[2]
    assert (k, m) == (4, 2)
    S = VMS.small_s(k, m)
    masks = masks + [exactly_k]
    sweep("chunked-" + label, k, m, S, masks, flip_set(k, m, S, masks), want_r, chunk=3)


def test_other_route_13_2():
    """k > 12: the call has no per-stripe fallback.  Every stripe, exactly-k ones
    included, gets LOC_SKIPPED and is counted; nothing is launched."""
    k, m, S = 13, 2, 301
    masks = [lose(k, m, 4), lose(k, m, 13), lose(k, m, 0, 14)]
    q, shard, pos, val = VMS.flip_set(k, m, S, masks)
    sweep("other-route", k, m, S, masks, Flips(q, shard, pos, val), {1}, route="other")


# ---- 8. the masks give the roles the cases name (host only) -------------------

def test_cases_cover_what_they_name():
    by = {c[0]: c for c in CASES}
    # slot 9 (the s_hi word) a parity shard, flipped at every byte of a column
    s, c, _ = roles(10, 4, by["10+4"][3][0])
    assert s[8:] == [9, 10] and c == [11, 12, 13]
    s, c, _ = roles(12, 4, by["12+4"][3][0])
    assert len(s) == 12 and c == [12, 13, 14, 15]
    s, c, _ = roles(12, 4, by["12+4"][3][1])
    assert s[5:] == [6, 7, 8, 9, 10, 11, 12] and c == [14, 15]  # slot 11 a parity shard, R = 2
    assert {r for c in CASES for r in c[4]} == {1, 2, 3, 4}
    # every tile instance R inside every kernel instance RMAX
    pairs = set()
    for rmax in (1, 2, 3, 4):
        masks = tiles_masks(rmax)
        counts = [sum(x) - TILES_K for x in masks]
        assert max(counts) == rmax and min(counts) == 0
        pairs |= {(r, rmax) for r in counts if r}
        for r in range(1, min(rmax, 3) + 1):  # both kinds of mask with r checked shards
            slot11 = {roles(TILES_K, TILES_M, x)[0][11] for x in TILES_MASKS[r]}
            assert 11 in slot11 and any(s >= TILES_K for s in slot11), (r, slot11)
    assert pairs == {(r, rmax) for rmax in (1, 2, 3, 4) for r in range(1, rmax + 1)} and len(pairs) == 10
    assert roles(TILES_K, TILES_M, TILES_MASKS[4][0])[0][11] == 11
    for r, masks in TILES_MASKS.items():
        assert all(len(roles(TILES_K, TILES_M, x)[1]) == r for x in masks)
    # the value and dword shapes: R = 2, 2, 3, 4; 8+3 with one lost: slot 7 is parity 8
    assert [c[4] for c in VALUE_CASES] == [2, 2, 3, 4]
    for _, k, m, mask, r, ek in VALUE_CASES:
        assert len(roles(k, m, mask)[1]) == r and sum(ek) == k
        shard_pairs(k, m, mask)
    assert roles(8, 3, VALUE_CASES[1][3])[0][7] == 8
    # slot(p, k) unties the slot from the byte lane where p % k ties them
    for k in (4, 8, 12):
        P = np.arange(4 * W)
        assert all(len(set((P[P % k == t] % 4).tolist())) == 1 for t in range(k))
        assert all(set((P[slot(P, k) == t] % 16).tolist()) == set(range(16)) for t in range(k))
