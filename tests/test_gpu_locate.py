"""hbec_locate_plan_mixed: which shard of each inconsistent stripe of a plan is
the corrupt one, in one call (csrc/locate.hip, behind plan.locate_mixed).

Expected words never come from the product.  Per stripe the oracle takes the
first k present shards as survivors, computes the syndrome of every checked
shard with oracle.coracle.apply on oracle.lagrange.lagrange_row(survivors, c)
XORed with the stored bytes, and for every non-zero byte position searches the
candidates by brute force: the present shards j for which some e in 1..255 gives
oracle.MUL[e][column_j] == syndrome.  Every present shard but the candidates is
ruled out.  Comparisons are exact equality of whole `where` arrays.  Buffers and
layouts are test_gpu_mixed_plan.Case's (random slack, odd offsets), sizes and
flip positions test_gpu_verify_mixed's.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_mixed_plan as MP
import test_gpu_verify_mixed as VM
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LAYOUTS = MP.LAYOUTS
W = VM.W
U32P = C.POINTER(C.c_uint32)
BAD, SKIPPED, NOTHING = N.LOC_BAD, N.LOC_SKIPPED, N.LOC_NOTHING


def tile():
    t = B.locate_plan_tile_bytes()
    assert t == VM.tile() == 4 * W
    return t


# ---- the oracle ----

def candidates(cols, s):
    """Bit j for every (shard j, column) with e * column == s for some e in 1..255."""
    cand = 0
    for j, col in cols:
        ok = np.ones(255, bool)
        for q, cq in enumerate(col):
            ok &= O.MUL[1:, cq] == s[q]
        if ok.any():
            cand |= 1 << j
    return cand


def oracle_where(c, bufs, present, examined=None):
    """The words one call must OR in, from the oracle alone.  examined: per entry,
    whether the filter lets it through (None: all)."""
    k, n = c.k, c.k + c.m
    want = np.zeros(len(c.sizes), np.uint32)
    for e in c.live:
        s, where = c.sizes[e], c.shards[e]
        here = [i for i in range(n) if present[e][i]]
        surv, checked = here[:k], here[k:]
        if not checked:
            want[e] = NOTHING
            continue
        if examined is not None and not examined[e]:
            continue
        rows = [VM.lagrange_row(tuple(surv), ch) for ch in checked]
        data = [bufs[b][o:o + s] for b, o in (where[i] for i in surv)]
        synd = np.stack([implied ^ bufs[where[ch][0]][where[ch][1]:where[ch][1] + s]
                         for ch, implied in zip(checked, CO.apply(rows, data))])
        bad = np.nonzero(synd.any(axis=0))[0]
        if bad.size == 0:
            continue
        word = BAD
        if len(checked) >= 2:
            pbits = sum(1 << i for i in here)
            cols = [(j, [int(rows[q][t]) for q in range(len(checked))]) for t, j in enumerate(surv)]
            cols += [(j, [1 if q == p else 0 for q in range(len(checked))]) for p, j in enumerate(checked)]
            for vec in np.unique(synd[:, bad], axis=1).T:
                word |= pbits & ~candidates(cols, [int(x) for x in vec])
        want[e] = word
    return want


def zeros_like_case(c, prefill=0):
    return torch.from_numpy(np.full(len(c.sizes), prefill, np.uint32).view(np.int32)).cuda()


def words(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32).copy()


def locate(c, bufs, present, flags=None, prefill=0):
    """One call over `bufs`; returns (where, tensors, plan)."""
    enc = RS.New(c.k, c.m)
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    where = zeros_like_case(c, prefill)
    torch.cuda.synchronize()
    plan.locate_mixed(present, where, flags=flags)
    torch.cuda.synchronize()
    return words(where), t, plan


def corrupt(c, bufs, e, shard, pos, value):
    b, o = c.shards[e][shard]
    assert 0 <= pos < c.sizes[e] and value
    bufs[b][o + pos] ^= value


def culprits(c, bufs, present):
    """Per live entry, the present shards whose bytes differ from the clean codeword."""
    out = {}
    for e in c.live:
        s = c.sizes[e]
        out[e] = [i for i, (b, o) in enumerate(c.shards[e])
                  if present[e][i] and not np.array_equal(bufs[b][o:o + s], c.bufs[b][o:o + s])]
    return out


def n_checked(c, present, e):
    return int(np.sum(np.asarray(present[e]) != 0)) - c.k


def decode(c, present, where):
    return B.locate_decode(c.k, c.m, present, where)


# ---- 1. clean codewords ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4), (10, 4), (3, 1), (2, 2)])
def test_clean_codewords_say_nothing(k, m, layout):
    if (k, m) in ((4, 2), (8, 3)):
        masks = VM.masks_up_to(k + m, m)  # every mask with >= k present
        assert len(masks) == {6: 22, 11: 232}[k + m]
    else:
        masks = VM.random_masks(k, m, 40, k) + [[1] * (k + m)]
    c = VM.case(k, m, layout, len(masks))
    assert len(c.live) >= len(masks)
    present = MP.spread(c, masks, 1)
    assert {tuple(present[e]) for e in c.live} == {tuple(x) for x in masks}
    inp, _ = c.garble(present, seed=2)  # garbage in every missing shard
    want = oracle_where(c, inp, present)
    exactly_k = np.array([NOTHING if s and n_checked(c, present, e) == 0 else 0 for e, s in enumerate(c.sizes)],
                         np.uint32)
    assert np.array_equal(want, exactly_k)
    s0 = B.locate_plan_stats()
    got, t, _ = locate(c, inp, present)
    s1 = B.locate_plan_stats()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    MP.check_equal(t, inp)  # read-only, slack included
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1 and s1["skipped_entries"] == s0["skipped_entries"]
    names = decode(c, present, got)
    for e, s in enumerate(c.sizes):
        assert names[e] == (N.LOC_UNCHECKED if exactly_k[e] else N.LOC_CLEAN)


def test_present_none_means_every_shard():
    c = VM.case(4, 2, "stripes")
    bufs = [x.copy() for x in c.bufs]
    e = c.live[3]
    corrupt(c, bufs, e, 2, c.sizes[e] - 1, 0x40)
    enc = RS.New(4, 2)
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    where = zeros_like_case(c)
    plan.locate_mixed(None, where)
    torch.cuda.synchronize()
    full = np.ones((len(c.sizes), 6), np.uint8)
    assert np.array_equal(words(where), oracle_where(c, bufs, full))
    assert B.locate_decode(4, 2, None, words(where))[e] == 2


# ---- 2. one flipped bit, one shard ----

NAMES = ["0", "1", "15", "16", "S-17", "S-2", "S-1", "W-1", "W", "T-1", "T", "byte"]


def masks_by_checked(k, m):
    by_r = {}
    for mask in VM.masks_up_to(k + m, m):
        by_r.setdefault(sum(mask) - k, []).append(mask)
    return by_r


def flipped(c, flips, present, in_missing):
    """Buffers with one bit flipped per listed stripe.  in_missing: in a shard its
    mask (already in `present`) calls missing.  Otherwise the stripe gets a mask
    (three of four flips one with two or more checked shards, the fourth one
    with a single checked shard) and per (position name, count of checked) the
    present shards are flipped in turn.  Returns (bufs, {entry: shard},
    {(role, name)} covered under masks with r >= 2)."""
    k, m, n = c.k, c.m, c.k + c.m
    by_r = masks_by_checked(k, m)
    many = [mk for r in sorted(by_r) if r >= 2 for mk in by_r[r]]
    one = by_r[1]
    bufs = [x.copy() for x in c.bufs]
    hit, roles, turn = {}, set(), {}
    for q, (e, p, names) in enumerate(flips):
        names = names or ("byte",)
        if in_missing:
            gone = [i for i in range(n) if not present[e][i]]
            i = gone[q % len(gone)]
        else:
            single = q % 4 == 3
            present[e] = one[(q // 4) % len(one)] if single else many[(q - q // 4) % len(many)]
            here = [j for j in range(n) if present[e][j]]
            key = (names[0], single)
            role = turn.get(key, 0) % len(here)
            turn[key] = role + 1
            i = here[role]
            if not single:
                roles |= {(role if role < k else ("checked", role - k), nm) for nm in names}
        hit[e] = i
        corrupt(c, bufs, e, i, p, 1 << (q % 8))
    return bufs, hit, roles


def check_flips(k, m, layout):
    c, flips = VM.flip_case(k, m, layout)
    n = k + m
    flip_entries = {e for e, _, _ in flips}
    assert len(c.live) == 2 * len(flips) and c.sizes.count(0) == 4
    for s in VM.SMALL + [W - 1, W, W + 1, tile() - 1, tile(), tile() + 1, 2 * tile() + 17]:
        assert s in c.sizes
    # (a) flips in present shards
    anym = VM.masks_up_to(n, m)
    present = np.ones((len(c.sizes), n), np.uint8)
    for q, e in enumerate(c.live):
        present[e] = anym[(7 * q + 2) % len(anym)]
    bufs, hit, roles = flipped(c, flips, present, in_missing=False)
    # every role at every named position under two or more checked shards (checked
    # q exists in some mask for q < m; the last one only with every shard present)
    for role in list(range(k)) + [("checked", q) for q in range(2)]:
        for nm in NAMES:
            assert (role, nm) in roles, (role, nm)
    assert culprits(c, bufs, present) == {e: ([hit[e]] if e in hit else []) for e in c.live}
    want = oracle_where(c, bufs, present)
    assert {e for e in c.live if want[e] & BAD} == flip_entries  # exactly the flipped stripes
    got, t, _ = locate(c, bufs, present)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    MP.check_equal(t, bufs)
    names = decode(c, present, got)
    seen = set()
    for e in c.live:
        r = n_checked(c, present, e)
        if e not in hit:
            assert names[e] == (N.LOC_CLEAN if r else N.LOC_UNCHECKED)
        elif r >= 2:
            assert names[e] == hit[e], (e, present[e], hit[e], hex(got[e]))
            seen.add(r)
        else:
            assert r == 1 and names[e] == N.LOC_AMBIGUOUS and got[e] == BAD
            seen.add(r)
    assert seen == set(range(1, m + 1))
    # (b) the same flips in missing shards change nothing
    lossy = VM.masks_up_to(n, m, lost_min=1)
    for q, e in enumerate(c.live):
        present[e] = lossy[(5 * q + 1) % len(lossy)] if e in flip_entries else anym[(7 * q + 2) % len(anym)]
    bufs, _, _ = flipped(c, flips, present, in_missing=True)
    want = oracle_where(c, bufs, present)
    assert not (want & BAD).any()
    got, _, _ = locate(c, bufs, present)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_single_bit_flips_name_exactly_their_shard(k, m, layout):
    check_flips(k, m, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_checked_shard_is_ambiguous_3_1(layout):
    """3+1: r = 1 whenever anything can be checked."""
    k, m = 3, 1
    c = VM.case(k, m, layout)
    present = np.ones((len(c.sizes), 4), np.uint8)
    bufs = [x.copy() for x in c.bufs]
    hit = {}
    for q, e in enumerate(c.live):
        if q % 2:
            continue
        hit[e] = q // 2 % 4
        pos = [0, c.sizes[e] - 1, c.sizes[e] // 2][q // 2 % 3]
        corrupt(c, bufs, e, hit[e], pos, 1 << (q % 8))
    want = oracle_where(c, bufs, present)
    assert set(want.tolist()) == {0, BAD} and {e for e in c.live if want[e]} == set(hit)
    got, _, _ = locate(c, bufs, present)
    assert np.array_equal(got, want)
    names = decode(c, present, got)
    assert all(names[e] == (N.LOC_AMBIGUOUS if e in hit else N.LOC_CLEAN) for e in c.live)


# ---- 3. many bad bytes in one shard ----

@functools.lru_cache(maxsize=None)
def long_case(k, m, layout):
    T = tile()
    sizes = [0, 2 * T + 17, 65, 9 * T + 5, T + 1, 0, 5 * T - 1, W + 1, 3 * T, 0]
    return MP.Case(k, m, layout, sizes, 900 + k)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4)])
def test_many_bad_bytes_in_one_shard_keep_the_culprit(k, m, layout):
    n = k + m
    c = long_case(k, m, layout)
    rng = np.random.default_rng(30 + k)
    masks = [mk for r, ms in masks_by_checked(k, m).items() if r >= 2 for mk in ms] if n <= 11 else [[1] * n]
    present = np.ones((len(c.sizes), n), np.uint8)
    bufs = [x.copy() for x in c.bufs]
    hit = {}
    for q, e in enumerate(c.live):
        present[e] = masks[q % len(masks)]
        here = [i for i in range(n) if present[e][i]]
        hit[e] = here[(3 * q + 1) % len(here)]
        s = c.sizes[e]
        # spread over every tile and over lanes, first and last byte included
        pos = {0, s - 1} | {int(x) for x in rng.integers(0, s, min(s, 40 + s // 500))}
        for p in pos:
            corrupt(c, bufs, e, hit[e], p, int(rng.integers(1, 256)))
        assert len({p // tile() for p in pos}) == -(-s // tile())
    want = oracle_where(c, bufs, present)
    got, t, _ = locate(c, bufs, present)
    assert np.array_equal(got, want), (got, want)
    MP.check_equal(t, bufs)
    names = decode(c, present, got)
    assert {e: int(names[e]) for e in c.live} == hit


# ---- 4. two corrupt shards ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m,same", [(4, 2, False), (8, 3, False), (8, 3, True), (12, 4, False), (12, 4, True)])
def test_two_corrupt_shards_are_multiple(k, m, same, layout):
    n = k + m
    c = long_case(k, m, layout)
    rng = np.random.default_rng(40 + k)
    present = np.ones((len(c.sizes), n), np.uint8)
    bufs = [x.copy() for x in c.bufs]
    for q, e in enumerate(c.live):
        j1, j2 = [int(x) for x in rng.choice(n, size=2, replace=False)]
        if q == 0:
            j1, j2 = 0, n - 1  # a survivor and the last checked shard
        s = c.sizes[e]
        p1 = int(rng.integers(s))
        p2 = p1 if same else (p1 + 1 + int(rng.integers(s - 1))) % s
        corrupt(c, bufs, e, j1, p1, int(rng.integers(1, 256)))
        corrupt(c, bufs, e, j2, p2, int(rng.integers(1, 256)))
    want = oracle_where(c, bufs, present)
    assert all(want[e] == BAD | ((1 << n) - 1) for e in c.live)  # provable: nobody is left
    got, _, _ = locate(c, bufs, present)
    assert np.array_equal(got, want), (got, want)
    assert all(x == N.LOC_MULTIPLE for x in decode(c, present, got)[c.live])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_corrupt_shards_at_one_position_4_2_equal_the_oracle_word(layout):
    """Distance 3: the word may name a third shard, and must be the oracle's."""
    k, m, n = 4, 2, 6
    c = VM.case(k, m, layout, 60)
    rng = np.random.default_rng(45)
    present = np.ones((len(c.sizes), n), np.uint8)
    bufs = [x.copy() for x in c.bufs]
    for e in c.live:
        j1, j2 = [int(x) for x in rng.choice(n, size=2, replace=False)]
        p = int(rng.integers(c.sizes[e]))
        corrupt(c, bufs, e, j1, p, int(rng.integers(1, 256)))
        corrupt(c, bufs, e, j2, p, int(rng.integers(1, 256)))
    want = oracle_where(c, bufs, present)
    assert all(want[e] & BAD for e in c.live)
    got, _, _ = locate(c, bufs, present)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


# ---- 5. the filter ----

def corrupt_every_other(c, present, seed):
    """One corrupt byte in a present shard of every second live stripe."""
    rng = np.random.default_rng(seed)
    n = c.k + c.m
    bufs, _ = c.garble(present, seed=seed)
    hit = {}
    for e in c.live[::2]:
        here = [i for i in range(n) if present[e][i]]
        hit[e] = here[int(rng.integers(len(here)))]
        corrupt(c, bufs, e, hit[e], int(rng.integers(c.sizes[e])), int(rng.integers(1, 256)))
    return bufs, hit


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_filter_reads_only_flagged_entries(k, m, layout):
    n = k + m
    c = VM.case(k, m, layout, 60)
    present = MP.spread(c, VM.masks_up_to(n, m), 50)
    bufs, hit = corrupt_every_other(c, present, 51)
    full = oracle_where(c, bufs, present)
    bad = [e for e in c.live if full[e] & BAD]
    assert len(bad) > 10 and any(full[e] & NOTHING for e in c.live)
    # a hand-made flags tensor: half of the corrupt stripes (other bits are not the filter)
    chosen = set(bad[::2])
    hand = np.array([(1 if e in chosen else 0) | (2 if e % 3 == 0 else 0) | (4 if e % 5 == 0 else 0)
                     for e in range(len(c.sizes))], np.int32)
    flags = torch.from_numpy(hand).cuda()
    want = oracle_where(c, bufs, present, examined=hand & 1)
    assert all(want[e] == (full[e] if e in chosen else 0) for e in bad)
    got, t, plan = locate(c, bufs, present, flags=flags)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert np.array_equal(flags.cpu().numpy(), hand)  # read, never written
    # verify_mixed -> locate_mixed(flags=...) equals the unfiltered call
    vflags = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    plan.verify_mixed(present, vflags)
    where = zeros_like_case(c)
    plan.locate_mixed(present, where, flags=vflags)
    torch.cuda.synchronize()
    assert np.array_equal(vflags.cpu().numpy().astype(np.uint32), VM.oracle_flags(c, bufs, present))
    assert np.array_equal(words(where), full)
    MP.check_equal(t, bufs)
    with pytest.raises(ValueError):
        plan.locate_mixed(present, where, flags=where)  # aliasing
    with pytest.raises(ValueError):
        plan.locate_mixed(present, where[:-1])
    with pytest.raises(ValueError):
        plan.locate_mixed(present, where, flags=torch.zeros(len(c.sizes), dtype=torch.int64, device="cuda"))


# ---- 6. OR semantics and launches ----

@pytest.mark.parametrize("dtype", [torch.int32, torch.uint32])
def test_where_is_ored_into_what_the_caller_had(dtype):
    k, m = 4, 2
    c = VM.case(k, m, "stripes", 30)
    present = MP.spread(c, VM.masks_up_to(6, 2), 60)
    bufs, _ = corrupt_every_other(c, present, 61)
    pre = 0x10000 | (1 << 28) | 0x8  # a bit of the mask and two the call never sets
    enc = RS.New(k, m)
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    where = zeros_like_case(c, pre).view(dtype)
    plan.locate_mixed(present, where)
    torch.cuda.synchronize()
    want = oracle_where(c, bufs, present) | np.uint32(pre)
    assert np.array_equal(words(where), want)
    assert all(want[e] == pre for e, s in enumerate(c.sizes) if s == 0)
    assert (want & BAD).any() and (want & NOTHING).any()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_launch_boundaries_anywhere_in_the_tile_list(layout):
    k, m = 4, 2
    c = VM.case(k, m, layout, 22)
    present = MP.spread(c, VM.masks_up_to(6, 2), 62)
    bufs, _ = corrupt_every_other(c, present, 63)
    want = oracle_where(c, bufs, present)
    n_tiles = sum(-(-s // tile()) for s in c.sizes)
    assert n_tiles > 70
    for chunk in (1, 3):
        B.set_locate_plan_chunk_tiles(chunk)
        try:
            s0 = B.locate_plan_stats()
            got, _, _ = locate(c, bufs, present)
            s1 = B.locate_plan_stats()
        finally:
            B.set_locate_plan_chunk_tiles(0)
        assert np.array_equal(got, want), chunk
        assert s1["kernel_launches"] - s0["kernel_launches"] == -(-n_tiles // chunk)


def test_launches_do_not_depend_on_stripes_or_masks():
    k, m = 4, 2
    small, large = VM.case(k, m, "stripes", 40), VM.case(k, m, "stripes", 400)
    assert len(small.live) < 100 and len(large.live) >= 400
    masks = VM.masks_up_to(6, 2)
    d = []
    for c, ms in ((small, masks[1:2]), (small, masks), (large, masks[1:2]), (large, masks)):
        present = MP.spread(c, ms, 3)
        bufs, _ = corrupt_every_other(c, present, 64)
        s0 = B.locate_plan_stats()
        got, _, _ = locate(c, bufs, present)
        s1 = B.locate_plan_stats()
        assert np.array_equal(got, oracle_where(c, bufs, present))
        assert s1["skipped_entries"] == s0["skipped_entries"]
        d.append(s1["kernel_launches"] - s0["kernel_launches"])
    assert d == [1, 1, 1, 1]


# ---- 7. the other route ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(13, 2), (4, 5)])
def test_other_route_is_skipped_and_counted(k, m, layout):
    n = k + m
    sizes = [0, 17, 1, 4097, 1985, 0, 10_001, 33, 64, 993, 31, 3969, 15, 65, 0]
    c = MP.Case(k, m, layout, sizes, 70 + k)
    assert len(c.live) == 12
    rng = np.random.default_rng(71)
    present = np.ones((len(sizes), n), np.uint8)
    for e, lost in zip(c.live, [1, 2, 0, m, 1, 2, 0, m, 1, 2, 1, 2]):
        present[e][rng.choice(n, size=lost, replace=False)] = 0
    bufs, _ = c.garble(present)
    for e in c.live[::2]:
        corrupt(c, bufs, e, [i for i in range(n) if present[e][i]][0], 0, 0x21)
    want = np.array([SKIPPED if s else 0 for s in sizes], np.uint32)
    s0 = B.locate_plan_stats()
    got, t, _ = locate(c, bufs, present)
    s1 = B.locate_plan_stats()
    assert np.array_equal(got, want), (got, want)
    MP.check_equal(t, bufs)
    assert s1["skipped_entries"] - s0["skipped_entries"] == 12
    assert s1["kernel_launches"] == s0["kernel_launches"]
    assert all(x == N.LOC_UNCHECKED for x in decode(c, present, got)[c.live])


# ---- 8. errors leave no trace ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_errors_leave_no_trace(layout):
    k, m = 4, 2
    c = VM.case(k, m, layout)
    enc = RS.New(k, m)
    n = len(c.sizes)
    present = MP.spread(c, VM.masks_up_to(6, 2), 80)
    bufs, _ = corrupt_every_other(c, present, 81)
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    where = torch.zeros(n, dtype=torch.int32, device="cuda")
    pats, idx = np.unique(present, axis=0, return_inverse=True)
    pats = np.ascontiguousarray(pats, np.uint8)
    idx = np.ascontiguousarray(idx.reshape(-1), np.uint32)

    def call(p, i, n_patterns=None, e=enc, flags=None, out=where):
        return N.lib().hbec_locate_plan_mixed(e.handle, plan._h, p.ctypes.data_as(N._U8P),
                                              p.shape[0] if n_patterns is None else n_patterns,
                                              i.ctypes.data_as(U32P), flags,
                                              None if out is None else C.c_void_p(out.data_ptr()), None)

    s0 = B.locate_plan_stats()
    assert call(pats, idx, e=RS.New(8, 3)) == N.ERR_INVALID_ARG
    bad = idx.copy()
    bad[n - 1] = pats.shape[0]  # the last entry is zero-length: checked all the same
    assert c.sizes[n - 1] == 0
    assert call(pats, bad) == N.ERR_INVALID_ARG and "index" in N.last_error()
    few = np.vstack([pats, np.array([[1, 1, 1, 0, 0, 0]], np.uint8)])  # listed, unused
    assert call(few, idx) == N.ERR_TOO_FEW_SHARDS
    assert call(pats, idx, n_patterns=0) == N.ERR_INVALID_ARG
    assert call(pats, idx, n_patterns=65537) == N.ERR_INVALID_ARG
    assert call(pats, idx, out=None) == N.ERR_INVALID_ARG
    assert call(pats, idx, flags=C.c_void_p(where.data_ptr())) == N.ERR_INVALID_ARG and "alias" in N.last_error()
    torch.cuda.synchronize()
    assert B.locate_plan_stats() == s0
    assert not where.cpu().numpy().any()
    assert call(pats, idx) == N.HBEC_OK
    torch.cuda.synchronize()
    want = oracle_where(c, bufs, present)
    assert np.array_equal(words(where), want) and (want & BAD).any()
    MP.check_equal(t, bufs)


# ---- 9. repair end to end ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (10, 4)])
def test_verify_locate_reconstruct_repairs_the_plan(k, m, layout):
    n = k + m
    c = VM.case(k, m, layout, 40)
    rng = np.random.default_rng(90 + k)
    # some stripes already miss shards; those about to be corrupted (every third)
    # never so many that fewer than 2 are checked, no stripe all of its spares
    present = np.ones((len(c.sizes), n), np.uint8)
    for q, e in enumerate(c.live):
        lost = (q // 3) % (m - 1) if q % 3 == 0 else q % m
        present[e][rng.choice(n, size=lost, replace=False)] = 0
    bufs, _ = c.garble(present, seed=91)
    hit = {}
    for e in c.live[::3]:
        here = [i for i in range(n) if present[e][i]]
        hit[e] = here[int(rng.integers(len(here)))]
        s = c.sizes[e]
        lo = int(rng.integers(s))
        hi = min(s, lo + 1 + int(rng.integers(300)))
        b, o = c.shards[e][hit[e]]
        bufs[b][o + lo:o + hi] ^= rng.integers(1, 256, hi - lo, dtype=np.uint8)
    enc = RS.New(k, m)
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    flags = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    where = zeros_like_case(c)
    plan.verify_mixed(present, flags)
    plan.locate_mixed(present, where, flags=flags)
    torch.cuda.synchronize()
    assert set(np.nonzero(flags.cpu().numpy() & 1)[0].tolist()) == set(hit)
    got = words(where)
    assert np.array_equal(got, oracle_where(c, bufs, present))
    names = decode(c, present, got)
    assert {e: int(names[e]) for e in hit} == hit
    assert all(names[e] == N.LOC_CLEAN for e in c.live if e not in hit)
    repaired = present.copy()
    for e in hit:
        repaired[e][names[e]] = 0
    plan.reconstruct_mixed(repaired)
    torch.cuda.synchronize()
    MP.check_equal(t, c.bufs)  # the original codewords, slack included
