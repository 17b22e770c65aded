"""hbec_heal_plan_mixed: the shard hbec_locate_plan_mixed named is rebuilt, with
the missing ones, on the same plan and with nothing copied back.

Expected bytes and flags never come from the product.  The shard a word names
is batch.locate_decode's answer (hbec_locate_decode, host only).  For an entry
with named shard j the oracle clears j in the mask, takes the first k present
shards as survivors, and a rewritten shard is oracle.coracle.apply of
oracle.lagrange.lagrange_row(survivors, shard) on the bytes actually in the
survivor slots; flag bit 0 is a non-zero syndrome of lagrange_row(survivors, c)
for another present shard c, bit 1 says that none is left, HEAL_DONE joins them.
An inconsistent entry with no shard named gets HEAL_UNNAMED and keeps its
bytes; every other entry keeps bytes and flag.  Buffers are laid out by
test_gpu_mixed_plan.Case in both layouts with size_set's sizes; whole buffers,
slack included, and whole flag arrays are compared exactly.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_mixed_plan as MP
import test_gpu_repair_mixed as RG
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

LAYOUTS = MP.LAYOUTS
U32P = C.POINTER(C.c_uint32)
DONE, UNNAMED = N.HEAL_DONE, N.HEAL_UNNAMED


def tile():
    return B.heal_plan_tile_bytes()


@functools.lru_cache(maxsize=None)
def case(k, m, layout, n_live=1):
    return MP.Case(k, m, layout, MP.sizes_for(n_live, 100 * k + m), 7 * k + m + len(layout))


def oracle_heal(c, bufs, present, where):
    """(buffers, flags) one call must leave on zeroed flags, from the oracle alone."""
    k, n = c.k, c.k + c.m
    want = [x.copy() for x in bufs]
    flags = np.zeros(len(c.sizes), np.uint32)
    named = B.locate_decode(k, c.m, present, where)
    for e in c.live:
        d = int(named[e])
        if d in (N.LOC_CLEAN, N.LOC_UNCHECKED):
            continue
        mask = np.asarray(present[e]) != 0
        if d >= 0:
            assert mask[d]
            mask[d] = False
        if d < 0 or int(mask.sum()) < k:
            flags[e] = UNNAMED
            continue
        s, at = c.sizes[e], c.shards[e]
        here = [i for i in range(n) if mask[i]]
        surv, checked = here[:k], here[k:]
        outs = [i for i in range(n) if not mask[i]]
        rows = [RG.lagrange_row(tuple(surv), i) for i in outs + checked]
        implied = CO.apply(rows, [bufs[b][o:o + s] for b, o in (at[i] for i in surv)])
        for i, x in zip(outs, implied):
            b, o = at[i]
            want[b][o:o + s] = x
        flags[e] = DONE | (0 if checked else 2)
        for i, x in zip(checked, implied[len(outs):]):
            b, o = at[i]
            if not np.array_equal(x, bufs[b][o:o + s]):
                flags[e] |= 1
    return want, flags


def dev(a, dtype=torch.int32):
    return torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).cuda().view(dtype)


def host(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32).copy()


def heal(c, bufs, present, where, prefill=0, dtype=torch.int32, stream=None):
    """One call over `bufs` with the words `where`; returns (flags, tensors, plan)."""
    enc = RS.New(c.k, c.m)
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    flags = torch.full((len(c.sizes),), prefill, dtype=torch.int32, device="cuda").view(dtype)
    w = dev(where, dtype)
    torch.cuda.synchronize()
    plan.heal_mixed(present, w, flags, stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(host(w), np.asarray(where, np.uint32))  # read only
    return host(flags), t, plan


def check(c, bufs, present, where, want=None):
    want_bufs, want_flags = want or oracle_heal(c, bufs, present, where)
    got, t, _ = heal(c, bufs, present, where)
    assert np.array_equal(got, want_flags), [(int(e), int(got[e]), int(want_flags[e]))
                                             for e in np.nonzero(got != want_flags)[0][:10]]
    MP.check_equal(t, want_bufs)
    return got


def bits_of(row):
    return int(sum(1 << i for i, x in enumerate(row) if x))


def naming(row, j):
    """A word that names present shard j under mask `row`: every other present shard ruled out."""
    return N.LOC_BAD | (bits_of(row) & ~(1 << j))


# ---- 1. repair -> locate -> heal restores the codewords ----

PIPE = [(4, 2, (0,)), (8, 3, (0, 1)), (10, 4, (0, 1, 2))]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m,losses", PIPE, ids=[f"{k}+{m}" for k, m, _ in PIPE])
def test_repair_locate_heal_restores_every_codeword_without_a_sync(k, m, losses, layout):
    n = k + m
    assert all(m - lost >= 2 for lost in losses)  # r >= 2 checked shards: one flipped byte is always named
    combos = [(lost, role) for lost in losses for role in range(n - lost)]  # every survivor slot and checked shard
    c = case(k, m, layout, 3 * len(combos))
    rng = np.random.default_rng(200 + k)
    present = np.ones((len(c.sizes), n), np.uint8)
    hit = {}
    for q, e in enumerate(c.live):
        lost, role = combos[(q // 3) % len(combos)]
        if q % 3 != 0:
            lost = losses[q % len(losses)]
        present[e][rng.choice(n, size=lost, replace=False)] = 0
        if q % 3 == 0:
            hit[e] = [i for i in range(n) if present[e][i]][role]
    seen = {(int(n - present[e].sum()), [i for i in range(n) if present[e][i]].index(i)) for e, i in hit.items()}
    assert seen == set(combos)
    inp, _ = c.garble(present, seed=21)
    for q, (e, i) in enumerate(hit.items()):
        b, o = c.shards[e][i]
        inp[b][o + int(rng.integers(c.sizes[e]))] ^= 1 + q % 255
    enc = RS.New(k, m)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    flags = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    where = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    healed = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s0 = B.heal_plan_stats()
    plan.repair_mixed(present, flags)
    plan.locate_mixed(present, where, flags=flags)
    plan.heal_mixed(present, where, healed)
    torch.cuda.synchronize()
    s1 = B.heal_plan_stats()
    assert {f: s1[f] - s0[f] for f in s0} == {"kernel_launches": 1, "skipped_entries": 0}
    f, w, h = host(flags), host(where), host(healed)
    assert {e for e in range(len(c.sizes)) if f[e] & 1} == set(hit)
    named = B.locate_decode(k, m, present, w)
    assert {e: int(named[e]) for e in hit} == hit  # no case left out: every flipped shard is named
    want_h = np.zeros(len(c.sizes), np.uint32)
    want_h[list(hit)] = DONE  # exactly the corrupted stripes, and bit 0 on none
    assert np.array_equal(h, want_h)
    MP.check_equal(t, c.bufs)  # the original codewords, lost shards included, slack untouched
    # and the oracle, step by step, says the same
    after_repair, _ = RG.oracle_repair(c, inp, present)
    want_bufs, want_flags = oracle_heal(c, after_repair, present, w)
    assert np.array_equal(want_flags, want_h)
    for x, y in zip(want_bufs, c.bufs):
        assert np.array_equal(x, y)


# ---- 2. the same as repair_mixed on the cleared mask, for data that are no codewords ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_same_as_repair_on_the_cleared_mask_when_two_corrupt_shards_imitate_a_third(layout):
    k, m, n = 4, 2, 6
    c = case(k, m, layout, 40)
    surv = (0, 1, 2, 3)
    rows = [RG.lagrange_row(surv, 4), RG.lagrange_row(surv, 5)]
    rng = np.random.default_rng(31)
    present = np.ones((len(c.sizes), n), np.uint8)
    inp = [x.copy() for x in c.bufs]
    blamed = {}
    for q, e in enumerate(c.live):
        if q % 2:
            continue
        # errors x, y at one position of the two parity shards with (x, y) = err * column of data shard t
        t_, err, p = q // 2 % k, 1 + q % 255, int(rng.integers(c.sizes[e]))
        for shard, row in zip((4, 5), rows):
            b, o = c.shards[e][shard]
            inp[b][o + p] ^= O.MUL[err][row[t_]]
        blamed[e] = t_
    enc = RS.New(k, m)
    t_heal, t_rep = c.upload(inp), c.upload(inp)
    plan_heal, plan_rep = c.plan(enc, t_heal), c.plan(enc, t_rep)
    where = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    f_heal = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    f_rep = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    plan_heal.locate_mixed(present, where)
    plan_heal.heal_mixed(present, where, f_heal)
    torch.cuda.synchronize()
    w = host(where)
    named = B.locate_decode(k, m, present, w)
    assert {e: int(named[e]) for e in blamed} == blamed  # an intact shard takes the blame
    assert all(int(named[e]) == N.LOC_CLEAN for e in c.live if e not in blamed)
    # the second upload: a plan of the named entries only, their masks with the named shard cleared
    cleared = present.copy()
    for e, j in blamed.items():
        cleared[e][j] = 0
    order = sorted(blamed)
    if layout == "stripes":
        sub = B.StripePlan(enc, stripes=[(t_rep[0].data_ptr() + c.base[e][0], c.sizes[e]) for e in order])
    else:
        sub = B.StripePlan(enc, objects=[(t_rep[0].data_ptr() + c.base[e][0], t_rep[1].data_ptr() + c.base[e][1],
                                          c.sizes[e]) for e in order])
    sub_flags = torch.zeros(len(order), dtype=torch.int32, device="cuda")
    sub.repair_mixed(cleared[order], sub_flags)
    torch.cuda.synchronize()
    f_rep[order] = sub_flags
    for x, y in zip(t_heal, t_rep):
        assert torch.equal(x, y)
    h, r = host(f_heal), host(f_rep)
    assert np.array_equal(h & 3, r) and np.array_equal(h & ~np.uint32(3), np.where(np.isin(np.arange(len(h)), order),
                                                                                   DONE, 0))
    want_bufs, want_flags = oracle_heal(c, inp, present, w)
    assert np.array_equal(h, want_flags)
    MP.check_equal(t_heal, want_bufs)
    changed = [e for e in blamed if not np.array_equal(
        want_bufs[c.shards[e][blamed[e]][0]][c.shards[e][blamed[e]][1]:][:c.sizes[e]],
        c.bufs[c.shards[e][blamed[e]][0]][c.shards[e][blamed[e]][1]:][:c.sizes[e]])]
    assert len(changed) == len(blamed)  # the data are no codewords: the blamed shard is rewritten wrongly, as repair would


# ---- 3. entries that are none of the call's business ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_clean_unchecked_and_unnamed_entries_are_not_touched(k, m, layout):
    """Words 0, NOTHING and SKIPPED (forged on stripes that are no codewords, so
    a rewrite would show) and the words locate itself gives where it cannot name
    a shard: AMBIGUOUS at 4+2 with one shard lost (r = 1), MULTIPLE at 8+3 all
    present with two corrupt shards (r = 3)."""
    n = k + m
    c = case(k, m, layout, 40)
    rng = np.random.default_rng(40 + k)
    present = np.ones((len(c.sizes), n), np.uint8)
    if m == 2:
        for e in c.live:
            present[e][int(rng.integers(n))] = 0
    inp, _ = c.garble(present, seed=41)
    for e in c.live:
        here = [i for i in range(n) if present[e][i]]
        for i in (here[:1] if m == 2 else rng.choice(here, size=2, replace=False)):
            b, o = c.shards[e][i]
            inp[b][o + int(rng.integers(c.sizes[e]))] ^= 0x5A
    enc = RS.New(k, m)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    where = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    plan.locate_mixed(present, where)
    torch.cuda.synchronize()
    w = host(where)
    verdict = N.LOC_AMBIGUOUS if m == 2 else N.LOC_MULTIPLE
    assert all(int(x) == verdict for x in B.locate_decode(k, m, present, w)[c.live])
    real = set(c.live[3::4])
    for q, e in enumerate(c.live):
        j = [i for i in range(n) if present[e][i]][q % k]
        if q % 4 == 0:
            w[e] = 0
        elif q % 4 == 1:
            w[e] = N.LOC_NOTHING | (naming(present[e], j) if q % 8 == 1 else 0)
        elif q % 4 == 2:
            w[e] = N.LOC_SKIPPED | (naming(present[e], j) if q % 8 == 2 else 0)
    for e, s in enumerate(c.sizes):  # a zero-length entry whose word names a shard
        if s == 0:
            w[e] = naming(present[e], 0)
    flags = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    where.copy_(dev(w))
    s0 = B.heal_plan_stats()
    plan.heal_mixed(present, where, flags)
    torch.cuda.synchronize()
    s1 = B.heal_plan_stats()
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1
    want = np.zeros(len(c.sizes), np.uint32)
    want[sorted(real)] = UNNAMED
    assert np.array_equal(host(flags), want)
    assert np.array_equal(oracle_heal(c, inp, present, w)[1], want)
    MP.check_equal(t, inp)
    assert np.array_equal(host(where), w)


# ---- 4. every (mask, named shard) pair, through forged words ----

def forged_case(c, masks_and_j, seed):
    """Stripe q of c.live gets masks_and_j[q % len]: garbage in its missing shards
    and in shard j, and in every fifth stripe one flipped byte in the last
    present shard that is not j.  Returns (present, where, input buffers)."""
    n = c.k + c.m
    rng = np.random.default_rng(seed)
    present = np.ones((len(c.sizes), n), np.uint8)
    where = np.zeros(len(c.sizes), np.uint32)
    picks = {}
    for q, e in enumerate(c.live):
        row, j = masks_and_j[q % len(masks_and_j)]
        present[e] = row
        where[e] = naming(row, j) | (q % 3 << 16)  # bits 16.. are nobody's: they ride along
        picks[e] = j
    inp, _ = c.garble(present, seed=seed)
    for q, e in enumerate(c.live):
        s = c.sizes[e]
        b, o = c.shards[e][picks[e]]
        inp[b][o:o + s] = rng.integers(0, 256, s, dtype=np.uint8)
        if q % 5 == 0:
            last = [i for i in range(n) if present[e][i] and i != picks[e]][-1]
            b, o = c.shards[e][last]
            inp[b][o + int(rng.integers(s))] ^= 0x40
    return present, where, inp


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_every_mask_and_every_named_shard(k, m, layout):
    n = k + m
    every = [(row, j) for row in MP.masks_with_missing(n, range(0, m + 1)) for j in range(n) if row[j]]
    healable = [(row, j) for row, j in every if sum(row) >= k + 1]
    assert len(healable) == {6: 36, 11: 616}[n]
    pairs = healable + [(row, j) for row, j in every if sum(row) == k][::8]  # and some that leave k - 1
    assert len(pairs) > len(healable)
    c = case(k, m, layout, len(pairs))
    assert len(c.live) >= len(pairs)
    present, where, inp = forged_case(c, pairs, 50 + k)
    want_bufs, want_flags = oracle_heal(c, inp, present, where)
    # a forged word that would leave fewer than k present counts as unnamed; every other pair is healed
    exactly_k = np.array([s > 0 and int(present[e].sum()) == k for e, s in enumerate(c.sizes)])
    live = np.array([s > 0 for s in c.sizes])
    assert np.array_equal(want_flags & UNNAMED != 0, exactly_k) and np.array_equal(want_flags & DONE != 0,
                                                                                    live & ~exactly_k)
    assert {1, 2} <= {int(x) & 3 for x in want_flags}  # still-inconsistent and nothing-left-to-check both occur
    s0 = B.heal_plan_stats()
    check(c, inp, present, where, want=(want_bufs, want_flags))
    s1 = B.heal_plan_stats()
    assert {f: s1[f] - s0[f] for f in s0} == {"kernel_launches": 1, "skipped_entries": 0}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(12, 4), (10, 4), (3, 1), (2, 2)])
def test_sampled_masks_and_named_shards(k, m, layout):
    n = k + m
    rng = np.random.default_rng(60 + k)
    pairs = []
    for row in RG.split_masks(k, m, 60, k):
        pairs.append((row, int(rng.choice([i for i in range(n) if row[i]]))))
    assert {sum(row) for row, _ in pairs} == set(range(k, n + 1))
    c = case(k, m, layout, len(pairs))
    present, where, inp = forged_case(c, pairs, 70 + k)
    want = oracle_heal(c, inp, present, where)
    assert (want[1] & UNNAMED).any() and (want[1] & DONE).any()
    s0 = B.heal_plan_stats()
    check(c, inp, present, where, want=want)
    s1 = B.heal_plan_stats()
    assert {f: s1[f] - s0[f] for f in s0} == {"kernel_launches": 1, "skipped_entries": 0}


# ---- 5. launches and flags ----

def mixed_words_case(k, m, layout, n_live, seed):
    """Named, unnamed, clean and unchecked words side by side."""
    n = k + m
    c = case(k, m, layout, n_live)
    pairs = [(row, j) for row in MP.masks_with_missing(n, range(0, m + 1)) for j in range(n) if row[j]]
    present, where, inp = forged_case(c, pairs[::3], seed)
    for q, e in enumerate(c.live):
        if q % 4 == 1:
            where[e] = 0
        elif q % 4 == 2:
            where[e] = N.LOC_BAD  # nothing ruled out
        elif q % 8 == 3:
            where[e] |= N.LOC_NOTHING
    return c, present, where, inp


@pytest.mark.parametrize("layout", LAYOUTS)
def test_launch_boundaries_anywhere_in_the_tile_list_and_preset_flags_stay(layout):
    k, m = 4, 2
    c, present, where, inp = mixed_words_case(k, m, layout, 30, 80)
    T = tile()
    n_tiles = sum(-(-s // T) for s in c.sizes)
    assert n_tiles > 30
    want_bufs, want_flags = oracle_heal(c, inp, present, where)
    assert {0, UNNAMED, DONE} <= set(want_flags.tolist()) and (want_flags & 1).any()
    try:
        for chunk in (1, 2, 3, n_tiles - 1):
            B.set_heal_plan_chunk_tiles(chunk)
            s0 = B.heal_plan_stats()
            got, t, _ = heal(c, inp, present, where, prefill=0x30)
            s1 = B.heal_plan_stats()
            assert np.array_equal(got, want_flags | 0x30)  # zero-length and untouched entries keep 0x30 alone
            MP.check_equal(t, want_bufs)
            assert s1["kernel_launches"] - s0["kernel_launches"] == -(-n_tiles // chunk)
            assert s1["skipped_entries"] == s0["skipped_entries"]
    finally:
        B.set_heal_plan_chunk_tiles(0)


def launches_of(c, present, where, inp):
    s0 = B.heal_plan_stats()
    check(c, inp, present, where)
    s1 = B.heal_plan_stats()
    assert s1["skipped_entries"] == s0["skipped_entries"]
    return s1["kernel_launches"] - s0["kernel_launches"]


def test_launches_do_not_depend_on_stripes_masks_or_words():
    k, m, n = 4, 2, 6
    small, large = case(k, m, "stripes", 40), case(k, m, "stripes", 200)
    pairs = [(row, j) for row in MP.masks_with_missing(n, range(0, m + 1)) for j in range(n) if row[j]]
    d = []
    for c in (small, large):
        for chosen in (pairs[:1], pairs):
            present, where, inp = forged_case(c, chosen, 90)
            d.append(launches_of(c, present, where, inp))
        present, where, inp = forged_case(c, pairs, 91)
        d.append(launches_of(c, present, np.zeros_like(where), inp))  # nothing named: the list is still walked once
    assert d == [1] * 6


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_plan_healed_under_changing_masks(layout):
    """A plan keeps the records of its last call's masks: the same masks again,
    other masks, and the first ones once more all give what the oracle gives."""
    k, m = 8, 3
    n = k + m
    c = case(k, m, layout, 60)
    pairs = [(row, j) for row in MP.masks_with_missing(n, range(0, m)) for j in range(n) if row[j]]
    first = forged_case(c, pairs[::5], 120)
    second = forged_case(c, pairs[3::7], 121)
    enc = RS.New(k, m)
    bufs = first[2]
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    torch.cuda.synchronize()
    for q, (present, where, _) in enumerate((first, first, second, second, first)):
        if q in (2, 4):  # garbage again where this call's words point
            for e in c.live:
                j = int(B.locate_decode(k, m, present[e:e + 1], where[e:e + 1])[0])
                b, o = c.shards[e][j]
                bufs[b][o:o + c.sizes[e]] ^= 0x3C
            for x, y in zip(t, bufs):
                x.copy_(torch.from_numpy(y))
        bufs, want_flags = oracle_heal(c, bufs, present, where)
        flags = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
        plan.heal_mixed(present, dev(where), flags)
        torch.cuda.synchronize()
        assert np.array_equal(host(flags), want_flags), q
        MP.check_equal(t, bufs)
        assert (want_flags & DONE).any()


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint32])
def test_tensor_checks_are_repair_mixeds(dtype):
    k, m = 4, 2
    c, present, where, inp = mixed_words_case(k, m, "stripes", 20, 95)
    want_bufs, want_flags = oracle_heal(c, inp, present, where)
    got, t, plan = heal(c, inp, present, where, prefill=0x100, dtype=dtype)
    assert np.array_equal(got, want_flags | 0x100)
    MP.check_equal(t, want_bufs)
    n = len(c.sizes)
    good = torch.zeros(n, dtype=torch.int32, device="cuda").view(dtype)
    w = dev(where, dtype)
    for bad in (torch.zeros(n - 1, dtype=torch.int32, device="cuda").view(dtype),  # short
                torch.zeros(n, dtype=torch.int32).view(dtype),  # on the host
                torch.zeros(n, dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            plan.heal_mixed(present, w, bad)
        with pytest.raises(ValueError):
            plan.heal_mixed(present, bad, good)
    with pytest.raises(ValueError):
        plan.heal_mixed(present[:-1], w, good)
    with pytest.raises(ValueError):
        plan.heal_mixed(present, w, w)
    torch.cuda.synchronize()
    assert not host(good).any()
    MP.check_equal(t, want_bufs)


# ---- 6. the other route ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(13, 2), (4, 5)])
def test_other_route_is_untouched_and_counted(k, m, layout):
    n = k + m
    sizes = [0, 17, 1, 4097, 1985, 0, 10_001, 33, 64, 993, 31, 3969, 15, 65, 0]
    c = MP.Case(k, m, layout, sizes, 60 + k)
    assert len(c.live) == 12
    rng = np.random.default_rng(61)
    present = np.ones((len(sizes), n), np.uint8)
    inp = [x.copy() for x in c.bufs]
    for e in c.live:
        b, o = c.shards[e][int(rng.integers(n))]
        inp[b][o + int(rng.integers(c.sizes[e]))] ^= 0x11
    enc = RS.New(k, m)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    where = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
    flags = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
    plan.locate_mixed(present, where)
    torch.cuda.synchronize()
    w = host(where)
    assert all(w[e] == N.LOC_SKIPPED for e in c.live)
    s0 = B.heal_plan_stats()
    plan.heal_mixed(present, where, flags)
    # and with words that name a shard outright: the route decides, not the word
    forged = dev([naming(present[e], e % n) for e in range(len(sizes))])
    plan.heal_mixed(present, forged, flags)
    torch.cuda.synchronize()
    s1 = B.heal_plan_stats()
    assert {f: s1[f] - s0[f] for f in s0} == {"kernel_launches": 0, "skipped_entries": 24}
    assert not host(flags).any()
    MP.check_equal(t, inp)


# ---- 7. errors leave no trace ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_errors_leave_no_trace(layout):
    k, m = 4, 2
    c, present, where, bufs = mixed_words_case(k, m, layout, 20, 100)
    enc = RS.New(k, m)
    n = len(c.sizes)
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    w = dev(where)
    pats, idx = np.unique(present, axis=0, return_inverse=True)
    pats = np.ascontiguousarray(pats, np.uint8)
    idx = np.ascontiguousarray(idx.reshape(-1), np.uint32)

    def call(p, i, n_patterns=None, e=enc, f=flags, wh=w, pl=plan):
        return N.lib().hbec_heal_plan_mixed(e.handle if e else None, pl._h if pl else None,
                                            p.ctypes.data_as(N._U8P) if p is not None else None,
                                            (p.shape[0] if p is not None else 1) if n_patterns is None else n_patterns,
                                            i.ctypes.data_as(U32P) if i is not None else None,
                                            C.c_void_p(wh.data_ptr()) if wh is not None else None,
                                            C.c_void_p(f.data_ptr()) if f is not None else None, None)

    s0 = B.heal_plan_stats()
    assert call(pats, idx, e=RS.New(8, 3)) == N.ERR_INVALID_ARG  # another codec's plan
    bad = idx.copy()
    bad[n - 1] = pats.shape[0]  # the last entry is zero-length: checked all the same
    assert c.sizes[n - 1] == 0
    assert call(pats, bad) == N.ERR_INVALID_ARG and "index" in N.last_error()
    few = np.vstack([pats, np.array([[1, 1, 1, 0, 0, 0]], np.uint8)])  # listed, unused
    assert call(few, idx) == N.ERR_TOO_FEW_SHARDS
    assert call(pats, idx, n_patterns=0) == N.ERR_INVALID_ARG
    assert call(pats, idx, n_patterns=65537) == N.ERR_INVALID_ARG
    assert call(pats, idx, f=None) == N.ERR_INVALID_ARG  # null d_flags
    assert call(pats, idx, wh=None) == N.ERR_INVALID_ARG  # null d_where
    assert call(pats, idx, f=w) == N.ERR_INVALID_ARG and "alias" in N.last_error()
    assert call(None, idx) == N.ERR_INVALID_ARG
    assert call(pats, None) == N.ERR_INVALID_ARG
    assert call(pats, idx, e=None) == N.ERR_INVALID_ARG
    assert call(pats, idx, pl=None) == N.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert B.heal_plan_stats() == s0
    assert not host(flags).any() and np.array_equal(host(w), where)
    MP.check_equal(t, bufs)
    assert call(pats, idx) == N.HBEC_OK
    torch.cuda.synchronize()
    want_bufs, want_flags = oracle_heal(c, bufs, present, where)
    assert np.array_equal(host(flags), want_flags) and (want_flags & DONE).any()
    MP.check_equal(t, want_bufs)


# ---- 8. two streams, one plan ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_heal_and_repair_from_two_streams_keep_their_words_apart(layout):
    """Calls on one plan take turns in the order they were made, whatever their
    streams: heal, then a repair that sees what heal left, then heal again."""
    k, m = 8, 3
    n = k + m
    c = case(k, m, layout, 60)
    pairs = [(row, j) for row in MP.masks_with_missing(n, range(0, m)) for j in range(n) if row[j]]
    present, where, inp = forged_case(c, pairs[::5], 110)
    after_heal, want_h = oracle_heal(c, inp, present, where)
    after_repair, want_r = RG.oracle_repair(c, after_heal, present)
    after_all, want_h2 = oracle_heal(c, after_repair, present, where)
    assert (want_h & 1).any() and (want_h & DONE).any() and (want_r & 1).any()
    enc = RS.New(k, m)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    f_h = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    f_r = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    f_h2 = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    w = dev(where)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.heal_mixed(present, w, f_h, stream=s1)
    plan.repair_mixed(present, f_r, stream=s2)
    plan.heal_mixed(present, w, f_h2, stream=s1)
    torch.cuda.synchronize()
    assert np.array_equal(host(f_h), want_h)
    assert np.array_equal(host(f_r), want_r)
    assert np.array_equal(host(f_h2), want_h2)
    MP.check_equal(t, after_all)
