"""hbec_repair_plan_mixed: the missing shards of every stripe of a plan rebuilt
and its surplus present shards checked in one call that reads the survivors
once.

Expected bytes and flags never come from the product.  Per stripe the oracle
takes the first k present shards as survivors; a rebuilt shard is
oracle.coracle.apply of oracle.lagrange.lagrange_row(survivors, shard) on the
bytes actually in the survivor slots (so a corrupt survivor gives the corrupt
shard Reconstruct would give), and the flags are the syndromes of
lagrange_row(survivors, c) for every other present shard c on the bytes in the
buffer: bit 0 on a difference, bit 1 when exactly k are present.  Buffers are
laid out by test_gpu_mixed_plan.Case (random slack before, between and after the
stripes, odd offsets, 16-aligned stripes alternating aligned and odd); whole
buffers, slack included, and whole flag arrays are compared exactly.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_mixed_plan as MP
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO
from oracle import lagrange as LG

pytestmark = pytest.mark.gpu

LAYOUTS = MP.LAYOUTS
W = 992  # one 64-lane window of the kernel (unaligned_tile.h)
U32P = C.POINTER(C.c_uint32)


def tile():
    return B.repair_plan_tile_bytes()


@functools.lru_cache(maxsize=None)
def case(k, m, layout, n_live=1):
    """MP.size_set's sizes (1, 3, 15..17, 31, 33, 63..65, W +- 1, T +- 1, 2T + 17,
    ~20 random ones, zero-length entries first, last and interior), repeated
    until there are n_live non-empty stripes."""
    return MP.Case(k, m, layout, MP.sizes_for(n_live, 100 * k + m), 7 * k + m + len(layout))


@functools.lru_cache(maxsize=None)
def lagrange_row(surv, c):
    return LG.lagrange_row(list(surv), c)


def oracle_repair(c, bufs, present, data_only=False):
    """(buffers, flags) one call must leave, from the oracle alone."""
    k, n = c.k, c.k + c.m
    want = [x.copy() for x in bufs]
    flags = np.zeros(len(c.sizes), np.uint32)
    for e in c.live:
        s, where = c.sizes[e], c.shards[e]
        here = [i for i in range(n) if present[e][i]]
        surv, checked = here[:k], here[k:]
        outs = [i for i in range(n) if not present[e][i] and (i < k or not data_only)]
        if not checked:
            flags[e] = 2
        if not checked and not outs:
            continue
        rows = [lagrange_row(tuple(surv), i) for i in outs + checked]
        data = [bufs[b][o:o + s] for b, o in (where[i] for i in surv)]
        implied = CO.apply(rows, data)
        for i, x in zip(outs, implied):
            b, o = where[i]
            want[b][o:o + s] = x
        for i, x in zip(checked, implied[len(outs):]):
            b, o = where[i]
            if not np.array_equal(x, bufs[b][o:o + s]):
                flags[e] |= 1
    return want, flags


def repair(c, bufs, present, data_only=False, prefill=0, dtype=torch.int32, stream=None):
    """One call over `bufs`; returns (flags, tensors, plan)."""
    enc = RS.New(c.k, c.m)
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    flags = torch.full((len(c.sizes),), prefill, dtype=torch.int32, device="cuda").view(dtype)
    torch.cuda.synchronize()
    plan.repair_mixed(present, flags, data_only=data_only, stream=stream)
    torch.cuda.synchronize()
    return flags.view(torch.int32).cpu().numpy().astype(np.uint32), t, plan


def check(c, bufs, present, data_only=False, want=None):
    """One call; buffers and flags against the oracle.  Returns the flags."""
    want_bufs, want_flags = want or oracle_repair(c, bufs, present, data_only)
    got, t, _ = repair(c, bufs, present, data_only)
    assert np.array_equal(got, want_flags), np.nonzero(got != want_flags)[0][:10]
    MP.check_equal(t, want_bufs)
    return got


def exactly_k(c, present):
    return np.array([2 if s and int(np.sum(np.asarray(present[e]) != 0)) == c.k else 0
                     for e, s in enumerate(c.sizes)], np.uint32)


def check_clean(c, present, data_only=False, seed=1):
    """Clean codewords with garbage in every missing shard: every rebuilt shard
    comes back clean, flags are 0 or 2, nothing else changes."""
    inp, clean = c.garble(present, data_only=data_only, seed=seed)
    want_bufs, want_flags = oracle_repair(c, inp, present, data_only)
    for w, x in zip(want_bufs, clean):  # the oracle agrees with the codewords
        assert np.array_equal(w, x)
    assert np.array_equal(want_flags, exactly_k(c, present))
    check(c, inp, present, data_only, want=(want_bufs, want_flags))


# ---- 1. clean codewords under every mask ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_every_mask_rebuilds_clean_and_flags_only_exactly_k(k, m, layout):
    masks = MP.masks_with_missing(k + m, range(0, m + 1))  # all present included
    assert len(masks) == {6: 22, 11: 232}[k + m]
    c = case(k, m, layout, len(masks))
    assert len(c.live) >= len(masks) and c.sizes[0] == 0 and c.sizes[-1] == 0
    present = MP.spread(c, masks, 1)
    assert {tuple(present[e]) for e in c.live} == {tuple(x) for x in masks}
    s0 = B.repair_plan_stats()
    check_clean(c, present)
    s1 = B.repair_plan_stats()
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1


# ---- 2. every (r_o, r_c) split ----

def split_masks(k, m, count, seed):
    """Masks with every (lost, surplus) split of m, lost shards sampled."""
    rng = np.random.default_rng(seed)
    out = []
    for q in range(count):
        lost = rng.choice(k + m, size=q % (m + 1), replace=False)
        out.append([0 if i in lost else 1 for i in range(k + m)])
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(12, 4), (10, 4), (3, 1), (2, 2)])
def test_every_split_of_outputs_and_checked_runs_on_the_kernel(k, m, layout):
    masks = split_masks(k, m, 60, k)
    assert {(row.count(0), m - row.count(0)) for row in masks} == {(o, m - o) for o in range(m + 1)}
    c = case(k, m, layout, len(masks))
    present = MP.spread(c, masks, 3)
    assert {present[e].tolist().count(0) for e in c.live} == set(range(m + 1))
    s0 = B.repair_plan_stats()
    check_clean(c, present)
    s1 = B.repair_plan_stats()
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1


# ---- 3. one flipped bit per chosen stripe ----

def named_positions(s):
    T = tile()
    names = {"0": 0, "1": 1, "15": 15, "16": 16, "S-17": s - 17, "S-2": s - 2, "S-1": s - 1, "W-1": W - 1, "W": W,
             "T-1": T - 1, "T": T}
    return {n: p for n, p in names.items() if 0 <= p < s}


@functools.lru_cache(maxsize=None)
def flip_case(k, m, layout):
    """A stripe list that repeats the size set: one stripe per flip (every byte
    of the sizes <= 65, the named positions of the others), an unflipped stripe
    after each.  Returns (case, [(entry, position, names)])."""
    base = [s for s in MP.size_set(300 + k) if s]
    calm = [s for s in base if s <= tile() + 1]
    sizes, flips = [], []
    for s in base:
        if s <= 65:
            todo = [(p, ()) for p in range(s)]
        else:
            by_pos = {}
            for name, p in named_positions(s).items():
                by_pos.setdefault(p, []).append(name)
            todo = [(p, tuple(nm)) for p, nm in sorted(by_pos.items())]
        for p, nm in todo:
            flips.append((len(sizes), p, nm))
            sizes += [s, calm[len(flips) % len(calm)]]
    # zero-length entries first, interior and last, keeping the flips' entry numbers right
    cuts = sorted({0, len(sizes) // 3, 2 * len(sizes) // 3, len(sizes)})
    out, shift, moved = [], {}, 0
    for i, s in enumerate(sizes + [None]):
        if i in cuts:
            out.append(0)
            moved += 1
        shift[i] = i + moved
        if s is not None:
            out.append(s)
    c = MP.Case(k, m, layout, out, 31 * k + m + len(layout))
    return c, [(shift[e], p, nm) for e, p, nm in flips]


def flipped(c, flips, present, in_missing):
    """Garbled buffers with one bit flipped per listed stripe.  in_missing: in a
    shard its mask (already in `present`) calls missing.  Otherwise in a present
    shard: per position name the roles survivor 0..k-1, checked 0..m-1 are taken
    in turn, and the stripe gets a mask under which that role exists: a survivor
    any mask with 1..m shards lost (with m lost the stripe has no checked shard),
    checked q one with at least k + q + 1 present and, but for q = m - 1,
    something lost.  Returns the buffers and the (role, name) pairs covered."""
    k, m, n = c.k, c.m, c.k + c.m
    roles, turn, where = set(), {}, []
    for q, (e, p, names) in enumerate(flips):
        names = names or ("byte",)
        if in_missing:
            gone = [i for i in range(n) if not present[e][i]]
            i = gone[q % len(gone)]
        else:
            role = turn.get(names[0], 0) % n
            turn[names[0]] = role + 1
            lost = range(1, m + 1) if role < k else range(0 if role - k == m - 1 else 1, m - (role - k))
            fits = MP.masks_with_missing(n, lost)
            present[e] = fits[(5 * q + 1) % len(fits)]
            i = [j for j in range(n) if present[e][j]][role]
            roles |= {(role if role < k else ("checked", role - k), nm) for nm in names}
        where.append((e, i, p, q))
    bufs, _ = c.garble(present, seed=9)
    for e, i, p, q in where:
        b, o = c.shards[e][i]
        assert c.sizes[e] > p
        bufs[b][o + p] ^= 1 << (q % 8)
    return bufs, roles


def check_flips(k, m, layout):
    c, flips = flip_case(k, m, layout)
    n = k + m
    flip_entries = {e for e, _, _ in flips}
    assert len(c.live) == 2 * len(flips) and c.sizes[0] == 0 and c.sizes[-1] == 0 and c.sizes.count(0) == 4
    anym = MP.masks_with_missing(n, range(0, m + 1))
    present = np.ones((len(c.sizes), n), np.uint8)
    for q, e in enumerate(c.live):
        present[e] = anym[(7 * q + 2) % len(anym)]
    # (a) flips in present shards, survivors and checked
    bufs, roles = flipped(c, flips, present, in_missing=False)
    names = ["0", "1", "15", "16", "S-17", "S-2", "S-1", "W-1", "W", "T-1", "T", "byte"]
    for role in list(range(k)) + [("checked", q) for q in range(m)]:
        for nm in names:
            assert (role, nm) in roles, (role, nm)
    want_bufs, want_flags = oracle_repair(c, bufs, present)
    checked_flips = {e for e in flip_entries if int(present[e].sum()) > k}
    assert {e for e in c.live if want_flags[e] & 1} == checked_flips  # exactly the flipped stripes with a checked shard
    assert checked_flips and checked_flips != flip_entries
    _, clean = c.garble(present, seed=9)
    dirty = set()  # stripes whose rebuilt shards are not the clean codeword's: exactly those with a survivor flipped
    for e in c.live:
        for i in range(n):
            b, o = c.shards[e][i]
            if not present[e][i] and not np.array_equal(want_bufs[b][o:o + c.sizes[e]], clean[b][o:o + c.sizes[e]]):
                dirty.add(e)
    survivor_flips = set()
    for e, p, _ in flips:
        here = [i for i in range(n) if present[e][i]]
        for i in here[:k]:
            b, o = c.shards[e][i]
            if bufs[b][o + p] != c.bufs[b][o + p]:
                survivor_flips.add(e)
    assert dirty == survivor_flips and dirty and dirty != flip_entries
    check(c, bufs, present, want=(want_bufs, want_flags))
    # (b) the same flips in missing shards flag nothing and are overwritten
    lossy = MP.masks_with_missing(n, range(1, m + 1))
    for q, e in enumerate(c.live):
        present[e] = lossy[(5 * q + 1) % len(lossy)] if e in flip_entries else anym[(7 * q + 2) % len(anym)]
    bufs, _ = flipped(c, flips, present, in_missing=True)
    want_bufs, want_flags = oracle_repair(c, bufs, present)
    assert not (want_flags & 1).any()
    _, clean = c.garble(present, seed=9)
    for w, x in zip(want_bufs, clean):
        assert np.array_equal(w, x)
    check(c, bufs, present, want=(want_bufs, want_flags))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_single_bit_flips_flag_exactly_their_stripes(k, m, layout):
    check_flips(k, m, layout)


# ---- 4. data_only ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_data_only_leaves_missing_parity_as_it_was(k, m, layout):
    c = case(k, m, layout)
    masks = MP.masks_with_missing(k + m, range(0, m + 1))
    masks = masks[::max(1, len(masks) // 30)]  # 4+2: all 22; 8+3: 34 of every loss count
    assert len(masks) <= len(c.live)
    present = MP.spread(c, masks, 4)
    assert any(not present[e][k:].all() and present[e][:k].all() for e in c.live)  # parity-only losses occur
    inp, clean = c.garble(present, data_only=True)
    want_bufs, want_flags = oracle_repair(c, inp, present, data_only=True)
    for w, x in zip(want_bufs, clean):  # missing parity keeps its garbage
        assert np.array_equal(w, x)
    assert np.array_equal(want_flags, oracle_repair(c, inp, present)[1])  # flags as with data_only=False
    assert np.array_equal(want_flags, exactly_k(c, present)) and (want_flags == 2).any()
    check(c, inp, present, data_only=True, want=(want_bufs, want_flags))


# ---- 5. the same as verify_mixed then reconstruct_mixed ----

@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4)])
def test_same_as_verify_then_reconstruct(k, m, layout, data_only):
    c = case(k, m, layout, 60)
    n = k + m
    masks = MP.masks_with_missing(n, range(0, m + 1)) if n < 12 else split_masks(k, m, 60, 5)
    present = MP.spread(c, masks, 5)
    inp, _ = c.garble(present, seed=5)
    rng = np.random.default_rng(55)
    for q, e in enumerate(c.live):  # non-codewords: random bytes in a survivor, a flip in a surplus shard
        here = [i for i in range(n) if present[e][i]]
        if q % 3 == 0:
            b, o = c.shards[e][here[q % k]]
            inp[b][o:o + c.sizes[e]] = rng.integers(0, 256, c.sizes[e], dtype=np.uint8)
        elif q % 3 == 1 and len(here) > k:
            b, o = c.shards[e][here[-1]]
            inp[b][o + int(rng.integers(c.sizes[e]))] ^= 0x20
    enc = RS.New(k, m)
    t_pair, t_one = c.upload(inp), c.upload(inp)
    plan_pair, plan_one = c.plan(enc, t_pair), c.plan(enc, t_one)
    f_pair = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    f_one = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    plan_pair.verify_mixed(present, f_pair)
    plan_pair.reconstruct_mixed(present, data_only=data_only)
    plan_one.repair_mixed(present, f_one, data_only=data_only)
    torch.cuda.synchronize()
    assert torch.equal(f_pair, f_one) and (f_one & 1).any() and (f_one == 0).any()
    for x, y in zip(t_pair, t_one):
        assert torch.equal(x, y)
    want_bufs, want_flags = oracle_repair(c, inp, present, data_only)
    assert np.array_equal(f_one.cpu().numpy().astype(np.uint32), want_flags)
    MP.check_equal(t_one, want_bufs)


# ---- 6. launch boundaries ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_launch_boundaries_anywhere_in_the_tile_list(layout):
    k, m = 4, 2
    masks = MP.masks_with_missing(6, range(0, 3))
    c = case(k, m, layout, len(masks))
    present = MP.spread(c, masks, 1)
    T = tile()
    n_tiles = sum(-(-s // T) for s in c.sizes)
    assert n_tiles > 30
    inp, _ = c.garble(present)
    for e in c.live[::4]:  # some flags too
        b, o = c.shards[e][[i for i in range(6) if present[e][i]][0]]
        inp[b][o + c.sizes[e] // 2] ^= 0x08
    want = oracle_repair(c, inp, present)
    assert (want[1] & 1).any()
    try:
        for chunk in (1, 2, 3, n_tiles - 1):
            B.set_repair_plan_chunk_tiles(chunk)
            s0 = B.repair_plan_stats()
            check(c, inp, present, want=want)
            s1 = B.repair_plan_stats()
            assert s1["kernel_launches"] - s0["kernel_launches"] == -(-n_tiles // chunk)
            assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    finally:
        B.set_repair_plan_chunk_tiles(0)


def launches_of(c, present):
    inp, _ = c.garble(present)
    s0 = B.repair_plan_stats()
    check(c, inp, present)
    s1 = B.repair_plan_stats()
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    return s1["kernel_launches"] - s0["kernel_launches"]


def test_launches_do_not_depend_on_stripes_or_masks():
    k, m = 4, 2
    small, large = case(k, m, "stripes", 40), case(k, m, "stripes", 200)
    assert len(small.live) >= 40 and len(large.live) >= 200 and len(small.live) < 100
    masks = MP.masks_with_missing(6, range(0, 3))
    d = [launches_of(small, MP.spread(small, masks[1:2], 3)), launches_of(small, MP.spread(small, masks, 3)),
         launches_of(large, MP.spread(large, masks[1:2], 3)), launches_of(large, MP.spread(large, masks, 3))]
    assert d == [1, 1, 1, 1]


# ---- 7. flags ----

@pytest.mark.parametrize("dtype", [torch.int32, torch.uint32])
def test_flags_are_ored_into_what_the_caller_had(dtype):
    k, m = 4, 2
    c = case(k, m, "stripes")
    rng = np.random.default_rng(50)
    bufs = [x.copy() for x in c.bufs]
    for e in c.live[::2]:
        b, o = c.shards[e][5]  # the last shard: checked whenever it and > k shards are present
        bufs[b][o + int(rng.integers(c.sizes[e]))] ^= 0x10
    first = MP.spread(c, MP.masks_with_missing(6, [0, 1]), 51)
    second = MP.spread(c, MP.masks_with_missing(6, [1, 2]), 52)
    want_bufs, f1 = oracle_repair(c, bufs, first)
    got, t, plan = repair(c, bufs, first, prefill=4, dtype=dtype)
    want = 4 | f1
    zero_len = [e for e, s in enumerate(c.sizes) if s == 0]
    want[zero_len] = 4  # zero-length entries are untouched
    assert np.array_equal(got, want)
    MP.check_equal(t, want_bufs)
    # a second call on the same flags and buffers: bit 1 joins bit 0
    flags = torch.from_numpy(got.astype(np.int32)).cuda().view(dtype)
    plan.repair_mixed(second, flags)
    torch.cuda.synchronize()
    want_bufs, f2 = oracle_repair(c, want_bufs, second)
    want |= f2
    assert np.array_equal(flags.view(torch.int32).cpu().numpy().astype(np.uint32), want)
    MP.check_equal(t, want_bufs)
    assert {4, 5, 6, 7} == set(want.tolist())
    n = len(c.sizes)
    for bad in (torch.zeros(n - 1, dtype=torch.int32, device="cuda").view(dtype),  # short
                torch.zeros(n, dtype=torch.int32).view(dtype),  # on the host
                torch.zeros(n, dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            plan.repair_mixed(first, bad)
    with pytest.raises(ValueError):
        plan.repair_mixed(first[:-1], flags)
    torch.cuda.synchronize()
    MP.check_equal(t, want_bufs)


# ---- 8. the other route ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(13, 2), (16, 4), (4, 5)])
def test_other_route_is_exact_and_counted(k, m, layout):
    n = k + m
    sizes = [0, 17, 1, 4097, 1985, 0, 10_001, 33, 64, 993, 31, 3969, 15, 65, 0]
    c = MP.Case(k, m, layout, sizes, 60 + k)
    assert len(c.live) == 12
    rng = np.random.default_rng(61)
    present = np.ones((len(sizes), n), np.uint8)
    losses = [1, 2, 0, m, 1, 2, 0, m, 1, 2, 1, 2]  # one and two, all present, exactly k
    for e, lost in zip(c.live, losses):
        present[e][rng.choice(n, size=lost, replace=False)] = 0
    inp, _ = c.garble(present)
    for q, e in enumerate(c.live):
        if q % 3 == 0:
            continue
        here = [i for i in range(n) if present[e][i]]
        b, o = c.shards[e][here[q % len(here)]]
        inp[b][o + int(rng.integers(c.sizes[e]))] ^= 1 << (q % 8)
    want = oracle_repair(c, inp, present)
    assert {0, 1, 2} == set(want[1].tolist())
    s0 = B.repair_plan_stats()
    check(c, inp, present, want=want)
    s1 = B.repair_plan_stats()
    assert s1["per_stripe_calls"] - s0["per_stripe_calls"] == 12
    assert s1["kernel_launches"] == s0["kernel_launches"]


# ---- 9. errors leave no trace ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_errors_leave_no_trace(layout):
    k, m = 4, 2
    c = case(k, m, layout)
    enc = RS.New(k, m)
    n = len(c.sizes)
    present = MP.spread(c, MP.masks_with_missing(6, range(0, 3)), 70)
    bufs, _ = c.garble(present)
    for e in c.live[::3]:
        b, o = c.shards[e][[i for i in range(6) if present[e][i]][0]]
        bufs[b][o] ^= 0x80
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    pats, idx = np.unique(present, axis=0, return_inverse=True)
    pats = np.ascontiguousarray(pats, np.uint8)
    idx = np.ascontiguousarray(idx.reshape(-1), np.uint32)

    def call(p, i, n_patterns=None, e=enc, f=flags, pl=plan):
        return N.lib().hbec_repair_plan_mixed(e.handle if e else None, pl._h if pl else None,
                                              p.ctypes.data_as(N._U8P) if p is not None else None,
                                              (p.shape[0] if p is not None else 1) if n_patterns is None else n_patterns,
                                              i.ctypes.data_as(U32P) if i is not None else None, 0,
                                              C.c_void_p(f.data_ptr()) if f is not None else None, None)

    s0 = B.repair_plan_stats()
    assert call(pats, idx, e=RS.New(8, 3)) == N.ERR_INVALID_ARG
    bad = idx.copy()
    bad[n - 1] = pats.shape[0]  # the last entry is zero-length: checked all the same
    assert c.sizes[n - 1] == 0
    assert call(pats, bad) == N.ERR_INVALID_ARG and "index" in N.last_error()
    few = np.vstack([pats, np.array([[1, 1, 1, 0, 0, 0]], np.uint8)])  # listed, unused
    assert call(few, idx) == N.ERR_TOO_FEW_SHARDS
    assert call(pats, idx, n_patterns=0) == N.ERR_INVALID_ARG
    assert call(pats, idx, n_patterns=65537) == N.ERR_INVALID_ARG
    assert call(pats, idx, f=None) == N.ERR_INVALID_ARG  # null d_flags
    assert call(None, idx) == N.ERR_INVALID_ARG
    assert call(pats, None) == N.ERR_INVALID_ARG
    assert call(pats, idx, e=None) == N.ERR_INVALID_ARG
    assert call(pats, idx, pl=None) == N.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert B.repair_plan_stats() == s0
    assert not flags.cpu().numpy().any()
    MP.check_equal(t, bufs)
    assert call(pats, idx) == N.HBEC_OK
    torch.cuda.synchronize()
    want_bufs, want_flags = oracle_repair(c, bufs, present)
    assert np.array_equal(flags.cpu().numpy().astype(np.uint32), want_flags) and (want_flags & 1).any()
    MP.check_equal(t, want_bufs)


# ---- 10. two streams, one plan ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_verify_reconstruct_and_repair_from_two_streams_keep_their_words_apart(layout):
    k, m = 8, 3
    n = k + m
    c = case(k, m, layout, 60)
    rng = np.random.default_rng(80)
    # B (reconstruct) and R (repair) rebuild the same two shards, one after the other
    # on one stream; every call's mask calls them missing, so nothing written is read
    mask_b = np.ones((len(c.sizes), n), np.uint8)
    mask_a, mask_r = mask_b.copy(), mask_b.copy()
    for q, e in enumerate(c.live):
        lost = rng.choice(n, size=2, replace=False)
        mask_a[e][lost] = 0
        mask_b[e][lost] = 0
        mask_r[e][lost] = 0
        spare = [i for i in range(n) if mask_b[e][i]][k:]  # one shard: present, read by no reconstruct
        if q % 3 == 0:
            mask_a[e][spare] = 0  # exactly k left for A
    inp, rebuilt = c.garble(mask_b)
    for q, e in enumerate(c.live):  # corrupt the spare shard only: every rebuild still gives clean bytes
        if q % 4 < 2:
            spare = [i for i in range(n) if mask_b[e][i]][k:]
            b, o = c.shards[e][spare[0]]
            for buf in (inp, rebuilt):
                buf[b][o + c.sizes[e] // 2] ^= 0x04
    _, want_a = oracle_repair(c, inp, mask_a)
    want_bufs, want_r = oracle_repair(c, inp, mask_r)
    for w, x in zip(want_bufs, rebuilt):
        assert np.array_equal(w, x)
    assert (want_a & 1).any() and (want_a & 2).any() and (want_r & 1).any() and not np.array_equal(want_a, want_r)
    enc = RS.New(k, m)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    flags_a = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    flags_r = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    flags_a2 = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.verify_mixed(mask_a, flags_a, stream=s1)
    plan.repair_mixed(mask_r, flags_r, stream=s2)
    plan.verify_mixed(mask_a, flags_a2, stream=s1)
    plan.reconstruct_mixed(mask_b, stream=s2)
    torch.cuda.synchronize()
    assert np.array_equal(flags_a.cpu().numpy().astype(np.uint32), want_a)
    assert np.array_equal(flags_a2.cpu().numpy().astype(np.uint32), want_a)
    assert np.array_equal(flags_r.cpu().numpy().astype(np.uint32), want_r)
    MP.check_equal(t, rebuilt)


# ---- 11. the whole pipeline ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (10, 4)])
def test_repair_locate_and_second_repair_end_with_clean_codewords(k, m, layout):
    n = k + m
    c = case(k, m, layout, 40)
    rng = np.random.default_rng(110 + k)
    present = np.ones((len(c.sizes), n), np.uint8)
    hit = {}
    for q, e in enumerate(c.live):
        # one lost; at 4+2 every sixth stripe keeps all six, so that two checked shards can name the flipped one
        if not (m == 2 and q % 6 == 3):
            present[e][int(rng.integers(n))] = 0
        if q % 3 == 0:  # one bit of one survivor
            hit[e] = [i for i in range(n) if present[e][i]][:k][q % k]
    inp, _ = c.garble(present, seed=11)
    for q, (e, i) in enumerate(hit.items()):
        b, o = c.shards[e][i]
        inp[b][o + int(rng.integers(c.sizes[e]))] ^= 1 << (q % 8)
    enc = RS.New(k, m)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    flags = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    where = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    plan.repair_mixed(present, flags)
    plan.locate_mixed(present, where, flags=flags)
    torch.cuda.synchronize()
    f = flags.cpu().numpy().astype(np.uint32)
    want_bufs, want_flags = oracle_repair(c, inp, present)
    assert np.array_equal(f, want_flags)
    MP.check_equal(t, want_bufs)
    flagged = [e for e in range(len(c.sizes)) if f[e] & 1]
    assert set(flagged) == set(hit)
    named = B.locate_decode(k, m, present, where.cpu().numpy()).copy()
    one_check = [e for e in flagged if int(present[e].sum()) == k + 1]
    assert bool(one_check) == (m == 2) and len(one_check) < len(flagged)
    for e in one_check:
        # 4+2 with one lost has one checked shard: every present shard stays a candidate, and the
        # caller needs a second source to choose (here: the test knows)
        assert named[e] == N.LOC_AMBIGUOUS
        named[e] = hit[e]
    assert {e: int(named[e]) for e in flagged} == hit
    # the second repair: a plan of the flagged stripes, the named shard cleared in the mask
    again = present.copy()
    for e in flagged:
        again[e][int(named[e])] = 0
    if c.layout == "stripes":
        sub = B.StripePlan(enc, stripes=[(t[0].data_ptr() + c.base[e][0], c.sizes[e]) for e in flagged])
    else:
        sub = B.StripePlan(enc, objects=[(t[0].data_ptr() + c.base[e][0], t[1].data_ptr() + c.base[e][1], c.sizes[e])
                                         for e in flagged])
    flags2 = torch.zeros(len(flagged), dtype=torch.int32, device="cuda")
    sub.repair_mixed(again[flagged], flags2)
    torch.cuda.synchronize()
    assert flags2.cpu().numpy().tolist() == [0 if int(again[e].sum()) > k else 2 for e in flagged]
    MP.check_equal(t, c.bufs)  # every stripe equals its clean codeword, slack untouched
