"""hbec_verify_plan_mixed: Verify of a plan (stripes or objects of any sizes at
any alignment) whose entries are missing different shards, in one call.

Expected flags never come from the product.  Per stripe the oracle takes the
first k present shards as survivors, recomputes every other present shard from
them with oracle.coracle.apply on oracle.lagrange.lagrange_row(survivors, c) and
compares with the bytes in the buffer: bit 0 on a difference, bit 1 when exactly
k are present.  Buffers are laid out by test_gpu_mixed_plan.Case: random slack
before, between and after the stripes, odd offsets, 16-aligned stripes
alternating aligned and odd.
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
SMALL = [1, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65]


def tile():
    return B.verify_mixed_plan_tile_bytes()


def live_sizes(seed, n_random=20):
    T = tile()
    rng = np.random.default_rng(seed)
    sizes = SMALL + [W - 1, W, W + 1, T - 1, T, T + 1, 2 * T + 17]
    sizes += [int(x) for x in rng.integers(1, 40_001, n_random)]
    return [sizes[i] for i in rng.permutation(len(sizes))]


def with_zeros(sizes, seed):
    """Zero-length entries first, last and interior."""
    rng = np.random.default_rng(seed)
    sizes = list(sizes)
    for _ in range(3):
        sizes.insert(int(rng.integers(1, len(sizes))), 0)
    return [0] + sizes + [0]


def sizes_for(n_live, seed):
    sizes = []
    while len(sizes) < n_live:
        sizes += live_sizes(seed + len(sizes))
    return with_zeros(sizes, seed)


@functools.lru_cache(maxsize=None)
def case(k, m, layout, n_live=1):
    return MP.Case(k, m, layout, sizes_for(n_live, 100 * k + m), 7 * k + m + len(layout))


@functools.lru_cache(maxsize=None)
def lagrange_row(surv, c):
    return LG.lagrange_row(list(surv), c)


def oracle_flags(c, bufs, present):
    """The flags one call must OR in, from the oracle alone."""
    k, n = c.k, c.k + c.m
    want = np.zeros(len(c.sizes), np.uint32)
    for e in c.live:
        s, where = c.sizes[e], c.shards[e]
        here = [i for i in range(n) if present[e][i]]
        surv, checked = here[:k], here[k:]
        if not checked:
            want[e] = 2
            continue
        rows = [lagrange_row(tuple(surv), ch) for ch in checked]
        data = [bufs[b][o:o + s] for b, o in (where[i] for i in surv)]
        for ch, implied in zip(checked, CO.apply(rows, data)):
            b, o = where[ch]
            if not np.array_equal(implied, bufs[b][o:o + s]):
                want[e] |= 1
    return want


def masks_up_to(n, lost_max, lost_min=0):
    return MP.masks_with_missing(n, range(lost_min, lost_max + 1))


def random_masks(k, m, count, seed, lost_min=1):
    rng = np.random.default_rng(seed)
    out = []
    for q in range(count):
        lost = rng.choice(k + m, size=lost_min + q % (m - lost_min + 1), replace=False)
        out.append([0 if i in lost else 1 for i in range(k + m)])
    return out


def verify_mixed(c, bufs, present, prefill=0, dtype=torch.int32):
    """One call over `bufs`; returns (flags, tensors, plan)."""
    enc = RS.New(c.k, c.m)
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    flags = torch.full((len(c.sizes),), prefill, dtype=torch.int32, device="cuda").view(dtype)
    torch.cuda.synchronize()
    plan.verify_mixed(present, flags)
    torch.cuda.synchronize()
    return flags.view(torch.int32).cpu().numpy().astype(np.uint32), t, plan


def check_clean(c, present, seed=1):
    """Test 1 on one case: clean codewords, garbage in every missing shard."""
    inp, _ = c.garble(present, seed=seed)
    want = oracle_flags(c, inp, present)
    exactly_k = np.array([2 if s and int(np.sum(present[e] != 0)) == c.k else 0 for e, s in enumerate(c.sizes)],
                         np.uint32)
    assert np.array_equal(want, exactly_k)  # the oracle agrees: clean survivors, nothing else flagged
    got, t, _ = verify_mixed(c, inp, present)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    MP.check_equal(t, inp)  # read-only, slack included


# ---- 1. clean codewords ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (10, 4), (12, 4), (3, 1)])
def test_clean_codewords_flag_only_exactly_k(k, m, layout):
    if (k, m) in ((4, 2), (8, 3)):
        masks = masks_up_to(k + m, m)  # every mask with >= k present
        assert len(masks) == {6: 22, 11: 232}[k + m]
    else:
        masks = random_masks(k, m, 60, k) + [[1] * (k + m)]
    c = case(k, m, layout, len(masks))
    assert len(c.live) >= len(masks)
    present = MP.spread(c, masks, 1)
    assert {tuple(present[e]) for e in c.live} == {tuple(x) for x in masks}
    s0 = B.verify_mixed_plan_stats()
    check_clean(c, present)
    s1 = B.verify_mixed_plan_stats()
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1


# ---- 2. all present: Encoder.Verify ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4)])
def test_all_present_equals_plan_verify(k, m, layout):
    c = case(k, m, layout)
    rng = np.random.default_rng(20 + k)
    bufs = [x.copy() for x in c.bufs]
    hit = set()
    for e in c.live:
        if rng.integers(3) == 0:
            b, o = c.shards[e][int(rng.integers(k + m))]
            bufs[b][o + int(rng.integers(c.sizes[e]))] ^= 1 << int(rng.integers(8))
            hit.add(e)
    assert hit and len(hit) < len(c.live)
    present = np.ones((len(c.sizes), k + m), np.uint8)
    got, t, plan = verify_mixed(c, bufs, present)
    ref = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    plan.verify(ref)
    torch.cuda.synchronize()
    assert np.array_equal(got, ref.cpu().numpy().astype(np.uint32))
    assert np.array_equal(got, oracle_flags(c, bufs, present))
    assert set(np.nonzero(got)[0].tolist()) == hit


# ---- 3. exact flags under single-bit flips ----

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
    base = live_sizes(300 + k)
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
    """Buffers with one bit flipped per listed stripe.  in_missing: in a shard its
    mask (already in `present`) calls missing.  Otherwise in a present shard: per
    position name the roles survivor 0..k-1, checked 0..m-1 are taken in turn,
    and the stripe gets a mask under which that role exists (checked q needs
    k + q + 1 present); returns the (role, name) pairs covered."""
    k, m, n = c.k, c.m, c.k + c.m
    bufs = [x.copy() for x in c.bufs]
    roles, turn = set(), {}
    for q, (e, p, names) in enumerate(flips):
        names = names or ("byte",)
        if in_missing:
            gone = [i for i in range(n) if not present[e][i]]
            i = gone[q % len(gone)]
        else:
            role = turn.get(names[0], 0) % n
            turn[names[0]] = role + 1
            fits = masks_up_to(n, m - 1 - max(0, role - k))
            present[e] = fits[(5 * q + 1) % len(fits)]
            i = [j for j in range(n) if present[e][j]][role]
            roles |= {(role if role < k else ("checked", role - k), nm) for nm in names}
        b, o = c.shards[e][i]
        assert c.sizes[e] > p
        bufs[b][o + p] ^= 1 << (q % 8)
    return bufs, roles


def check_flips(k, m, layout):
    c, flips = flip_case(k, m, layout)
    n = k + m
    flip_entries = {e for e, _, _ in flips}
    assert len(c.live) == 2 * len(flips) and c.sizes[0] == 0 and c.sizes[-1] == 0 and c.sizes.count(0) == 4
    # (a) flips in present shards (flipped() gives those stripes a mask with a spare shard)
    anym = masks_up_to(n, m)
    present = np.ones((len(c.sizes), n), np.uint8)
    for q, e in enumerate(c.live):
        present[e] = anym[(7 * q + 2) % len(anym)]
    bufs, roles = flipped(c, flips, present, in_missing=False)
    names = ["0", "1", "15", "16", "S-17", "S-2", "S-1", "W-1", "W", "T-1", "T", "byte"]
    for role in list(range(k)) + [("checked", q) for q in range(m)]:
        for nm in names:
            assert (role, nm) in roles, (role, nm)
    want = oracle_flags(c, bufs, present)
    assert {e for e in c.live if want[e] & 1} == flip_entries  # exactly the flipped stripes
    got, t, _ = verify_mixed(c, bufs, present)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    MP.check_equal(t, bufs)
    # (b) the same flips in missing shards flag nothing
    lossy = masks_up_to(n, m, lost_min=1)
    for q, e in enumerate(c.live):
        present[e] = lossy[(5 * q + 1) % len(lossy)] if e in flip_entries else anym[(7 * q + 2) % len(anym)]
    bufs, _ = flipped(c, flips, present, in_missing=True)
    want = oracle_flags(c, bufs, present)
    assert not (want & 1).any()
    got, _, _ = verify_mixed(c, bufs, present)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_single_bit_flips_flag_exactly_their_stripes(k, m, layout):
    check_flips(k, m, layout)


# ---- 4. patterns and stripes do not cost launches ----

def launches_of(c, present):
    inp, _ = c.garble(present)
    s0 = B.verify_mixed_plan_stats()
    got, _, _ = verify_mixed(c, inp, present)
    s1 = B.verify_mixed_plan_stats()
    assert np.array_equal(got, oracle_flags(c, inp, present))
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    return s1["kernel_launches"] - s0["kernel_launches"]


def test_launches_do_not_depend_on_stripes_or_masks():
    k, m = 4, 2
    small, large = case(k, m, "stripes", 40), case(k, m, "stripes", 400)
    assert len(small.live) >= 40 and len(large.live) >= 400 and len(small.live) < 100
    masks = masks_up_to(6, 2)
    assert len(masks) == 22
    d = [launches_of(small, MP.spread(small, masks[1:2], 3)), launches_of(small, MP.spread(small, masks, 3)),
         launches_of(large, MP.spread(large, masks[1:2], 3)), launches_of(large, MP.spread(large, masks, 3))]
    assert d == [1, 1, 1, 1]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_launch_boundaries_anywhere_in_the_tile_list(layout):
    k, m = 4, 2
    masks = masks_up_to(6, 2)
    c = case(k, m, layout, len(masks))
    present = MP.spread(c, masks, 1)
    T = tile()
    n_tiles = sum(-(-s // T) for s in c.sizes)
    assert n_tiles > 70
    B.set_verify_mixed_plan_chunk_tiles(7)
    try:
        s0 = B.verify_mixed_plan_stats()
        check_clean(c, present)
        s1 = B.verify_mixed_plan_stats()
        check_flips(k, m, layout)
    finally:
        B.set_verify_mixed_plan_chunk_tiles(0)
    assert s1["kernel_launches"] - s0["kernel_launches"] == -(-n_tiles // 7)


# ---- 5. flags are ORed ----

@pytest.mark.parametrize("dtype", [torch.int32, torch.uint32])
def test_flags_are_ored_into_what_the_caller_had(dtype):
    k, m = 4, 2
    c = case(k, m, "stripes")
    rng = np.random.default_rng(50)
    bufs = [x.copy() for x in c.bufs]
    for e in c.live[::2]:
        b, o = c.shards[e][5]  # the last shard: checked whenever it and > k shards are present
        bufs[b][o + int(rng.integers(c.sizes[e]))] ^= 0x10
    first = MP.spread(c, masks_up_to(6, 1), 51)
    second = MP.spread(c, MP.masks_with_missing(6, [1, 2]), 52)
    got, t, plan = verify_mixed(c, bufs, first, prefill=4, dtype=dtype)
    want = 4 | oracle_flags(c, bufs, first)
    want[[e for e, s in enumerate(c.sizes) if s == 0]] = 4
    assert np.array_equal(got, want)
    # a second call on the same flags: bit 1 joins bit 0
    flags = torch.from_numpy(got.astype(np.int32)).cuda().view(dtype)
    plan.verify_mixed(second, flags)
    torch.cuda.synchronize()
    want |= oracle_flags(c, bufs, second)
    assert np.array_equal(flags.view(torch.int32).cpu().numpy().astype(np.uint32), want)
    assert {4, 5, 6, 7} == set(want.tolist())
    n = len(c.sizes)
    for bad in (torch.zeros(n - 1, dtype=torch.int32, device="cuda").view(dtype),  # short
                torch.zeros(n, dtype=torch.int32).view(dtype),  # on the host
                torch.zeros(n, dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            plan.verify_mixed(first, bad)
    with pytest.raises(ValueError):
        plan.verify_mixed(first[:-1], flags)


# ---- 6. the other route ----

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(13, 2), (4, 5)])
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
    want = oracle_flags(c, inp, present)
    assert {0, 1, 2} == set(want.tolist())
    s0 = B.verify_mixed_plan_stats()
    got, t, _ = verify_mixed(c, inp, present)
    s1 = B.verify_mixed_plan_stats()
    assert np.array_equal(got, want), (got, want)
    MP.check_equal(t, inp)
    assert s1["per_stripe_calls"] - s0["per_stripe_calls"] == 12
    assert s1["kernel_launches"] == s0["kernel_launches"]


# ---- 7. errors leave no trace ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_errors_leave_no_trace(layout):
    k, m = 4, 2
    c = case(k, m, layout)
    enc = RS.New(k, m)
    n = len(c.sizes)
    present = MP.spread(c, masks_up_to(6, 2), 70)
    bufs = [x.copy() for x in c.bufs]
    for e in c.live[::3]:
        b, o = c.shards[e][[i for i in range(6) if present[e][i]][0]]
        bufs[b][o] ^= 0x80
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    pats, idx = np.unique(present, axis=0, return_inverse=True)
    pats = np.ascontiguousarray(pats, np.uint8)
    idx = np.ascontiguousarray(idx.reshape(-1), np.uint32)

    def call(p, i, n_patterns=None, e=enc):
        return N.lib().hbec_verify_plan_mixed(e.handle, plan._h, p.ctypes.data_as(N._U8P),
                                              p.shape[0] if n_patterns is None else n_patterns,
                                              i.ctypes.data_as(U32P), C.c_void_p(flags.data_ptr()), None)

    s0 = B.verify_mixed_plan_stats()
    assert call(pats, idx, e=RS.New(8, 3)) == N.ERR_INVALID_ARG
    bad = idx.copy()
    bad[n - 1] = pats.shape[0]  # the last entry is zero-length: checked all the same
    assert c.sizes[n - 1] == 0
    assert call(pats, bad) == N.ERR_INVALID_ARG and "index" in N.last_error()
    few = np.vstack([pats, np.array([[1, 1, 1, 0, 0, 0]], np.uint8)])  # listed, unused
    assert call(few, idx) == N.ERR_TOO_FEW_SHARDS
    assert call(pats, idx, n_patterns=0) == N.ERR_INVALID_ARG
    assert call(pats, idx, n_patterns=65537) == N.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert B.verify_mixed_plan_stats() == s0
    assert not flags.cpu().numpy().any()
    assert call(pats, idx) == N.HBEC_OK
    torch.cuda.synchronize()
    want = oracle_flags(c, bufs, present)
    assert np.array_equal(flags.cpu().numpy().astype(np.uint32), want) and (want & 1).any()
    MP.check_equal(t, bufs)


# ---- 8. two streams, one plan ----

@pytest.mark.parametrize("layout", LAYOUTS)
def test_verify_and_reconstruct_from_two_streams_keep_their_words_apart(layout):
    k, m = 8, 3
    n = k + m
    c = case(k, m, layout, 60)
    rng = np.random.default_rng(80)
    # B rebuilds `lost`; A and C call those shards missing too, so nothing B writes is read
    mask_b = np.ones((len(c.sizes), n), np.uint8)
    mask_a, mask_c = mask_b.copy(), mask_b.copy()
    for q, e in enumerate(c.live):
        lost = rng.choice(n, size=1 + q % 2, replace=False)
        mask_b[e][lost] = 0
        mask_a[e][lost] = 0
        mask_c[e][lost] = 0
        spare = [i for i in range(n) if mask_b[e][i]][k:]  # present, not read by the reconstruct
        if q % 3 == 0:
            mask_c[e][spare] = 0  # exactly k left
        elif q % 3 == 1:
            mask_a[e][spare[-1]] = 0
    inp, rebuilt = c.garble(mask_b)
    for q, e in enumerate(c.live):  # corrupt spare shards only: the reconstruct still rebuilds clean bytes
        if q % 4 < 2:
            spare = [i for i in range(n) if mask_b[e][i]][k:]
            b, o = c.shards[e][spare[0]]
            for buf in (inp, rebuilt):
                buf[b][o + c.sizes[e] // 2] ^= 0x04
    want_a, want_c = oracle_flags(c, inp, mask_a), oracle_flags(c, inp, mask_c)
    assert (want_a & 1).any() and (want_c & 2).any() and not np.array_equal(want_a, want_c)
    enc = RS.New(k, m)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    flags_a = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    flags_c = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.verify_mixed(mask_a, flags_a, stream=s1)
    plan.reconstruct_mixed(mask_b, stream=s2)
    plan.verify_mixed(mask_c, flags_c, stream=s2)
    torch.cuda.synchronize()
    assert np.array_equal(flags_a.cpu().numpy().astype(np.uint32), want_a)
    assert np.array_equal(flags_c.cpu().numpy().astype(np.uint32), want_c)
    MP.check_equal(t, rebuilt)
