"""Exhaustive single-flip sweep of gf_verify_mixed_plan<RMAX> (csrc/vmixed.hip,
behind plan.verify_mixed): one stripe per flip, every byte position of every
checked shard and every position p of survivor number p % k, under every mask
of a case in ONE call.

The kernel has a tile of its own (verify_mixed_tile<R>: the accumulators start
as the stored columns, its own compare mask and lane predicate), so the sweep
of unaligned_tile's VERIFY mode says nothing about it.  A wrong predicate here
writes no wrong byte: it calls a corrupt survivor safe to rebuild from.

Expected flags follow from the oracle alone.  The clean codeword is coracle's
(build_matrix / apply).  The decode row of a checked shard over the survivors
is a Lagrange basis evaluated off the survivor points (oracle/lagrange.py), so
it has no zero entry - asserted per mask with lagrange_row - hence a single-bit
flip in any present shard makes the stripe inconsistent and a flip in a missing
shard changes nothing: 1 on every flipped stripe, 0 on every control (every
61st stripe), 2 on every stripe whose mask leaves exactly k, flipped (in a
missing shard) or not; on the all-clean replica 0, and 2 on exactly-k.  Missing
shards hold garbage that differs from the codeword at every byte.  The buffer
must be bit-identical after the call.  No tolerance, no sampling of positions.

Layout, placement and the flipped bit are test_gpu_verify_sweep's: base offset
3 and an odd pitch, so the stripes take all 16 alignments (asserted), S odd, so
the shards of one stripe differ in alignment; flips in a seeded random order,
so the masks are interleaved in stripe order and consecutive tiles of a wave's
walk change R and pattern record (asserted).  With T =
verify_mixed_plan_tile_bytes() = 4 x 992: S = T + 992 + 37 for k + m <= 7 and
T + 37 above - three window seams, the tile seam, a ragged end inside a lane.

  every-length  8+3 and 4+2 plans with stripes of every S = 1 .. T + 992 + 64,
                bases cycling through all 16 alignments: a flip at S - 1 of a
                checked shard whose successor in memory is a missing shard, and
                at S - 1 of a survivor whose successor is one - a compare or a
                multiply that reaches one byte past S reads garbage and raises
                a false flag on the controls.
  chunked       the 4+2 case under hbec_set_verify_mixed_plan_chunk_tiles(3).
  other route   13+2, degraded masks, S = 301: the same flip set through
                apply + gf_vm_compare, counted per stripe.
"""
import numpy as np
import pytest
import torch

from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import lagrange as LG

import test_gpu_verify_sweep as VS

pytestmark = pytest.mark.gpu

W = 992  # one 64-lane window of the kernel (unaligned_tile.h)


def tile():
    return B.verify_mixed_plan_tile_bytes()


def roles(k, m, mask):
    """(survivors, checked, missing) shard indices under a present mask."""
    here = [i for i in range(k + m) if mask[i]]
    assert len(here) >= k
    return here[:k], here[k:], [i for i in range(k + m) if not mask[i]]


def lose(k, m, *lost):
    return tuple(0 if i in lost else 1 for i in range(k + m))


def assert_any_flip_shows(k, m, mask):
    """No zero in the decode row of any checked shard: a flip in any survivor
    changes what every checked shard must be, a flip in a checked shard itself."""
    surv, checked, _ = roles(k, m, mask)
    for c in checked:
        assert all(x != 0 for x in LG.lagrange_row(surv, c)), (mask, c)


def bit(pos, role):
    return (1 << ((pos + pos // 8 + role) % 8)).astype(np.uint8)


def flip_set(k, m, S, masks):
    """(mask index, shard, position, xor value) of every flip.  A mask with R
    checked shards: each at every position (role r), then survivor p % k at
    every position p (role R).  An exactly-k mask: 32 positions over the shard,
    in its missing shards in turn."""
    P = np.arange(S, dtype=np.int64)
    q_, sh_, pos_, val_ = [], [], [], []
    for q, mask in enumerate(masks):
        surv, checked, gone = roles(k, m, mask)
        if checked:
            assert_any_flip_shows(k, m, mask)
            shard = np.concatenate([np.full(S, c, np.int64) for c in checked] + [np.array(surv, np.int64)[P % k]])
            pos = np.tile(P, len(checked) + 1)
            role = np.repeat(np.arange(len(checked) + 1, dtype=np.int64), S)
            # every checked role at every position, every survivor slot
            assert S >= k and set(shard.tolist()) == set(surv) | set(checked)
        else:
            pos = np.unique(np.linspace(0, S - 1, 32).astype(np.int64))
            shard = np.array(gone, np.int64)[np.arange(pos.size) % len(gone)]
            role = np.zeros(pos.size, np.int64)
        q_.append(np.full(pos.size, q, np.int64))
        sh_.append(shard)
        pos_.append(pos)
        val_.append(bit(pos, role))
    return tuple(np.concatenate(x) for x in (q_, sh_, pos_, val_))


def stats_delta(s0):
    s1 = B.verify_mixed_plan_stats()
    return {f: s1[f] - s0[f] for f in s0}


def sweep(label, k, m, S, masks, want_r, route="kernel", chunk=0):
    """One case: all masks in one call, flagged and then all-clean."""
    masks = [tuple(x) for x in masks]
    checked_counts = {len(roles(k, m, x)[1]) for x in masks}
    assert checked_counts == set(want_r) | {0}, checked_counts  # every R named, and an exactly-k mask
    fq, shard, pos, val = flip_set(k, m, S, masks)
    n, obj = VS.placement(fq.size, 1000 * k + m)
    stripe_mask = np.empty(n, np.int64)
    stripe_mask[obj] = fq
    ctrl = np.setdiff1d(np.arange(n), obj)
    assert ctrl.size >= n // VS.CONTROL_EVERY and np.all((np.arange(n) % VS.CONTROL_EVERY != VS.CONTROL_EVERY - 1)
                                                         | np.isin(np.arange(n), ctrl))  # every 61st is a control
    stripe_mask[ctrl] = np.arange(ctrl.size) % len(masks)
    if len(masks) > 2:  # fully swept masks interleaved: a wave's next tile is often another R and record
        assert (np.diff(stripe_mask) != 0).sum() >= n // 4
    marr = np.array(masks, np.uint8)
    present = marr[stripe_mask]
    exactly_k = present.sum(axis=1) == k
    assert exactly_k.any() and exactly_k[ctrl].any()
    want_clean = np.where(exactly_k, 2, 0).astype(np.int32)
    want = want_clean.copy()
    want[obj] = 1
    want[exactly_k] = 2

    lay = VS.Layout(k, m, S, aligned=False)
    (_, _, off, pitch), = lay.parts
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
    for q, mask in enumerate(masks):
        idx = torch.from_numpy(np.nonzero(stripe_mask == q)[0]).cuda()
        for g in roles(k, m, mask)[2]:
            junk = cw[g * S:(g + 1) * S] ^ rng.integers(1, 256, S, dtype=np.uint8)
            rows[idx, g * S:(g + 1) * S] = torch.from_numpy(junk).cuda()
    VS.xor_flips(bufs, lay, obj, shard, pos, val)
    keep = buf.clone()

    enc = RS.New(k, m)
    base = buf.data_ptr() + off
    plan = B.StripePlan(enc, stripes=[(base + o * pitch, S) for o in range(n)])
    n_tiles = n * -(-S // tile())
    if route == "kernel":
        want_delta = {"kernel_launches": -(-n_tiles // chunk) if chunk else 1, "per_stripe_calls": 0}
    else:
        want_delta = {"kernel_launches": 0, "per_stripe_calls": n}

    def call(expect, what):
        flags = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        s0 = B.verify_mixed_plan_stats()
        plan.verify_mixed(present, flags)
        torch.cuda.synchronize()
        d = stats_delta(s0)
        got = flags.cpu().numpy()
        if not np.array_equal(got, expect):
            flipped = np.zeros(n, bool)
            flipped[obj] = what == "flipped"
            where = np.full(n, -1, np.int64)
            where[obj] = np.arange(obj.size)
            missed = np.nonzero(flipped & (got != expect))[0]
            other = np.nonzero(~flipped & (got != expect))[0]
            pytest.fail(f"{label} {k}+{m} S={S} {what}: {missed.size} of {obj.size} flipped stripes wrong, first "
                        f"(mask, shard, position, got): "
                        f"{[(masks[fq[where[o]]], int(shard[where[o]]), int(pos[where[o]]), int(got[o])) for o in missed[:8]]}"
                        f"; {other.size} unflipped stripes wrong, first (stripe, mask, got, want): "
                        f"{[(int(o), masks[stripe_mask[o]], int(got[o]), int(expect[o])) for o in other[:8]]}")
        assert d == want_delta, (label, what, d, want_delta)
        return d

    try:
        if chunk:
            B.set_verify_mixed_plan_chunk_tiles(chunk)
        call(want, "flipped")
        assert torch.equal(buf, keep), (label, "the buffer was written")
        VS.xor_flips(bufs, lay, obj, shard, pos, val)  # the clean replica
        d = call(want_clean, "clean")
    finally:
        if chunk:
            B.set_verify_mixed_plan_chunk_tiles(0)
    print(f"SWEEP vmixed-{label} {k}+{m} S={S} masks={len(masks)} R={sorted(checked_counts)} stripes={n} "
          f"flips={obj.size} exactly_k={int(exactly_k.sum())} resident={resident} per call {d}")


def small_s(k, m):
    return tile() + (W if k + m <= 7 else 0) + 37


# (id, k, m, masks with something to check, the counts of checked shards they give, the exactly-k mask)
CASES = [
    # K = 1, R = 4: the j + 1 < K prefetch is never taken
    ("1+4", 1, 4, [lose(1, 4)], {4}, lose(1, 4, 0, 1, 3, 4)),
    ("3+1", 3, 1, [lose(3, 1)], {1}, lose(3, 1, 1)),
    # R = 2; one data lost: R = 1 with parity 4 among the survivors; one parity lost: R = 1
    ("4+2", 4, 2, [lose(4, 2), lose(4, 2, 1), lose(4, 2, 4)], {2, 1}, lose(4, 2, 0, 5)),
    # R = 3, 2, 1; two data lost: survivors 6 and 7 are parity
    ("8+3", 8, 3, [lose(8, 3), lose(8, 3, 2), lose(8, 3, 1, 5)], {3, 2, 1}, lose(8, 3, 0, 4, 9)),
    # R = 3 with survivors 8 and 9 from the s_hi word, slot 9 a parity shard
    ("10+4", 10, 4, [lose(10, 4, 3)], {3}, lose(10, 4, 2, 7, 10, 13)),
    # R = 4 with K = 12; one data and one parity lost: R = 2
    ("12+4", 12, 4, [lose(12, 4), lose(12, 4, 5, 13)], {4, 2}, lose(12, 4, 0, 6, 12, 15)),
]


def test_cases_cover_what_they_name():
    """Host only: the roles of the masks above."""
    by = {c[0]: c for c in CASES}
    s, c, _ = roles(4, 2, by["4+2"][3][1])
    assert 4 in s and c == [5]
    s, c, _ = roles(8, 3, by["8+3"][3][2])
    assert s[6:] == [8, 9] and c == [10]
    s, c, _ = roles(10, 4, by["10+4"][3][0])
    assert s[8:] == [9, 10] and c == [11, 12, 13]
    s, c, _ = roles(12, 4, by["12+4"][3][0])
    assert len(s) == 12 and c == [12, 13, 14, 15]
    assert {r for c in CASES for r in c[4]} == {1, 2, 3, 4}  # every R occurs
    for _, k, m, masks, _, ek in CASES:
        assert sum(ek) == k and all(sum(x) > k for x in masks)


@pytest.mark.parametrize("label,k,m,masks,want_r,exactly_k", CASES, ids=[c[0] for c in CASES])
def test_every_byte_of_every_role(label, k, m, masks, want_r, exactly_k):
    sweep(label, k, m, small_s(k, m), masks + [exactly_k], want_r)


def test_chunked_launches_4_2():
    label, k, m, masks, want_r, exactly_k = CASES[2]
    sweep("chunked-" + label, k, m, small_s(k, m), masks + [exactly_k], want_r, chunk=3)


def test_other_route_13_2():
    """k > 12: every stripe one at a time; degraded masks go through an apply
    into scratch and gf_vm_compare."""
    k, m = 13, 2
    sweep("other-route", k, m, 301, [lose(k, m, 4), lose(k, m, 13), lose(k, m, 0, 14)], {1}, route="other")


# ---- every length -------------------------------------------------------------

@pytest.mark.parametrize("k,m,lost_a,flip_a,lost_b,flip_b", [(8, 3, 10, 9, 3, 2), (4, 2, 5, 4, 2, 1)],
                         ids=["8+3", "4+2"])
def test_every_length(k, m, lost_a, flip_a, lost_b, flip_b):
    """Three stripes per length S = 1 .. T + 992 + 64: mask A flipped at S - 1
    of checked shard flip_a (the next shard in memory, lost_a, is missing), a
    control (mask A for even S, B for odd), mask B flipped at S - 1 of survivor
    flip_b (the next shard, lost_b, is missing)."""
    L = k + m
    top = tile() + W + 64
    mask_a, mask_b = lose(k, m, lost_a), lose(k, m, lost_b)
    assert flip_a in roles(k, m, mask_a)[1] and lost_a == flip_a + 1
    assert flip_b in roles(k, m, mask_b)[0] and lost_b == flip_b + 1
    assert_any_flip_shows(k, m, mask_a)
    assert_any_flip_shows(k, m, mask_b)
    cw = VS.codeword(k, m, top, 97 * k + m).reshape(L, top)  # a prefix of a codeword is a codeword
    rng = np.random.default_rng(5 * k + m)
    n = 3 * top
    S = np.repeat(np.arange(1, top + 1, dtype=np.int64), 3)
    kind = np.tile(np.array([0, 1, 2]), top)
    use_b = (kind == 2) | ((kind == 1) & (S % 2 == 1))
    base = np.empty(n, np.int64)
    cur = 0
    for q in range(n):  # at least 5 slack bytes, then up to the alignment q % 16
        o = cur + 5
        o += (q - o) % 16
        base[q] = o
        cur = o + L * int(S[q])
    total = cur + 11
    assert 2 * total <= VS.CAP
    host = np.full(total, VS.FILL, np.uint8)
    for s in range(1, top + 1):
        row = np.ascontiguousarray(cw[:, :s]).reshape(-1)
        for q in range(3 * (s - 1), 3 * s):
            g = lost_b if use_b[q] else lost_a
            at = int(base[q])
            host[at:at + L * s] = row
            host[at + g * s:at + (g + 1) * s] ^= rng.integers(1, 256, s, dtype=np.uint8)  # garbage, every byte
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    for kd in (0, 2):
        assert set((base[kind == kd] % 16).tolist()) == set(range(16))  # all 16 alignments, both flips
    present = np.where(use_b[:, None], np.array(mask_b, np.uint8), np.array(mask_a, np.uint8))
    fshard = np.where(kind == 0, flip_a, flip_b)
    flipped = kind != 1
    idx = torch.from_numpy((base + fshard * S + S - 1)[flipped]).cuda()
    val = torch.from_numpy(bit(S - 1, fshard)[flipped]).cuda()
    enc = RS.New(k, m)
    plan = B.StripePlan(enc, stripes=[(buf.data_ptr() + int(b), int(s)) for b, s in zip(base, S)])

    def call(expect, what):
        flags = torch.zeros(n, dtype=torch.int32, device="cuda")
        s0 = B.verify_mixed_plan_stats()
        plan.verify_mixed(present, flags)
        torch.cuda.synchronize()
        assert stats_delta(s0) == {"kernel_launches": 1, "per_stripe_calls": 0}
        got = flags.cpu().numpy()
        bad = np.nonzero(got != expect)[0]
        assert bad.size == 0, (f"{k}+{m} every-length {what}: {bad.size} stripes wrong, first (S, kind, base mod 16, "
                               f"got, want): {[(int(S[i]), int(kind[i]), int(base[i] % 16), int(got[i]), int(expect[i])) for i in bad[:12]]}")

    call(np.zeros(n, np.int32), "clean")
    buf[idx] = buf[idx] ^ val
    keep = buf.clone()
    call(flipped.astype(np.int32), "flipped")
    assert torch.equal(buf, keep)
    print(f"SWEEP vmixed-every-length {k}+{m} S=1..{top} stripes={n} flips={int(flipped.sum())} resident={2 * total}")
