"""Blind-spot sweep of gf_repair_mixed_plan<RMAX> (csrc/repair.hip, behind
plan.repair_mixed): every shard length around the window and tile seams at every
alignment, and one flipped bit at every byte position of one checked shard and
of one survivor slot, in ONE call per case.

The kernel's tile stores some rows (unaligned_tile's aligned-block, bytewise-tail
and head logic) and tests the others (verify_mixed_tile's compare mask and lane
predicate) after one multiply loop, so neither of the sweeps of those two tiles
says anything about it.  A wrong store predicate writes a wrong byte or a byte
outside its shard; a wrong compare predicate writes nothing wrong: it calls a
corrupt survivor safe to commit from.

Stripes of a case (one mask for all, so one (r_o, r_c) tile; W = 992, T =
repair_plan_tile_bytes() = 4 W):

  lengths  one stripe of every S in 1 .. W + 64, T - 64 .. T + 64 and
           2T - 64 .. 2T + 64, unflipped.  Stripe q of these sits at a base of
           class (q // 16) % 16 mod 16, so every (S mod 16, base mod 16) class
           occurs: asserted on the layout before the GPU is touched.  S mostly
           odd, so the shards of one stripe differ in alignment.
  flips    for every byte position p in [0, 2T): one stripe with one bit flipped
           at p of the first checked shard and one with one bit flipped at p of
           survivor slot p % k.  Their lengths are taken in turn from the lengths
           above that hold p (the nearest of the three ranges), so the flip falls
           at every distance from a ragged end.

Every stripe is a prefix of one codeword from the oracle (coracle build_matrix /
apply; a prefix of a codeword is a codeword) with garbage in its missing shards.
Expected bytes: the clean codeword in every missing shard; under a flipped
survivor, the clean bytes with, at p, the product of the flipped bits and the
decode coefficient of that survivor (coracle.apply of lagrange_row(survivors,
shard) on the difference alone).  Expected flags: 1 on every flipped stripe (no
decode row of a checked shard has a zero entry: asserted), 0 on every other.
Bytes outside the shards hold a fill pattern.  The WHOLE buffer and the WHOLE
flag array are compared exactly.
"""
import numpy as np
import pytest
import torch

from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO
from oracle import lagrange as LG

pytestmark = pytest.mark.gpu

W = 992  # one 64-lane window of the kernel (unaligned_tile.h)
FILL = 0xA5
CAP = 4 << 30  # bytes resident per case


def tile():
    return B.repair_plan_tile_bytes()


def lengths():
    T = tile()
    return list(range(1, W + 65)) + list(range(T - 64, T + 65)) + list(range(2 * T - 64, 2 * T + 65))


def lose(k, m, *lost):
    return tuple(0 if i in lost else 1 for i in range(k + m))


# (id, k, m, mask): one (r_o, r_c) split per total R = 1..4; K = 4, 8 and 12 at R = 4
CASES = [
    ("R1-3+1-(0,1)", 3, 1, lose(3, 1)),
    ("R2-4+2-(1,1)", 4, 2, lose(4, 2, 1)),
    ("R3-8+3-(1,2)", 8, 3, lose(8, 3, 2)),
    ("R4-4+4-(2,2)", 4, 4, lose(4, 4, 0, 5)),
    ("R4-8+4-(1,3)", 8, 4, lose(8, 4, 3)),
    ("R4-12+4-(3,1)", 12, 4, lose(12, 4, 1, 7, 13)),
]


def roles(k, m, mask):
    here = [i for i in range(k + m) if mask[i]]
    return here[:k], here[k:], [i for i in range(k + m) if not mask[i]]


def test_cases_cover_what_they_name():
    """Host only."""
    splits = {}
    for label, k, m, mask in CASES:
        _, checked, gone = roles(k, m, mask)
        assert len(gone) + len(checked) == m and checked  # something to flip in a checked shard
        assert f"({len(gone)},{len(checked)})" in label
        splits.setdefault(m, set()).add((k, len(gone), len(checked)))
    assert set(splits) == {1, 2, 3, 4} and {k for k, _, _ in splits[4]} == {4, 8, 12}
    assert any(o and c for s in splits.values() for _, o, c in s)
    T = tile()
    L = lengths()
    assert len(L) == len(set(L)) == W + 64 + 2 * 129 and max(L) == 2 * T + 64


def layout(k, m):
    """Sizes, bases and the flips of one case: (S[n], base[n], flip stripe
    indices, shard-relative role (0 checked, 1 survivor), positions)."""
    T = tile()
    L = np.array(lengths(), np.int64)
    ranges = [L[L <= W + 64], L[(L > W + 64) & (L <= T + 64)], L[L > T + 64]]
    sizes, kind, pos = list(L), [-1] * len(L), [0] * len(L)
    turn = 0
    for p in range(2 * T):
        fits = next(r[r > p] for r in ranges if (r > p).any())
        for role in (0, 1):
            sizes.append(int(fits[turn % fits.size]))
            kind.append(role)
            pos.append(p)
            turn += 7
    S = np.array(sizes, np.int64)
    n = S.size
    base = np.empty(n, np.int64)
    cur = 0
    for q in range(n):  # at least 5 bytes of fill, then up to the stripe's alignment class
        cls = (q // 16) % 16 if q < L.size else q % 16
        o = cur + 5
        o += (cls - o) % 16
        base[q] = o
        cur = o + (k + m) * int(S[q])
    return S, base, cur + 11, np.array(kind, np.int64), np.array(pos, np.int64), L.size


@pytest.mark.parametrize("label,k,m,mask", CASES, ids=[c[0] for c in CASES])
def test_every_length_alignment_and_flip_position(label, k, m, mask):
    n_sh = k + m
    T = tile()
    surv, checked, gone = roles(k, m, mask)
    for c in checked:  # a flip in any survivor changes what every checked shard must be
        assert all(x != 0 for x in LG.lagrange_row(surv, c)), (mask, c)
    S, base, total, kind, pos, n_len = layout(k, m)
    n = S.size
    assert 2 * total <= CAP, total
    # every (S mod 16, base mod 16) class among the unflipped stripes of every length
    assert {(int(s) % 16, int(b) % 16) for s, b in zip(S[:n_len], base[:n_len])} == {(a, b) for a in range(16)
                                                                                     for b in range(16)}
    flips = np.nonzero(kind >= 0)[0]
    assert flips.size == 2 * 2 * T and (S[flips] > pos[flips]).all() and S[flips].max() <= 2 * T + 64
    for role in (0, 1):  # every position of each role, at several distances from the end of the shard
        sel = flips[kind[flips] == role]
        assert np.array_equal(np.sort(pos[sel]), np.arange(2 * T))
        assert np.unique((S[sel] - pos[sel])[pos[sel] < W]).size > 100

    top = int(S.max())
    rng = np.random.default_rng(97 * k + m)
    data = [rng.integers(0, 256, top, dtype=np.uint8) for _ in range(k)]
    cw = np.stack(data + list(CO.apply(CO.build_matrix(k, m)[k:], data)))  # [k + m, top]
    junk = rng.integers(0, 256, top + n, dtype=np.uint8)
    inp = np.full(total, FILL, np.uint8)
    want = np.full(total, FILL, np.uint8)
    for q in range(n):
        s, at = int(S[q]), int(base[q])
        row = np.ascontiguousarray(cw[:, :s]).reshape(-1)
        want[at:at + n_sh * s] = row
        inp[at:at + n_sh * s] = row
        for g in gone:
            inp[at + g * s:at + (g + 1) * s] = junk[q:q + s]
    # the flips: bit (p + role) % 8 at position p of checked[0] / survivor slot p % k
    fshard = np.where(kind[flips] == 0, checked[0], np.array(surv, np.int64)[pos[flips] % k])
    bit = (pos[flips] + kind[flips]) % 8
    at = base[flips] + fshard * S[flips] + pos[flips]
    inp[at] ^= (1 << bit).astype(np.uint8)
    want[at] ^= (1 << bit).astype(np.uint8)  # present shards are not written
    # under a flipped survivor every rebuilt shard differs at p by coefficient x flipped bit
    if gone:
        rows = [LG.lagrange_row(surv, g) for g in gone]
        for j in range(k):
            delta = [np.zeros(8, np.uint8) for _ in range(k)]
            delta[j] = (1 << np.arange(8)).astype(np.uint8)
            out = CO.apply(rows, delta)  # [r_o][8]: what bit b of survivor slot j adds to each output
            sel = (kind[flips] == 1) & (pos[flips] % k == j)
            for g, d in zip(gone, out):
                assert d.all()
                want[base[flips][sel] + g * S[flips][sel] + pos[flips][sel]] ^= np.asarray(d, np.uint8)[bit[sel]]
    want_flags = (kind >= 0).astype(np.int32)

    buf = torch.from_numpy(inp).cuda()
    ref = torch.from_numpy(want).cuda()
    enc = RS.New(k, m)
    plan = B.StripePlan(enc, stripes=[(buf.data_ptr() + int(b), int(s)) for b, s in zip(base, S)])
    present = np.tile(np.array(mask, np.uint8), (n, 1))
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s0 = B.repair_plan_stats()
    plan.repair_mixed(present, flags)
    torch.cuda.synchronize()
    s1 = B.repair_plan_stats()
    got = flags.cpu().numpy()
    bad = np.nonzero(got != want_flags)[0]
    assert bad.size == 0, (f"{label}: {bad.size} flags wrong, first (stripe, S, base mod 16, role, position, got): "
                           f"{[(int(q), int(S[q]), int(base[q] % 16), int(kind[q]), int(pos[q]), int(got[q])) for q in bad[:10]]}")
    if not torch.equal(buf, ref):
        diff = torch.nonzero(buf != ref).reshape(-1).cpu().numpy()
        q = np.searchsorted(base, diff, side="right") - 1
        where = [(int(i), int(S[j]), int(base[j] % 16), int((d - base[j]) // S[j]), int((d - base[j]) % S[j]))
                 for i, j, d in zip(q[:10], q[:10], diff[:10])]
        pytest.fail(f"{label}: {diff.size} bytes wrong, first (stripe, S, base mod 16, shard, position): {where}")
    assert {f: s1[f] - s0[f] for f in s0} == {"kernel_launches": 1, "per_stripe_calls": 0}
    print(f"SWEEP repair-{label} mask={mask} stripes={n} lengths={n_len} flips={flips.size} resident={2 * total}")
