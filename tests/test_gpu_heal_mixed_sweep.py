"""Blind-spot sweep of gf_heal_mixed_plan<RMAX> (csrc/heal.hip, behind
plan.heal_mixed): every shard length around the window and tile seams at every
alignment, with the named shard rewritten in place, in ONE call per case.

A heal rewrites a shard that sits between shards it reads: the named shard is a
present one, so its neighbours on both sides are survivors or checked shards of
the same stripe, and a head, tail or realigned store that strays by one byte
lands in data the same tile is reading or has just checked.  gf_repair_mixed_plan
never sees that: its outputs are shards the mask calls missing.  These are the
smallest shapes at which those stores can go wrong.

Stripes of a case (one mask for all; W = 992, T = heal_plan_tile_bytes() = 4 W):
one stripe of every S in 1 .. W + 64, T - 64 .. T + 64 and 2T - 64 .. 2T + 64.
Stripe q sits at a base of class (q // 16) % 16 mod 16, so every (S mod 16, base
mod 16) class occurs: asserted on the layout before the GPU is touched.  The
word of stripe q is forged so that the named shard is

  (a) survivor slot q % k of the mask: a later present shard moves into the
      survivor set, or
  (b) checked shard q % r of the mask.

Every stripe is a prefix of one codeword from the oracle (coracle build_matrix /
apply; a prefix of a codeword is a codeword) with garbage in its missing shards
and in its named shard.  Expected: the clean codeword everywhere, a fill pattern
outside the shards, HEAL_DONE in every flag (the remaining surplus shards agree;
none of the masks is left with exactly k).  The WHOLE buffer and ALL flags are
compared exactly.
"""
import numpy as np
import pytest
import torch

from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO

pytestmark = pytest.mark.gpu

W = 992  # one 64-lane window of the kernel (unaligned_tile.h)
FILL = 0xA5


def tile():
    return B.heal_plan_tile_bytes()


def lengths():
    T = tile()
    return list(range(1, W + 65)) + list(range(T - 64, T + 65)) + list(range(2 * T - 64, 2 * T + 65))


def lose(k, m, *lost):
    return tuple(0 if i in lost else 1 for i in range(k + m))


SHAPES = [("4+2", 4, 2, lose(4, 2)), ("8+3-one-lost", 8, 3, lose(8, 3, 2)), ("12+4", 12, 4, lose(12, 4))]
CASES = [(f"{label}-{role}", k, m, mask, role) for label, k, m, mask in SHAPES for role in ("survivor", "checked")]


def layout(n_sh):
    L = np.array(lengths(), np.int64)
    base = np.empty(L.size, np.int64)
    cur = 0
    for q in range(L.size):  # at least 5 bytes of fill, then up to the stripe's alignment class
        o = cur + 5
        o += ((q // 16) % 16 - o) % 16
        base[q] = o
        cur = o + n_sh * int(L[q])
    return L, base, cur + 11


def test_cases_cover_what_they_name():
    """Host only."""
    T = tile()
    L = lengths()
    assert T == 4 * W and len(L) == len(set(L)) == W + 64 + 2 * 129 and max(L) == 2 * T + 64
    for _, k, m, mask, _ in CASES:
        here = [i for i in range(k + m) if mask[i]]
        assert len(here) - 1 - k >= 1  # a checked shard is left after the named one goes
    assert {(k, m) for _, k, m, _, _ in CASES} == {(4, 2), (8, 3), (12, 4)}


@pytest.mark.parametrize("label,k,m,mask,role", CASES, ids=[c[0] for c in CASES])
def test_every_length_and_alignment_with_the_named_shard_rewritten_in_place(label, k, m, mask, role):
    n_sh = k + m
    here = [i for i in range(n_sh) if mask[i]]
    gone = [i for i in range(n_sh) if not mask[i]]
    surv, checked = here[:k], here[k:]
    S, base, total = layout(n_sh)
    n = S.size
    # every (S mod 16, base mod 16) class
    assert {(int(s) % 16, int(b) % 16) for s, b in zip(S, base)} == {(a, b) for a in range(16) for b in range(16)}
    named = np.array([surv[q % k] if role == "survivor" else checked[q % len(checked)] for q in range(n)], np.int64)
    assert set(named.tolist()) == set(surv if role == "survivor" else checked)
    if role == "survivor":  # the first checked shard becomes the last survivor
        assert all(([i for i in here if i != j][:k])[-1] == checked[0] for j in surv)

    top = int(S.max())
    rng = np.random.default_rng(131 * k + m)
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
        for g in gone + [int(named[q])]:
            inp[at + g * s:at + (g + 1) * s] = junk[q:q + s] ^ np.uint8(g + 1)
    bits = sum(1 << i for i in here)
    where = np.array([N.LOC_BAD | (bits & ~(1 << int(j))) for j in named], np.uint32)
    present = np.tile(np.array(mask, np.uint8), (n, 1))
    assert np.array_equal(B.locate_decode(k, m, present, where), named)
    want_flags = np.full(n, N.HEAL_DONE, np.int32)

    buf = torch.from_numpy(inp).cuda()
    ref = torch.from_numpy(want).cuda()
    enc = RS.New(k, m)
    plan = B.StripePlan(enc, stripes=[(buf.data_ptr() + int(b), int(s)) for b, s in zip(base, S)])
    w = torch.from_numpy(where.view(np.int32).copy()).cuda()
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s0 = B.heal_plan_stats()
    plan.heal_mixed(present, w, flags)
    torch.cuda.synchronize()
    s1 = B.heal_plan_stats()
    got = flags.cpu().numpy()
    bad = np.nonzero(got != want_flags)[0]
    assert bad.size == 0, (f"{label}: {bad.size} flags wrong, first (stripe, S, base mod 16, named, got): "
                           f"{[(int(q), int(S[q]), int(base[q] % 16), int(named[q]), int(got[q])) for q in bad[:10]]}")
    if not torch.equal(buf, ref):
        diff = torch.nonzero(buf != ref).reshape(-1).cpu().numpy()
        q = np.searchsorted(base, diff, side="right") - 1
        at = [(int(j), int(S[j]), int(base[j] % 16), int(named[j]), int((d - base[j]) // S[j]), int((d - base[j]) % S[j]))
              for j, d in zip(q[:10], diff[:10])]
        pytest.fail(f"{label}: {diff.size} bytes wrong, first (stripe, S, base mod 16, named, shard, position): {at}")
    assert {f: s1[f] - s0[f] for f in s0} == {"kernel_launches": 1, "skipped_entries": 0}
    print(f"SWEEP heal-{label} mask={mask} stripes={n} resident={2 * total}")
