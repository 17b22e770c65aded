"""Ranges swept through the range kernel, one plan and one call per case.

(A) 4+2: every (s, e) with 0 <= s < e <= k S for S in {5, 16, 17, 33}, some 13 400
entries.  (B) 8+3 with S0 = T + W + 33: every pair s < e of the cut points
{0, k S0} and {j S0 + p + d} for j < k, p in {0, T, S0} and d in {-16, -1, 0, 1, 16}.
The masks rotate over all present, data shard 0 lost, data shard k-1 lost and
both lost, slipping one place every 16 entries; entry (s, e) has destination
residue (7 s + e) mod 16.  This is where a head at a residue, a tail clip, a
junction byte, the gap between the two parts of a straddling range, or a tile
wrongly taken as a gather goes wrong if it can.

Glue only reads shards, so the entries of a `shards=` plan point at one stored
codeword per (S, mask): those are the entries of a tests/test_gpu_glue_plan.py
Glue, whose constructor has checked each object to be oracle.ec_glue of its
surviving shards and put random bytes into the shards its mask calls missing and
into the present ones beyond the first k.  What the call must write is
obj[s:e]; the whole destination arena (0xC3 sentinels around and between the
destinations) and every shard buffer are compared."""
import itertools

import numpy as np
import pytest
import torch

import test_gpu_glue_plan as GP
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

pytestmark = pytest.mark.gpu

SENT = GP.SENT


def sweep(k, m, shard_sizes, cases):
    """cases: (index into shard_sizes, s, e) per entry."""
    n = k + m
    variants = [[1] * n, [0] + [1] * (n - 1), [1] * (k - 1) + [0] + [1] * m, [0] + [1] * (k - 2) + [0] + [1] * m]
    # one stored codeword per (S, mask)
    g = GP.Glue(k, m, "shards", [S for S in shard_sizes for _ in variants],
                np.array([v for _ in shard_sizes for v in variants], np.uint8), seed=31 * k + len(cases) % 7)
    case = [(i + i // 16) % 4 for i in range(len(cases))]
    res = [(7 * s + e) % 16 for _, s, e in cases]
    host = g.shard_bufs()
    t = [torch.from_numpy(x.copy()).cuda() for x in host]
    assert all(x.data_ptr() % 16 == 0 for x in t)
    addr = [[t[b].data_ptr() + o for b, o in g.at[v]] for v in range(len(g.sizes))]
    offs, total = g.dst_layout([e - s for _, s, e in cases], res)
    want = np.full(total, SENT, np.uint8)
    for (z, s, e), c, o in zip(cases, case, offs):
        want[o:o + e - s] = g.objs[4 * z + c][s:e]
    dst = torch.full((total,), SENT, dtype=torch.uint8, device="cuda")
    plan = B.StripePlan(RS.New(k, m), shards=[(addr[4 * z + c], shard_sizes[z]) for (z, _, _), c in zip(cases, case)])
    masks = np.array([variants[c] for c in case], np.uint8)
    torch.cuda.synchronize()
    s0 = B.glue_range_stats()
    plan.glue_range(masks, [dst.data_ptr() + o for o in offs], [s for _, s, _ in cases], [e - s for _, s, e in cases])
    torch.cuda.synchronize()
    s1 = B.glue_range_stats()
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    got = dst.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:6], [(cases[i], case[i], o) for i, o in enumerate(offs)
                                     if o - 16 <= bad[0] <= o + cases[i][2] - cases[i][1] + 16])
    for b, (x, h) in enumerate(zip(t, host)):
        assert np.array_equal(x.cpu().numpy(), h), ("a shard buffer was written", b)
    return case, res


def test_every_range_of_four_shard_lengths():
    k, m = 4, 2
    sizes = [5, 16, 17, 33]
    cases = [(z, s, e) for z, S in enumerate(sizes) for s in range(k * S) for e in range(s + 1, k * S + 1)]
    assert len(cases) == sum(k * S * (k * S + 1) // 2 for S in sizes) == 13414
    case, res = sweep(k, m, sizes, cases)
    # every (s mod 16, e mod 16) that can occur, with the residue class it fixes, meets every mask
    seen = {(s % 16, e % 16, r, c) for (_, s, e), r, c in zip(cases, res, case)}
    assert seen == {(a, b, (7 * a + b) % 16, c) for a in range(16) for b in range(16) for c in range(4)}


def test_cut_points_around_every_junction_and_tile_edge():
    k, m = 8, 3
    T = GP.tile()
    S0 = T + GP.W + 33
    pts = {0, k * S0} | {j * S0 + p + d for j in range(k) for p in (0, T, S0) for d in (-16, -1, 0, 1, 16)}
    pts = sorted(p for p in pts if 0 <= p <= k * S0)
    assert len(pts) == 3 + 5 * (2 * k - 1) + 3
    cases = [(0, s, e) for s, e in itertools.combinations(pts, 2)]
    case, res = sweep(k, m, [S0], cases)
    assert {(r, c) for r, c in zip(res, case)} == {(r, c) for r in range(16) for c in range(4)}
