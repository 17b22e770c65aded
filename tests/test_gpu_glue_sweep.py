"""Every shard length 1..T+W+33 through the glue kernel, as the entries of one
plan per shape and one call per plan: 4+2 on a stripes plan, 8+3 on a shards
plan.  Entry S has destination residue (7 S) mod 16 and length k S - (S mod k),
and the masks rotate over all present, data shard 0 lost, data shard k-1 lost,
and both lost.  This is where a junction byte between two output shards, a head
at a residue or a tail clip goes wrong if it can: the whole destination arena
and the whole shard arena are compared under the common discipline of
tests/test_gpu_glue_plan.py, against the objects' own bytes, which the
constructor has checked to be oracle.ec_glue of the surviving shards."""
import numpy as np
import pytest

import test_gpu_glue_plan as GP
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k,m,kind", [(4, 2, "stripes"), (8, 3, "shards")], ids=["4+2-stripes", "8+3-shards"])
def test_every_length_in_one_call(k, m, kind):
    T = GP.tile()
    sizes = list(range(1, T + GP.W + 33 + 1))
    n = k + m
    cases = [[1] * n, [0] + [1] * (n - 1), [1] * (k - 1) + [0] + [1] * m, [0] + [1] * (k - 2) + [0] + [1] * m]
    # the rotation slips one place every 16 lengths, so every length mod 16 (and with it every
    # residue) meets every mask, 70 times and more
    case = [(i + i // 16) % 4 for i in range(len(sizes))]
    masks = np.array([cases[c] for c in case], np.uint8)
    lens = [max(1, k * s - s % k) for s in sizes]
    res = [(7 * s) % 16 for s in sizes]
    assert {(s % 16, r, c) for s, r, c in zip(sizes, res, case)} == \
        {(a, (7 * a) % 16, c) for a in range(16) for c in range(4)}
    assert set(res) == set(range(16))
    g = GP.Glue(k, m, kind, sizes, masks, seed=k)
    s0 = B.glue_plan_stats()
    g.run(RS.New(k, m), lens, res)
    s1 = B.glue_plan_stats()
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
