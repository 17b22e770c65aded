"""Every shard length 1..T+W+33 through the split kernel, as the entries of one
plan per shape and one call per plan: 4+2 on a stripes plan, 8+3 on a shards
plan.  Entry S has source residue (7 S) mod 16 and length k S - (S mod k)
(clipped so that the piece has a byte).  This is where a junction byte between
two data shards of a databuf, a head at a residue, a tail clip or a pad that
reads through goes wrong if it can: the whole shard arenas and the whole source
arena are compared under the common discipline of tests/test_gpu_split_plan.py,
against oracle.ec_split's shards, which the constructor has checked to glue back
to the piece."""
import pytest

import test_gpu_split_plan as SP
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k,m,kind", [(4, 2, "stripes"), (8, 3, "shards")], ids=["4+2-stripes", "8+3-shards"])
def test_every_length_in_one_call(k, m, kind):
    T = SP.tile()
    sizes = list(range(1, T + SP.W + 33 + 1))
    pads = [min(s % k, k * s - 1) for s in sizes]
    res = [(7 * s) % 16 for s in sizes]
    # every length mod 16 with its residue, and with it every residue, 300 times and more; every pad too
    assert {(s % 16, r) for s, r in zip(sizes, res)} == {(a, (7 * a) % 16) for a in range(16)}
    assert set(res) == set(range(16)) and set(pads) == set(range(k))
    g = SP.Split(k, m, kind, sizes, pads, seed=k)
    assert all(ln >= 1 for ln in g.lens)
    s0 = B.split_plan_stats()
    g.run(RS.New(k, m), res)
    s1 = B.split_plan_stats()
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
