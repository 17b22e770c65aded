"""The sweep the ETag call closes: repair_mixed, then etag_mixed with all-present
masks and the stored ETags as expected, queued on one stream with no
synchronisation in between.  A rebuilt data shard has no stored ShardHash, and
with exactly k survivors repair can check nothing (flags & 2): a corrupted
survivor among them is rebuilt into wrong data that nothing but the ETag catches.

The ETags are hashlib.md5 of oracle.object_bytes; the codewords, their garbage
in the missing shards and the read-only check are tests/test_gpu_etag_plan.py's."""
import numpy as np
import pytest
import torch

import test_gpu_etag_plan as EP
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_repair_then_etag_catches_the_corrupted_survivor(kind):
    k, m = 4, 2
    enc = RS.New(k, m)
    n = k + m
    arena, masks, lens, md5s, role = EP.Arena(kind), [], [], [], []
    for e in range(240):
        S = [1, 5, 16, 33, 64, 100][e % 6]
        w = EP.word(k, m, S)
        ln = k * S - (e % 3 if k * S > 3 else 0)
        what = ["healthy", "one lost", "k left", "k left, survivor corrupt"][(e // 6) % 4]
        lost = {"healthy": (), "one lost": (e % k,), "k left": (e % k, k + e % m),
                "k left, survivor corrupt": (e % k, k + e % m)}[what]
        flip = None
        if what == "k left, survivor corrupt":  # one bit of a surviving data shard; 2 S <= lens, so below lens
            flip = (0 if e % k else 1, e % S, e % 8)
        masks.append(EP.mask_of(n, lost))
        arena.put(w, masks[-1], residue=e, flip=flip)
        lens.append(ln)
        md5s.append(w.md5(ln))
        role.append(what)
    plan = arena.build(enc)
    flags = torch.zeros(240, dtype=torch.int32, device="cuda")
    dig, bad = EP.slots(240)
    bad.zero_()
    expected = EP.expected_of(md5s)
    torch.cuda.synchronize()  # the buffers are filled; from here on one stream and no synchronisation
    stream = torch.cuda.Stream()
    s0 = B.etag_plan_stats()
    with torch.cuda.stream(stream):
        plan.repair_mixed(masks, flags, stream=stream)
        plan.etag_mixed(None, lens, digests=dig, expected=expected, bad=bad, stream=stream)
    stream.synchronize()
    f, b = flags.cpu().numpy(), bad.cpu().numpy()
    got = dig.cpu().numpy().tobytes()
    for e, what in enumerate(role):
        corrupt = what == "k left, survivor corrupt"
        assert bool(f[e] & 2) == what.startswith("k left"), (e, what, f[e])
        assert not f[e] & 1, (e, what)  # repair saw no mismatch: with k survivors there is nothing to compare
        assert b[e] == (1 if corrupt else 0), (e, what, b[e])
        assert (got[16 * e:16 * e + 16] == md5s[e]) == (not corrupt), (e, what)
    s1 = B.etag_plan_stats()
    assert s1["decoded_entries"] == s0["decoded_entries"]  # all-present masks: the repaired shards are read as they lie
    assert s1["kernel_launches"] - s0["kernel_launches"] == 1
    # the repair wrote the missing shards, and the true ones where the survivors were clean
    assert not arena.unchanged()
    img = arena.dev.cpu().numpy()
    for e, what in enumerate(role):
        if what in ("one lost", "k left"):
            spec, w = arena.spec[e], EP.word(k, m, arena.spec[e][-1])
            S = spec[-1]
            for j in range(k):
                off = spec[1] + j * S if kind != "shards" else spec[1][j]
                assert np.array_equal(img[off:off + S], w.shards[j]), (e, what, j)
