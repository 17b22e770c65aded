"""hbec_split_plan_files: whole objects into their k+m shard files in one call,
the stabilize path of a batch (ecObject.Stabilize -> ecSplit).  Every ec_split
case of tests/golden/vectors.json, and the 10 000-byte object of
shard_hashes_4_2_chunk1k, goes into one plan per (k, m, chunk), grouped as
tests/test_gpu_file_plan.py groups them, with an object of no bytes moved
between two others where the group has one.

Nothing expected comes from the product: the objects are oracle.object_bytes,
the files oracle.ec_split's (and the committed SHA-256 and small files where
the vectors have them), the ShardHashes oracle.ec_split_hashes (and the
committed ones for the 10 000-byte object), and glue_files of the written files
must return the objects.  The common discipline of tests/test_gpu_split_plan.py
holds: whole buffers are compared, the file buffers start as random bytes
between 0xC3 sentinels, the objects lie in one arena with 0xC3 between them,
and that arena must come back as it was."""
import hashlib

import numpy as np
import pytest
import torch

import test_gpu_file_plan as FP
import test_gpu_glue_files as GF
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SENT = FP.SENT


def test_a_zero_length_object_sits_between_two_others():
    seen = False
    for k, m in FP.SHAPES:
        for f in FP.groups(k, m):
            sizes = [c["size"] for c in GF.ordered(f).cases]
            seen = seen or any(a and not b and c for a, b, c in zip(sizes, sizes[1:], sizes[2:]))
    assert seen


@pytest.mark.parametrize("k,m", FP.SHAPES, ids=["4+2", "3+2", "8+3"])
def test_split_files_of_every_vector_case(k, m):
    enc = RS.New(k, m)
    n = k + m
    rng = np.random.default_rng(1000 * k + m + 1)
    for f in FP.groups(k, m):
        f = GF.ordered(f)
        no = len(f.cases)
        objs = [O.object_bytes(c["object_seed_index"], c["size"]).tobytes() for c in f.cases]
        clean = f.host()
        before = [[b.copy() for b in row] for row in clean]
        for g in range(no):
            for j in range(n):
                lo, size = f.lead[g][j], f.want[g][j].size
                before[g][j][lo:lo + size] = rng.integers(0, 256, size, dtype=np.uint8)
        t = f.upload(before)
        plan = f.plan(enc, t)
        assert plan.object_start.tolist() == np.cumsum([0] + f.counts()).tolist()
        # the objects in one arena, residues in turn, sentinels between
        offs, at = [], 0
        for g, c in enumerate(f.cases):
            o = at + 1
            o += ((5 * g + 3) % 16 - o) % 16
            offs.append(o)
            at = o + c["size"]
        arena = np.full(at + 7, SENT, np.uint8)
        for g, o in enumerate(offs):
            arena[o:o + len(objs[g])] = np.frombuffer(objs[g], np.uint8)
        src = torch.from_numpy(arena.copy()).cuda()
        torch.cuda.synchronize()
        s0 = B.split_plan_stats()
        plan.split_files([src.data_ptr() + o for o in offs])
        torch.cuda.synchronize()
        s1 = B.split_plan_stats()
        assert s1["kernel_launches"] - s0["kernel_launches"] == (1 if any(objs) else 0)
        assert s1["per_stripe_calls"] == s0["per_stripe_calls"]

        # every file, with the sentinels around it, is the reference's
        FP.check_equal(t, clean)
        assert np.array_equal(src.cpu().numpy(), arena)
        for g, c in enumerate(f.cases):
            files = [t[g][j].cpu().numpy()[f.lead[g][j]:f.lead[g][j] + f.want[g][j].size] for j in range(n)]
            assert [x.tobytes() for x in files] == O.ec_split(k, m, objs[g], f.chunk), c["size"]
            if "file_sha256" in c:
                assert [hashlib.sha256(x.tobytes()).hexdigest() for x in files] == c["file_sha256"], c["size"]
            if c.get("small_files") is not None:
                assert [x.tolist() for x in files] == c["small_files"]

        # the ShardHash of every written file is what the receiving StablePut computes
        dig = torch.full((max(1, no * n * 16),), 0xA5, dtype=torch.uint8, device="cuda")
        plan.hash_files(plan.object_start, None, digests=dig)
        torch.cuda.synchronize()
        got = dig.cpu().numpy()[:no * n * 16].reshape(no, n, 16)
        for g, c in enumerate(f.cases):
            if not c["size"]:
                assert got[g].tobytes() == bytes([0xA5] * 16 * n)
                continue
            want = O.ec_split_hashes(k, m, objs[g], f.chunk)
            assert [got[g, j].tobytes().hex() for j in range(n)] == want, c["size"]
            if "md5" in c:
                assert want == c["md5"]

        # and glue_files of them returns the objects
        ne = int(plan.object_start[-1])
        out = torch.full((arena.size,), SENT, dtype=torch.uint8, device="cuda")
        plan.glue_files(np.ones((ne, n), np.uint8), [out.data_ptr() + o for o in offs])
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), arena)
        for g in range(no):
            files = [t[g][j].cpu().numpy()[f.lead[g][j]:f.lead[g][j] + f.want[g][j].size].tobytes() for j in range(n)]
            assert O.ec_glue(k, m, files, f.chunk, len(objs[g])) == objs[g]
