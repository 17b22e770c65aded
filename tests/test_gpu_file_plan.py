"""hbec_plan_files: objects given as their k+m shard files, as ecSplit writes
them, coded and hashed where they lie.  Every ec_split case of
tests/golden/vectors.json goes into one plan per (k, m): the data files are the
oracle's split of the seeded object, the parity files start zeroed, and each
file sits in a buffer of its own at an odd offset with sentinel bytes around it.

Nothing expected comes from the product: file contents and SHA-256 are the
committed vectors and the oracle's split, MD5s are hashlib's and, for the
10 000-byte object of shard_hashes_4_2_chunk1k, the committed ShardHashes.  Whole
buffers are compared, sentinels included."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
VEC = json.loads((ROOT / "tests" / "golden" / "vectors.json").read_text())
SENT = 0xC3
SHAPES = [(4, 2), (3, 2), (8, 3)]


def cases_of(k, m):
    """The vector cases of one shape, and for 4+2 the object whose ShardHashes are committed."""
    out = [dict(c) for c in VEC["ec_split"] if (c["k"], c["m"]) == (k, m)]
    if (k, m) == (4, 2):
        h = VEC["shard_hashes_4_2_chunk1k"]
        out.append({"k": 4, "m": 2, "size": h["len"], "chunk": h["chunk"], "object_seed_index": h["object"],
                    "md5": h["hashes"]})
    return out


class Files:
    """One (k, m, chunk) group of objects: want[g][j] the oracle's file, each in a
    host buffer of its own with `lead` sentinel bytes before it and 9 behind."""

    def __init__(self, k, m, chunk, cases):
        self.k, self.m, self.n, self.chunk, self.cases = k, m, k + m, chunk, cases
        self.want, self.lead = [], []
        for g, c in enumerate(cases):
            obj = O.object_bytes(c["object_seed_index"], c["size"]).tobytes()
            self.want.append([np.frombuffer(f, np.uint8) for f in O.ec_split(k, m, obj, chunk)])
            self.lead.append([1 + (3 * g + 5 * j) % 16 for j in range(self.n)])  # residues differ within an object

    def host(self, parity=True):
        bufs = []
        for g, files in enumerate(self.want):
            row = []
            for j, f in enumerate(files):
                b = np.full(self.lead[g][j] + f.size + 9, SENT, np.uint8)
                b[self.lead[g][j]:self.lead[g][j] + f.size] = f if (parity or j < self.k) else 0
                row.append(b)
            bufs.append(row)
        return bufs

    def upload(self, bufs):
        return [[torch.from_numpy(b.copy()).cuda() for b in row] for row in bufs]

    def plan(self, enc, t):
        return B.StripePlan(enc, files=[([t[g][j].data_ptr() + self.lead[g][j] for j in range(self.n)],
                                         self.cases[g]["size"]) for g in range(len(self.cases))],
                            chunk_size=self.chunk)

    def counts(self):
        full = self.k * self.chunk
        return [(c["size"] + full - 1) // full for c in self.cases]


def groups(k, m):
    """A plan takes one chunk size: the shape's cases, by chunk."""
    by = {}
    for c in cases_of(k, m):
        by.setdefault(c["chunk"], []).append(c)
    return [Files(k, m, chunk, cs) for chunk, cs in sorted(by.items())]


def check_equal(t, want):
    torch.cuda.synchronize()
    for g, row in enumerate(want):
        for j, b in enumerate(row):
            got = t[g][j].cpu().numpy()
            assert np.array_equal(got, b), (g, j, np.flatnonzero(got != b)[:4])


def test_every_vector_case_is_in_a_plan():
    seen = []
    for k, m in SHAPES:
        for f in groups(k, m):
            seen += [(k, m, c["size"], f.chunk) for c in f.cases]
    want = [(c["k"], c["m"], c["size"], c["chunk"]) for c in VEC["ec_split"]]
    assert sorted(set(seen)) == sorted(set(want + [(4, 2, 10000, 1024)])) and len(want) == 10
    assert {(4, 2, s, 1 << 20) for s in (0, 1, 7, 1001, 4097, (1 << 20) + 1)} <= set(seen)
    assert {(4, 2, 10000, 1024), (3, 2, 7, 100), (8, 3, 4097, 1 << 20), (8, 3, 100000, 4096)} <= set(seen)


@pytest.mark.parametrize("k,m", SHAPES, ids=["4+2", "3+2", "8+3"])
def test_encode_hash_and_repair_shard_files(k, m):
    enc = RS.New(k, m)
    n = k + m
    for f in groups(k, m):
        clean = f.host()
        t = f.upload(f.host(parity=False))
        plan = f.plan(enc, t)
        counts = f.counts()
        assert plan.object_start.dtype == np.uint32
        assert plan.object_start.tolist() == np.cumsum([0] + counts).tolist()
        ne, no = int(plan.object_start[-1]), len(f.cases)
        assert plan.info()["shard_bytes"] == sum(w[0].size for w in f.want)
        for c, w in zip(f.cases, f.want):
            assert [x.size for x in w] == c.get("file_len", [x.size for x in w])

        # encode: the parity files are the reference's
        plan.encode()
        check_equal(t, clean)
        for g, c in enumerate(f.cases):
            files = [t[g][j].cpu().numpy()[f.lead[g][j]:f.lead[g][j] + f.want[g][j].size] for j in range(n)]
            if "file_sha256" in c:
                assert [hashlib.sha256(x.tobytes()).hexdigest() for x in files] == c["file_sha256"], c["size"]
            if c.get("small_files") is not None:
                assert [x.tolist() for x in files] == c["small_files"]

        # hash_files over the plan's own object table: hashlib's MD5 of each file
        dig = torch.full((max(1, no * n * 16),), 0xA5, dtype=torch.uint8, device="cuda")
        plan.hash_files(plan.object_start, None, digests=dig)
        torch.cuda.synchronize()
        got = dig.cpu().numpy()[:no * n * 16].reshape(no, n, 16)
        for g, c in enumerate(f.cases):
            for j in range(n):
                want = hashlib.md5(f.want[g][j].tobytes()).digest() if c["size"] else bytes([0xA5] * 16)
                assert got[g, j].tobytes() == want, (c["size"], j)
            if "md5" in c:
                assert [got[g, j].tobytes().hex() for j in range(n)] == c["md5"]

        # two files of each object garbled and masked missing: repair_mixed restores them
        rng = np.random.default_rng(7 * k + m)
        present = np.ones((ne, n), np.uint8)
        bufs = [[b.copy() for b in row] for row in clean]
        for g in range(no):
            lost = rng.choice(n, size=min(2, m), replace=False)
            for j in lost:
                lo = f.lead[g][j]
                bufs[g][j][lo:lo + f.want[g][j].size] = rng.integers(0, 256, f.want[g][j].size, dtype=np.uint8)
            present[plan.object_start[g]:plan.object_start[g + 1], lost] = 0  # the object's row, per entry
        t2 = f.upload(bufs)
        plan2 = f.plan(enc, t2)
        flags = torch.zeros(max(1, ne), dtype=torch.int32, device="cuda")
        plan2.repair_mixed(present, flags)
        check_equal(t2, clean)
        # exactly k present where m == 2 (bit 1), one surplus shard that agrees where m == 3 (nothing)
        assert flags.cpu().numpy()[:ne].tolist() == [2 if m == 2 else 0] * ne
