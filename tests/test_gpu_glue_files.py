"""hbec_glue_plan_files: whole objects from their k+m shard files in one call,
the GET path of a batch (ecObject.Copy -> ecGlue).  Every ec_split case of
tests/golden/vectors.json, and the 10 000-byte object of shard_hashes_4_2_chunk1k,
goes into one plan per (k, m, chunk), grouped as tests/test_gpu_file_plan.py
groups them.

Nothing expected comes from the product: the objects are oracle.object_bytes,
the files oracle.ec_split, and what must be written is the object's own bytes,
which must also be oracle.ec_glue of the surviving files; the ETag a GET checks
is hashlib's MD5.  The common discipline of tests/test_gpu_glue_plan.py holds:
whole buffers are compared, the outputs with 0xC3 sentinels around and between
them, every file buffer must come back as it was, and the files a mask calls
missing, like the present ones beyond an entry's first k present, hold random
bytes (per entry: a file may be read in one stripe and not in the next)."""
import hashlib

import numpy as np
import pytest
import torch

import test_gpu_file_plan as FP
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from hummingbird_amd import shardhash as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SENT = FP.SENT


def ordered(f):
    """The group with an object of no bytes, if it has one, moved between two others."""
    zero = [i for i, c in enumerate(f.cases) if c["size"] == 0]
    if zero and len(f.cases) >= 3:
        order = [i for i in range(len(f.cases)) if i != zero[0]]
        order.insert(1, zero[0])
        f.cases = [f.cases[i] for i in order]
        f.want = [f.want[i] for i in order]
        f.lead = [f.lead[i] for i in order]
    return f


def entry_cuts(k, chunk, L):
    """(file offset, shard length) of every stripe, the oracle's sizes."""
    cuts, off = [], 0
    for s in O._stripe_sizes(k, chunk, L):
        cuts.append((off, s))
        off += s
    return cuts


def run(f, enc, present_of, cut_short=None):
    """glue_files on the group with mask present_of(g, t) for stripe t of object g.
    cut_short: {(g, j): bytes kept} for the oracle's view of a file that failed mid-stream."""
    k, m, n = f.k, f.m, f.n
    rng = np.random.default_rng(1000 * k + m)
    no = len(f.cases)
    objs = [O.object_bytes(c["object_seed_index"], c["size"]).tobytes() for c in f.cases]
    host, present = [], []
    for g, c in enumerate(f.cases):
        row = []
        for j in range(n):
            b = np.full(f.lead[g][j] + f.want[g][j].size + 9, SENT, np.uint8)
            b[f.lead[g][j]:f.lead[g][j] + f.want[g][j].size] = f.want[g][j]
            row.append(b)
        for t, (off, s) in enumerate(entry_cuts(k, f.chunk, c["size"])):
            mask = np.asarray(present_of(g, t), np.uint8)
            assert mask.sum() >= k
            present.append(mask)
            read = [j for j in range(n) if mask[j]][:k]
            for j in range(n):
                if j not in read:  # missing, or never to be read: random bytes
                    lo = f.lead[g][j] + off
                    row[j][lo:lo + s] = rng.integers(0, 256, s, dtype=np.uint8)
        host.append(row)
    t = f.upload(host)
    plan = f.plan(enc, t)
    assert int(plan.object_start[-1]) == len(present)
    # the outputs in one arena, residues in turn, sentinels between
    offs, at = [], 0
    for g, c in enumerate(f.cases):
        o = at + 1
        o += ((5 * g + 3) % 16 - o) % 16
        offs.append(o)
        at = o + c["size"]
    want = np.full(at + 7, SENT, np.uint8)
    for g, o in enumerate(offs):
        want[o:o + len(objs[g])] = np.frombuffer(objs[g], np.uint8)
    out = torch.full((at + 7,), SENT, dtype=torch.uint8, device="cuda")
    s0 = B.glue_plan_stats()
    plan.glue_files(np.array(present, np.uint8).reshape(len(present), n), [out.data_ptr() + o for o in offs])
    torch.cuda.synchronize()
    launches = B.glue_plan_stats()["kernel_launches"] - s0["kernel_launches"]
    assert launches == (1 if any(objs) else 0)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:6]
    FP.check_equal(t, host)  # read-only on the files
    live = [g for g in range(no) if objs[g]]
    digests = H.md5_list([(out.data_ptr() + offs[g], len(objs[g])) for g in live]).cpu().numpy()
    for i, g in enumerate(live):
        c = f.cases[g]
        files = []
        for j in range(n):
            cuts = entry_cuts(k, f.chunk, c["size"])
            keep = (cut_short or {}).get((g, j))
            if keep is not None:
                files.append(f.want[g][j].tobytes()[:keep])
            else:
                files.append(f.want[g][j].tobytes() if all(present_of(g, tt)[j] for tt in range(len(cuts))) else None)
        glued = O.ec_glue(k, m, files, f.chunk, c["size"])
        mine = got[offs[g]:offs[g] + c["size"]].tobytes()
        assert mine == objs[g] == glued, c["size"]
        # the ETag check a GET makes, on the device's own hash of what was written
        assert digests[i].tobytes() == hashlib.md5(mine).digest() == hashlib.md5(objs[g]).digest()
    return f


def test_a_zero_length_object_sits_between_two_others():
    seen = False
    for k, m in FP.SHAPES:
        for f in FP.groups(k, m):
            f = ordered(f)
            sizes = [c["size"] for c in f.cases]
            seen = seen or any(a and not b and c for a, b, c in zip(sizes, sizes[1:], sizes[2:]))
    assert seen


@pytest.mark.parametrize("k,m", FP.SHAPES, ids=["4+2", "3+2", "8+3"])
def test_glue_files_of_every_vector_case(k, m):
    enc = RS.New(k, m)
    n = k + m
    for f in FP.groups(k, m):
        f = ordered(f)
        full = [1] * n
        run(f, enc, lambda g, t: full)                                               # a healthy read
        run(f, enc, lambda g, t: [0 if j == g % k else 1 for j in range(n)])         # one data file lost
        run(f, enc, lambda g, t: [0 if j < m else 1 for j in range(n)])              # m files lost, data first


def test_a_file_that_fails_between_two_stripes():
    """Stripe 0 of the 10 000-byte object reads all its files; from stripe 1 on file 1
    is gone, and file 4 from stripe 2 on.  ecGlue sees a file too short for the stripe
    (len(f) >= off + s fails) and rebuilds from the others."""
    k, m = 4, 2
    enc = RS.New(k, m)
    f = [ordered(x) for x in FP.groups(k, m) if x.chunk == 1024][0]
    g0 = [g for g, c in enumerate(f.cases) if c["size"] == 10000][0]
    assert [s for _, s in entry_cuts(k, 1024, 10000)] == [1024, 1024, 452]

    def present_of(g, t):
        if g != g0:
            return [1] * (k + m)
        return [0 if (j == 1 and t >= 1) or (j == 4 and t >= 2) else 1 for j in range(k + m)]

    run(f, enc, present_of, cut_short={(g0, 1): 1024 + 17, (g0, 4): 2048})
