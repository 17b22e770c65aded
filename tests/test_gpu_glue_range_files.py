"""hbec_glue_plan_files_range: byte ranges of objects from their k+m shard files
in one call, the ranged GET path of a batch (ecObject.CopyRange's decode, in
object bytes).  Every ec_split case of tests/golden/vectors.json, and the
10 000-byte object of shard_hashes_4_2_chunk1k, goes into one plan per
(k, m, chunk), grouped as tests/test_gpu_file_plan.py groups them.

A plan only reads its files, so an object is entered once per range, every time
over the same file buffers: one call glues every range of every object of the
group.  The ranges of an object are: whole, empty at 0 and at L, the first byte,
the last byte, and every pair of cut points from {stripe boundary - 1, boundary,
boundary + 1} for every stripe boundary (0 and L among them) and {chunk boundary
- 1, chunk boundary + 1} for every shard junction inside every stripe.

Nothing expected comes from the product: the objects are oracle.object_bytes,
the files oracle.ec_split, and what must be written is obj[start:end], which
must also be oracle.ec_glue_range of the surviving files.  The discipline is
tests/test_gpu_glue_files.py's: whole buffers are compared, the outputs with 0xC3
sentinels around and between them, every file buffer must come back as it was,
and the files a mask calls missing, like the present ones beyond an entry's
first k present, hold random bytes per entry."""
import itertools

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


def ranges_of(k, chunk, L):
    if L == 0:
        return [(0, 0)]
    pts = set()
    for off, s in GF.entry_cuts(k, chunk, L):
        at = off * k  # the stripe's first object byte: the stripes before it are whole
        pts |= {at - 1, at, at + 1}
        for j in range(1, k):  # its shard junctions
            pts |= {at + j * s - 1, at + j * s + 1}
    pts |= {L - 1, L, L + 1}
    pts = sorted(p for p in pts if 0 <= p <= L)
    out = [(0, L), (0, 0), (L, L), (0, 1), (L - 1, L)] + list(itertools.combinations(pts, 2))
    return list(dict.fromkeys(out))


def expectation(f, present_of, cut_short=None):
    """Per object its bytes and ranges, each range's bytes checked against the oracle's ranged glue."""
    k, m, n = f.k, f.m, f.n
    objs, ranges = [], []
    for g, c in enumerate(f.cases):
        L = c["size"]
        obj = O.object_bytes(c["object_seed_index"], L).tobytes()
        cuts = GF.entry_cuts(k, f.chunk, L)
        files = []
        for j in range(n):
            keep = (cut_short or {}).get((g, j))
            if keep is not None:
                files.append(f.want[g][j].tobytes()[:keep])
            else:
                files.append(f.want[g][j].tobytes() if all(present_of(g, tt)[j] for tt in range(len(cuts))) else None)
        rs = ranges_of(k, f.chunk, L)
        for a, b in rs:
            assert 0 <= a <= b <= L
            if a < b:
                assert O.ec_glue_range(k, m, files, f.chunk, L, a, b) == obj[a:b], (L, a, b)
        objs.append(obj)
        ranges.append(rs)
    return objs, ranges


def run(f, enc, present_of, cut_short=None):
    k, m, n = f.k, f.m, f.n
    objs, ranges = expectation(f, present_of, cut_short)
    rng = np.random.default_rng(2000 * k + m)
    host, masks = [], []
    for g, c in enumerate(f.cases):
        row = []
        for j in range(n):
            b = np.full(f.lead[g][j] + f.want[g][j].size + 9, SENT, np.uint8)
            b[f.lead[g][j]:f.lead[g][j] + f.want[g][j].size] = f.want[g][j]
            row.append(b)
        per_entry = []
        for t, (off, s) in enumerate(GF.entry_cuts(k, f.chunk, c["size"])):
            mask = np.asarray(present_of(g, t), np.uint8)
            assert mask.sum() >= k
            per_entry.append(mask)
            read = [j for j in range(n) if mask[j]][:k]
            for j in range(n):
                if j not in read:  # missing, or never to be read: random bytes
                    lo = f.lead[g][j] + off
                    row[j][lo:lo + s] = rng.integers(0, 256, s, dtype=np.uint8)
        host.append(row)
        masks.append(per_entry)
    t = f.upload(host)
    # one object of the plan per (object, range), all over the same files
    files, present, starts, ends, offs, at = [], [], [], [], [], 0
    for g, c in enumerate(f.cases):
        addrs = [t[g][j].data_ptr() + f.lead[g][j] for j in range(n)]
        for a, b in ranges[g]:
            files.append((addrs, c["size"]))
            present += masks[g]
            starts.append(a)
            ends.append(b)
            o = at + 1
            o += ((5 * len(offs) + 3) % 16 - o) % 16
            offs.append((o, g))
            at = o + (b - a)
    plan = B.StripePlan(enc, files=files, chunk_size=f.chunk)
    assert int(plan.object_start[-1]) == len(present)
    want = np.full(at + 7, SENT, np.uint8)
    for (o, g), a, b in zip(offs, starts, ends):
        want[o:o + b - a] = np.frombuffer(objs[g], np.uint8)[a:b]
    out = torch.full((at + 7,), SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s0 = B.glue_range_stats()
    plan.glue_range_files(np.array(present, np.uint8).reshape(len(present), n), [out.data_ptr() + o for o, _ in offs],
                          starts, ends)
    torch.cuda.synchronize()
    s1 = B.glue_range_stats()
    assert s1["kernel_launches"] - s0["kernel_launches"] == (1 if any(b > a for a, b in zip(starts, ends)) else 0)
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"]
    got = out.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:6], [(g, a, b) for (o, g), a, b in zip(offs, starts, ends)
                                     if o - 16 <= bad[0] <= o + b - a + 16])
    FP.check_equal(t, host)  # read-only on the files


def test_the_ranges_cut_at_every_stripe_and_at_junctions():
    r = ranges_of(4, 1024, 10000)
    for want in ((0, 10000), (0, 0), (10000, 10000), (0, 1), (9999, 10000), (4095, 4097), (4096, 8192), (1023, 1025),
                 (3073, 8191), (8192 + 451, 8192 + 453), (8192 + 3 * 452 - 1, 9999), (1, 9999)):
        assert want in r, want
    assert len(r) == len(set(r)) and all(0 <= a <= b <= 10000 for a, b in r)
    assert ranges_of(4, 1 << 20, 0) == [(0, 0)] and (0, 1) in ranges_of(4, 1 << 20, 1)


@pytest.mark.parametrize("k,m", FP.SHAPES, ids=["4+2", "3+2", "8+3"])
def test_ranges_of_every_vector_case(k, m):
    enc = RS.New(k, m)
    n = k + m
    for f in FP.groups(k, m):
        f = GF.ordered(f)
        full = [1] * n
        run(f, enc, lambda g, t: full)                                               # a healthy read
        run(f, enc, lambda g, t: [0 if j == g % k else 1 for j in range(n)])         # one data file lost


def test_a_file_that_fails_between_two_stripes():
    """Stripe 0 of the 10 000-byte object reads all its files; from stripe 1 on file 1
    is gone, and file 4 from stripe 2 on: a range inside stripe 0 or inside file 0's,
    2's or 3's part of a later stripe is gathered, the others are decoded."""
    k, m = 4, 2
    enc = RS.New(k, m)
    f = [GF.ordered(x) for x in FP.groups(k, m) if x.chunk == 1024][0]
    g0 = [g for g, c in enumerate(f.cases) if c["size"] == 10000][0]

    def present_of(g, t):
        if g != g0:
            return [1] * (k + m)
        return [0 if (j == 1 and t >= 1) or (j == 4 and t >= 2) else 1 for j in range(k + m)]

    run(f, enc, present_of, cut_short={(g0, 1): 1024 + 17, (g0, 4): 2048})
