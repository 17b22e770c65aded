"""hbec_glue_plan_checked (csrc/gluecheck.hip).  Nothing expected comes from the product: the object is
oracle.object_bytes where every bad column has a candidate and oracle.ec_glue (ReconstructData) of the survivors
as they are left where not; whole arenas are compared, as in test_gpu_glue_plan (its Glue is used)."""
import numpy as np
import pytest
import torch

import test_gpu_glue_plan as GP
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BAD, SKIPPED, NOTHING, LEFT = N.COR_BAD, N.COR_SKIPPED, N.COR_NOTHING, N.COR_LEFT
PRE = 1 << 20  # the caller's own bit: must survive


def masks_for(k, m):
    # every (r, o): `lost` shards missing, o of them data (spread), the others the first parity; then each
    # single data loss the list does not hold yet
    gone = [[(5 * i + lost) % k for i in range(o)] + [k + i for i in range(lost - o)]
            for lost in range(m + 1) for o in range(lost + 1)]
    gone += [[j] for j in range(k) if [j] not in gone]
    assert all(len(set(g)) == len(g) for g in gone)
    return [[0 if j in g else 1 for j in range(k + m)] for g in gone]


class Checked(GP.Glue):
    # the whole codeword in the present shards, 0xD7 in the missing ones; stored: what the device sees,
    # left: the codeword with the bad bytes that must be left alone
    def __init__(self, k, m, kind, sizes, masks, seed):
        super().__init__(k, m, kind, sizes, masks, seed)
        mat = CO.build_matrix(k, m)
        self.fixed = np.full(len(self.sizes), PRE, np.uint32)
        self.left = {}
        for e in self.live:
            s = self.sizes[e]
            data = [self.objs[e][j * s:(j + 1) * s] for j in range(k)]
            code = data + [np.asarray(p, np.uint8) for p in CO.apply(mat[k:], data)]
            self.stored[e] = [code[j].copy() if self.masks[e][j] else np.full(s, 0xD7, np.uint8)
                              for j in range(self.n)]
            self.left[e] = [x.copy() for x in self.stored[e]]

    def here(self, e):
        return [j for j in range(self.n) if self.masks[e][j]]

    def bad(self, e, j, x, v, leave):
        self.stored[e][j][x] ^= v
        if leave:
            self.left[e][j][x] ^= v

    def settle(self):
        # every entry's object is what ReconstructData makes of the survivors as they are left
        for e in self.live:
            s, read = self.sizes[e], self.here(e)[:self.k]
            files = [self.left[e][j].tobytes() if j in read else None for j in range(self.n)]
            self.objs[e] = np.frombuffer(O.ec_glue(self.k, self.m, files, s, self.k * s), np.uint8)

    def check(self, lens, stream=None):
        fixed = torch.from_numpy(np.full(len(self.sizes), PRE, np.uint32).view(np.int32)).cuda()
        self.run(RS.New(self.k, self.m), lens, [(7 * e + 3) % 16 for e in range(len(self.sizes))],  # every residue
                 call=lambda plan, dsts: plan.glue_checked(self.masks, dsts, lens, fixed, stream=stream))
        got = fixed.cpu().numpy().view(np.uint32)  # run synchronizes the device before and after the call
        assert np.array_equal(got, self.fixed), [(e, hex(x), hex(y)) for e, (x, y) in enumerate(zip(got, self.fixed))
                                                 if x != y][:6]


def build(k, m, kind, repeat=3):
    # an entry's role follows from its mask's r and a counter.  r >= 2: one bad byte per column in each present
    # shard in turn, or clean, or (r >= 3) a column of two bad bytes amid them; r = 1: undecidable; r = 0: nothing
    T, W = B.glue_checked_tile_bytes(), GP.W
    assert T == 4 * W == B.correct_plan_tile_bytes()
    sizes = [0, 1, 15, 16, 17, W - 1, W, W + 1, 0, T - 1, T, T + 1, 2 * T + 1, 0] * repeat
    ms = masks_for(k, m)
    masks, q = np.ones((len(sizes), k + m), np.uint8), 0
    for e, s in enumerate(sizes):
        if s:
            masks[e], q = ms[q % len(ms)], q + 1
    c = Checked(k, m, kind, sizes, masks, seed=13 * k + m)
    lens = [0] * len(c.sizes)
    for q, e in enumerate(c.live):
        s, here = c.sizes[e], c.here(e)
        r = len(here) - k
        ln = lens[e] = min(k * s, [s, 1, s - 1, k * s, s + 1, k * s - (k - 1)][(q // len(ms) + q) % 6])
        sr = min(s, ln)
        if ln == 0:  # skipped, word and all
            continue
        c.fixed[e] |= NOTHING if r == 0 else 0
        turn = q // len(ms) % 3  # how often the mask has come up
        if r >= 2 and (turn == 2 or (turn == 1 and r == 2)):  # clean
            continue
        twice = sr // 2 if r >= 3 and turn == 1 and sr >= 3 else None
        bits = 0
        # 0, the last examined, both sides of every window (and so half-tile and tile) seam
        seams = {0, sr - 1} | {x for w in range(W, sr + 1, W) for x in (w - 1, w) if x < sr}
        for i, x in enumerate(sorted(seams - {twice})):
            j = here[(i + q) % len(here)]  # survivor, surplus, data and parity in turn
            c.bad(e, j, x, 1 + (37 * x + e) % 255, leave=r < 2)
            bits |= 1 << j
        if twice is not None:  # a survivor and a checked shard bad in one column
            for j in (here[0], here[-1]):
                c.bad(e, j, twice, 0x35, leave=True)
        if sr < s:  # just past what is examined: neither taken into the object nor reported
            c.bad(e, here[q % len(here)], sr, 0x5A, leave=False)
        if r >= 1:
            c.fixed[e] |= BAD | (bits if r >= 2 else 0) | (LEFT if r == 1 or twice is not None else 0)
    assert m < 3 or any(w & LEFT and w & 0xFFFF for w in c.fixed)  # a left column amid corrected ones
    c.settle()
    return c, lens


@pytest.mark.parametrize("kind", GP.KINDS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4), (3, 2)])
def test_bad_bytes_are_corrected_in_the_object_and_only_there(k, m, kind):
    c, lens = build(k, m, kind)
    gs = [tuple(np.flatnonzero(c.masks[e] == 0)) for e in c.live if lens[e]]
    assert {(m - len(g), sum(j < k for j in g)) for g in gs} == {(r, o) for r in range(m + 1) for o in range(m + 1 - r)}
    assert {(j,) for j in range(k)} <= set(gs)  # every (r, o), 15 at 12+4, and each data shard lost alone
    assert {LEFT | BAD, NOTHING, 0} <= {int(w) & (LEFT | BAD | NOTHING) for w in c.fixed} and len(c.sizes) >= 16
    n_tiles, side = sum(-(-s // B.glue_checked_tile_bytes()) for s in c.sizes), torch.cuda.Stream()
    for chunk, stream in ((0, None), (1, side), (3, None)):  # launch boundaries anywhere in the list; a side stream
        s0 = B.glue_checked_stats()
        B.set_glue_checked_chunk_tiles(chunk)
        try:
            c.check(lens, stream)
        finally:
            B.set_glue_checked_chunk_tiles(0)
        s1 = B.glue_checked_stats()
        assert s1["kernel_launches"] - s0["kernel_launches"] == (-(-n_tiles // chunk) if chunk else 1)
        assert s1["per_stripe_calls"] == s0["per_stripe_calls"]


@pytest.mark.parametrize("k,m", [(13, 2), (4, 5)])
def test_other_route_is_glued_unchecked_and_counted(k, m):
    sizes = [0, 1, 17, GP.W + 1, 0, 333]
    masks = np.ones((len(sizes), k + m), np.uint8)
    masks[2, 1] = masks[3, k] = masks[5, 0] = 0
    c = Checked(k, m, "stripes", sizes, masks, seed=91)
    lens = [0, k, 17 * k - 3, GP.W + 2, 0, 333 * k]
    for e in c.live:
        c.bad(e, c.here(e)[0], 0, 0x21, leave=True)  # not examined: glued as it is
        c.fixed[e] |= SKIPPED
    c.settle()
    calls = 0  # test_gpu_glue_plan's count of the per-entry route: copies, an apply, a copy more where cut
    for e, s in enumerate(sizes):
        valid = [max(0, min(s, lens[e] - j * s)) for j in range(k)]
        lost = [valid[j] for j in range(k) if valid[j] and not masks[e][j]]
        calls += sum(1 for j in range(k) if valid[j] and masks[e][j]) + (1 if lost else 0) + sum(v < s for v in lost)
    s0 = B.glue_checked_stats()
    c.check(lens)
    assert B.glue_checked_stats() == dict(s0, per_stripe_calls=s0["per_stripe_calls"] + calls)


@pytest.mark.parametrize("chunk", [5, 64])
def test_files_form_with_a_file_corrupt_in_one_stripe_only(chunk):
    k, m, enc = 4, 2, RS.New(4, 2)
    objs = [O.object_bytes(900 + g, L).tobytes() for g, L in enumerate([2 * k * chunk + 7, 3, 3 * k * chunk])]
    files = [[np.frombuffer(f, np.uint8).copy() for f in O.ec_split(k, m, o, chunk)] for o in objs]
    files[0][1][chunk + 1] ^= 0x44  # object 0, data file 1, stripe 1
    files[2][k][2 * chunk] ^= 0x17  # object 2, parity file 0, stripe 2
    flat = [np.concatenate([np.full(1 + j, GP.SENT, np.uint8), f]) for fs in files for j, f in enumerate(fs)]
    t = torch.from_numpy(np.concatenate(flat)).cuda()
    ends = t.data_ptr() + np.cumsum([x.size for x in flat])
    addr = [[int(ends[g * (k + m) + j]) - f.size for j, f in enumerate(fs)] for g, fs in enumerate(files)]
    plan = B.StripePlan(enc, files=[(a, len(o)) for a, o in zip(addr, objs)], chunk_size=chunk)
    n = 3 + 1 + 3
    offs = np.cumsum([5] + [len(o) + 9 for o in objs])[:3]
    want = np.full(int(offs[-1]) + len(objs[-1]) + 9, GP.SENT, np.uint8)
    for o, b in zip(offs, objs):
        want[o:o + len(b)] = np.frombuffer(b, np.uint8)
    out = torch.full((want.size,), GP.SENT, dtype=torch.uint8, device="cuda")
    fixed = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.glue_files_checked(np.ones((n, k + m), np.uint8), [out.data_ptr() + int(o) for o in offs], fixed)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), np.concatenate(flat))
    assert fixed.cpu().numpy().view(np.uint32).tolist() == [0, BAD | 2, 0, 0, 0, 0, BAD | 1 << k]


def test_argument_errors_launch_nothing():
    k, m, (c, lens) = 4, 2, build(4, 2, "stripes")
    t = [torch.from_numpy(x.copy()).cuda() for x in c.shard_bufs()]
    plan, n = c.plan(RS.New(k, m), t), len(c.sizes)
    dst = torch.zeros(k * sum(c.sizes) + 64, dtype=torch.uint8, device="cuda")
    fixed = torch.zeros(n, dtype=torch.int32, device="cuda")
    dsts = [dst.data_ptr() + int(o) for o in np.cumsum([0] + [k * s for s in c.sizes])[:n]]
    own = [t[b].data_ptr() + o for b, o in (c.at[e][0] for e in range(n))]
    few = c.masks.copy()
    few[c.live[0], :m + 1] = 0
    s0 = B.glue_checked_stats()
    for word, args in (("dst_lens exceeds", (c.masks, dsts, [k * s + 1 for s in c.sizes])),
                       ("null destination", (c.masks, [0] * n, lens)), ("overlaps shard", (c.masks, own, lens)),
                       ("too few", (few, dsts, lens))):
        with pytest.raises(RS.ReedSolomonError, match=word):
            plan.glue_checked(*args, fixed)
    plan.glue_checked(c.masks, dsts, [0] * n, fixed)  # nothing asked for: no launch, no word
    e = c.live[10]  # d_fixed's words inside a destination
    inside = dst[dsts[e] - dst.data_ptr() + lens[e] - 4 & ~3:][:4 * n].view(torch.int32)
    with pytest.raises(RS.ErrInvalidArg, match="aliases a destination"):
        plan.glue_checked(c.masks, dsts, lens, inside)
    torch.cuda.synchronize()
    assert B.glue_checked_stats() == s0 and not fixed.cpu().numpy().any() and not dst.cpu().numpy().any()
    assert all(np.array_equal(x.cpu().numpy(), h) for x, h in zip(t, c.shard_bufs()))
