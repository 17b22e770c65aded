"""hbec_glue_plan_range_checked (csrc/gluerangecheck.hip).  Nothing expected comes from the product: the range is
oracle.object_bytes(...)[s:e] where every bad examined column has a candidate and oracle.ec_glue (ReconstructData)
of the survivors as they are left, [s:e], where not.  The discipline is test_gpu_glue_plan's Glue.run with
test_gpu_glue_checked's codewords and test_gpu_glue_range_plan's ranges, all imported as they stand."""
import numpy as np
import pytest
import torch

import test_gpu_glue_checked as GC
import test_gpu_glue_plan as GP
import test_gpu_glue_range_plan as GR
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

BAD, SKIPPED, NOTHING, LEFT, PRE = GC.BAD, GC.SKIPPED, GC.NOTHING, GC.LEFT, GC.PRE


def positions(S, s, e):
    """The shard positions with a wanted byte in some data shard, as intervals."""
    j0, j1 = s // S, (e - 1) // S
    ps, pe = s - j0 * S, e - j1 * S
    return [(ps, pe)] if j0 == j1 else [(0, pe), (ps, S)] if j1 == j0 + 1 and pe < ps else [(0, S)]


def run(c, starts, lens, stream=None, method="glue_range_checked"):
    """One call under Glue.run's discipline; returns the arena's bytes and the words."""
    fixed = torch.from_numpy(np.full(len(c.sizes), PRE, np.uint32).view(np.int32)).cuda()
    extra = (fixed,) if method == "glue_range_checked" else ()
    got = GR.run_range(c, RS.New(c.k, c.m), starts, lens, [(7 * e + 3) % 16 for e in range(len(c.sizes))],
                       call=lambda plan, dsts: getattr(plan, method)(c.masks, dsts, starts, lens, *extra,
                                                                     stream=stream))
    return got, fixed.cpu().numpy().view(np.uint32)  # run_range synchronizes the device after the call


def build(k, m, kind, corrupt=True, repeat=4):
    # an entry's role follows from its mask's r and a counter.  r >= 2: one bad byte per column in each present
    # shard in turn, or clean, or (r >= 3) a column of two bad bytes amid them; r = 1: undecidable; r = 0: nothing
    T = B.glue_range_checked_tile_bytes()
    W = T // 4
    assert W == GP.W and T == B.glue_range_tile_bytes()
    sizes = [0, 1, 16, 17, W - 1, W + 1, 0, T - 1, T + 1, 2 * T + 1, 0] * repeat
    ms = GC.masks_for(k, m)
    masks, q = np.ones((len(sizes), k + m), np.uint8), 0
    for e, s in enumerate(sizes):
        if s:
            masks[e], q = ms[q % len(ms)], q + 1
    c = GC.Checked(k, m, kind, sizes, masks, seed=29 * k + m)
    starts, lens = GR.ranges_for(k, c.sizes, c.masks, shift=5)  # the eleven kinds in rotation
    wide = 0
    for q, e in enumerate(c.live):
        S, here = c.sizes[e], c.here(e)
        r = len(here) - k
        c.fixed[e] |= NOTHING if r == 0 else 0
        if not corrupt or r == 0 or (r >= 2 and q % 5 == 4):  # clean
            continue
        P = positions(S, starts[e], starts[e] + lens[e])
        inside = lambda x: any(lo <= x < hi for lo, hi in P)
        # the first and last of each interval, both sides of every window (and so half-tile and tile) seam in it
        spots = {x for lo, hi in P for x in [lo, hi - 1] + [w - d for w in range(W, hi, W) for d in (1, 0)] if inside(x)}
        lo, hi = P[0]
        wide += r >= 3 and hi - lo >= 3  # every other such entry gets a column of two bad bytes, the first one too
        twice = (lo + hi) // 2 if r >= 3 and hi - lo >= 3 and wide % 2 else None
        bits = 0
        for i, x in enumerate(sorted(spots - {twice})):
            j = here[(i + q) % len(here)]  # survivor, surplus, data and parity in turn
            c.bad(e, j, x, 1 + (37 * x + e) % 255, leave=r < 2)
            bits |= 1 << j
        if twice is not None:  # a survivor and a checked shard bad in one column
            for j in (here[0], here[-1]):
                c.bad(e, j, twice, 0x35, leave=True)
        for x in {x for lo, hi in P for x in (lo - 1, hi) if 0 <= x < S and not inside(x)}:
            c.bad(e, here[(q + x) % len(here)], x, 0x5A, leave=False)  # just outside P: neither taken nor reported
        c.fixed[e] |= BAD | (bits if r >= 2 else 0) | (LEFT if r == 1 or twice is not None else 0)
    c.settle()
    return c, starts, lens


@pytest.mark.parametrize("kind", GP.KINDS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4), (3, 2)])
def test_bad_bytes_in_the_examined_positions_are_corrected_in_the_range_and_only_there(k, m, kind):
    c, starts, lens = build(k, m, kind)
    gs = [tuple(np.flatnonzero(c.masks[e] == 0)) for e in c.live]
    assert {(m - len(g), sum(j < k for j in g)) for g in gs} == {(r, o) for r in range(m + 1) for o in range(m + 1 - r)}
    assert {(j,) for j in range(k)} <= set(gs)  # every (r, o) and each data shard lost alone
    assert {LEFT | BAD, NOTHING, 0, BAD} <= {int(w) & (LEFT | BAD | NOTHING) for w in c.fixed}
    assert m < 3 or any(w & LEFT and w & 0xFFFF for w in c.fixed)  # a left column amid corrected ones
    n_tiles, side = sum(-(-s // B.glue_range_checked_tile_bytes()) for s in c.sizes), torch.cuda.Stream()
    for chunk, stream in ((0, None), (1, side), (3, None)):  # launch boundaries anywhere in the list; a side stream
        s0 = B.glue_range_checked_stats()
        B.set_glue_range_checked_chunk_tiles(chunk)
        try:
            _, words = run(c, starts, lens, stream)
        finally:
            B.set_glue_range_checked_chunk_tiles(0)
        assert np.array_equal(words, c.fixed), [(e, hex(x), hex(y)) for e, (x, y) in enumerate(zip(words, c.fixed))
                                                if x != y][:6]
        s1 = B.glue_range_checked_stats()
        assert s1["kernel_launches"] - s0["kernel_launches"] == (-(-n_tiles // chunk) if chunk else 1)
        assert s1["per_stripe_calls"] == s0["per_stripe_calls"]


@pytest.mark.parametrize("kind", ["stripes", "shards"])
@pytest.mark.parametrize("k,m", [(4, 2), (12, 4)])
def test_start_zero_is_glue_checked_and_a_clean_call_is_glue_range(k, m, kind):
    c, lens = GC.build(k, m, kind)  # glue_checked's own corrupt prefixes
    fixed = torch.from_numpy(np.full(len(c.sizes), PRE, np.uint32).view(np.int32)).cuda()
    res = [(7 * e + 3) % 16 for e in range(len(c.sizes))]
    want = c.run(RS.New(k, m), lens, res, call=lambda plan, dsts: plan.glue_checked(c.masks, dsts, lens, fixed))
    got, words = run(c, [0] * len(lens), lens)
    assert np.array_equal(got, want) and np.array_equal(words, fixed.cpu().numpy().view(np.uint32))
    c, starts, lens = build(k, m, kind, corrupt=False, repeat=2)
    got, words = run(c, starts, lens)
    assert np.array_equal(got, run(c, starts, lens, method="glue_range")[0]) and np.array_equal(words, c.fixed)


@pytest.mark.parametrize("k,m", [(13, 2), (4, 5)])
def test_other_route_is_glued_unchecked_and_counted(k, m):
    sizes = [0, 1, 17, GP.W + 1, 0, 333]
    masks = np.ones((len(sizes), k + m), np.uint8)
    masks[2, 1] = masks[3, k] = masks[5, 0] = 0
    c = GC.Checked(k, m, "stripes", sizes, masks, seed=92)
    starts, lens = [0, 1, 16, GP.W, 0, 300], [0, k - 1, 17 * k - 19, GP.W + 2, 0, 400]
    for e in c.live:
        c.bad(e, c.here(e)[0], 0, 0x21, leave=True)  # not examined: glued as it is
        c.fixed[e] |= SKIPPED
    c.settle()
    calls = 0  # test_gpu_glue_range_plan's count of the per-entry route
    for e, s in enumerate(sizes):
        win = [(max(0, min(s, starts[e] - j * s)), max(0, min(s, starts[e] + lens[e] - j * s))) for j in range(k)]
        lost = [w for j, w in enumerate(win) if w[0] < w[1] and not masks[e][j]]
        calls += sum(1 for j, w in enumerate(win) if w[0] < w[1] and masks[e][j])
        calls += 1 + sum(w != (min(a for a, _ in lost), max(b for _, b in lost)) for w in lost) if lost else 0
    s0 = B.glue_range_checked_stats()
    _, words = run(c, starts, lens)
    assert np.array_equal(words, c.fixed)
    assert B.glue_range_checked_stats() == dict(s0, per_stripe_calls=s0["per_stripe_calls"] + calls)


@pytest.mark.parametrize("chunk", [5, 64])
def test_files_form_with_ranges_cut_around_stripe_boundaries(chunk):
    k, m, enc = 4, 2, RS.New(4, 2)
    objs = [O.object_bytes(910 + g, L).tobytes() for g, L in enumerate([2 * k * chunk + 7, 3, 3 * k * chunk])]
    rng = [(k * chunk - 1, 2 * k * chunk + 1), (1, 3), (k * chunk + 1, 3 * k * chunk - 1)]
    files = [[np.frombuffer(f, np.uint8).copy() for f in O.ec_split(k, m, o, chunk)] for o in objs]
    files[0][1][chunk + 1] ^= 0x44  # object 0, data file 1, stripe 1: inside the range
    files[2][k][2 * chunk] ^= 0x17  # object 2, parity file 0, stripe 2
    files[2][0][0] ^= 0x61          # object 2, stripe 0: the range starts behind it
    flat = [np.concatenate([np.full(1 + j, GP.SENT, np.uint8), f]) for fs in files for j, f in enumerate(fs)]
    t = torch.from_numpy(np.concatenate(flat)).cuda()
    ends = t.data_ptr() + np.cumsum([x.size for x in flat])
    addr = [[int(ends[g * (k + m) + j]) - f.size for j, f in enumerate(fs)] for g, fs in enumerate(files)]
    plan = B.StripePlan(enc, files=[(a, len(o)) for a, o in zip(addr, objs)], chunk_size=chunk)
    n = 3 + 1 + 3
    offs = np.cumsum([5] + [b - a + 9 for a, b in rng])[:3]
    want = np.full(int(offs[-1]) + rng[-1][1] - rng[-1][0] + 9, GP.SENT, np.uint8)
    for o, b, (s, e) in zip(offs, objs, rng):
        want[o:o + e - s] = np.frombuffer(b, np.uint8)[s:e]
    out = torch.full((want.size,), GP.SENT, dtype=torch.uint8, device="cuda")
    fixed = torch.zeros(n, dtype=torch.int32, device="cuda")
    plan.glue_range_files_checked(np.ones((n, k + m), np.uint8), [out.data_ptr() + int(o) for o in offs],
                                  [s for s, _ in rng], [e for _, e in rng], fixed)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(t.cpu().numpy(), np.concatenate(flat))
    assert fixed.cpu().numpy().view(np.uint32).tolist() == [0, BAD | 2, 0, 0, 0, 0, BAD | 1 << k]


def test_argument_errors_launch_nothing():
    k, m, (c, starts, lens) = 4, 2, build(4, 2, "stripes", repeat=2)
    t = [torch.from_numpy(x.copy()).cuda() for x in c.shard_bufs()]
    plan, n = c.plan(RS.New(k, m), t), len(c.sizes)
    dst = torch.zeros(k * sum(c.sizes) + 64, dtype=torch.uint8, device="cuda")
    fixed = torch.zeros(n, dtype=torch.int32, device="cuda")
    dsts = [dst.data_ptr() + int(o) for o in np.cumsum([0] + [k * s for s in c.sizes])[:n]]
    own = [t[b].data_ptr() + o for b, o in (c.at[e][0] for e in range(n))]
    few = c.masks.copy()
    few[c.live[0], :m + 1] = 0
    s0 = B.glue_range_checked_stats()
    for word, args in (("starts \\+ lens exceeds", (c.masks, dsts, starts, [k * s + 1 for s in c.sizes])),
                       ("null destination", (c.masks, [0] * n, starts, lens)),
                       ("overlaps shard", (c.masks, own, starts, lens)), ("too few", (few, dsts, starts, lens))):
        with pytest.raises(RS.ReedSolomonError, match=word):
            plan.glue_range_checked(*args, fixed)
    plan.glue_range_checked(c.masks, dsts, starts, [0] * n, fixed)  # nothing asked for: no launch, no word
    e = c.live[-1]  # d_fixed's words inside a destination
    inside = dst[dsts[e] - dst.data_ptr() + lens[e] - 4 & ~3:][:4 * n].view(torch.int32)
    with pytest.raises(RS.ErrInvalidArg, match="aliases a destination"):
        plan.glue_range_checked(c.masks, dsts, starts, lens, inside)
    torch.cuda.synchronize()
    assert B.glue_range_checked_stats() == s0 and not fixed.cpu().numpy().any() and not dst.cpu().numpy().any()
    assert all(np.array_equal(x.cpu().numpy(), h) for x, h in zip(t, c.shard_bufs()))
