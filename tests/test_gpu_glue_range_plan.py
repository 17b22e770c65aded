"""hbec_glue_plan_range on the device: any byte range of every entry of a plan
from its shards, degraded or not, in one call, on all four kinds of plan.

Nothing expected comes from the product.  Entry e's object is
oracle.object_bytes, its codeword coracle's (tests/test_gpu_glue_plan.py's Glue,
which asserts that oracle.ec_glue of the surviving shards is the object), and
what the call must write is obj[s:e].  The discipline is Glue.run's, used as it
stands with the range's expectation put in: the whole destination arena is
compared, 0xC3 sentinels around and between the destinations; every shard
buffer must come back bit-identical; the shards a mask calls missing hold random
bytes, and so do the present shards beyond the entry's first k present."""
import numpy as np
import pytest
import torch

import test_glue_range_host as GRH
import test_gpu_glue_plan as GP
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SENT, W = GP.SENT, GP.W
N_KINDS = 11


class _Ranged:
    """A Glue whose expected bytes are obj[s:s + len] instead of obj[:len]."""

    def __init__(self, g, starts):
        self._g, self._starts = g, starts

    def __getattr__(self, name):
        return getattr(self._g, name)

    def expect(self, lens, offs, total):
        want = np.full(total, SENT, np.uint8)
        for e, (ln, o) in enumerate(zip(lens, offs)):
            want[o:o + ln] = self.objs[e][self._starts[e]:self._starts[e] + ln]
        return want


def run_range(g, enc, starts, lens, residues, call=None):
    """Glue.run with the range's call and expectation; returns the arena's bytes."""
    assert all(s + ln <= g.k * S for s, ln, S in zip(starts, lens, g.sizes) if ln)
    if call is None:
        def call(plan, dsts):
            plan.glue_range(g.masks, dsts, starts, lens)
    return GP.Glue.run(_Ranged(g, starts), enc, lens, residues, call)


def clip(k, S, a, b):
    a, b = max(0, min(a, k * S)), max(0, min(b, k * S))
    return (a, b) if a < b else (0, k * S)


def ranges_for(k, sizes, masks, shift=0):
    """The eleven kinds of range in turn over the entries with bytes, from `shift` on."""
    starts, lens, kinds, i = [], [], [], 0
    for e, S in enumerate(sizes):
        if not S:
            starts.append(7 * e)  # whatever: lens = 0 skips the entry
            lens.append(0)
            continue
        lost = [j for j in range(k) if not masks[e][j]]
        present = [j for j in range(k) if masks[e][j]]
        kind = (i + shift) % N_KINDS
        if kind == 8:  # inside one data shard: a lost one and a present one alternately
            j = lost[0] if lost and (i // N_KINDS) % 2 == 0 else present[len(present) // 2]
            a, b = j * S + S // 3, j * S + max(S // 3 + 1, S - S // 4)
        else:
            a, b = [(0, k * S), (1, k * S), (0, k * S - 1), (0, 1), (S - 1, S), (S, S + 1), (k * S - 1, k * S),
                    (S - 1, S + 1), None, (S - 1, 2 * S + 1), (S // 2, k * S - S // 2)][kind]
        a, b = clip(k, S, a, b)
        starts.append(a)
        lens.append(b - a)
        kinds.append(kind)
        i += 1
    assert set(kinds) == set(range(N_KINDS))
    return starts, lens


@pytest.mark.parametrize("kind", GP.KINDS)
@pytest.mark.parametrize("k,m", GP.SHAPES, ids=["4+2", "8+3", "12+4"])
def test_range_every_kind_of_plan(k, m, kind):
    enc = RS.New(k, m)
    g = GP.glue_of(k, m, kind)
    res = GP.residues_for(g.sizes)
    s0 = B.glue_range_stats()
    for n, shift in enumerate((0, 4, 9)):  # other ranges on the same sizes and masks, at other residues
        starts, lens = ranges_for(k, g.sizes, g.masks, shift)
        run_range(g, enc, starts, lens, res[3 * n:] + res[:3 * n])
        s1 = B.glue_range_stats()
        assert s1["kernel_launches"] - s0["kernel_launches"] == n + 1  # whatever the entries, masks or ranges
        assert s1["per_stripe_calls"] == s0["per_stripe_calls"]


@pytest.mark.parametrize("kind", ["stripes", "files"])
@pytest.mark.parametrize("k,m", [(4, 2), (12, 4)], ids=["4+2", "12+4"])
def test_start_zero_writes_what_glue_mixed_writes(k, m, kind):
    enc = RS.New(k, m)
    g = GP.glue_of(k, m, kind)
    res = GP.residues_for(g.sizes)
    for lens in (GP.trunc_lens(k, g.sizes), GP.prefix_lens(k, g.sizes)):
        mixed = g.run(enc, lens, res)
        assert np.array_equal(run_range(g, enc, [0] * len(lens), lens, res), mixed)


@pytest.mark.parametrize("kind", ["stripes", "shards"])
def test_launches_cut_by_the_hook_write_the_same_bytes(kind):
    k, m = 4, 2
    enc = RS.New(k, m)
    g = GP.glue_of(k, m, kind)
    res = GP.residues_for(g.sizes)
    starts, lens = ranges_for(k, g.sizes, g.masks, 2)
    one = run_range(g, enc, starts, lens, res)
    n_tiles = sum((s + GP.tile() - 1) // GP.tile() for s in g.sizes)
    s0 = B.glue_range_stats()
    B.set_glue_range_chunk_tiles(3)
    try:
        cut = run_range(g, enc, starts, lens, res)
    finally:
        B.set_glue_range_chunk_tiles(0)
    assert B.glue_range_stats()["kernel_launches"] - s0["kernel_launches"] == (n_tiles + 2) // 3 > 10
    assert np.array_equal(one, cut)


def test_other_streams_write_the_same_bytes():
    k, m = 8, 3
    enc = RS.New(k, m)
    g = GP.glue_of(k, m, "objects")
    res = GP.residues_for(g.sizes)
    starts, lens = ranges_for(k, g.sizes, g.masks, 5)
    one = run_range(g, enc, starts, lens, res)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def on_stream(plan, dsts):
        plan.glue_range(g.masks, dsts, starts, lens, stream=s1)
        s1.synchronize()

    assert np.array_equal(run_range(g, enc, starts, lens, res, call=on_stream), one)

    # two calls back to back on two streams: the second's staging waits for the first's launches.
    # The first writes the ranges' first bytes, the second the whole ranges over them.
    pre = [min(ln, 5) for ln in lens]

    def two_streams(plan, dsts):
        plan.glue_range(g.masks, dsts, starts, pre, stream=s1)
        plan.glue_range(g.masks, dsts, starts, lens, stream=s2)
        s1.synchronize()
        s2.synchronize()

    assert np.array_equal(run_range(g, enc, starts, lens, res, call=two_streams), one)


def test_13_plus_2_goes_entry_by_entry():
    k, m = 13, 2
    enc = RS.New(k, m)
    sizes = [0, 1, 17, 64, W + 1, 0, 4099, 333, 16, 2 * W, 5, 0, 40, 77, 130]
    masks = GP.masks_for(k, m, len(sizes))
    for kind in ("stripes", "shards"):
        g = GP.Glue(k, m, kind, sizes, masks, seed=133)
        res = [(3 * e) % 16 for e in range(len(sizes))]
        for shift in (0, 6):
            starts, lens = ranges_for(k, sizes, masks, shift)
            # what the per-entry route costs, from the masks and windows alone: a copy per present data shard
            # with a byte wanted; where a missing one has a byte wanted, one apply over the positions [A, B)
            # the missing shards' windows span, and a copy more for each of them whose window is not all of it
            calls = 0
            for e, s in enumerate(sizes):
                if not lens[e]:
                    continue
                win = [(max(0, min(s, starts[e] - j * s)), max(0, min(s, starts[e] + lens[e] - j * s)))
                       for j in range(k)]
                calls += sum(1 for j in range(k) if win[j][0] < win[j][1] and masks[e][j])
                lost = [win[j] for j in range(k) if win[j][0] < win[j][1] and not masks[e][j]]
                if lost:
                    hull = (min(w[0] for w in lost), max(w[1] for w in lost))
                    calls += 1 + sum(1 for w in lost if w != hull)
            s0 = B.glue_range_stats()
            run_range(g, enc, starts, lens, res)
            s1 = B.glue_range_stats()
            assert s1["kernel_launches"] == s0["kernel_launches"]
            assert s1["per_stripe_calls"] - s0["per_stripe_calls"] == calls > 0


@pytest.mark.parametrize("kind", ["stripes", "shards"])
def test_four_lost_data_shards_around_the_half_tile(kind):
    """With four data shards to rebuild the kernel codes a tile as two halves of
    T / 2 shard bytes: windows that begin and end just before, at and just behind
    a half's edge, in lost shards and in present ones, four data shards lost in
    every entry (and, in turn, none to three beside them in a second call's masks)."""
    k, m = 12, 4
    enc = RS.New(k, m)
    T, H = GP.tile(), GP.tile() // 2
    sizes = [H - 1, H, H + 1, H + 17, T - 1, T, T + 1, T + H - 1, T + H, T + H + 1, 2 * T + H + 5, 1, 16, T + H + 40]
    lost = [(0, 1, 2, 3), (8, 9, 10, 11), (0, 5, 6, 11), (1, 3, 7, 10)]
    four = np.array([[0 if j in lost[e % 4] else 1 for j in range(k + m)] for e in range(len(sizes))], np.uint8)
    g = GP.Glue(k, m, kind, sizes, four, seed=126)
    res = [(11 * e + 2) % 16 for e in range(len(sizes))]

    def ranges(shift):
        starts, lens = [], []
        for e, S in enumerate(sizes):
            a, b = [(H - 1, H + 1),                        # two bytes across the edge, shard 0
                    (3 * S + H, 4 * S + H),                # a junction; the two parts meet at H
                    (3 * S + H + 1, 4 * S + H - 1),        # they do not: positions H - 1 and H stay untouched
                    (H + 1, k * S - H - 1),
                    (8 * S, 8 * S + H),                    # ends at the edge
                    (11 * S + H, 12 * S),                  # begins at it
                    (5 * S + H - 1, 5 * S + T + H + 1),    # from before one half's edge to behind the next one's
                    (T, T + 1)][(e + shift) % 8]
            a, b = clip(k, S, a, b)
            starts.append(a)
            lens.append(b - a)
        return starts, lens

    s0 = B.glue_range_stats()
    for shift in range(0, 8, 3):
        run_range(g, enc, *ranges(shift), res)
    assert B.glue_range_stats()["kernel_launches"] - s0["kernel_launches"] == 3
    mixed = np.array([[0 if j in lost[e % 4][:e % 5] else 1 for j in range(k + m)] for e in range(len(sizes))],
                     np.uint8)
    run_range(GP.Glue(k, m, kind, sizes, mixed, seed=127), enc, *ranges(5), res)


def test_destinations_that_touch_own_shards_pass():
    """A destination may end where one of the entry's shards begins and begin where
    another ends: ranges that touch do not overlap.  One byte further is refused.
    The destination is lens bytes long wherever the range starts."""
    k, m, S = 4, 2, 50
    enc = RS.New(k, m)
    obj = np.asarray(O.object_bytes(78, k * S), np.uint8)
    par = CO.apply(CO.build_matrix(k, m)[k:], [obj[j * S:(j + 1) * S] for j in range(k)])
    stripe = np.concatenate([obj] + [np.asarray(p, np.uint8) for p in par])
    # [9 sentinels][hole of k S][stripe of (k+m) S][hole of k S][9 sentinels]
    host = np.full(18 + 2 * k * S + (k + m) * S, SENT, np.uint8)
    base = 9 + k * S
    host[base:base + (k + m) * S] = stripe
    t = torch.from_numpy(host.copy()).cuda()
    plan = B.StripePlan(enc, stripes=[(t.data_ptr() + base, S)])
    mask = np.array([[0, 1, 1, 1, 1, 1]], np.uint8)
    start, ln = S - 3, 2 * S + 7  # from the lost shard into two present ones
    for at in (base - ln, base + (k + m) * S):
        plan.glue_range(mask, [t.data_ptr() + at], [start], [ln])
        torch.cuda.synchronize()
        host[at:at + ln] = obj[start:start + ln]
        assert np.array_equal(t.cpu().numpy(), host)
    for at in (base - ln + 1, base + (k + m) * S - 1):
        with pytest.raises(RS.ErrInvalidArg, match="overlaps"):
            plan.glue_range(mask, [t.data_ptr() + at], [start], [ln])
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), host)


@pytest.mark.parametrize("kind", ["stripes", "shards"])
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)], ids=["4+2", "8+3"])
def test_a_range_inside_present_shards_of_a_degraded_entry_decodes_nothing(k, m, kind):
    """Entries with data shards lost (r > 0) and a range that touches present data
    shards alone.  Every shard buffer holds random bytes that are NOT a codeword,
    so anything decoded would be wrong: the expected bytes are the stored bytes of
    the data shards the range lies in, and a tile taken as coded could at best
    write them by luck of also gathering."""
    enc = RS.New(k, m)
    T = GP.tile()
    S = 2 * T + 17
    rng = np.random.default_rng(4100 + k)
    cases = [((0,), (2 * S + 5, 3 * S - 3)),             # inside data shard 2
             ((0,), (S, k * S)),                         # every present data shard, whole
             ((0, 3), (S + 1, 3 * S - 1)),               # two present shards between two lost ones
             ((k - 1,), (0, (k - 1) * S)),
             ((1,), (0, S)),
             ((0, 1), (2 * S + T - 1, 2 * S + T + 1))]   # two bytes across a tile's edge
    n = k + m
    shards = [[rng.integers(0, 256, S, dtype=np.uint8) for _ in range(n)] for _ in cases]
    masks = np.array([[0 if j in lost else 1 for j in range(n)] for lost, _ in cases], np.uint8)
    starts, lens = [a for _, (a, b) in cases], [b - a for _, (a, b) in cases]
    src = np.full(len(cases) * (n * S + 16) + 16, SENT, np.uint8)
    at = [7 + e * (n * S + 16) + (3 * e) % 16 for e in range(len(cases))]
    for e, a in enumerate(at):
        src[a:a + n * S] = np.concatenate(shards[e])
    t = torch.from_numpy(src.copy()).cuda()
    if kind == "stripes":
        plan = B.StripePlan(enc, stripes=[(t.data_ptr() + a, S) for a in at])
    else:
        plan = B.StripePlan(enc, shards=[([t.data_ptr() + a + j * S for j in range(n)], S) for a in at])
    offs, total = [], 5
    for ln in lens:
        offs.append(total)
        total += ln + 3
    dst = torch.full((total + 9,), SENT, dtype=torch.uint8, device="cuda")
    want = np.full(total + 9, SENT, np.uint8)
    for e, (o, a, ln) in enumerate(zip(offs, starts, lens)):
        want[o:o + ln] = np.concatenate(shards[e][:k])[a:a + ln]
    torch.cuda.synchronize()
    s0 = B.glue_range_stats()
    plan.glue_range(masks, [dst.data_ptr() + o for o in offs], starts, lens)
    torch.cuda.synchronize()
    assert B.glue_range_stats()["kernel_launches"] - s0["kernel_launches"] == 1
    assert np.array_equal(dst.cpu().numpy(), want)
    assert np.array_equal(t.cpu().numpy(), src)


def test_range_errors_with_a_device():
    """tests/test_glue_range_host.py's checks on entries with bytes in them, which
    need a device to build their plans on: here there is one."""
    assert GRH.range_errors() is True
