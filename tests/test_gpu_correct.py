"""hbec_correct_plan_mixed (csrc/correct.hip, behind plan.correct_mixed).  The
reference is the clean codeword: test_gpu_mixed_plan.Case encodes with the
oracle, non-zero values are XORed into bytes of present shards, and after the
call the WHOLE buffers (slack and missing shards' garbage included) must equal
the copy taken before the XORs, or the input where a position must stay."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_locate as LOC
import test_gpu_mixed_plan as MP
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

pytestmark = pytest.mark.gpu

BAD, SKIPPED, NOTHING, LEFT = N.COR_BAD, N.COR_SKIPPED, N.COR_NOTHING, N.COR_LEFT


def both(f):
    shapes = pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4), (3, 2)])
    return pytest.mark.parametrize("layout", MP.LAYOUTS + ["shards"])(shapes(f))


@functools.lru_cache(maxsize=None)
def case(k, m, layout, repeat=3):
    T, W = B.correct_plan_tile_bytes(), B.correct_plan_tile_bytes() // 4
    sizes = [0, 1, 15, 16, 17, W - 1, W, W + 1, 0, T - 1, T, T + 1, 2 * T + 1, 0] * repeat
    c = MP.Case(k, m, "objects" if layout == "shards" else layout, sizes, 11 * k + m)
    if layout == "shards":  # the objects layout handed over as a pointer per shard: the _rows kernels
        c.plan = lambda enc, t: B.StripePlan(enc, shards=[([t[b].data_ptr() + o for b, o in where], s)
                                                          for where, s in zip(c.shards, c.sizes)])
    return c


def positions(s):  # 0, S - 1, the head, both sides of every window / tile seam, 32 bytes of every later window
    W = B.correct_plan_tile_bytes() // 4
    pos = {0, s - 1} | set(range(min(s, 40)))
    for w in range(W, s, W):
        pos |= {w - 1} | set(range(w, min(s, w + 32)))
    return sorted(pos)


def masks_with(c, rs, seed=0):  # a mask per entry, r checked shards cycling over rs; garbage in the missing shards
    by_r = LOC.masks_by_checked(c.k, c.m)
    present = np.ones((len(c.sizes), c.k + c.m), np.uint8)
    for q, e in enumerate(c.live):
        ms = by_r[rs[q % len(rs)]]
        present[e] = ms[(7 * q + seed) % len(ms)]
    return present, c.garble(present, seed=3)[0]


def xor_columns(c, targets, e, present, skip=()):
    """One bad byte per column of positions(S), the present shards in turn (neighbours in a dword
    differ in shard), into every set of buffers in `targets`.  Returns the shards' bits."""
    here = [i for i in range(c.k + c.m) if present[e][i]]
    bits = 0
    for i, p in enumerate(x for x in positions(c.sizes[e]) if x not in skip):
        for bufs in targets:
            LOC.corrupt(c, bufs, e, here[(i + e) % len(here)], p, 1 + (37 * p + e) % 255)
        bits |= 1 << here[(i + e) % len(here)]
    return bits


def correct(c, bufs, present):
    """One call over `bufs`; returns (words, tensors, plan, kernel launches)."""
    t = c.upload(bufs)
    plan = c.plan(RS.New(c.k, c.m), t)
    fixed = LOC.zeros_like_case(c)
    s0 = B.correct_plan_stats()
    plan.correct_mixed(present, fixed)
    torch.cuda.synchronize()
    return LOC.words(fixed), t, plan, B.correct_plan_stats()["kernel_launches"] - s0["kernel_launches"]


def many_shards(c):
    # (present, clean, corrupted, expected words): every present shard of every entry is bad somewhere
    present, clean = masks_with(c, list(range(2, c.m + 1)))
    bufs = [x.copy() for x in clean]
    want = np.array([BAD | xor_columns(c, [bufs], e, present) if s else 0 for e, s in enumerate(c.sizes)],
                    np.uint32)
    assert all(want[e] == BAD | sum(1 << i for i in np.nonzero(present[e])[0]) for e in c.live if c.sizes[e] >= 40)
    return present, clean, bufs, want


@both
def test_one_bad_byte_per_column_in_many_shards(k, m, layout):
    c = case(k, m, layout)
    present, clean, bufs, want = many_shards(c)
    assert {int(present[e].sum()) - k for e in c.live} == set(range(2, m + 1))
    n_tiles = sum(-(-s // B.correct_plan_tile_bytes()) for s in c.sizes)
    for chunk in (0, 1, 3):  # launch boundaries anywhere in the tile list
        B.set_correct_plan_chunk_tiles(chunk)
        try:
            got, t, plan, launches = correct(c, bufs, present)
        finally:
            B.set_correct_plan_chunk_tiles(0)
        MP.check_equal(t, clean)
        assert np.array_equal(got, want), (chunk, np.nonzero(got != want)[0][:10])
        assert launches == (-(-n_tiles // chunk) if chunk else 1)
    flags = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    plan.verify_mixed(present, flags)
    assert not flags.cpu().numpy().any()
    small = case(k, m, layout, 1)  # a third of the entries, every shard present (None), no errors: one launch too
    got, _, _, launches = correct(small, small.bufs, None)
    assert not got.any() and launches == 1


@both
def test_what_must_be_left_alone(k, m, layout):
    c = case(k, m, layout)
    roles = ["one", "k", "clean"] + (["two"] if m >= 3 else [])
    present, clean = masks_with(c, [{"one": 1, "k": 0, "clean": 2, "two": 3}[x] for x in roles])
    bufs, want_bufs = [x.copy() for x in clean], [x.copy() for x in clean]
    want = np.zeros(len(c.sizes), np.uint32)
    for q, e in enumerate(c.live):
        role, x = roles[q % len(roles)], c.sizes[e] // 2
        if role in ("one", "k"):  # undecidable with one checked shard; nothing to check with none
            xor_columns(c, [bufs, want_bufs], e, present)
            want[e] = BAD | LEFT if role == "one" else NOTHING
        elif role == "two":  # a survivor and a checked shard bad in column x; single bad bytes elsewhere
            for i in np.nonzero(present[e])[0][[0, -1]]:
                for b in (bufs, want_bufs):
                    LOC.corrupt(c, b, e, int(i), x, 0x35)
            want[e] = BAD | LEFT | xor_columns(c, [bufs], e, present, skip=(x,))
    got, t, _, _ = correct(c, bufs, present)
    MP.check_equal(t, want_bufs)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]


@both
def test_filter_and_or(k, m, layout):
    c = case(k, m, layout, 2)
    present, clean = masks_with(c, [2, 0, m, m], seed=1)
    bufs, want_bufs = [x.copy() for x in clean], [x.copy() for x in clean]
    pre = (1 << 20) | 0x8000  # a bit the call never sets and a shard bit of the caller's own
    want = np.full(len(c.sizes), pre, np.uint32)
    want[c.live[1::4]] |= NOTHING  # exactly k present: said although Verify's flag (2) keeps the entry out
    for q, e in enumerate(c.live[::2]):  # every second entry is corrupt; every second of those is filtered out
        bits = xor_columns(c, [bufs, want_bufs] if q % 2 else [bufs], e, present)
        want[e] |= 0 if q % 2 else BAD | bits
    t = c.upload(bufs)
    plan = c.plan(RS.New(k, m), t)
    flags = torch.zeros(len(c.sizes), dtype=torch.int32, device="cuda")
    plan.verify_mixed(present, flags)
    assert set(np.nonzero(flags.cpu().numpy() & 1)[0].tolist()) == set(c.live[::2])
    flags[torch.tensor(c.live[2::4], device="cuda")] &= ~1
    fixed = LOC.zeros_like_case(c, pre)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    plan.correct_mixed(present, fixed, flags=flags, stream=side)
    side.synchronize()
    MP.check_equal(t, want_bufs)
    assert np.array_equal(LOC.words(fixed), want)
    with pytest.raises(ValueError):
        plan.correct_mixed(present, fixed, flags=fixed)  # aliasing


@pytest.mark.parametrize("layout", MP.LAYOUTS)
@pytest.mark.parametrize("k,m", [(13, 2), (4, 5)])
def test_other_route_is_skipped_and_counted(k, m, layout):
    c = case(k, m, layout, 1)
    bufs = [x.copy() for x in c.bufs]
    for e in c.live:
        LOC.corrupt(c, bufs, e, e % (k + m), c.sizes[e] - 1, 0x21)
    s0 = B.correct_plan_stats()
    got, t, _, launches = correct(c, bufs, None)
    assert np.array_equal(got, np.array([SKIPPED if s else 0 for s in c.sizes], np.uint32))
    MP.check_equal(t, bufs)
    assert B.correct_plan_stats()["skipped_entries"] - s0["skipped_entries"] == len(c.live) and launches == 0


@both
def test_errors_leave_no_trace(k, m, layout):
    c = case(k, m, layout, 1)
    present, clean, bufs, want = many_shards(c)
    enc, n = RS.New(k, m), len(c.sizes)
    t = c.upload(bufs)
    plan = c.plan(enc, t)
    fixed = torch.zeros(n, dtype=torch.int32, device="cuda")
    pats, idx = np.unique(present, axis=0, return_inverse=True)
    pats, idx = np.ascontiguousarray(pats, np.uint8), np.ascontiguousarray(idx.reshape(-1), np.uint32)

    def call(p=pats, i=idx, n_patterns=None, e=enc, flags=None, out=fixed):
        return N.lib().hbec_correct_plan_mixed(e.handle, plan._h, p.ctypes.data_as(N._U8P),
                                               p.shape[0] if n_patterns is None else n_patterns,
                                               i.ctypes.data_as(LOC.U32P), flags,
                                               None if out is None else C.c_void_p(out.data_ptr()), None)

    s0 = B.correct_plan_stats()
    bad = idx.copy()
    bad[n - 1] = pats.shape[0]  # the last entry is zero-length: checked all the same
    few = np.vstack([pats, np.array([[1] * (k - 1) + [0] * (m + 1)], np.uint8)])  # listed, unused
    assert call(e=RS.New(k + 1, m)) == call(i=bad) == call(n_patterns=0) == call(n_patterns=65537) \
        == call(out=None) == call(flags=C.c_void_p(fixed.data_ptr())) == N.ERR_INVALID_ARG
    assert "alias" in N.last_error() and call(p=few) == N.ERR_TOO_FEW_SHARDS
    assert B.correct_plan_stats() == s0 and not fixed.cpu().numpy().any()
    MP.check_equal(t, bufs)
    assert call() == N.HBEC_OK and np.array_equal(LOC.words(fixed), want)
    MP.check_equal(t, clean)
