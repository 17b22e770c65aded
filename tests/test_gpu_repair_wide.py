"""hbec_repair_plan_wide: repair_mixed's contract for stripes of up to 32 data
shards in one launch, on every kind of plan.  Expected bytes and flags are
test_gpu_repair_mixed.oracle_repair's (never another GPU call); whole buffers,
slack included, and whole flag arrays are compared exactly.  The sizes cross the
992-B window and the 3968-B tile and have heads and tails shorter than 16 B."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_mixed_plan as MP
import test_gpu_repair_mixed as RM
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

pytestmark = pytest.mark.gpu

SIZES = [0, 17, 1, 4097, 1985, 0, 10_001, 33, 64, 993, 31, 3969, 15, 65, 0]
LAYOUTS = ["stripes", "objects", "shards", "files"]
SHAPES = [(13, 2), (16, 4), (17, 3), (20, 4), (32, 4), (4, 2)]


class Case(MP.Case):
    """MP.Case; as "shards" or "files" the object layout's buffers with every shard named.
    A files plan has no zero-length entries: `entries` are its entries' positions in `sizes`."""
    def __init__(self, k, m, layout, sizes, seed):
        super().__init__(k, m, layout if layout == "stripes" else "objects", sizes, seed)
        self.kind = layout
        self.entries = self.live if layout == "files" else list(range(len(sizes)))

    def plan(self, enc, t):
        if self.kind in MP.LAYOUTS:
            return super().plan(enc, t)
        addrs = [[t[b].data_ptr() + o for b, o in self.shards[e]] for e in self.entries]
        if self.kind == "shards":
            return B.StripePlan(enc, shards=[(a, self.sizes[e]) for a, e in zip(addrs, self.entries)])
        return B.StripePlan(enc, files=[(a, self.k * self.sizes[e]) for a, e in zip(addrs, self.entries)],
                            chunk_size=1 << 20)


@functools.lru_cache(maxsize=None)
def problem(k, m, layout, masks=None, data_only=False):
    """(case, input, present, oracle's (buffers, flags)): one and two losses, all present and exactly k
    present (or `masks` in turn), one bit flipped in a survivor or surplus shard of two entries in three."""
    n = k + m
    c = Case(k, m, layout, SIZES, 60 + k)
    rng = np.random.default_rng(61)
    present = np.ones((len(SIZES), n), np.uint8)
    for q, (e, lost) in enumerate(zip(c.live, [1, 2, 0, m, 1, 2, 0, m, 1, 2, 1, 2])):
        present[e][[i for i in range(n) if not masks[q % len(masks)][i]] if masks
                   else rng.choice(n, size=lost, replace=False)] = 0
    inp, _ = c.garble(present, data_only=data_only)
    for q, e in enumerate(c.live):
        if q % 3:
            here = [i for i in range(n) if present[e][i]]
            b, o = c.shards[e][here[q % len(here)]]
            inp[b][o + int(rng.integers(c.sizes[e]))] ^= 1 << (q % 8)
    want = RM.oracle_repair(c, inp, present, data_only)
    assert {0, 1, 2} == set(want[1].tolist())
    return c, inp, present, want


def run(c, bufs, present, data_only=False, call="repair_wide"):
    t = c.upload(bufs)
    plan = c.plan(RS.New(c.k, c.m), t)
    flags = torch.zeros(len(c.entries), dtype=torch.int32, device="cuda")
    getattr(plan, call)(present[c.entries], flags, data_only=data_only)
    torch.cuda.synchronize()
    full = np.zeros(len(c.sizes), np.uint32)  # flags by position in c.sizes
    full[c.entries] = flags.cpu().numpy().astype(np.uint32)
    return full, t


def check(c, bufs, present, want, data_only=False, launches=1):
    s0, r0 = B.repair_wide_stats(), B.repair_plan_stats()
    got, t = run(c, bufs, present, data_only)
    assert np.array_equal(got, want[1]), (got, want[1])
    MP.check_equal(t, want[0])
    assert B.repair_wide_stats()["kernel_launches"] - s0["kernel_launches"] == launches
    assert B.repair_plan_stats() == r0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", SHAPES)
def test_exact_and_counted(k, m, layout):
    check(*problem(k, m, layout))


# 16+4 under data_only: r_o = 0 with four and with two checked, r_c = 0 with four
# rebuilt, (2, 2) and (1, 3), and four parity shards lost: no row at all
DATA_ONLY_MASKS = tuple(tuple(0 if i in lost else 1 for i in range(20))
                        for lost in [(), (0, 5, 9, 15), (3, 11), (16, 18), (7,), (16, 17, 18, 19), (2, 12, 17)])


@pytest.mark.parametrize("data_only", [True, False])
@pytest.mark.parametrize("layout", ["objects", "shards"])
def test_data_only_row_sets(layout, data_only):
    check(*problem(16, 4, layout, DATA_ONLY_MASKS, data_only), data_only)


@pytest.mark.parametrize("chunk", [1, 2])
def test_chunk_hook_cuts_the_list_anywhere(chunk):
    c, inp, present, want = problem(20, 4, "stripes")
    n_tiles = sum(-(-s // B.repair_plan_tile_bytes()) for s in SIZES)  # 16
    B.set_repair_wide_chunk_tiles(chunk)
    try:
        check(c, inp, present, want, launches=-(-n_tiles // chunk))
    finally:
        B.set_repair_wide_chunk_tiles(0)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4)])
def test_same_result_as_repair_mixed(k, m, layout):
    c, inp, present, want = problem(k, m, layout)
    wide, t_wide = run(c, inp, present)
    mixed, t_mixed = run(c, inp, present, call="repair_mixed")
    assert np.array_equal(wide, mixed) and np.array_equal(wide, want[1])
    for x, y in zip(t_wide, t_mixed):
        assert torch.equal(x, y)
    MP.check_equal(t_wide, want[0])


@pytest.mark.parametrize("k,m,what,code", [
    (33, 4, "shape", N.ERR_INVALID_ARG), (4, 5, "shape", N.ERR_INVALID_ARG), (16, 4, "null", N.ERR_INVALID_ARG),
    (16, 4, "index", N.ERR_INVALID_ARG), (16, 4, "few", N.ERR_TOO_FEW_SHARDS)])
def test_errors_leave_no_trace(k, m, what, code):
    c = Case(k, m, "stripes", SIZES, 5)
    present = np.ones((len(SIZES), k + m), np.uint8)
    present[c.live[0]][0] = 0  # something to rebuild, were the call to run
    bufs, _ = c.garble(present)
    enc, t, flags = RS.New(k, m), c.upload(bufs), torch.zeros(len(SIZES), dtype=torch.int32, device="cuda")
    plan = c.plan(enc, t)
    pats, idx = plan._patterns(present)
    if what == "index":
        idx[-1] = pats.shape[0]  # a zero-length entry: checked all the same
    if what == "few":
        pats = np.vstack([pats, np.array([[1] * (k - 1) + [0] * (m + 1)], np.uint8)])  # listed, unused
    s0 = B.repair_wide_stats()
    rc = N.lib().hbec_repair_plan_wide(enc.handle, plan._h, None if what == "null" else pats.ctypes.data_as(N._U8P),
                                       pats.shape[0], idx.ctypes.data_as(C.POINTER(C.c_uint32)), 0,
                                       C.c_void_p(flags.data_ptr()), None)
    torch.cuda.synchronize()
    assert rc == code and B.repair_wide_stats() == s0 and not flags.cpu().numpy().any()
    MP.check_equal(t, bufs)
