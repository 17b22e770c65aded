"""hbec_split_plan_wide on the device, under tests/test_gpu_split_plan.py's class Split as it
stands.  The shard lengths cross the 992-B window and the 3968-B tile, have heads and tails
under 16 B, and S = 1 and S = 5 lie below k, where the pad covers whole trailing shards."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_split_plan as SP
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 17, 64, 993, 0, 4099, 333, 16, 1984, 5, 3969, 0]


def pads_of(k, second=False):
    """0 and 1; k-1 on S = 1 (every other data shard pad), on S = 4099 and on S = 5 (whole pad
    shards after a partial one), or 5 there in the second run (no partial input)."""
    pads = [0, k - 1, 0, 1, 2, 0, k - 1, 3, 0, 1, min(5, k - 1) if second else k - 1, 2, 0]
    assert all(p <= min(k - 1, max(k * s - 1, 0)) for p, s in zip(pads, SIZES))
    return pads


@functools.lru_cache(maxsize=None)
def split_of(k, m, kind, second=False):
    return SP.Split(k, m, kind, SIZES, pads_of(k, second), seed=37 * k + m + (500 if second else 0))


def residues(g, shift=0):  # 0..15 in turn over the pieces with bytes: ten a run, two runs cover them
    live = np.cumsum([1 if s else 0 for s in g.sizes]) - 1
    return [int(shift + i) % 16 for i in live]


def counted(g, enc, res, launches=1):
    w0, s0 = B.split_wide_stats(), B.split_plan_stats()
    got = g.run(enc, res, call=lambda plan, srcs, lens: plan.split_wide(srcs, lens))
    assert B.split_wide_stats()["kernel_launches"] - w0["kernel_launches"] == launches and B.split_plan_stats() == s0
    return got


@pytest.mark.parametrize("k,m,kind", [(k, m, q) for k, m in [(13, 2), (16, 4), (17, 3), (32, 4)] for q in SP.KINDS] +
                         [(15, 1, "stripes"), (15, 1, "shards")])
def test_exact_and_counted(k, m, kind):
    enc, g = RS.New(k, m), split_of(k, m, kind)
    counted(g, enc, residues(g))
    g = split_of(k, m, kind, second=True)
    assert g.lens[g.sizes.index(5)] == 5 * (k - 1)  # whole shards, then pad: no partial input
    counted(g, enc, residues(g, shift=10))


@pytest.mark.parametrize("kind", ["stripes", "shards"])
@pytest.mark.parametrize("k,m", [(4, 2), (12, 4)])
def test_same_bytes_as_split(k, m, kind):
    enc, g = RS.New(k, m), split_of(k, m, kind)
    res = residues(g, shift=5)
    assert all(np.array_equal(a, b) for a, b in zip(counted(g, enc, res), g.run(enc, res)))


@pytest.mark.parametrize("chunk", [1, 3])
def test_chunk_hook_cuts_the_list_anywhere(chunk):
    k, m = 20, 4
    enc, g = RS.New(k, m), split_of(k, m, "stripes")
    one = counted(g, enc, residues(g))
    n_tiles = sum(-(-s // B.split_plan_tile_bytes()) for s in SIZES)  # 12
    B.set_split_wide_chunk_tiles(chunk)
    try:
        cut = counted(g, enc, residues(g), launches=-(-n_tiles // chunk))
    finally:
        B.set_split_wide_chunk_tiles(0)
    assert all(np.array_equal(a, b) for a, b in zip(one, cut))


def test_files_objects_of_several_stripes():
    """Objects of one to three stripes into their files; then glue_files_wide with shards lost."""
    k, m, chunk = 16, 4, 1000
    n, enc = k + m, RS.New(16, 4)
    lengths = [k * 37 + 5, k * chunk + k * 41 + 3, 2 * k * chunk + k * 700 + 11]
    cuts = [O._stripe_sizes(k, chunk, L) for L in lengths]
    assert [len(c) for c in cuts] == [1, 2, 3] and cuts[2][2] == 701
    objs = [np.asarray(O.object_bytes(700 + g, L), np.uint8) for g, L in enumerate(lengths)]
    rng = np.random.default_rng(165)
    host = np.full(sum(n * (sum(c) + 16) for c in cuts) + 16, SP.SENT, np.uint8)
    want, files, at = host.copy(), [], 0
    for g, L in enumerate(lengths):
        addrs = []
        for j, body in enumerate(O.ec_split(k, m, objs[g].tobytes(), chunk)):
            at += 1 + (5 * j + g) % 16
            want[at:at + len(body)] = np.frombuffer(body, np.uint8)
            host[at:at + len(body)] = rng.integers(0, 256, len(body), dtype=np.uint8)
            addrs.append(at)
            at += len(body)
        files.append(addrs)
    offs, end = [], 0
    for g, L in enumerate(lengths):
        offs.append(end + 1 + (7 * g + 3) % 16)
        end = offs[-1] + L
    arena = np.full(end + 9, SP.SENT, np.uint8)
    for o, obj in zip(offs, objs):
        arena[o:o + obj.size] = obj
    t, src = torch.from_numpy(host.copy()).cuda(), torch.from_numpy(arena.copy()).cuda()
    plan = B.StripePlan(enc, files=[([t.data_ptr() + a for a in addrs], L) for addrs, L in zip(files, lengths)],
                        chunk_size=chunk)
    torch.cuda.synchronize()
    w0, s0 = B.split_wide_stats(), B.split_plan_stats()
    plan.split_files_wide([src.data_ptr() + o for o in offs])
    torch.cuda.synchronize()
    assert B.split_wide_stats()["kernel_launches"] - w0["kernel_launches"] == 1 and B.split_plan_stats() == s0
    assert np.array_equal(t.cpu().numpy(), want) and np.array_equal(src.cpu().numpy(), arena)
    present = np.ones((6, n), np.uint8)
    for e, g, stripe, lost in [(1, 1, 0, (0, 16, 17, 18)), (4, 2, 1, (14,))]:  # entry, its object and stripe
        present[e][list(lost)] = 0
        for j in lost:
            a, s = files[g][j] + sum(cuts[g][:stripe]), cuts[g][stripe]
            t[a:a + s] = torch.from_numpy(rng.integers(0, 256, s, dtype=np.uint8)).cuda()
    out = torch.full((arena.size,), SP.SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    plan.glue_files_wide(present, [out.data_ptr() + o for o in offs])
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), arena)


@pytest.mark.parametrize("k,m,what", [(33, 4, "shape"), (4, 5, "shape"), (16, 0, "shape"), (16, 4, "null"),
                                      (16, 4, "long"), (16, 4, "null source"), (16, 4, "overlap")])
def test_errors_leave_no_trace(k, m, what):
    enc, g = RS.New(k, m), SP.Split(k, m, "stripes", [0, 17, 333], [0, 0, 0], seed=6)
    offs, arena = g.src_arena([0, 3, 7])
    host = g.shard_bufs(after=False)
    t, src = [torch.from_numpy(x.copy()).cuda() for x in host], torch.from_numpy(arena.copy()).cuda()
    plan = g.plan(enc, t)
    addrs = [src.data_ptr() + o for o in offs]
    lens = list(g.lens)
    lens[2] += 1 if what == "long" else 0  # k S + 1
    addrs[1] = 0 if what == "null source" else addrs[1]
    if what == "overlap":  # the piece's last byte is the first of the entry's own shard 3
        addrs[2] = t[0].data_ptr() + g.at[2][3][1] - lens[2] + 1
    torch.cuda.synchronize()
    w0, s0 = B.split_wide_stats(), B.split_plan_stats()
    rc = N.lib().hbec_split_plan_wide(enc.handle, plan._h, None if what == "null" else (C.c_void_p * 3)(*addrs),
                                      np.array(lens, np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)), None)
    torch.cuda.synchronize()
    assert rc == N.ERR_INVALID_ARG and B.split_wide_stats() == w0 and B.split_plan_stats() == s0
    assert np.array_equal(src.cpu().numpy(), arena)
    for x, h in zip(t, host):
        assert np.array_equal(x.cpu().numpy(), h)
