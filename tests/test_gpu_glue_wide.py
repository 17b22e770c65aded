"""hbec_glue_plan_wide on the device: glue_mixed's contract for stripes of up to 32
data shards in one launch, on every kind of plan, under tests/test_gpu_glue_plan.py's
class Glue as it stands (oracle bytes, whole arena with sentinels, shard buffers
unchanged).  The shard lengths cross the 992-B window and the 3968-B tile and have
heads and tails shorter than 16 B."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_gpu_glue_plan as GP
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 17, 64, 993, 0, 4099, 333, 16, 1984, 5, 3969, 0]
RES = [(3 * e) % 16 for e in range(len(SIZES))]


def lost_sets(k, m):
    """Healthy; data shard 0, 12 (the first the 12-wide record cannot name) and k-1 lost; min(m, 4)
    data shards lost; parity alone lost; data shard 0 and all parity but the last shard lost."""
    n = k + m
    return [(), (0,), (min(12, k - 1),), (k - 1,), tuple(sorted({0, k - 1, min(12, k - 1), 5}))[-min(m, 4):],
            tuple(range(k, n)), (0,) + tuple(range(k, n - 1))]


def masks_of(k, m, sizes):
    """The lost sets in turn over the entries with bytes."""
    sets, live = lost_sets(k, m), 0
    masks = np.ones((len(sizes), k + m), np.uint8)
    for e, s in enumerate(sizes):
        if s:
            masks[e][list(sets[live % len(sets)])] = 0
            live += 1
    return masks


@functools.lru_cache(maxsize=None)
def glue_of(k, m, kind, wide_masks=True):
    masks = masks_of(k, m, SIZES) if wide_masks else GP.masks_for(k, m, len(SIZES))
    return GP.Glue(k, m, kind, SIZES, masks, seed=31 * k + m)


def counted(g, enc, lens, res, launches=1):
    w0, m0 = B.glue_wide_stats(), B.glue_plan_stats()
    got = g.run(enc, lens, res, call=lambda plan, dsts: plan.glue_wide(g.masks, dsts, lens))
    assert B.glue_wide_stats()["kernel_launches"] - w0["kernel_launches"] == launches and B.glue_plan_stats() == m0
    return got


@pytest.mark.parametrize("kind", GP.KINDS)
@pytest.mark.parametrize("k,m", [(13, 2), (16, 4), (17, 3), (32, 4)])
def test_exact_and_counted(k, m, kind):
    enc, g = RS.New(k, m), glue_of(k, m, kind)
    res = RES[:len(g.sizes)]
    counted(g, enc, GP.trunc_lens(k, g.sizes), res)
    counted(g, enc, GP.prefix_lens(k, g.sizes), res[5:] + res[:5])  # ends before, at and after the lost shards


@pytest.mark.parametrize("kind", ["stripes", "shards"])
@pytest.mark.parametrize("k,m", [(4, 2), (12, 4)])
def test_same_bytes_as_glue_mixed(k, m, kind):
    enc, g = RS.New(k, m), glue_of(k, m, kind, wide_masks=False)
    for lens in (GP.trunc_lens(k, g.sizes), GP.prefix_lens(k, g.sizes)):
        assert np.array_equal(counted(g, enc, lens, RES), g.run(enc, lens, RES))


@pytest.mark.parametrize("chunk", [1, 3])
def test_chunk_hook_cuts_the_list_anywhere(chunk):
    k, m = 20, 4
    enc, g, lens = RS.New(k, m), glue_of(k, m, "stripes"), GP.trunc_lens(k, SIZES)
    one = counted(g, enc, lens, RES)
    n_tiles = sum(-(-s // B.glue_plan_tile_bytes()) for s in SIZES)  # 12
    B.set_glue_wide_chunk_tiles(chunk)
    try:
        cut = counted(g, enc, lens, RES, launches=-(-n_tiles // chunk))
    finally:
        B.set_glue_wide_chunk_tiles(0)
    assert np.array_equal(one, cut)


def test_files_objects_of_several_stripes():
    """Objects of one, two and three stripes, odd last ones; entries 1, 3 and 4 lose different shards."""
    k, m, chunk = 16, 4, 1000
    n, enc = k + m, RS.New(16, 4)
    lengths = [k * 37 + 5, k * chunk + k * 41 + 3, 2 * k * chunk + k * 700 + 11]
    cuts = [O._stripe_sizes(k, chunk, L) for L in lengths]
    assert [len(c) for c in cuts] == [1, 2, 3] and cuts[2][2] == 701
    lost = {1: (0, 16, 17, 18), 3: (2,), 4: (14,)}  # by entry
    objs = [np.asarray(O.object_bytes(900 + g, L), np.uint8) for g, L in enumerate(lengths)]
    rng = np.random.default_rng(164)
    host = np.full(sum(n * (sum(c) + 16) for c in cuts) + 16, GP.SENT, np.uint8)
    files, present, at = [], [], 0
    for g, L in enumerate(lengths):
        addrs = []
        for j, body in enumerate(O.ec_split(k, m, objs[g].tobytes(), chunk)):
            at += 1 + (5 * j + g) % 16
            body, off = np.frombuffer(body, np.uint8).copy(), 0
            for t, s in enumerate(cuts[g]):
                if j in lost.get(len(present) + t, ()):
                    body[off:off + s] = rng.integers(0, 256, s, dtype=np.uint8)  # never to be read
                off += s
            host[at:at + body.size] = body
            addrs.append(at)
            at += body.size
        files.append(addrs)
        present += [[0 if j in lost.get(len(present) + t, ()) else 1 for j in range(n)] for t in range(len(cuts[g]))]
    t = torch.from_numpy(host.copy()).cuda()
    plan = B.StripePlan(enc, files=[([t.data_ptr() + a for a in addrs], L) for addrs, L in zip(files, lengths)],
                        chunk_size=chunk)
    assert plan.object_start.tolist() == [0, 1, 3, 6]
    offs, end = [], 0
    for g, L in enumerate(lengths):
        offs.append(end + 1 + (7 * g + 3) % 16)
        end = offs[-1] + L
    want = np.full(end + 9, GP.SENT, np.uint8)
    for o, obj in zip(offs, objs):
        want[o:o + obj.size] = obj
    out = torch.full((end + 9,), GP.SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w0, m0 = B.glue_wide_stats(), B.glue_plan_stats()
    plan.glue_files_wide(np.array(present, np.uint8), [out.data_ptr() + o for o in offs])
    torch.cuda.synchronize()
    assert B.glue_wide_stats()["kernel_launches"] - w0["kernel_launches"] == 1 and B.glue_plan_stats() == m0
    got = out.cpu().numpy()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:6]
    assert np.array_equal(t.cpu().numpy(), host)


@pytest.mark.parametrize("k,m,what,code", [
    (33, 4, "shape", N.ERR_INVALID_ARG), (4, 5, "shape", N.ERR_INVALID_ARG), (16, 4, "null", N.ERR_INVALID_ARG),
    (16, 4, "long", N.ERR_INVALID_ARG), (16, 4, "overlap", N.ERR_INVALID_ARG), (16, 4, "few", N.ERR_TOO_FEW_SHARDS)])
def test_errors_leave_no_trace(k, m, what, code):
    sizes = [0, 17, 333]
    masks = np.ones((3, k + m), np.uint8)
    masks[1][0] = 0  # something to decode, were the call to run
    enc, g = RS.New(k, m), GP.Glue(k, m, "stripes", sizes, masks, seed=5)
    lens = [0, k * 17, k * 333 + (1 if what == "long" else 0)]
    offs, total = g.dst_layout(lens, [3, 7, 11])
    host = g.shard_bufs()
    t = [torch.from_numpy(x.copy()).cuda() for x in host]
    dst = torch.full((total,), GP.SENT, dtype=torch.uint8, device="cuda")
    plan = g.plan(enc, t)
    addrs = [dst.data_ptr() + o for o in offs]
    if what == "overlap":
        addrs[2] = t[0].data_ptr() + g.at[2][3][1] + 5  # inside the entry's own shard 3
    pats, idx = plan._patterns(masks)
    if what == "few":
        pats = np.vstack([pats, np.array([[1] * (k - 1) + [0] * (m + 1)], np.uint8)])  # listed, unused
    torch.cuda.synchronize()
    s0 = B.glue_wide_stats()
    rc = N.lib().hbec_glue_plan_wide(enc.handle, plan._h, pats.ctypes.data_as(N._U8P), pats.shape[0],
                                     idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     None if what == "null" else (C.c_void_p * 3)(*addrs),
                                     np.array(lens, np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)), None)
    torch.cuda.synchronize()
    assert rc == code and B.glue_wide_stats() == s0
    assert (dst.cpu().numpy() == GP.SENT).all()
    for x, h in zip(t, host):
        assert np.array_equal(x.cpu().numpy(), h)
