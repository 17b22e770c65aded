"""hbec_reconstruct_batch_mixed on the GPU: a batch whose objects have lost
different shards (a repair sweep: shard i of an object lives on
ring.GetNodes(partition)[i], objectserver/ecobj.go:348-357) rebuilt by one
call, as ecReconstruct / ecGlue do per object (ecutils.go:94-111,151-168).

Every case: the oracle (oracle.coracle, the klauspost restatement) encodes n
objects into one buffer at a pitch with slack bytes between objects; a clone
is kept; each object's missing shards are overwritten with 0x6B; the call
runs; the WHOLE buffer, slack included, must equal the clone: the rebuilt
bytes are the oracle's codeword and nothing else was written."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO

pytestmark = pytest.mark.gpu

GONE = 0x6B


def masks_upto(k, m, e):
    """Every present mask of k+m shards with at most e missing (the complete one first)."""
    out = []
    for lost in range(e + 1):
        for miss in itertools.combinations(range(k + m), lost):
            out.append([0 if i in miss else 1 for i in range(k + m)])
    return np.array(out, dtype=np.uint8)


class Batch:
    """n oracle-encoded objects in one device buffer: shard i of object o at
    off + o * pitch + i * s; `keep` is the untouched clone."""

    def __init__(self, k, m, n, s, seed, slack=48, off=0):
        self.k, self.m, self.n, self.s, self.off = k, m, n, s, off
        self.pitch = (k + m) * s + slack
        rng = np.random.default_rng(seed)
        data = rng.integers(0, 256, (n, k, s), dtype=np.uint8)
        par = CO.apply(CO.build_matrix(k, m)[k:], [data[:, j, :].reshape(-1) for j in range(k)])
        host = rng.integers(0, 256, off + n * self.pitch + 64, dtype=np.uint8)  # slack: random bytes
        rows = host[off:off + n * self.pitch].reshape(n, self.pitch)
        rows[:, :k * s] = data.reshape(n, k * s)
        for r in range(m):
            rows[:, (k + r) * s:(k + r + 1) * s] = par[r].reshape(n, s)
        self.buf = torch.from_numpy(host).cuda()
        self.keep = self.buf.clone()
        self.views = [(self.buf.data_ptr() + off + i * s, self.pitch) for i in range(k + m)]
        self.enc = RS.New(k, m)

    def shards(self, t=None):
        """[n, k+m, s] view of the shards of buffer t (default: the live buffer)."""
        t = self.buf if t is None else t
        k, m, n, s = self.k, self.m, self.n, self.s
        return t[self.off:self.off + n * self.pitch].view(n, self.pitch)[:, :(k + m) * s].view(n, k + m, s)

    def erase(self, present, t=None, value=GONE):
        gone = torch.from_numpy(np.asarray(present) == 0).cuda()
        self.shards(t)[gone] = value

    def intact(self):
        return torch.equal(self.buf, self.keep)


def run_mixed(b, present, **kw):
    s0 = B.mixed_stats()
    B.reconstruct_views_mixed(b.enc, b.views, present, b.n, b.s, **kw)
    torch.cuda.synchronize()
    s1 = B.mixed_stats()
    return s1["mixed"] - s0["mixed"], s1["runs"] - s0["runs"]


def shuffled(masks, times, seed):
    p = np.concatenate([masks] * times)
    np.random.default_rng(seed).shuffle(p, axis=0)
    return p


T4 = B.mixed_tile_bytes(4)
T8 = B.mixed_tile_bytes(8)


# 1. every pattern in one call
@pytest.mark.parametrize("s", [16, T4 - 16, T4, T4 + 16, 2 * T4 + 16])
def test_every_pattern_4_2(s):
    present = shuffled(masks_upto(4, 2, 2), 2, seed=s)
    assert len(present) == 44
    b = Batch(4, 2, len(present), s, seed=100 + s)
    b.erase(present)
    assert not b.intact()
    mixed, runs = run_mixed(b, present)
    assert b.intact()
    assert mixed >= 1 and runs == 0, (mixed, runs)


@pytest.mark.parametrize("s", [528, T8 + 16])
def test_every_pattern_8_3(s):
    present = shuffled(masks_upto(8, 3, 3), 1, seed=s)
    assert len(present) == 232
    b = Batch(8, 3, len(present), s, seed=200 + s)
    b.erase(present)
    mixed, runs = run_mixed(b, present)
    assert b.intact()
    assert mixed >= 3 and runs == 0, (mixed, runs)  # one launch per output count 1, 2, 3


def test_sampled_patterns_6_4():
    allm = masks_upto(6, 4, 4)
    assert len(allm) == 386
    pick = np.sort(np.random.default_rng(64).choice(len(allm), 200, replace=False))
    present = shuffled(allm[pick], 1, seed=64)
    assert (present.sum(axis=1) == 6).sum() >= 50  # R = 4 instances run
    b = Batch(6, 4, len(present), 1040, seed=640)
    b.erase(present)
    mixed, runs = run_mixed(b, present)
    assert b.intact()
    assert mixed >= 4 and runs == 0, (mixed, runs)


# 2. data_only: missing parity stays as it was, missing data is rebuilt
def test_data_only():
    present = shuffled(masks_upto(4, 2, 2), 2, seed=2)
    b = Batch(4, 2, len(present), 1040, seed=2)
    b.erase(present)
    want = b.keep.clone()
    parity_gone = present.copy()
    parity_gone[:, :4] = 1
    b.erase(parity_gone, want)
    mixed, runs = run_mixed(b, present, data_only=True)
    assert torch.equal(b.buf, want)
    assert mixed >= 1 and runs == 0


# 3. survivors are the first k present shards; later present shards are not read
def test_first_k_survivors_only():
    present = shuffled(masks_upto(8, 3, 2), 1, seed=3)
    present = present[present.sum(axis=1) > 8]
    b = Batch(8, 3, len(present), 528, seed=3)
    beyond = np.ones_like(present)  # 0 = a present shard after the first k present ones
    for o, row in enumerate(present):
        for i in np.flatnonzero(row)[8:]:
            beyond[o, i] = 0
    assert (beyond == 0).any()
    b.erase(beyond, b.keep, value=0xE7)  # garbage in the expected buffer and in the live one
    b.erase(beyond, value=0xE7)
    b.erase(present)
    run_mixed(b, present)
    assert b.intact()


# 4. one pattern for every object: the same bytes as hbec_reconstruct_batch
def test_same_bytes_as_uniform_entry():
    mask = [1, 0, 1, 1, 0, 1]
    b = Batch(4, 2, 37, 2064, seed=4)
    present = np.array([mask] * b.n, dtype=np.uint8)
    b.erase(present)
    second = b.buf.clone()
    v2 = [(second.data_ptr() + i * b.s, b.pitch) for i in range(6)]
    B.reconstruct_views(b.enc, v2, mask, b.n, b.s)
    mixed, runs = run_mixed(b, present)
    assert torch.equal(b.buf, second)
    assert b.intact()
    assert mixed == 1 and runs == 0


# 5. more tiles than resident waves: every wave loops
def test_looping_waves():
    three = np.array([[0, 1, 1, 0, 1, 1], [1, 0, 1, 1, 1, 0], [1, 1, 0, 1, 0, 1]], dtype=np.uint8)
    n, s = 128, 65552
    assert n * -(-s // T4) > 8192
    present = three[np.arange(n) % 3]
    b = Batch(4, 2, n, s, seed=5)
    b.erase(present)
    mixed, runs = run_mixed(b, present)
    assert b.intact()  # compared on the device
    assert mixed == 1 and runs == 0


def test_looping_waves_grid_stride():
    """Few records over long shards: the launch walks its tiles grid-stride
    (hbec.cpp mixed_contiguous; the case above gives each wave a contiguous
    run), several tiles per wave, the record changing between a wave's tiles."""
    two = np.array([[0, 1, 1, 0, 1, 1], [1, 1, 0, 1, 0, 1]], dtype=np.uint8)
    n, s = 192, 65552
    present = two[(np.arange(n) // 5) % 2]
    b = Batch(4, 2, n, s, seed=55)
    b.erase(present)
    mixed, runs = run_mixed(b, present)
    assert b.intact()
    assert mixed == 1 and runs == 0


# 6. a batch that crosses launch boundaries
def test_launch_boundaries():
    three = np.array([[0, 0, 1, 1, 1, 1], [1, 1, 1, 0, 1, 0], [1, 0, 1, 1, 0, 1]], dtype=np.uint8)
    n, s = 60, 2064  # 3 tiles per object
    present = three[np.random.default_rng(6).integers(0, 3, n)]
    b = Batch(4, 2, n, s, seed=6)
    b.erase(present)
    try:
        B.set_mixed_chunk_tiles(40)  # 13 objects per launch
        mixed, runs = run_mixed(b, present)
    finally:
        B.set_mixed_chunk_tiles(0)
    assert b.intact()
    assert mixed >= 3 and runs == 0, (mixed, runs)


# 7. queued on the caller's stream
def test_side_stream():
    present = shuffled(masks_upto(4, 2, 2), 2, seed=7)
    b = Batch(4, 2, len(present), 4112, seed=7)
    b.erase(present)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    B.reconstruct_views_mixed(b.enc, b.views, present, b.n, b.s, stream=side)
    side.synchronize()
    assert b.intact()


# 8. shapes the mixed kernel does not take: one launch per run of equal patterns
def test_run_route_unaligned():
    present = shuffled(masks_upto(4, 2, 2), 2, seed=8)
    b = Batch(4, 2, len(present), 1001, seed=8, slack=5, off=3)
    b.erase(present)
    mixed, runs = run_mixed(b, present)
    assert b.intact()
    assert mixed == 0 and runs >= 1, (mixed, runs)


def test_run_route_k10():
    present = shuffled(masks_upto(10, 4, 2), 1, seed=9)
    assert len(present) == 106
    b = Batch(10, 4, len(present), 1040, seed=9)
    b.erase(present)
    mixed, runs = run_mixed(b, present)
    assert b.intact()
    assert mixed == 0 and runs >= 1, (mixed, runs)


def test_run_route_control_is_fast():
    b = Batch(4, 2, 44, 1040, seed=10)
    present = np.array([[1, 1, 0, 1, 1, 0]] * b.n, dtype=np.uint8)
    b.erase(present)
    mixed, runs = run_mixed(b, present)
    assert b.intact()
    assert mixed == 1 and runs == 0, (mixed, runs)


# 9. argument errors with real device views: nothing is queued
def test_errors_leave_the_buffer_unchanged():
    b = Batch(4, 2, 12, 1040, seed=11)
    present = np.array([[0, 1, 1, 1, 1, 1]] * b.n, dtype=np.uint8)
    b.erase(present)
    before = b.buf.clone()
    views = B._views(b.views)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(patterns, idx):
        pat = np.ascontiguousarray(patterns, dtype=np.uint8)
        ix = np.ascontiguousarray(idx, dtype=np.uint32)
        return N.lib().hbec_reconstruct_batch_mixed(b.enc.handle, views, pat.ctypes.data_as(N._U8P), pat.shape[0],
                                                    ix.ctypes.data_as(C.POINTER(C.c_uint32)), b.n, b.s, 0, stream)

    good = [0, 1, 1, 1, 1, 1]
    assert call([good, [1] * 6], [0] * 11 + [2]) == N.ERR_INVALID_ARG  # the last object's index
    assert call([good, [1, 1, 0, 0, 0, 1]], [0] * 11 + [1]) == N.ERR_TOO_FEW_SHARDS
    torch.cuda.synchronize()
    assert torch.equal(b.buf, before)
    assert call([good], [0] * 12) == N.HBEC_OK  # and the same views do rebuild
    torch.cuda.synchronize()
    assert b.intact()
