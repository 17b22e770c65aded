"""The store schedule of the pipelined kernel gf_apply_vec_pipe2: a wave keeps
the outputs of T tiles (T = the store depth, kernels.h pipe2_store_depth) in
registers and stores them in one burst, in groups of T steps, then single
steps, then the last tile; with the run walk a block takes 4 T consecutive
tiles per group.  The hooks hbec_set_vec_grid_cap / hbec_set_vec_chunk_tiles
shrink the grid to G blocks (nw = 4 G waves) and the launch to a few tiles, so
kilobytes of data walk every trip count around the group size, put the masked
store in every slot of a burst, straddle objects and cross launches.

Expected bytes always come from the oracle (coracle.apply_batch over the same
strided views, on a host copy of the device buffer), and the WHOLE buffer is
compared: 64-B canaries before and after, the slack between rows and every
shard the call must not touch included (reedsolomon Encode / Reconstruct,
objectserver/ecutils.go:59,111)."""
import numpy as np
import pytest
import torch

from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import coracle as CO

pytestmark = pytest.mark.gpu

CANARY = 64


@pytest.fixture(autouse=True)
def _hooks():
    yield
    B.set_vec_grid_cap(0)
    B.set_vec_chunk_tiles(0)


def depth():
    return B.pipe2_store_depth(4, 2)[0]


def layout(kind, k, m, s, n):
    """(buffer bytes, [(offset, stride)] of the k + m shards): `split` is the
    benchmark's (objects and parity in two arrays), `databuf` ecSplit's (parity
    behind the data in the same row), `pitch` a parity pitch beyond m S."""
    if kind == "databuf":
        row = (k + m) * s
        return 2 * CANARY + n * row, [(CANARY + i * s, row) for i in range(k + m)]
    gap = 48 if kind == "pitch" else 0
    drow, prow = k * s, m * s + gap
    pbase = CANARY + n * drow + CANARY
    views = [(CANARY + j * s, drow) for j in range(k)] + [(pbase + r * s, prow) for r in range(m)]
    return pbase + n * prow + CANARY, views


def encode_case(k, m, s, n, kind="split", seed=1):
    """Encode n objects on the device and on the oracle; compare whole buffers."""
    size, views = layout(kind, k, m, s, n)
    buf = torch.empty(size, dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf.view(1, -1), size, first=seed)
    want = buf.cpu().numpy().copy()
    base = want.ctypes.data
    CO.apply_batch(CO.build_matrix(k, m)[k:], [(base + o, st) for o, st in views[:k]],
                   [(base + o, st) for o, st in views[k:]], n, s)
    B.encode_views(RS.New(k, m), [(buf.data_ptr() + o, st) for o, st in views], n, s)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{k}+{m} S={s} n={n} {kind}: {bad.size} bytes differ, first at {bad[0]} of {size}")
    return buf, views, want


def reconstruct_case(k, m, s, n, lost, kind="databuf", seed=2):
    """Stripes coded by the oracle, `lost` shards overwritten, rebuilt in place."""
    size, views = layout(kind, k, m, s, n)
    buf = torch.empty(size, dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf.view(1, -1), size, first=seed)
    want = buf.cpu().numpy().copy()
    base = want.ctypes.data
    CO.apply_batch(CO.build_matrix(k, m)[k:], [(base + o, st) for o, st in views[:k]],
                   [(base + o, st) for o, st in views[k:]], n, s)
    hurt = want.copy()
    for i in lost:
        o, st = views[i]
        for j in range(n):
            hurt[o + j * st:o + j * st + s] = 0x5A
    buf.copy_(torch.from_numpy(hurt))
    B.reconstruct_views(RS.New(k, m), [(buf.data_ptr() + o, st) for o, st in views],
                        [0 if i in lost else 1 for i in range(k + m)], n, s)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{k}+{m} S={s} n={n} lost={lost}: {bad.size} bytes differ, first at {bad[0]}")


def trip_counts(g):
    """Tile counts nw i + d around every group boundary of the walk."""
    t, nw = depth(), 4 * g
    out = []
    for i in sorted({0, 1, t - 1, t, t + 1, 2 * t, 2 * t + 1}):
        for d in sorted({0, 1, 3, nw - 1}):
            if nw * i + d > 0:
                out.append(nw * i + d)
    return sorted(set(out))


def test_shapes_take_the_pipelined_kernel():
    # 4+2 from S = 2 KiB on (shorter shards take the packed kernel), and the
    # other instances used below
    for k, r, s in [(4, 2, 2048), (4, 2, 4096), (4, 2, 65536), (4, 1, 4096), (3, 2, 4096), (2, 1, 4096)]:
        assert B.kernel_info(k, r, s)["kind"] == "pipelined", (k, r, s)
    t, _ = B.pipe2_store_depth(4, 2)
    assert 1 <= t <= 16
    assert B.pipe2_store_depth(3, 2)[0] == 1 and B.pipe2_store_depth(4, 1)[0] == 1


# n_tiles = nw i + d exactly where S divides it (always at 1 KiB: one tile per
# object), else the next object count above it: the last row then has blocks
# whose first wave is live and whose others are stand-ins, and blocks that
# return at once.  1 KiB shards take the packed kernel (the route is the
# product's); 2 KiB is the shortest pipelined shard.
@pytest.mark.parametrize("g", [1, 2, 8])
@pytest.mark.parametrize("s", [1024, 2048, 4096, 65536])
def test_trip_counts(g, s):
    B.set_vec_grid_cap(g)
    tpo = s // 1024
    for n in sorted({-(-tiles // tpo) for tiles in trip_counts(g)}):
        encode_case(4, 2, s, n, "split", seed=g * 1000 + n)


# S = 1024 q + 16 p: the masked store in the first, a middle and the last slot
# of a burst (the partial tile is every (q + 1)-th of the walk), with 1, 2 and
# 8 blocks
@pytest.mark.parametrize("g", [1, 2, 8])
@pytest.mark.parametrize("p", [1, 63])
def test_partial_tiles_in_a_group(g, p):
    B.set_vec_grid_cap(g)
    t = depth()
    for q in sorted({1, 2, 3, t}):
        s = 1024 * q + 16 * p
        for n in sorted({1, 3, 4 * g + 1, 4 * g * t // (q + 1) + 2}):
            encode_case(4, 2, s, n, "split", seed=p * 100 + q)


# groups that straddle objects: data and parity pitches differ
@pytest.mark.parametrize("kind", ["split", "databuf", "pitch"])
@pytest.mark.parametrize("g", [1, 2, 8])
def test_groups_straddle_objects(kind, g):
    B.set_vec_grid_cap(g)
    t = depth()
    for s in (2048, 3072, 5120):
        tpo = s // 1024
        for n in sorted({2, 7, -(-4 * g * t // tpo) + 1, -(-4 * g * (2 * t + 1) // tpo) + 1}):
            encode_case(4, 2, s, n, kind, seed=s + n)


# rebuilt shards written into their own slots of the rows the survivors are
# read from: {0, 1} is the 4 x 2 instance, one lost shard the 4 x 1 (depth 1)
@pytest.mark.parametrize("g", [1, 2, 8])
@pytest.mark.parametrize("lost", [[0, 1], [1, 4], [2]])
def test_reconstruct_in_place(g, lost):
    B.set_vec_grid_cap(g)
    t = depth()
    for s in (2048, 4096 + 16 * 5):
        tpo = -(-s // 1024)
        for n in sorted({1, 5, -(-4 * g * (t + 1) // tpo) + 1}):
            reconstruct_case(4, 2, s, n, lost, "databuf", seed=s + n)
            reconstruct_case(4, 2, s, n, lost, "pitch", seed=s + n + 1)


# a batch of a few objects in 2 and in 3 launches (whole objects per launch)
@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("chunk,launches", [(12, 2), (8, 3), (4, 5)])
def test_launch_boundaries(g, chunk, launches):
    B.set_vec_grid_cap(g)
    B.set_vec_chunk_tiles(chunk)
    assert B.vec_launch_config() == (chunk, g)
    s, n = 4096, 5
    assert -(-n // (chunk // (s // 1024))) == launches
    encode_case(4, 2, s, n, "split", seed=chunk)
    encode_case(4, 2, s, n, "databuf", seed=chunk + 1)
    reconstruct_case(4, 2, s, n, [0, 1], "databuf", seed=chunk + 2)
    # launches longer than a group: 17 objects of 9 tiles, 4 objects per launch
    B.set_vec_chunk_tiles(36)
    encode_case(4, 2, 9 * 1024 - 16, 17, "pitch", seed=chunk + 3)


# an instance left at depth 1 walks as it did: 3+2 and 2+1 encode (2 KiB
# tiles at K = 2), 3+2 with two lost shards
@pytest.mark.parametrize("g", [1, 8])
def test_depth_one_instances(g):
    B.set_vec_grid_cap(g)
    for k, m, s in [(3, 2, 4096), (3, 2, 3072 + 16), (2, 1, 4096), (2, 1, 2048 + 32)]:
        for n in (1, 4 * g + 1, 8 * g + 3):
            encode_case(k, m, s, n, "split", seed=k * 10 + n)
            encode_case(k, m, s, n, "databuf", seed=k * 10 + n + 1)
    reconstruct_case(3, 2, 4096, 4 * g + 3, [0, 2], "databuf")
