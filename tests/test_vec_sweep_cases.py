"""What the aligned apply sweep's cases cover (tests/vec_sweep_cases.py),
asserted on the cases themselves before any GPU sees them, and the argument
handling of hbec_vec_kernel_stats and of the launch hooks: no GPU."""
import ctypes as C

import pytest

import vec_sweep_cases as V
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B

BY_KERNEL = {k: [i for i in V.INSTANCES if i.kernel == k] for k in V.KERNELS}
IDS = [i.name for i in V.INSTANCES]


@pytest.fixture(autouse=True)
def _restore():
    yield
    B.set_vec_chunk_tiles(0)
    B.set_vec_grid_cap(0)


def test_kernel_stats_entry_point_answers_without_a_device():
    L = N.lib()
    v = [C.c_uint64(1 << 40) for _ in range(5)]
    assert L.hbec_vec_kernel_stats(None, None, None, None, None) == 0
    for i in range(5):
        args = [None] * 5
        args[i] = C.byref(v[i])
        assert L.hbec_vec_kernel_stats(*args) == 0
    s = B.vec_kernel_stats()
    assert list(s) == list(V.KERNELS) == ["packed", "pipe2", "pipe", "vec", "stream"]
    assert [x.value for x in v] == list(s.values())  # nothing was coded in between


def test_hooks_round_trip_through_vec_launch_config():
    tiles0, cap0 = B.vec_launch_config()
    assert tiles0 > 0 and cap0 == 0
    for tiles, cap in ((4, 1), (22, 1), (1 << 31, 7)):
        B.set_vec_chunk_tiles(tiles)
        B.set_vec_grid_cap(cap)
        assert B.vec_launch_config() == (tiles, cap)
    B.set_vec_chunk_tiles(0)
    B.set_vec_grid_cap(0)
    assert B.vec_launch_config() == (tiles0, 0)


def test_the_table_of_instances():
    n = {k: len(v) for k, v in BY_KERNEL.items()}
    assert n == {"packed": 24, "pipe2": 12, "pipe": 12, "vec": 24, "stream": 3 + 12 + 4 + 2 + 2}
    assert len(set(IDS)) == len(IDS) == 95
    assert {(i.K, i.R) for i in BY_KERNEL["packed"]} == {(k, r) for k in range(1, 9) for r in (1, 2, 3)}
    assert {(i.K, i.R) for i in BY_KERNEL["pipe2"]} == {(k, r) for k in range(1, 5) for r in (1, 2, 3)}
    assert {(i.K, i.R) for i in BY_KERNEL["pipe"]} == {(k, r) for k in range(5, 9) for r in (1, 2, 3)}
    assert {(i.K, i.R, i.cols) for i in BY_KERNEL["vec"]} == {(k, r, 16 + k) for k in range(1, 9) for r in (1, 2, 3)}
    st = {(i.rows, i.cols, i.force) for i in BY_KERNEL["stream"]}
    assert st == ({(4, k, False) for k in (1, 4, 8)} | {(r, k, False) for k in (9, 13, 16) for r in (1, 2, 3, 4)}
                  | {(r, c, False) for c in (25, 32) for r in (2, 4)} | {(5, 4, False), (7, 4, False)}
                  | {(2, 4, True), (3, 8, True)})
    assert {i.R for i in BY_KERNEL["stream"]} == {1, 2, 3, 4}  # every gf_apply_vec_stream<R>


def test_tiles_and_limits_are_the_kernels():
    assert [V.pipe_u(k) for k in range(1, 9)] == [4, 2, 1, 1, 3, 3, 3, 3]
    assert [V.tile_kib(k) for k in range(1, 9)] == [4, 4, 1, 1, 1, 1, 1, 1]
    assert [V.packed_limit(k) for k in range(1, 9)] == [4096, 2048, 2048, 2048] + [V.PACKED_MAX_BIG] * 4
    assert V.PACKED_MAX_BIG == 32784 and V.WAVES == 4
    assert [V.packed_tile_elems(k) for k in range(1, 9)] == [256, 128, 64, 64, 64, 64, 64, 64]
    assert {V.tile_bytes(i) for i in BY_KERNEL["stream"]} == {4096}
    assert {(i.K, V.tile_bytes(i)) for i in BY_KERNEL["pipe2"]} == {(1, 4096), (2, 2048), (3, 1024), (4, 1024)}
    assert {V.tile_bytes(i) for i in BY_KERNEL["pipe"]} == {3072}


def test_the_rule_at_its_edges():
    K = V.pass_kernel
    assert K(1, 1, 4080, False)[0] == "packed" and K(1, 1, 4096, False) == ("pipe2", 4096)
    assert K(4, 2, 2032, False)[0] == "packed" and K(4, 2, 2048, False) == ("pipe2", 1024)
    assert K(8, 3, 32768, False)[0] == "packed" and K(8, 3, 32784, False) == ("pipe", 3072)
    assert K(8, 3, 512, True) == ("vec", 1024) and K(2, 1, 65536, True) == ("vec", 4096)
    assert K(8, 4, 512, False) == ("stream", 4096) and K(9, 1, 16, False)[0] == "stream"
    assert K(4, 2, 512, False, True)[0] == "stream" and K(9, 2, 512, True)[0] == "stream"
    assert [p[:4] for p in V.passes(7, 20, 4096)] == [("stream", 16, 4, False), ("stream", 4, 4, True),
                                                       ("stream", 16, 3, False), ("vec", 4, 3, True)]
    assert V.launches(5, 4, 1024) == {"packed": 1, "pipe2": 0, "pipe": 0, "vec": 0, "stream": 1}
    assert V.launches(5, 4, 2048) == {"packed": 0, "pipe2": 1, "pipe": 0, "vec": 0, "stream": 1}


@pytest.mark.parametrize("inst", V.INSTANCES, ids=IDS)
def test_every_case_runs_the_kernel_the_table_names(inst):
    for c in V.cases(inst):
        assert c.S % 16 == 0 and c.S >= 16 and c.n >= 2
        assert V.below_records(inst.cols, c.S), c
        ps = V.passes(inst.rows, inst.cols, c.S, inst.force)
        if inst.kernel in ("packed", "pipe2", "pipe"):
            assert [p[:4] for p in ps] == [(inst.kernel, inst.K, inst.R, False)], c
        elif inst.kernel == "vec":
            assert [p[:4] for p in ps] == [("stream", 16, inst.R, False), ("vec", inst.K, inst.R, True)], c
        elif inst.name.startswith("stream-acc"):
            assert [p[:4] for p in ps] == [("stream", 16, inst.R, False), ("stream", inst.K, inst.R, True)], c
        elif inst.name.startswith("stream-rows"):
            # the rows past the fourth are a pass of their own, packed below 2 KiB and pipelined from there
            second = "packed" if c.S < 2048 else "pipe2"
            assert [p[:4] for p in ps] == [("stream", 4, 4, False), (second, 4, inst.rows - 4, False)], c
        else:
            assert [p[:4] for p in ps] == [("stream", inst.K, inst.R, False)], c
        named = [p for p in ps if p[:3] == (inst.kernel, inst.K, inst.R)]
        assert named and all(p[4] == V.tile_bytes(inst) for p in named)
        assert sum(V.launches(inst.rows, inst.cols, c.S, inst.force).values()) == len(ps)


@pytest.mark.parametrize("inst", V.INSTANCES, ids=IDS)
def test_lengths_walk_every_residue_and_tile_count(inst):
    T, ls = V.tile_bytes(inst), V.lengths(inst)
    assert list(ls) == sorted(set(ls))
    if inst.kernel == "packed":
        lim = V.packed_limit(inst.K)
        assert ls[0] == 16 and ls[-1] == (lim - 1) // 16 * 16
        if inst.K <= 4:
            assert list(ls) == list(range(16, lim, 16))
        else:
            assert set(range(16, 4401, 16)) <= set(ls) and {32736, 32752, 32768} <= set(ls)
            for q in range(5, 33):
                assert {q * 1024 - 16, q * 1024} <= set(ls) and (q * 1024 + 16 in ls) == (q < 32)
        # every residue a packed shard can have: 0 only where a whole tile is still below the limit
        assert {s % T for s in ls} == set(range(16, T, 16)) | ({0} if lim > T else set())
        return
    lo = {"pipe2": V.packed_limit(inst.K), "pipe": 32784}.get(inst.kernel, 16)
    span = (T if inst.kernel == "pipe" else 2 * T) + 368
    assert list(ls) == list(range(lo, lo + span + 1, 16))
    assert {s % T for s in ls} == set(range(0, T, 16))
    tpo = sorted({-(-s // T) for s in ls})
    # tiles per object: 1, 2 and 3; the pipelined kernels start where the packed one ends, which
    # is two tiles for gf_apply_vec_pipe2<3..4> and eleven for gf_apply_vec_pipe (11 and 12)
    first = 11 if inst.kernel == "pipe" else (2 if inst.kernel == "pipe2" and inst.K >= 3 else 1)
    assert -(-lo // T) == first
    assert tpo == [11, 12] if inst.kernel == "pipe" else tpo[:3] == [first, first + 1, first + 2]
    # a full and a partial last tile at the first counts
    for t in tpo[:1 if inst.kernel == "pipe" else 2]:
        assert any(-(-s // T) == t and s % T == 0 for s in ls)
    for t in tpo[(1 if lo % T == 0 else 0):][:2]:   # the pipelined kernels' first length is whole tiles
        assert any(-(-s // T) == t and s % T for s in ls)


@pytest.mark.parametrize("inst", V.INSTANCES, ids=IDS)
def test_object_counts_and_rows_of_tiles(inst):
    cs, ls = V.cases(inst), V.lengths(inst)
    capped, free = [c for c in cs if c.cap == 1], [c for c in cs if c.cap == 0]
    assert len(capped) + len(free) == len(cs) and cs[:len(capped)] == tuple(capped)
    assert [c.S for c in free] == list(ls) and {c.n for c in free} == {2}
    extra = 2 if inst.kernel == "packed" else 0
    assert [c.S for c in capped[:len(ls)]] == list(ls) and len(capped) == len(ls) + extra
    for i, c in enumerate(capped[:len(ls)]):
        assert c.n == (2 + i % 2 if inst.kernel == "pipe" else 3 + i % 4) and c.split == (i % 3 == 2)
    assert [c.split for c in free] == [i % 3 == 2 for i in range(len(ls))]
    # one block of 4 waves: a last row of 1, 2, 3 tiles (the other waves past the end) and a full one.
    # gf_apply_vec_pipe's 11 and 12 tiles per object times 2 and 3 objects give 22, 33, 24 and 36
    # tiles: no rest of 3.  Its waves past the end leave the loop (there is no stand-in tile in that
    # kernel), and rests 1 and 2 are a last row with such waves.
    rests = {V.n_tiles(inst, c) % V.WAVES for c in capped}
    assert rests == ({0, 1, 2} if inst.kernel == "pipe" else {0, 1, 2, 3})
    # more than one row of tiles per wave, and a single one
    rows = {-(-V.n_tiles(inst, c) // V.WAVES) for c in capped}
    assert 1 in rows or inst.kernel in ("pipe", "pipe2")
    assert max(rows) >= 3


@pytest.mark.parametrize("inst", BY_KERNEL["packed"], ids=[i.name for i in BY_KERNEL["packed"]])
def test_packed_tiles_across_objects(inst):
    te = V.packed_tile_elems(inst.K)
    cs = V.cases(inst)
    spos = {c.S // 16 for c in cs}
    assert min(spos) == 1 and 64 in spos and {63, 65} <= spos and max(spos) >= 127
    ne = [c.n * (c.S // 16) for c in cs]
    assert any(x % te == 0 for x in ne) and any(x % te for x in ne)
    # the two long walks, one block
    a, b = [c for c in cs if c.cap == 1][-2:]
    assert (a.S, b.S) == (48, 1280) and a.cap == b.cap == 1
    assert 9 * te < a.n * 3 <= 9 * te + 3 and V.n_tiles(inst, a) == 10
    assert b.n * 80 == 5 * te and V.n_tiles(inst, b) == 5
    straddle = crowded = False
    for c in cs:
        spo = c.S // 16
        first = [o * spo // te for o in range(c.n)]
        last = [((o + 1) * spo - 1) // te for o in range(c.n)]
        straddle |= any(f != l for f, l in zip(first, last))
        for t in range(-(-c.n * spo // te)):
            crowded |= sum(f <= t <= l for f, l in zip(first, last)) > 3
    assert straddle and crowded


@pytest.mark.parametrize("inst", V.INSTANCES, ids=IDS)
def test_coefficients(inst):
    m = V.coeffs(inst)
    assert len(m) == inst.rows and all(len(r) == inst.cols for r in m)
    flat = [x for r in m for x in r]
    assert all(0 <= x <= 255 for x in flat)
    assert (1 in flat) == (len(flat) >= 2) and (0 in flat) == (len(flat) >= 3)
    assert len(set(m)) == inst.rows
    assert m == V.coeffs(inst)  # seeded


@pytest.mark.parametrize("inst", V.INSTANCES, ids=IDS)
def test_layout(inst):
    regs, size = V.layout(inst)
    assert [r.case for r in regs] == list(V.cases(inst)) and size < 1 << 30
    pos = 0
    for r in regs:
        c = r.case
        assert pos + V.CANARY <= r.begin < pos + V.CANARY + 128 and r.begin % 16 == 0
        spans = []
        views = r.in_views + r.out_views
        assert len(r.in_views) == inst.cols and len(r.out_views) == inst.rows
        for off, stride in views:
            assert off % 16 == 0 and stride % 16 == 0
            spans += [(off + o * stride, off + o * stride + c.S) for o in range(min(c.n, 8))]
            assert r.begin <= off and off + (c.n - 1) * stride + c.S <= r.end
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))   # no two shards overlap
        if c.split:
            assert len({s for _, s in r.in_views}) == 1 and len({s for _, s in r.out_views}) == 1
            assert r.in_views[0][1] != r.out_views[0][1]
            assert r.out_views[0][0] == r.in_views[0][0] + c.n * r.in_views[0][1] + V.CANARY
        else:
            assert len({s for _, s in views}) == 1 and views[0][1] == (inst.cols + inst.rows) * c.S + V.ROW_PAD
        assert [v[0] for v in r.in_views] == [r.in_views[0][0] + j * c.S for j in range(inst.cols)]
        assert [v[0] for v in r.out_views] == [r.out_views[0][0] + j * c.S for j in range(inst.rows)]
        pos = r.end
    assert size == pos + V.CANARY
    # from a 128-B-aligned buffer the regions' bases walk every 16-B residue of a line
    assert {r.begin % 128 for r in regs} == set(range(0, 128, 16))
    assert {r.out_views[0][0] % 128 for r in regs} == set(range(0, 128, 16))


def test_cut_launches():
    assert [c[0] for c in V.CUTS] == ["packed", "packed", "pipe", "pipe"]
    for kern, K, R, S, chunk, n, want in V.CUTS:
        assert V.passes(R, K, S) == [(kern, K, R, False, V.pass_kernel(K, R, S, False)[1])]
        assert V.cut_launches(kern, K, S, chunk, n) == want and want in (2, 3)
        assert V.below_records(K, S)
    assert {c[6] for c in V.CUTS if c[0] == "packed"} == {c[6] for c in V.CUTS if c[0] == "pipe"} == {2, 3}
