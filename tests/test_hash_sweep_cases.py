"""What the plan hash sweep's inputs cover (tests/hash_sweep_cases.py), asserted
from the schedule model alone, for every plan kind and shape, before any GPU
sees them: no GPU."""
import itertools

import pytest

import hash_sweep_cases as M

KS = [(kind, k, m) for kind in M.KINDS for k, m in M.SHAPES]
IDS = [f"{kind}-{k}+{m}" for kind, k, m in KS]
D, SLOTS, LONG = M.D, M.SLOTS, M.LONG


def scheds(call, kind, examined_only=False):
    for r, j in call.chains():
        if not examined_only or call.examined(r):
            yield r, j, call.sched(kind, r, j)


# ---- the model itself, on chains worked out by hand ---------------------------------------
def test_schedule_of_hand_made_chains():
    s = M.Sched([(3, 70), (100, 60)])
    assert (s.total, s.nb, s.rv) == (130, 2, 2)
    assert s.blocks == [("in", 3, 0), ("cut", 2, 6, 60)] and s.tail_span == 1 and s.first_cut() == 1
    s = M.Sched([(0, 64), (5, 64), (18, 3)])
    assert s.blocks == [("in", 0, 0), ("in", 1, 1)] and (s.rv, s.tail_span) == (3, 1) and s.first_cut() is None
    s = M.Sched([(2, 1)] * 64)
    assert s.blocks == [("cut", 64, 1, 1)] and (s.rv, s.tail_span) == (0, 0)
    s = M.Sched([(0, 100), (7, 20), (1, 9), (6, 130)])     # 259 bytes
    assert s.blocks[0] == ("in", 0, 0) and s.blocks[1] == ("cut", 3, 36, 20)   # bytes 64..127: 36 + 20 + 8
    assert s.blocks[2] == ("cut", 2, 1, 130) and s.blocks[3] == ("in", (6 + 192 - 129) & 3, 3)
    assert (s.nb, s.rv, s.tail_span) == (4, 3, 1)
    s = M.Sched([(0, 60), (0, 2), (0, 1)])
    assert (s.nb, s.rv, s.tail_span, s.blocks) == (0, 63, 3, [])
    s = M.Sched([(0, 64), (0, 50), (0, 7)])
    assert (s.nb, s.rv, s.tail_span) == (1, 57, 2)
    assert [s.state(i) for i in range(3)] == ["in", "past", "past"]
    assert [M.slot_trip(i) for i in (0, SLOTS - 1, SLOTS, 2 * SLOTS + 1, 5 * SLOTS)] == \
        [(0, 0), (SLOTS - 1, 0), (0, 1), (1, 2), (0, 2)]


def test_wave_composition_and_counters_of_hand_made_calls():
    # the layouts of the counter tests of test_gpu_hash_plan.py and test_gpu_hash_files.py
    c = M.Call("x", 4, 2, [5, 0, 70, 200, 0, 64])
    assert [r for r, j in c.chains() if j == 0] == [3, 2, 5, 0] and c.stats()[0] == 4 * 6
    assert c.chains()[:7] == [(3, j) for j in range(6)] + [(2, 0)]
    sel = [[0] * 6 for _ in range(6)]
    sel[0][2] = sel[1][3] = sel[3][0] = sel[3][5] = 1
    assert M.Call("x", 4, 2, [5, 0, 70, 200, 0, 64], select=sel).chains() == [(3, 0), (3, 5), (0, 2)]
    objs = [[5, 0, 70], [0], [200, 64], [], [0, 0]]
    f = M.Call("x", 4, 2, objs=objs)
    assert f.starts == [0, 3, 4, 6, 6, 8] and f.stats() == (2 * 6, 4 * 6)
    assert [r for r, j in f.chains() if j == 0] == [2, 0]
    sel = [[0] * 6 for _ in range(5)]
    sel[0][2] = sel[1][3] = sel[2][0] = sel[2][5] = 1
    assert M.Call("x", 4, 2, objs=objs, select=sel).stats() == (3, 6)
    # equal totals keep their order; 64 chains to a wave
    c = M.Call("x", 4, 2, [9, 9, 10, 9] * 6)
    assert [r for r, j in c.chains() if j == 0][:7] == [2, 6, 10, 14, 18, 22, 0]
    assert [len(w) for w in c.waves()] == [64, 64, 16]
    # the filter examines an object through any of its entries, a zero-length one too
    f = M.Call("x", 4, 2, objs=[[3, 0, 4], [5, 6]], flt=[0, 2, 0, 4, 4], fbits=3)
    assert f.examined(0) and not f.examined(1) and [f.passes(e) for e in range(5)] == [False, True, False] + [False] * 2


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_placements_follow_the_kind(kind, k, m):
    n = k + m
    for call in (M.f3_call(k, m), M.p2_calls(k, m)[LONG - 1], M.f2_call(k, m)):
        at, lens = call.place(kind)
        assert len(lens) == {"stripes": 1, "objects": 2, "shards": 3}[kind]
        spans = []
        for e, s in enumerate(call.sizes):
            if not s:
                assert at[e] is None            # a row of zeros in the plan
                continue
            assert len(at[e]) == n
            for j, (b, o) in enumerate(at[e]):
                spans.append((b, o, o + s))
                assert o >= 16 and o + s + 16 <= lens[b]
            r = call.res[e]
            if kind == "stripes":
                assert at[e][0][1] % 16 == r and [(b, o - at[e][0][1]) for b, o in at[e]] == [(0, j * s) for j in range(n)]
            elif kind == "objects":
                assert at[e][0][1] % 16 == r and at[e][k][1] % 16 == (r + 8) % 16
                assert [(b, o - at[e][0][1]) for b, o in at[e][:k]] == [(0, j * s) for j in range(k)]
                assert [(b, o - at[e][k][1]) for b, o in at[e][k:]] == [(1, j * s) for j in range(m)]
            else:
                assert [o % 16 for _, o in at[e]] == [(r + 5 * j) % 16 for j in range(n)]
        spans.sort()
        gap = 1 if kind == "shards" else 0      # slack around every shard of a shards plan
        assert all(x[0] != y[0] or y[1] - x[2] >= gap for x, y in zip(spans, spans[1:]))
        if kind == "shards":
            assert len({b for b, _, _ in spans}) == 3
            flat = sorted((b, o, e) for e, s in enumerate(call.sizes) if s for b, o in at[e])
            assert sum(1 for x, y in zip(flat, flat[1:]) if x[2] != y[2]) > 2 * len(call.sizes)  # interleaved


# ---- P. md5_plan --------------------------------------------------------------------------
@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_p1_every_length_at_every_start_residue(kind, k, m):
    call = M.p1_call(k, m)
    assert M.P_MAX == 64 * (4 * D + 2) + 63
    want = set(itertools.product(range(1, M.P_MAX + 1), range(16)))
    at, _ = call.place(kind)
    data, par = set(), set()
    for r, j in call.chains():
        (data if j < k else par).add((call.sizes[r], at[r][j][1] % 16))
    if kind == "objects":
        assert data == want and par == want      # both address rules
    else:
        assert data | par == want
    assert call.sizes.count(0) == 16 and 0 < call.sizes.index(0, 1) < len(call.sizes) - 1   # length 0, sixteen times
    assert call.stats()[0] == (16 * M.P_MAX + M.P1_EXTRA) * (k + m)
    assert call.select is None and call.flt is None
    # every step of the block count falls inside a wave, so lanes end at different blocks of a group
    mixed = set()
    for w in call.waves():
        nbs = {call.sizes[r] // 64 for r, _ in w}
        mixed |= {q for q in nbs if q - 1 in nbs}
    assert mixed == set(range(1, M.P_MAX // 64 + 1))


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_p2_what_one_wave_mixes(kind, k, m):
    calls = {c.name: c for c in M.p2_calls(k, m)}
    for nb_max in range(1, LONG + 1):
        c = calls[f"P2.nb_max{nb_max}"]
        (wave,) = c.waves()
        assert len(wave) <= 64 and len(wave) % 64
        lanes = [(c.examined(r), c.sched(kind, r, j)) for r, j in wave]
        assert {s.nb for ex, s in lanes if ex} == set(range(nb_max + 1))
        assert {s.rv for ex, s in lanes if ex} >= set(M.TAILS)
        ex = [e for e, _ in lanes]
        assert any(not ex[i] and any(ex[:i]) and any(ex[i + 1:]) for i in range(len(ex)))
        assert len({j for _, j in wave}) == k + m    # every shard index, data and parity rule
    assert len(calls["P2.full_wave"].chains()) == 64
    c = calls["P2.nothing_examined"]
    assert len(c.waves()) == 1 and not any(c.examined(r) for r, _ in c.chains())
    c = calls["P2.dead_wave"]
    w = c.waves()
    assert [len(x) for x in w] == [64, 40]
    assert not any(c.examined(r) for r, _ in w[0]) and all(c.examined(r) for r, _ in w[1])
    assert any(0 in c.sizes for c in calls.values())     # a zero-length entry among them


# ---- F. md5_files -------------------------------------------------------------------------
def test_pieces_are_short_and_objects_small():
    for k, m in M.SHAPES:
        for c in (M.f1_call(k, m), M.f2_call(k, m), M.f4_call(k, m)) + tuple(M.f5_calls(k, m)):
            assert max(c.sizes) <= 64 * (4 * D + 2) + 64 * D and all(len(o) <= 7 for o in c.objs), c.name
        assert max(M.f3_call(k, m).sizes) <= 64 * (4 * D + 2)


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_f1_a_cut_in_every_slot_trip_and_offset(kind, k, m):
    call = M.f1_call(k, m)
    got = set()
    for _, _, s in scheds(call, kind):
        for i, b in enumerate(s.blocks):
            if b[0] == "cut" and b[1] == 2 and b[3] >= 64 * (2 * D + 1):
                got.add(M.slot_trip(i) + (b[2],))
    assert got == set(itertools.product(range(SLOTS), (0, 1, 2), range(1, 64)))


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_f2_every_pair_of_shifts_across_a_boundary(kind, k, m):
    call = M.f2_call(k, m)
    cut, edge = set(), set()
    for _, _, s in scheds(call, kind):
        for i in range(1, s.nb):
            a, b = s.blocks[i - 1], s.blocks[i]
            if a[0] == "in" and b[0] == "in" and a[2] != b[2]:
                edge.add((a[1], b[1]))
            if a[0] == "in" and b[0] == "cut" and i + 1 < s.nb and s.blocks[i + 1][0] == "in":
                cut.add((a[1], s.blocks[i + 1][1]))
    assert cut == M.shift_pairs() and edge == M.shift_pairs()


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_f3_spans_zero_length_entries_and_runs(kind, k, m):
    call = M.f3_call(k, m)
    spans, run = set(), 0
    for r, _, s in scheds(call, kind):
        spans |= {b[1] for b in s.blocks if b[0] == "cut"}
        if max(call.objs[r]) < 64 and all(b[0] == "cut" for b in s.blocks):
            run = max(run, s.nb)
    assert spans >= set(range(2, 9)) | {64} and run >= LONG
    assert [1] * 64 in call.objs
    inside = first = last = False
    for o in call.objs:
        pos = 0
        for i, x in enumerate(o):
            if x == 0 and pos % 64 and pos // 64 < sum(o) // 64 and sum(o[i:]) >= 64 - pos % 64:
                inside = True    # a zero-length entry between two bytes of one whole block
            pos += x
        first = first or (len(o) > 1 and o[0] == 0 and sum(o) > 0)
        last = last or (len(o) > 1 and o[-1] == 0 and sum(o) > 0)
    assert inside and first and last
    assert [] in call.objs and [0] in call.objs and [0, 0, 0] in call.objs   # objects without a byte: no chain
    assert len(call.chains()) == (k + m) * sum(1 for o in call.objs if sum(o))


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_f4_every_tail_over_every_span_behind_both_kinds_of_block(kind, k, m):
    call = M.f4_call(k, m)
    got, short_parts = set(), set()
    for r, _, s in scheds(call, kind):
        got.add((s.rv, min(s.tail_span, 3), s.blocks[-1][0] if s.nb else "none"))
        if s.nb == 0:
            short_parts.add(len(call.objs[r]))
    want = M.f4_expected()
    assert len(want) == 2 + 3 * (1 + 2 + 3 * 61) and got == want
    assert all((rv, 2, last) in got and (rv, 3, last) in got for rv in (55, 56, 57) for last in ("in", "cut", "none"))
    assert short_parts == {1, 2, 3, 4, 5}
    assert {s.tail_span for _, _, s in scheds(call, kind)} >= {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_f5_waves(kind, k, m):
    calls = {c.name: c for c in M.f5_calls(k, m)}

    def lanes(c):
        (wave,) = c.waves()
        return [(c.examined(r), c.sched(kind, r, j)) for r, j in wave]

    ln = lanes(calls["F5.mixed_at_a_block"])
    assert any({s.state(i) for _, s in ln} == {"cut", "in", "past"} for i in range(8))
    ln = lanes(calls["F5.one_cut_lane"])
    assert sum(1 for _, s in ln if s.first_cut() is not None) == 1 and len(ln) > 30
    ln = lanes(calls["F5.short_among_long"])
    assert any(s.nb == 0 for _, s in ln) and any(s.nb >= LONG for _, s in ln)
    assert {s.nb for _, s in ln} <= {0} | set(range(LONG, 99))
    c = calls["F5.filtered"]
    ex = [e for e, _ in lanes(c)]
    assert any(not ex[i] and any(ex[:i]) and any(ex[i + 1:]) for i in range(len(ex)))
    single = [g for g in range(len(c.objs)) if len(c.objs[g]) >= 3 and
              sum(1 for e in c.entries_of(g) if c.passes(e)) == 1]
    assert any(all(c.sizes[e] for e in c.entries_of(g)) for g in single)          # one passing entry among several
    assert any(c.sizes[e] == 0 for g in single for e in c.entries_of(g) if c.passes(e))  # and a zero-length one
    w = calls["F5.partial_wave"].waves()
    assert len(w) >= 2 and len(w[-1]) < 64 and all(len(x) == 64 for x in w[:-1])
    for c in calls.values():
        n_ch, n_seg = c.stats()
        assert n_seg == sum(len(c.segs(kind, r, j)) for r, j in c.chains()) and n_ch == len(c.chains())


@pytest.mark.parametrize("k,m", M.SHAPES, ids=["4+2", "8+3"])
def test_f6_files_of_three_to_five_stripes_with_a_short_last_one(k, m):
    assert M.ec_stripes(10000, 4, 1024) == [1024, 1024, 452]          # the committed ShardHash object's cut
    assert M.ec_stripes(7, 3, 100) == [3] and M.ec_stripes(0, 4, 5) == [] and M.ec_stripes(40, 4, 5) == [5, 5]
    assert list(M.F6_CHUNKS) == list(range(1, 201))
    cut_offsets = set()
    for chunk in M.F6_CHUNKS:
        lengths, cuts, offs, size = M.f6_layout(k, m, chunk)
        assert [len(c) for c in cuts] == [3, 4, 5]
        for c in cuts:
            assert c[:-1] == [chunk] * (len(c) - 1) and 1 <= c[-1] <= max(1, chunk - 1)
        flat = sorted((o, o + sum(cuts[g])) for g, row in enumerate(offs) for o in row)
        assert all(b[0] - a[1] >= 1 for a, b in zip(flat, flat[1:])) and flat[0][0] >= 16 and flat[-1][1] + 16 <= size
        for g, row in enumerate(offs):
            assert len({o % 16 for o in row}) >= min(k + m, 8)           # residues differ within an object
            # stripe t of file j lies at the file's start + t chunk: the segments are contiguous
            s = M.Sched([(row[0] + t * chunk, n) for t, n in enumerate(cuts[g])])
            assert s.total == sum(cuts[g])
            cut_offsets |= {b[2] for b in s.blocks if b[0] == "cut"}
    assert cut_offsets == set(range(1, 64))


# ---- L. the bit count's upper word ----------------------------------------------------------
def test_l_crosses_32_bits_of_bit_count():
    assert M.L_TOTAL == (512 << 20) + 1 and (M.L_TOTAL * 8) >> 32 == 1
    assert M.L_OFFSETS == (0, 16, 5, 32, 48, 1, 64, 33) and M.L_PIECE == 64 << 20
    assert {o & 3 for o in M.L_OFFSETS} == {0, 1} and M.L2_BASE & 3
    assert max(M.L_OFFSETS) + 2 * M.L_PIECE <= M.L_BUFFER < 131 << 20
    # the nine pieces as a chain: every block inside, the shift changing on block edges, one tail byte
    total = len(M.L_OFFSETS) * M.L_PIECE + 1
    assert total == M.L_TOTAL and total // 64 == 8 << 20 and total % 64 == 1
