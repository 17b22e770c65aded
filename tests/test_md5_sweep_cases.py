"""What the MD5 chain sweep's inputs cover (tests/md5_sweep_cases.py), asserted
on the cases themselves before any GPU sees them, and the counter entry point's
argument handling: no GPU."""
import ctypes as C

import md5_sweep_cases as M
from hummingbird_amd import _native as N
from hummingbird_amd import shardhash as H


def test_route_stats_entry_point_answers_without_a_device():
    L = N.lib()
    v = [C.c_uint64(1 << 40) for _ in range(4)]
    assert L.hbec_md5_route_stats(None, None, None, None) == 0
    for i in range(4):
        args = [None] * 4
        args[i] = C.byref(v[i])
        assert L.hbec_md5_route_stats(*args) == 0
    s = H.md5_route_stats()
    assert list(s) == ["chains_aligned", "chains_unaligned", "list_aligned", "list_unaligned"]
    assert [x.value for x in v] == list(s.values())  # nothing was hashed in between


def test_expect_aligned_is_md5_steps_rule():
    assert M.expect_aligned([0, 16], [32, 0], 0)
    assert not M.expect_aligned([0, 1], [32, 32], 0)
    assert not M.expect_aligned([0, 16], [32, 8], 0)
    assert not M.expect_aligned([0], [16], 5)        # aligned base, 59 bytes to the first whole block
    assert M.expect_aligned([5], [16], 5)            # odd base, realigned by the carried tail
    assert M.expect_aligned([0], [16], 64 + 48) and M.expect_aligned([0], [16], 128)
    assert M.expect_aligned([0, 0], [0, 0], 16) and not M.expect_aligned([0, 0], [0, 0], 17)  # final()


def test_lengths_cover_every_block_count_rest_and_loop_phase():
    seen = {M.blocks_rest(n) for n in M.LENGTHS}
    assert {b for b, _ in seen} == set(range(15))
    for b in range(14):
        assert {r for x, r in seen if x == b} == set(range(64))
    # the ping-pong loops repeat every 4 blocks (D = 2) and every 2 (D = 1): each phase at least twice
    for d in (1, 2):
        for phase in range(2 * d):
            assert len({b for b, _ in seen if b and b % (2 * d) == phase}) >= 2
    assert any(r >= 56 for _, r in seen) and any(r == 55 for _, r in seen)


def test_a_one_misaligned_view_and_every_residue_in_every_view():
    assert M.A_STRIDE % 16 == 1 and M.A_STRIDE >= M.LENGTHS[-1] and len(M.A_BASES) == 16
    assert [b % 16 for b in M.A_BASES] == list(range(16))
    for b in M.A_BASES:
        assert {(b + o * M.A_STRIDE) % 16 for o in range(M.A_NOBJ)} == set(range(16))
    assert M.A_NOBJ == 65
    assert not M.expect_aligned(M.A_BASES, [M.A_STRIDE] * 16, 0)
    starts = {b + o * M.A_STRIDE for b in M.A_BASES for o in range(M.A_NOBJ)}
    assert len(starts) == 16 * M.A_NOBJ and max(starts) + M.LENGTHS[-1] <= M.A_POOL


def test_b_aligned_views_and_object_counts():
    assert [b % 64 for b in M.B_BASES] == [0, 16, 48]
    assert M.B_STRIDE % 16 == 0 and M.B_STRIDE % 64 != 0 and M.B_STRIDE >= M.LENGTHS[-1]
    assert M.expect_aligned(M.B_BASES, [M.B_STRIDE] * 3, 0)
    assert M.B_NOBJS == (1, 63, 64, 65, 129)
    for n in M.B_NOBJS:
        seen = {M.blocks_rest(x) for x in M.LENGTHS if M.b_nobj(x) == n}
        assert {b for b, _ in seen} == set(range(15)) and {r for _, r in seen} == set(range(64)), n
    assert {(b + o * M.B_STRIDE) % 64 for b in M.B_BASES for o in range(129)} == {0, 16, 32, 48}
    assert M.B_BASES[-1] + 128 * M.B_STRIDE + M.LENGTHS[-1] <= M.B_POOL
    assert len({b + o * M.B_STRIDE for b in M.B_BASES for o in range(129)}) == 3 * 129


def test_c_split_shapes_and_the_kernels_of_the_streaming_steps():
    assert M.C_NVIEWS == (32, 33, 64, 65) and M.C_NOBJS == (1, 65)
    assert M.C_LENGTHS == (0, 55, 56, 64, 200) and M.C_UPDATES == (37, 100, 0, 64)
    assert [M.launches(n) for n in M.C_NVIEWS] == [1, 2, 2, 3]
    assert sum(M.C_UPDATES) <= M.C_PITCH and max(M.C_LENGTHS) <= M.C_PITCH
    for n in M.C_NVIEWS:
        offs, stride = M.c_layout(n)
        assert M.expect_aligned(offs, [stride] * n, 0)
        steps = M.c_stream_steps(n)
        # a chain's bytes are contiguous from a multiple of 16, so the first whole block of every
        # update is at a multiple of 64 from it: aligned at any carry; the zero-length update
        # launches nothing; final() has no views and 9 bytes carried: bytewise
        assert [(s[2], s[3]) for s in steps] == [(M.launches(n), True), (M.launches(n), True), (0, True),
                                                 (M.launches(n), True), (M.launches(n), False)]


def test_d_every_carry_and_length_pair_in_every_class():
    chains = M.pair_chains()
    assert all(1 <= len(c) <= M.D_MAX_UPDATES for c in chains)
    want = M.all_pairs()
    assert len(want) == 64 * 321 - sum(range(64))
    seen = {p for c in chains for p in M.chain_pairs(c)}
    assert want <= seen and all(t <= M.D_TMAX for _, t in seen)
    # the pair is realised in the launch itself: per class, the step at that carry with that length
    for cls in M.D_CLASSES:
        got = {(tot & 63, (tot & 63) + u) for _, ui, u, tot, _, _, _ in M.d_steps(cls, chains) if ui is not None}
        assert want <= got, cls
    assert len(chains) < 3200


def test_d_triples_and_edge_chains():
    tr = M.triple_chains()
    assert set(tr) == M.all_triples() and len(tr) == 1830 + 1891 + 1953 + 2016
    assert all(min(t) >= 1 and sum(t) in (62, 63, 64, 65) for t in tr)
    # all but the 63 (c, 64 - c, 1) carry the tail twice without a block between
    assert [t for t in tr if t[0] + t[1] >= 64] == [(c, 64 - c, 1) for c in range(1, 64)]
    e = M.EDGE_CHAINS
    assert () in e[1:]                                     # final() with no update, on a used context too
    assert any(c and c[0] == 0 and len(c) > 1 for c in e)  # zero-length first update
    assert any(0 in c[1:-1] for c in e if len(c) > 2)      # zero-length update mid-chain
    assert (0,) in e


def test_d_placements_and_the_four_kernel_and_carry_combinations():
    combos = {}
    for cls in M.D_CLASSES:
        steps = M.d_steps(cls, M.EDGE_CHAINS + M.triple_chains()[:200])
        for _, ui, u, tot, offs, n, al in steps:
            if ui is None:
                continue
            c = tot & 63
            assert all(o + (M.D_NOBJ - 1) * M.D_STRIDE + u <= M.D_POOL for o in offs)
            if cls == "A":
                assert all(o % 16 == 0 for o in offs) and al == (c % 16 == 0)
            elif cls == "U":
                assert all((o + 64 - c) % 16 == 0 for o in offs) and al
            else:
                assert all((o - c) % 16 != 0 for o in offs) and not al
            if n:
                combos.setdefault(cls, set()).add((al, c != 0))
    assert M.D_STRIDE % 16 == 0 and M.D_STRIDE >= M.D_TMAX
    assert combos["A"] >= {(True, False), (False, True)}
    assert combos["U"] == {(True, False), (True, True)}
    assert combos["M"] == {(False, False), (False, True)}
    full = {cls: {(al, (tot & 63) != 0) for _, ui, _, tot, _, n, al in M.d_steps(cls, M.pair_chains()) if n and ui is not None}
            for cls in M.D_CLASSES}
    assert full["A"] == {(True, False), (True, True), (False, True)}   # aligned base, carry 16/32/48: aligned
    assert full["U"] == combos["U"] and full["M"] == combos["M"]
    # "odd address, aligned kernel" happens in U
    assert any(al and offs[0] % 16 for _, ui, _, _, offs, n, al in M.d_steps("U", M.pair_chains()) if n and ui is not None)


def test_e_list_cases_and_addresses():
    cases = dict(M.list_cases())
    assert cases["every_length"] == list(range(901))
    assert cases["long_first"][0] == 5000 and sorted(cases["long_first"][1:]) == list(range(63))
    assert cases["long_last"][-1] == 5000 and sorted(cases["long_last"][:-1]) == list(range(63))
    assert len(cases["long_first"]) == len(cases["long_last"]) == 64
    assert [len(cases[f"n{n}"]) for n in (1, 63, 64, 65, 129)] == [1, 63, 64, 65, 129]
    assert cases["all_empty"] and not any(cases["all_empty"])
    for name, lens in cases.items():
        offs, size = M.list_offsets(lens, True)
        assert all(o % 16 == 0 for o in offs), name
        uoffs, usize = M.list_offsets(lens, False)
        assert all(o % 16 for o in uoffs), name
        if len(lens) >= 15:
            assert {o % 16 for o in uoffs} == set(range(1, 16)), name
        for o, s in ((offs, size), (uoffs, usize)):
            assert all(a + n <= b for a, n, b in zip(o, lens, o[1:] + [s])), name
    # a wave's lanes end at different blocks: more than one block count within 64 sorted neighbours
    for name in ("n63", "n64", "n65", "n129", "every_length"):
        lens = sorted(cases[name], reverse=True)
        assert len({n // 64 for n in lens[:64]}) > 1, name


def test_f_crosses_32_bits_of_bit_count():
    assert M.F_TOTAL == (512 << 20) + 1 and (M.F_TOTAL * 8) >> 32 == 1
    assert len(set(M.F_OFFSETS)) == 8 and max(M.F_OFFSETS) <= 64
    assert any(o % 16 for o in M.F_OFFSETS) and any(o % 16 == 0 for o in M.F_OFFSETS)


def test_g_segment_shapes():
    assert M.G_PIPELINED == ((4, 2), (3, 2), (2, 1), (1, 1)) and M.G_SINGLE == ((8, 3), (16385, 40001))
    seg = {S: M.segments(S, 4) for S in M.G_SIZES}
    assert all(sum(v) == S for S, v in seg.items())
    assert seg[16383] == [16383] and seg[16384] == [16384]          # one segment
    assert seg[16385] == [16384, 1]                                 # a second segment of one byte
    assert [seg[16384 + x][-1] for x in (55, 56, 64)] == [55, 56, 64]   # last segment around the pad edge
    assert seg[32768] == [16384] * 2 and seg[131072] == [16384] * 8  # exact multiples
    assert seg[131073] == [16384] * 8 + [1]
    assert seg[135169][0] == 20480 and seg[139263] == [20480] * 6 + [16383]  # seg past 16 KiB
    assert sum(S % 2 for S in M.G_SIZES) >= 6
    assert all(M.segments(S, 8) == [S] for S in M.G_SINGLE[1])


def test_h_host_cases_close_chunks_both_ways():
    cases = dict(M.host_cases())
    assert cases["every_length"] == list(range(901)) and M.host_chunks(cases["every_length"]) == 1
    rec = cases["records"]
    assert len(rec) == 65541 and rec[:42] == list(range(41)) + [0]
    assert sum((n + 15) & ~15 for n in rec) < M.H_SLOT and M.host_chunks(rec) == 2      # closed by records
    big = cases["slot_bytes"]
    assert big[:70] == [(1 << 20) - i % 16 for i in range(70)] and len(big) == 110 and max(big[70:]) < 300
    assert len(big) < M.H_RECS and M.host_chunks(big) == 2                              # closed by slot bytes
    assert max(big) <= M.H_SLOT  # none streamed as a chain of its own
