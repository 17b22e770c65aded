"""What the tiled stripes sweep's cases cover (tests/stripes_sweep_cases.py),
asserted on the cases themselves before any GPU sees them: no GPU."""
import stripes_sweep_cases as S

ALL_KR = {(K, R) for K in range(1, 9) for R in (1, 2, 3)}


def device_calls():
    """(plan, order, operation, lost) of every call of the device sweep"""
    for p in S.PLANS:
        for o in S.orders(p):
            for name, lost in S.lost_patterns(p):
                if o.rotation and name != "encode":
                    continue
                yield p, o, name, lost


def test_tile_sizes_and_the_pass_rule():
    assert [S.tile_bytes(k) for k in (1, 2, 3, 4, 8, 9, 16, 24)] == [4096, 2048, 1024, 1024, 1024, 1024, 1024, 1024]
    assert S.passes(4, 2) == [("plain", 4, 2)]
    assert S.passes(4, 2, objects=True) == [("split", 4, 2)]
    assert S.passes(12, 3) == [("plain", 8, 3), ("accumulate", 4, 3)]
    assert S.passes(4, 4) == [("plain", 4, 3), ("plain", 4, 1)]
    assert S.passes(3, 5, objects=True) == [("split", 3, 3), ("split", 3, 2)]
    assert S.passes(17, 3) == [("plain", 8, 3), ("accumulate", 8, 3), ("accumulate", 1, 3)]
    assert S.passes(24, 4) == [("plain", 8, 3), ("accumulate", 8, 3), ("accumulate", 8, 3),
                               ("plain", 8, 1), ("accumulate", 8, 1), ("accumulate", 8, 1)]
    assert S.passes(10, 2, mirror=True) == [("mirror", 8, 2), ("mirror_accumulate", 2, 2)]
    assert S.launches(24, 4) == {"plain": 2, "split": 0, "accumulate": 4, "mirror": 0, "mirror_accumulate": 0}
    assert S.tiles_of(16, 1024) == [16] and S.tiles_of(1024, 1024) == [1024]
    assert S.tiles_of(2416, 1024) == [1024, 1024, 368] and S.tiles_of(2048, 2048) == [2048]


def test_the_plans():
    full = [p for p in S.PLANS if not p.spot]
    assert [(p.k, p.layout) for p in full] == ([(k, "stripes") for k in range(1, 17)]
                                               + [(k, "objects") for k in range(1, 9)])
    assert all(p.m == 3 for p in full)
    assert {(p.k, p.m, p.layout) for p in S.PLANS if p.spot} == {
        (4, 4, "stripes"), (4, 4, "objects"), (3, 5, "stripes"), (3, 5, "objects"), (17, 3, "stripes"),
        (24, 4, "stripes")}
    for p in S.PLANS:
        T = S.tile_bytes(p.k)
        if p.spot:
            assert S.lengths(p) == (16, T - 16, T, T + 16, 2 * T, 2 * T + 368)
        else:
            assert S.lengths(p) == tuple(range(16, 2 * T + 368 + 1, 16))
        assert S.boundary(p) == (() if p.spot or not 5 <= p.k <= 12 else
                                 ((S.REC_MIN_S_BIG if p.k > 8 else S.REC_MIN_S) - 16,
                                  S.REC_MIN_S_BIG if p.k > 8 else S.REC_MIN_S))
    # the largest plan: k = 1, 535 entries and at most 3 fillers, under 10 MB resident
    p1 = S.PLANS[0]
    assert len(S.lengths(p1)) == 535
    assert all(535 <= len(o.entries) <= 538 for o in S.orders(p1))
    assert max((p.k + p.m) * (sum(o.entries) + S.GAP * len(o.entries)) for p in S.PLANS for o in S.orders(p)) < 10e6


def test_every_instance_of_plain_split_and_accumulate_is_predicted():
    seen = {}
    for p, o, name, lost in device_calls():
        for v, K, R in S.op_passes(p, lost):
            seen.setdefault(v, set()).add((K, R))
    assert set(seen) == {"plain", "split", "accumulate"}
    assert seen["plain"] == ALL_KR and seen["split"] == ALL_KR and seen["accumulate"] == ALL_KR
    assert sum(len(v) for v in seen.values()) == 72


def test_every_mirrored_instance_is_predicted():
    seen = {}
    for c in S.HASH_CASES:
        assert c.lengths == S.seams(c.k)
        for v, K, R in S.hash_passes(c):
            seen.setdefault(v, set()).add((K, R))
    assert seen == {"mirror": ALL_KR, "mirror_accumulate": ALL_KR}
    assert S.hash_launches(S.HashCase(12, 2, ())) == {"plain": 0, "split": 0, "accumulate": 0, "mirror": 1,
                                                      "mirror_accumulate": 1}


def test_every_length_meets_every_instance():
    """16, 32, ..., 2 T + 368 with T the tile of the instance's plan, under the
    cap of one block (the two full orders run every operation)."""
    seen = {}
    for p, o, name, lost in device_calls():
        if p.spot or o.rotation:
            continue
        T = S.tile_bytes(p.k)
        tiled = frozenset(x for x in o.entries if not S.on_records(p.k, x))
        for inst in S.op_passes(p, lost):
            seen.setdefault((inst, T), set()).update(tiled)
    insts = {i for i, _ in seen}
    assert insts == {(v, K, R) for v in ("plain", "split", "accumulate") for K, R in ALL_KR}
    for (inst, T), ls in seen.items():
        assert set(range(16, 2 * T + 368 + 1, 16)) <= ls, (inst, T)
    # plain and split K = 1, 2 have their own tile sizes; accumulate passes always follow 8 inputs
    assert {T for (i, T) in seen if i[0] == "accumulate"} == {1024}
    assert {T for (i, T) in seen if i[1] == 1 and i[0] != "accumulate"} == {4096}
    assert {T for (i, T) in seen if i[1] == 2 and i[0] != "accumulate"} == {2048}


def test_orders():
    residues = set()
    for p in S.PLANS:
        T = S.tile_bytes(p.k)
        os_ = S.orders(p)
        assert [o.name for o in os_[:2]] == ["ascending", "shuffle"] and all(o.rotation for o in os_[2:])
        body = sorted(S.lengths(p) + S.boundary(p))
        for o in os_:
            fill = len(o.entries) - len(body)
            assert 0 <= fill <= 3 and sorted(o.entries) == sorted(body + [S.FILLER] * fill), (p, o.name)
            assert S.n_tiles(p, o) % 4 == S.residue_of(p, o.name)
            assert S.n_records(p, o) == (1 if S.boundary(p) else 0)
            if not o.rotation:
                residues.add(S.n_tiles(p, o) % 4)
        asc = [x for x in os_[0].entries[:len(body)]]
        assert asc == body
        v = S.valids(p, os_[1].entries)
        assert all(a != b or a == T for a, b in zip(v, v[4:]))  # one wave's consecutive tiles
        assert any(a != b for a, b in zip(v, v[1:]))
    assert residues == {0, 1, 2, 3}
    # a plan of a few hundred tiles: hundreds of loop iterations under one block
    assert min(S.n_tiles(p, o) for p in S.PLANS if not p.spot for o in S.orders(p)) > 250


def test_every_valid_value_meets_the_first_a_middle_and_the_last_iteration():
    first, middle, last = {}, {}, {}
    for p in S.PLANS:
        T = S.tile_bytes(p.k)
        for o in S.orders(p):
            a, b, c = S.rows_seen(p, o)
            assert len(a) == 4 and len(c) == (S.n_tiles(p, o) - 1) % 4 + 1
            first.setdefault(T, set()).update(a)
            middle.setdefault(T, set()).update(b)
            last.setdefault(T, set()).update(c)
    for T in (1024, 2048, 4096):
        every = set(range(16, T + 1, 16))
        assert first[T] >= every and middle[T] >= every and last[T] >= every, T
    # what it costs: 16 + 32 + 64 rotations, encode only
    assert sum(o.rotation for p in S.PLANS for o in S.orders(p)) == 112
