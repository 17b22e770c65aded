"""hbec_hash_plan_files: the ShardHash of multi-stripe shard files on a plan.  A
shard file is shard j of each of an object's entries back to back (ecSplit
appends it stripe by stripe), hashed as one stream, compared with the stored
hash on the device, and the result written per entry in the form heal_mixed
reads.

Expected digests never come from the product: every one is hashlib.md5 of the
concatenated bytes in the slots (or, for the pin, the committed hashes of the
reference's split).  The where word is the rule of include/hbec.h written out
here in Python.  Whole digest, bad and where arrays are compared, sentinel
filled, so a write outside the selected files of the examined objects shows.
"""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest
import torch

import test_gpu_hash_plan as HP
import test_gpu_mixed_plan as MP
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import oracle as O

pytestmark = pytest.mark.gpu

U32P = C.POINTER(C.c_uint32)
SENT, D = HP.SENT, HP.D
Lay, i32, u8, host, dev8, bits_of, where_word = HP.Lay, HP.i32, HP.u8, HP.host, HP.dev8, HP.bits_of, HP.where_word


def starts_of(objects):
    """(flat sizes, object_start) of a list of objects, each a list of piece lengths."""
    sizes = [s for o in objects for s in o]
    return sizes, np.cumsum([0] + [len(o) for o in objects]).astype(np.uint32)


def file_md5(sizes, at, bufs, starts, n):
    """[objects, n, 16] hashlib digests of every shard file (0 for objects without a byte)."""
    out = np.zeros((len(starts) - 1, n, 16), np.uint8)
    for g in range(len(starts) - 1):
        ents = [e for e in range(starts[g], starts[g + 1]) if sizes[e]]
        for j in range(n if ents else 0):
            h = hashlib.md5()
            for e in ents:
                b, o = at[e][j]
                h.update(bufs[b][o:o + sizes[e]].tobytes())
            out[g, j] = np.frombuffer(h.digest(), np.uint8)
    return out


def expect(sizes, starts, n, ref, select=None, exp=None, flt=None, fbits=1, kernel_route=True):
    """(digests, bad, where) as include/hbec.h says, from hashlib's digests `ref`."""
    no, ne = len(starts) - 1, len(sizes)
    want_d = np.full((no, n, 16), SENT, np.uint8)
    want_b, want_w = np.zeros(no, np.uint32), np.zeros(ne, np.uint32)
    for g in range(no):
        ents = range(starts[g], starts[g + 1])
        live = [e for e in ents if sizes[e]]
        passing = lambda e: flt is None or bool(flt[e] & fbits)  # noqa: E731
        if live and any(passing(e) for e in ents):
            for j in range(n):
                if select is None or select[g][j]:
                    want_d[g, j] = ref[g, j]
                    if exp is not None and not np.array_equal(exp[g, j], ref[g, j]):
                        want_b[g] |= 1 << j
        sel = (1 << n) - 1 if select is None else bits_of(select[g])
        for e in live:
            if not kernel_route:
                want_w[e] = N.LOC_SKIPPED
            elif passing(e):
                want_w[e] = where_word(sel, int(want_b[g]))
    return want_d, want_b, want_w


def run(plan, starts, ne, n, select=None, exp=None, flt=None, fbits=1, digests=True):
    no = len(starts) - 1
    dig, bad, where = u8(no * n * 16), i32(no), i32(ne)
    f = None if flt is None else torch.from_numpy(np.asarray(flt, np.uint32).view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    plan.hash_files(starts, select, digests=dig if digests else None, expected=None if exp is None else dev8(exp),
                    bad=bad, where=where, filter=f, filter_bits=fbits)
    torch.cuda.synchronize()
    return dig.cpu().numpy().reshape(no, n, 16), host(bad), host(where)


# ---- 1. boundaries ----

def boundary_objects():
    objs = []
    lens = list(range(1, 131)) + [4095, 4096, 4097]
    at, width = 0, 1
    while at < len(lens):  # every length, in objects of 1..5 entries
        objs.append(lens[at:at + width])
        at += width
        width = width % 5 + 1
    objs += [[7, 3, 11, 5, 20], [1, 1, 1, 1, 1], [20, 19, 18, 17, 16], [9, 1, 2, 2, 50]]  # blocks over 3+ segments
    objs += [[0, 50, 61], [50, 0, 61], [50, 61, 0], [0, 0, 0], [0], [], [0, 0, 77, 0, 0]]
    objs += [[30, 25], [30, 26], [30, 27], [100, 19], [100, 20], [31, 31, 57], [31, 31, 58]]  # around 56 mod 64
    for g in (1, 2, 3):
        for d in (-1, 0, 1):
            t = 64 * g * D + d
            objs.append([t - 13 - g, 13 + g])
            objs.append([5, t - 10 - g, 5 + g])
    for r in range(64):  # the stream position at the boundary takes every residue
        objs.append([r + 64 * (1 + r % 2), 37 + r])
    return objs


@pytest.mark.parametrize("objects", [False, True], ids=["stripes", "objects"])
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)], ids=["4+2", "8+3"])
def test_boundaries_match_hashlib(k, m, objects):
    n = k + m
    objs = boundary_objects()
    sizes, starts = starts_of(objs)
    lay = Lay(k, m, sizes, objects, seed=101 + k)
    # what the inputs cover, before the GPU sees them
    assert {len(o) for o in objs} >= {0, 1, 2, 3, 4, 5}
    pieces = {s for s in sizes}
    assert pieces >= set(range(0, 131)) | {4095, 4096, 4097} and max(pieces) <= 4400
    bound_res, start_res, mixed_res, three = set(), set(), False, False
    totals = set()
    for g, o in enumerate(objs):
        live = [e for e in range(starts[g], starts[g + 1]) if sizes[e]]
        totals.add(sum(o))
        pos = 0
        for e in live[:-1]:
            pos += sizes[e]
            bound_res.add(pos % 64)
        cuts = np.cumsum([sizes[e] for e in live])
        for b0 in range(0, int(cuts[-1]) - 63 if live else 0, 64):  # whole blocks
            three = three or int(np.sum((cuts > b0) & (cuts < b0 + 64))) >= 2
        for j in range(n):
            res = {lay.at[e][j][1] % 4 for e in live}
            start_res |= res
            mixed_res = mixed_res or len(res) > 1
    assert bound_res == set(range(64)) and start_res == set(range(4)) and mixed_res and three
    assert {t % 64 for t in totals} >= {55, 56, 57}
    assert totals >= {64 * g * D + d for g in (1, 2, 3) for d in (-1, 0, 1)}
    for o in ([0, 50, 61], [50, 0, 61], [50, 61, 0]):
        assert o in objs
    # the call's lanes: objects by total, longest first; waves mix segment counts
    order = sorted((g for g, o in enumerate(objs) if sum(o)), key=lambda g: -sum(objs[g]))
    lanes = [sum(1 for s in objs[g] if s) for g in order for _ in range(n)]
    assert len(lanes) >= 130 and any(len(set(lanes[w:w + 64])) > 1 for w in range(0, len(lanes), 64))

    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    ref = file_md5(sizes, lay.at, lay.bufs, starts, n)
    got_d, got_b, got_w = run(plan, starts, len(sizes), n, exp=ref)
    want_d, want_b, want_w = expect(sizes, starts, n, ref, exp=ref)
    wrong = [(objs[g], j) for g, j in zip(*np.nonzero((got_d != want_d).any(axis=2)))]
    assert not wrong, wrong[:10]  # (piece lengths, shard)
    assert not got_b.any() and not got_w.any()
    for x, y in zip(t, lay.bufs):
        assert np.array_equal(x.cpu().numpy(), y)  # read only


# ---- 2. one-stripe objects: the same bytes as hash_mixed ----

@pytest.mark.parametrize("objects", [False, True], ids=["stripes", "objects"])
def test_single_entry_objects_equal_hash_mixed(objects):
    k, m, n = 4, 2, 6
    rng = np.random.default_rng(202)
    sizes = HP.edge_sizes() + [0, 0]
    ne = len(sizes)
    lay = Lay(k, m, sizes, objects, seed=203)
    select = (rng.random((ne, n)) < 0.6).astype(np.uint8)
    select[3] = 0
    flt = rng.integers(0, 4, ne).astype(np.uint32)
    exp = HP.md5_of(sizes, lay.at, lay.bufs, n)
    exp[rng.random((ne, n)) < 0.2] ^= 0x04
    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    starts = np.arange(ne + 1, dtype=np.uint32)
    outs = []
    for files in (False, True):
        dig, bad, where = u8(ne * n * 16), i32(ne), i32(ne)
        f = torch.from_numpy(flt.view(np.int32).copy()).cuda()
        kw = dict(digests=dig, expected=dev8(exp), bad=bad, where=where, filter=f, filter_bits=2)
        torch.cuda.synchronize()
        if files:
            plan.hash_files(starts, select, **kw)
        else:
            plan.hash_mixed(select, **kw)
        torch.cuda.synchronize()
        outs.append((dig.cpu().numpy(), host(bad), host(where)))
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()
    assert outs[0][1].any() and outs[0][2].any() and (outs[0][0] != SENT).any()


# ---- 3. the reference-derived pin ----

def test_reference_split_of_a_three_stripe_object():
    v = json.loads((HP.ROOT / "tests" / "golden" / "vectors.json").read_text())["shard_hashes_4_2_chunk1k"]
    k, m, n, chunk = 4, 2, 6, v["chunk"]
    files = O.ec_split(k, m, bytes(O.object_bytes(v["object"], v["len"])), chunk)
    pieces = [1024, 1024, 452]
    assert all(len(f) == sum(pieces) for f in files)
    # three entries of one object, each ecSplit's databuf layout: the stripe's six pieces back to back
    buf, bases, pos = bytearray(), [], 0
    for s in pieces:
        buf += b"\0" * 5  # odd starts
        bases.append(len(buf))
        for f in files:
            buf += bytes(f[pos:pos + s])
        pos += s
    t = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    plan = B.StripePlan(RS.New(k, m), stripes=[(t.data_ptr() + b, s) for b, s in zip(bases, pieces)])
    dig = u8(n * 16)
    plan.hash_files([0, 3], digests=dig)
    torch.cuda.synchronize()
    got = [bytes(x).hex() for x in dig.cpu().numpy().reshape(n, 16)]
    assert got == v["hashes"]


# ---- 4. filter ----

@pytest.mark.parametrize("objects", [False, True], ids=["stripes", "objects"])
def test_filter_examines_whole_objects_and_marks_passing_entries(objects):
    k, m, n = 4, 2, 6
    rng = np.random.default_rng(404)
    objs = [[int(x) for x in rng.integers(1, 300, int(rng.integers(1, 6)))] for _ in range(40)]
    objs[5][0] = 0
    objs += [[33, 0, 71]]
    sizes, starts = starts_of(objs)
    ne, no = len(sizes), len(objs)
    lay = Lay(k, m, sizes, objects, seed=405)
    select = (rng.random((no, n)) < 0.6).astype(np.uint8)
    flt = (rng.integers(0, 8, ne) * (rng.random(ne) < 0.4)).astype(np.uint32)
    g1 = next(g for g, o in enumerate(objs) if len(o) >= 3)
    flt[starts[g1]:starts[g1 + 1]] = 0
    flt[starts[g1] + 1] = 7  # one passing entry among several
    select[g1] = 1
    flt[starts[no - 1]:starts[no]] = [0, 7, 0]  # only the zero-length entry passes: hashed, no where word
    select[no - 1] = 1
    ref = file_md5(sizes, lay.at, lay.bufs, starts, n)
    exp = ref.copy()
    exp[rng.random((no, n)) < 0.3] ^= 0x20
    exp[g1, 2] ^= 1
    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    for fbits in (1, 6):
        want = expect(sizes, starts, n, ref, select, exp, flt, fbits)
        got = run(plan, starts, ne, n, select, exp, flt, fbits)
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        examined = [(want[0][g] != SENT).any() for g in range(no)]
        assert any(examined) and not all(examined)
        # the object with one passing entry: hashed, bad, and only that entry has a word
        assert want[1][g1] & 4 and [bool(x) for x in want[2][starts[g1]:starts[g1 + 1]]][:3] == [False, True, False]
        assert (want[0][no - 1] != SENT).any() and not want[2][starts[no - 1]:].any()
    # no object passes: nothing is written
    got = run(plan, starts, ne, n, select, exp, np.full(ne, 8, np.uint32), 1)
    assert (got[0] == SENT).all() and not got[1].any() and not got[2].any()


# ---- 5. flips ----

def test_compare_names_the_flipped_file():
    k, m, n = 4, 2, 6
    P = [130, 999, 257]
    UNSEL, A, Bb = 1, 3, 5
    total = sum(P)
    kinds = [("one", 0), ("one", total - 1), ("one", 63), ("one", 64), ("one", P[0] - 1), ("one", P[0]),
             ("one", P[0] + P[1] - 1), ("one", P[0] + P[1]), ("two", 500), ("unselected", 200), ("expected", 7)]
    objs = [list(P) for _ in kinds] + [[0], [77, 78]]
    sizes, starts = starts_of(objs)
    ne, no = len(sizes), len(objs)
    lay = Lay(k, m, sizes, False, seed=505)
    exp = file_md5(sizes, lay.at, lay.bufs, starts, n)  # the stored hashes of the clean files
    bufs = [x.copy() for x in lay.bufs]
    want_b = np.zeros(no, np.uint32)
    want_named = np.full(ne, N.LOC_CLEAN, np.int64)

    def flip(g, j, p):
        e = int(starts[g])
        while p >= sizes[e]:
            p -= sizes[e]
            e += 1
        b, o = lay.at[e][j]
        bufs[b][o + p] ^= 1 << (g + p) % 8

    for g, (kind, p) in enumerate(kinds):
        ents = slice(starts[g], starts[g + 1])
        if kind == "one":
            flip(g, A, p)
            want_b[g], want_named[ents] = 1 << A, A
        elif kind == "two":
            flip(g, A, p)
            flip(g, Bb, p + 300)
            want_b[g], want_named[ents] = (1 << A) | (1 << Bb), N.LOC_MULTIPLE
        elif kind == "unselected":
            flip(g, UNSEL, p)
        else:
            exp[g, A, p] ^= 0x80
            want_b[g], want_named[ents] = 1 << A, A
    select = np.ones((no, n), np.uint8)
    select[:, UNSEL] = 0
    t = lay.upload(bufs)
    plan = lay.plan(RS.New(k, m), t)
    ref = file_md5(sizes, lay.at, bufs, starts, n)
    got = run(plan, starts, ne, n, select, exp)
    want = expect(sizes, starts, n, ref, select, exp)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert np.array_equal(got[1], want_b)
    present = np.repeat(select, [len(o) for o in objs], axis=0)
    named = B.locate_decode(k, m, present, got[2])
    live = [e for e in range(ne) if sizes[e]]
    assert np.array_equal(named[live], want_named[live]), named.tolist()


# ---- 6. the sweep ----

@pytest.mark.parametrize("k,m,lost", [(4, 2, 1), (8, 3, 2)], ids=["4+2", "8+3"])
def test_sweep_heals_multi_stripe_objects_without_a_sync(k, m, lost):
    n = k + m
    rng = np.random.default_rng(600 + k)
    objs = [[int(x) | 1 for x in rng.integers(1, 4100, 1 + g % 4)] for g in range(48)]
    sizes, starts = starts_of(objs)
    ne, no = len(sizes), len(objs)
    c = MP.Case(k, m, "stripes", sizes, 604 + k)
    present_obj = np.ones((no, n), np.uint8)
    for g in range(no):
        present_obj[g][rng.choice(n, size=lost, replace=False)] = 0  # a lost shard file is lost in every stripe
    present = np.repeat(present_obj, [len(o) for o in objs], axis=0)
    hit = {}  # entry -> file
    for q, g in enumerate(range(2, no, 6)):
        here = [i for i in range(n) if present_obj[g][i]]
        e = int(starts[g]) + q % len(objs[g])
        hit[e] = here[k] if q % 3 == 2 else here[(q * 3) % k]
    assert len(hit) == 8 and {int(r.sum()) for r in present} == {k + 1}
    assert {len(objs[g]) for g in range(2, no, 6)} >= {1, 3}
    inp, _ = c.garble(present, seed=605)
    for e, i in hit.items():
        b, o = c.shards[e][i]
        inp[b][o + int(rng.integers(sizes[e]))] ^= 1 << e % 8
    exp = dev8(file_md5(sizes, c.shards, c.bufs, starts, n))  # what IndexDB holds: the stored files' hashes
    enc = RS.New(k, m)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    flags, amb, where, healed = (i32(ne) for _ in range(4))
    bad, bad2 = i32(no), i32(no)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.repair_mixed(present, flags, stream=s)
    plan.locate_mixed(present, amb, flags=flags, stream=s)
    plan.hash_files(starts, present_obj, expected=exp, bad=bad, where=where, filter=flags, stream=s)
    plan.heal_mixed(present, where, healed, stream=s)
    plan.hash_files(starts, None, expected=exp, bad=bad2, stream=s)
    torch.cuda.synchronize()
    f = host(flags)
    assert {e for e in range(ne) if f[e]} == set(hit) and set(f[list(hit)]) == {1}
    assert [int(x) for x in B.locate_decode(k, m, present, host(amb))[list(hit)]] == [N.LOC_AMBIGUOUS] * 8
    obj_of = np.repeat(np.arange(no), [len(o) for o in objs])
    want_b = np.zeros(no, np.uint32)
    for e, i in hit.items():
        want_b[obj_of[e]] = 1 << i
    assert np.array_equal(host(bad), want_b)
    named = B.locate_decode(k, m, present, host(where))
    assert {e: int(named[e]) for e in hit} == hit
    assert all(int(named[e]) == N.LOC_CLEAN for e in range(ne) if e not in hit)
    want_h = np.zeros(ne, np.uint32)
    want_h[list(hit)] = N.HEAL_DONE | 2
    assert np.array_equal(host(healed), want_h)
    MP.check_equal(t, c.bufs)  # every shard of every entry is the oracle's codeword again
    assert not host(bad2).any()


# ---- 7. routes and limits ----

@pytest.mark.parametrize("k,m", [(13, 3), (20, 4)], ids=["13+3", "20+4"])
def test_other_route_shapes_are_hashed_and_marked_skipped(k, m):
    n = k + m
    objs = [[1, 63], [0], [64, 65, 333], [1027], [70, 0]]
    sizes, starts = starts_of(objs)
    lay = Lay(k, m, sizes, False, seed=700 + k)
    ref = file_md5(sizes, lay.at, lay.bufs, starts, n)
    exp = ref.copy()
    exp[0, n - 1, 3] ^= 1
    exp[2, 0, 15] ^= 0x40
    exp[2, k, 0] ^= 2
    flt = np.array([1, 1, 1, 0, 1, 0, 0, 1, 1], np.uint32)  # object 3 is filtered out
    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    got = run(plan, starts, len(sizes), n, None, exp, flt)
    want = expect(sizes, starts, n, ref, None, exp, flt, kernel_route=False)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert (got[0][3] == SENT).all() and got[1][0] == 1 << (n - 1) and got[1][2] == 1 | (1 << k)
    assert np.array_equal(got[2], np.array([N.LOC_SKIPPED if s else 0 for s in sizes], np.uint32))


def test_28_8_hashes_but_refuses_expected():
    k, m, n = 28, 8, 36
    objs = [[129, 0, 64], [1]]
    sizes, starts = starts_of(objs)
    lay = Lay(k, m, sizes, False, seed=758)
    ref = file_md5(sizes, lay.at, lay.bufs, starts, n)
    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    dig, bad = u8(2 * n * 16), i32(2, 7)
    with pytest.raises(RS.ErrInvalidArg):
        plan.hash_files(starts, None, digests=dig, expected=dev8(ref), bad=bad)
    torch.cuda.synchronize()
    assert (dig.cpu().numpy() == SENT).all() and (host(bad) == 7).all()
    plan.hash_files(starts, None, digests=dig)
    torch.cuda.synchronize()
    assert np.array_equal(dig.cpu().numpy().reshape(2, n, 16), ref)


def test_argument_errors_leave_the_outputs_unchanged():
    k, m, n = 4, 2, 6
    objs = [[100, 0], [333]]
    sizes, starts = starts_of(objs)
    ne, no = len(sizes), len(objs)
    lay = Lay(k, m, sizes, False, seed=760)
    t = lay.upload()
    enc, other = RS.New(k, m), RS.New(8, 3)
    plan = lay.plan(enc, t)
    exp = dev8(file_md5(sizes, lay.at, lay.bufs, starts, n) ^ 1)  # every file would count as bad
    # bad has a word per entry here, so that it can stand in for where and filter
    dig, bad, where, flt = u8(no * n * 16), i32(ne, 0x0F0F), i32(ne, 0x1111), i32(ne, 1)
    ones = np.ones((no, n), np.uint8)
    for kw in (dict(digests=dig, expected=exp, bad=bad, where=bad),  # aliasing, pair by pair
               dict(digests=dig, expected=exp, bad=bad, filter=bad),
               dict(digests=dig, expected=exp, bad=bad, where=where, filter=where),
               dict(digests=dig, where=where),  # where without bad
               dict(digests=dig, expected=exp)):  # expected without bad
        with pytest.raises(RS.ErrInvalidArg):
            plan.hash_files(starts, ones, **kw)
    big = u8(4 * n * 16)
    for st in ([0, 2], [1, 2, 3], [0, 3, 2, 3], [0, 2, 4], [0, 1, 2]):  # malformed object tables
        with pytest.raises(RS.ErrInvalidArg):
            plan.hash_files(st, None, digests=big, where=where, bad=i32(4), filter=flt)
    L = N.lib()
    row = np.ones(n, np.uint8)
    row11 = np.ones(11, np.uint8)

    def raw(e, rows, idx):
        idx = np.asarray(idx, np.uint32)
        return L.hbec_hash_plan_files(e.handle, plan._h, starts.ctypes.data_as(U32P), no,
                                      rows.ctypes.data_as(N._U8P), 1, idx.ctypes.data_as(U32P),
                                      C.c_void_p(flt.data_ptr()), 1, C.c_void_p(exp.data_ptr()),
                                      C.c_void_p(dig.data_ptr()), C.c_void_p(bad.data_ptr()),
                                      C.c_void_p(where.data_ptr()), None)

    assert raw(enc, row, [0, 1]) == N.ERR_INVALID_ARG  # index out of range
    assert raw(enc, row, [7, 0]) == N.ERR_INVALID_ARG
    assert raw(other, row11, [0, 0]) == N.ERR_INVALID_ARG  # a plan of another (k, m)
    torch.cuda.synchronize()
    assert (dig.cpu().numpy() == SENT).all() and (big.cpu().numpy() == SENT).all()
    assert (host(bad) == 0x0F0F).all() and (host(where) == 0x1111).all() and (host(flt) == 1).all()
    assert raw(enc, row, [0, 0]) == N.HBEC_OK  # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert (host(bad) == np.array([0x0F0F | 0x3F] * no + [0x0F0F] * (ne - no), np.uint32)).all()
    assert (host(where) == np.array([0x1111 | N.LOC_BAD | 0x3F, 0x1111, 0x1111 | N.LOC_BAD | 0x3F], np.uint32)).all()


def test_stats_count_launches_chains_and_segments():
    k, m, n = 4, 2, 6
    objs = [[5, 0, 70], [0], [200, 64], [], [0, 0]]
    sizes, starts = starts_of(objs)
    ne, no = len(sizes), len(objs)
    lay = Lay(k, m, sizes, False, seed=770)
    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    dig, bad, where = u8(no * n * 16), i32(no), i32(ne)
    exp = dev8(file_md5(sizes, lay.at, lay.bufs, starts, n))

    def delta(fn):
        a = B.hash_files_stats()
        fn()
        torch.cuda.synchronize()
        b = B.hash_files_stats()
        return {f: b[f] - a[f] for f in a}

    assert delta(lambda: plan.hash_files(starts, None, digests=dig)) == {
        "kernel_launches": 1, "chains": 2 * n, "segments": 4 * n}
    sel = np.zeros((no, n), np.uint8)
    sel[0, 2] = sel[1, 3] = sel[2, 0] = sel[2, 5] = 1  # object 1 has no byte: no chain
    assert delta(lambda: plan.hash_files(starts, sel, expected=exp, bad=bad, where=where)) == {
        "kernel_launches": 2, "chains": 3, "segments": 6}
    dig.fill_(SENT)
    assert delta(lambda: plan.hash_files(starts, np.zeros((no, n)), digests=dig, bad=bad, where=where)) == {
        "kernel_launches": 0, "chains": 0, "segments": 0}
    assert (dig.cpu().numpy() == SENT).all() and not host(bad).any() and not host(where).any()
    empty = B.StripePlan(RS.New(k, m), stripes=[])
    assert delta(lambda: empty.hash_files([0])) == {"kernel_launches": 0, "chains": 0, "segments": 0}
