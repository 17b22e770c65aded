"""hbec_hash_plan_mixed: the ShardHash of a plan's shards on the device, compared
with the stored ones, and the result in the form heal_mixed reads.

Expected digests never come from the product: every one is hashlib.md5 of the
bytes in the shard's slot.  The where word is the rule of include/hbec.h written
out here in Python, and what it names is batch.locate_decode's answer
(hbec_locate_decode, host only).  Codewords of the sweep come from the oracle
(test_gpu_mixed_plan.Case).  Whole digest, bad and where arrays are compared,
so a write outside the selected shards of the examined entries shows.
"""
import ctypes as C
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import test_gpu_mixed_plan as MP
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
U32P = C.POINTER(C.c_uint32)
SENT = 0xA5
D = int(re.search(r"#define HBEC_MD5_DEPTH_LIST (\d+)", (ROOT / "hummingbird_amd/csrc/tuning.h").read_text()).group(1))


class Lay:
    """Random bytes for entries of `sizes`, shard j of entry e at at[e][j] =
    (buffer, offset).  Entry e starts at residue e mod 16 (its parity arena at
    (5 e + 3) mod 16), so with odd and even sizes the shard starts cover every
    residue.  No codewords: the hash does not care."""

    def __init__(self, k, m, sizes, objects=False, seed=0):
        self.k, self.m, self.sizes, self.objects = k, m, list(sizes), objects
        rng = np.random.default_rng(seed)
        per = [k, m] if objects else [k + m]
        pos = [0] * len(per)
        self.at, self.base = [], []
        for e, s in enumerate(self.sizes):
            where, bases = [], []
            for b, cnt in enumerate(per):
                off = pos[b] + 3
                off += ((e if b == 0 else 5 * e + 3) - off) % 16
                bases.append(off)
                where += [(b, off + j * s) for j in range(cnt)]
                pos[b] = off + cnt * s
            self.at.append(where)
            self.base.append(bases)
        self.bufs = [rng.integers(0, 256, p + 19, dtype=np.uint8) for p in pos]
        self.live = [e for e, s in enumerate(self.sizes) if s]

    def upload(self, bufs=None):
        t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (bufs or self.bufs)]
        assert all(x.data_ptr() % 16 == 0 for x in t)
        return t

    def plan(self, enc, t):
        if self.objects:
            return B.StripePlan(enc, objects=[(t[0].data_ptr() + b[0], t[1].data_ptr() + b[1], s)
                                              for b, s in zip(self.base, self.sizes)])
        return B.StripePlan(enc, stripes=[(t[0].data_ptr() + b[0], s) for b, s in zip(self.base, self.sizes)])

    def residues(self, mod):
        return {o % mod for e in self.live for _, o in self.at[e]}


def md5_of(sizes, at, bufs, n):
    """[entries, n, 16] hashlib digests of what lies in every shard slot (0 for empty entries)."""
    out = np.zeros((len(sizes), n, 16), np.uint8)
    for e, s in enumerate(sizes):
        for j in range(n if s else 0):
            b, o = at[e][j]
            out[e, j] = np.frombuffer(hashlib.md5(bufs[b][o:o + s].tobytes()).digest(), np.uint8)
    return out


def where_word(sel_bits, bad_bits):
    """include/hbec.h: the word of an examined kernel-route entry."""
    if bad_bits == 0:
        return 0
    one = bad_bits & (bad_bits - 1) == 0
    return N.LOC_BAD | ((sel_bits & ~bad_bits if one else sel_bits) & 0xFFFF)


def bits_of(row):
    return int(sum(1 << i for i, x in enumerate(row) if x))


def i32(n, fill=0):
    return torch.full((n,), fill, dtype=torch.int32, device="cuda")


def u8(n, fill=SENT):
    return torch.full((n,), fill, dtype=torch.uint8, device="cuda")


def host(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32).copy()


def dev8(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8).reshape(-1).copy()).cuda()


def edge_sizes():
    s = list(range(1, 131))
    s += [64 * g * D + d for g in range(1, 6) for d in (-1, 0, 1)]
    s += [4095, 4096, 4097]
    s.insert(len(s) // 2, 0)
    return s


# ---- 1. every length and alignment ----

@pytest.mark.parametrize("objects", [False, True], ids=["stripes", "objects"])
def test_every_length_and_alignment_matches_hashlib(objects):
    k, m, n = 4, 2, 6
    lay = Lay(k, m, edge_sizes(), objects, seed=11)
    assert lay.residues(16) == set(range(16)) and lay.residues(4) == set(range(4))
    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    dig = u8(len(lay.sizes) * n * 16)
    torch.cuda.synchronize()
    plan.hash_mixed(None, digests=dig)
    torch.cuda.synchronize()
    got = dig.cpu().numpy().reshape(len(lay.sizes), n, 16)
    want = md5_of(lay.sizes, lay.at, lay.bufs, n)
    for e, s in enumerate(lay.sizes):
        if s == 0:
            want[e] = SENT  # the zero-length entry's slots are not written
    wrong = [(lay.sizes[e], j, lay.at[e][j][1] % 16) for e, j in zip(*np.nonzero((got != want).any(axis=2)))]
    assert not wrong, wrong[:10]  # (length, shard, start residue)
    for x, y in zip(t, lay.bufs):
        assert np.array_equal(x.cpu().numpy(), y)  # read only


# ---- 2. selection and filter ----

@pytest.mark.parametrize("objects", [False, True], ids=["stripes", "objects"])
def test_exactly_the_selected_shards_of_examined_entries_are_written(objects):
    k, m, n = 4, 2, 6
    rng = np.random.default_rng(22)
    sizes = [int(x) for x in rng.integers(1, 700, 150)]
    for z in (0, 40, 149):
        sizes[z] = 0
    lay = Lay(k, m, sizes, objects, seed=23)
    ne = len(sizes)
    select = (rng.random((ne, n)) < 0.5).astype(np.uint8)
    select[lay.live[0]] = 0  # nothing set
    select[lay.live[1]] = [0, 1, 0, 0, 0, 1]  # fewer than k
    select[lay.live[2]] = 1
    assert any(0 < r.sum() < k for r in select)
    flt = rng.integers(0, 8, ne).astype(np.uint32)
    ref = md5_of(sizes, lay.at, lay.bufs, n)
    exp = ref.copy()
    wrong = rng.random((ne, n)) < 0.15
    exp[wrong] ^= 0x10  # the stored hash differs: the shard counts as bad
    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    for fbits in (1, 6):
        dig, bad, where = u8(ne * n * 16), i32(ne), i32(ne)
        f = torch.from_numpy(flt.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        plan.hash_mixed(select, digests=dig, expected=dev8(exp), bad=bad, where=where, filter=f, filter_bits=fbits)
        torch.cuda.synchronize()
        want_d = np.full((ne, n, 16), SENT, np.uint8)
        want_b, want_w = np.zeros(ne, np.uint32), np.zeros(ne, np.uint32)
        n_examined = 0
        for e in lay.live:
            if not flt[e] & fbits:
                continue
            n_examined += 1
            for j in range(n):
                if select[e][j]:
                    want_d[e, j] = ref[e, j]
                    want_b[e] |= (1 << j) if wrong[e, j] else 0
            want_w[e] = where_word(bits_of(select[e]), int(want_b[e]))
        assert 0 < n_examined < len(lay.live)
        assert np.array_equal(dig.cpu().numpy().reshape(ne, n, 16), want_d)
        assert np.array_equal(host(bad), want_b)
        assert np.array_equal(host(where), want_w)
        assert np.array_equal(host(f), flt)  # read only
        assert len({int(x) for x in B.locate_decode(k, m, select, want_w)}) > 3  # shards, MULTIPLE and CLEAN all occur


# ---- 3. compare ----

def test_compare_names_the_flipped_shard():
    k, m, n = 4, 2, 6
    S = [130, 999, 4097, 257, 1024]
    positions = lambda s: [0, s - 1, 63, 64, s // 2]  # noqa: E731
    UNSEL, A, Bb = 1, 3, 5  # the unselected shard, and the shards that get flipped
    sizes, plan_of = [], []
    for kind in ("one", "two", "unselected", "expected"):
        for q in range(5):
            sizes.append(S[q])
            plan_of.append((kind, q))
    sizes += [0, 77]  # an empty and a clean entry
    lay = Lay(k, m, sizes, False, seed=33)
    ne = len(sizes)
    exp = md5_of(sizes, lay.at, lay.bufs, n)  # the stored hashes of the clean shards
    bufs = [x.copy() for x in lay.bufs]
    want_b = np.zeros(ne, np.uint32)
    want_named = np.full(ne, N.LOC_CLEAN, np.int64)
    for e, (kind, q) in enumerate(plan_of):
        p = positions(sizes[e])[q]

        def flip(j, e=e, p=p, q=q):
            b, o = lay.at[e][j]
            bufs[b][o + p] ^= 1 << (q + 2) % 8

        if kind == "one":
            flip(A)
            want_b[e], want_named[e] = 1 << A, A
        elif kind == "two":
            flip(A)
            flip(Bb)
            want_b[e], want_named[e] = (1 << A) | (1 << Bb), N.LOC_MULTIPLE
        elif kind == "unselected":
            flip(UNSEL)
        else:
            exp[e, A, q] ^= 0x80
            want_b[e], want_named[e] = 1 << A, A
    select = np.ones((ne, n), np.uint8)
    select[:, UNSEL] = 0
    t = lay.upload(bufs)
    plan = lay.plan(RS.New(k, m), t)
    bad, where = i32(ne), i32(ne)
    torch.cuda.synchronize()
    plan.hash_mixed(select, expected=dev8(exp), bad=bad, where=where)
    torch.cuda.synchronize()
    assert np.array_equal(host(bad), want_b)
    named = B.locate_decode(k, m, select, host(where))
    assert np.array_equal(named, want_named), list(zip(plan_of, named.tolist()))
    assert [int(named[5 * g]) for g in range(4)] == [A, N.LOC_MULTIPLE, N.LOC_CLEAN, A]


# ---- 4. the sweep with one surplus shard ----

@pytest.mark.parametrize("k,m,lost", [(4, 2, 1), (8, 3, 2)], ids=["4+2", "8+3"])
def test_sweep_heals_stripes_with_one_surplus_shard_without_a_sync(k, m, lost):
    n = k + m
    rng = np.random.default_rng(40 + k)
    sizes = [int(x) | 1 for x in rng.integers(1, 4100, 64)]
    c = MP.Case(k, m, "stripes", sizes, 44 + k)
    ne = len(sizes)
    present = np.ones((ne, n), np.uint8)
    for e in range(ne):
        present[e][rng.choice(n, size=lost, replace=False)] = 0
    hit = {}
    for q, e in enumerate(range(3, ne, 8)):  # 8 entries: survivors in some, the surplus shard in others
        here = [i for i in range(n) if present[e][i]]
        hit[e] = here[k] if q % 3 == 2 else here[(q * 3) % k]
    assert len(hit) == 8 and {present[e].sum() for e in range(ne)} == {k + 1}
    inp, _ = c.garble(present, seed=45)
    for e, i in hit.items():
        b, o = c.shards[e][i]
        inp[b][o + int(rng.integers(sizes[e]))] ^= 1 << e % 8
    exp = dev8(md5_of(sizes, c.shards, c.bufs, n))  # what IndexDB holds: the hashes of the stored codewords
    enc = RS.New(k, m)
    t = c.upload(inp)
    plan = c.plan(enc, t)
    flags, amb, bad, where, healed, bad2 = (i32(ne) for _ in range(6))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    plan.repair_mixed(present, flags, stream=s)
    plan.locate_mixed(present, amb, flags=flags, stream=s)
    plan.hash_mixed(present, expected=exp, bad=bad, where=where, filter=flags, stream=s)
    plan.heal_mixed(present, where, healed, stream=s)
    plan.hash_mixed(None, expected=exp, bad=bad2, stream=s)
    torch.cuda.synchronize()
    f = host(flags)
    assert {e for e in range(ne) if f[e]} == set(hit) and set(f[list(hit)]) == {1}
    # the gap: one surplus shard leaves the algebraic locate with every shard a candidate
    assert [int(x) for x in B.locate_decode(k, m, present, host(amb))[list(hit)]] == [N.LOC_AMBIGUOUS] * 8
    want_b = np.zeros(ne, np.uint32)
    for e, i in hit.items():
        want_b[e] = 1 << i
    assert np.array_equal(host(bad), want_b)
    named = B.locate_decode(k, m, present, host(where))
    assert {e: int(named[e]) for e in hit} == hit
    assert all(int(named[e]) == N.LOC_CLEAN for e in range(ne) if e not in hit)
    want_h = np.zeros(ne, np.uint32)
    want_h[list(hit)] = N.HEAL_DONE | 2
    assert np.array_equal(host(healed), want_h)
    MP.check_equal(t, c.bufs)  # every shard of every entry is the oracle's codeword again
    assert not host(bad2).any()


# ---- 5. other shapes ----

@pytest.mark.parametrize("k,m", [(13, 3), (20, 4)], ids=["13+3", "20+4"])
def test_other_route_shapes_are_hashed_and_marked_skipped(k, m):
    n = k + m
    sizes = [1, 63, 0, 64, 65, 333, 1027]
    lay = Lay(k, m, sizes, False, seed=50 + k)
    ne = len(sizes)
    ref = md5_of(sizes, lay.at, lay.bufs, n)
    exp = ref.copy()
    exp[1, n - 1, 3] ^= 1
    exp[4, 0, 15] ^= 0x40
    exp[4, k, 0] ^= 2
    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    dig, bad, where = u8(ne * n * 16), i32(ne), i32(ne)
    flt = torch.from_numpy(np.array([1, 1, 1, 1, 1, 0, 1], np.int32)).cuda()
    torch.cuda.synchronize()
    plan.hash_mixed(None, digests=dig, expected=dev8(exp), bad=bad, where=where, filter=flt)
    torch.cuda.synchronize()
    want_d = ref.copy()
    want_d[2] = SENT
    want_d[5] = SENT  # filtered out
    assert np.array_equal(dig.cpu().numpy().reshape(ne, n, 16), want_d)
    want_b = np.zeros(ne, np.uint32)
    want_b[1], want_b[4] = 1 << (n - 1), 1 | (1 << k)
    assert np.array_equal(host(bad), want_b)
    # skipped, filtered or not; the empty entry stays 0
    assert np.array_equal(host(where), np.array([N.LOC_SKIPPED if s else 0 for s in sizes], np.uint32))
    assert set(B.locate_decode(k, m, None, host(where))[lay.live]) == {N.LOC_UNCHECKED}


def test_28_8_hashes_but_refuses_expected():
    k, m, n = 28, 8, 36
    sizes = [129, 0, 64, 1]
    lay = Lay(k, m, sizes, False, seed=58)
    ne = len(sizes)
    ref = md5_of(sizes, lay.at, lay.bufs, n)
    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    dig, bad = u8(ne * n * 16), i32(ne, 7)
    with pytest.raises(RS.ErrInvalidArg):
        plan.hash_mixed(None, digests=dig, expected=dev8(ref), bad=bad)
    torch.cuda.synchronize()
    assert (dig.cpu().numpy() == SENT).all() and (host(bad) == 7).all()
    plan.hash_mixed(None, digests=dig)
    torch.cuda.synchronize()
    ref[1] = SENT
    assert np.array_equal(dig.cpu().numpy().reshape(ne, n, 16), ref)


# ---- 6. argument errors on a live plan ----

def test_argument_errors_leave_the_outputs_unchanged():
    k, m, n = 4, 2, 6
    sizes = [100, 0, 333]
    lay = Lay(k, m, sizes, False, seed=60)
    ne = len(sizes)
    t = lay.upload()
    enc, other = RS.New(k, m), RS.New(8, 3)
    plan = lay.plan(enc, t)
    exp = dev8(md5_of(sizes, lay.at, lay.bufs, n) ^ 1)  # every shard would count as bad
    dig, bad, where, flt = u8(ne * n * 16), i32(ne, 0x0F0F), i32(ne, 0x1111), i32(ne, 1)
    ones = np.ones((ne, n), np.uint8)
    for kw in (dict(digests=dig, expected=exp, bad=bad, where=bad),  # aliasing, pair by pair
               dict(digests=dig, expected=exp, bad=bad, filter=bad),
               dict(digests=dig, expected=exp, bad=bad, where=where, filter=where),
               dict(digests=dig, where=where),  # where without bad
               dict(digests=dig, expected=exp)):  # expected without bad
        with pytest.raises(RS.ErrInvalidArg):
            plan.hash_mixed(ones, **kw)
    L = N.lib()
    row = np.ones(n, np.uint8)
    row11 = np.ones(11, np.uint8)

    def raw(e, rows, idx):
        idx = np.asarray(idx, np.uint32)
        return L.hbec_hash_plan_mixed(e.handle, plan._h, rows.ctypes.data_as(N._U8P), 1, idx.ctypes.data_as(U32P),
                                      C.c_void_p(flt.data_ptr()), 1, C.c_void_p(exp.data_ptr()),
                                      C.c_void_p(dig.data_ptr()), C.c_void_p(bad.data_ptr()),
                                      C.c_void_p(where.data_ptr()), None)

    assert raw(enc, row, [0, 1, 0]) == N.ERR_INVALID_ARG  # index out of range, on the zero-length entry
    assert raw(enc, row, [0, 0, 7]) == N.ERR_INVALID_ARG
    assert raw(other, row11, [0, 0, 0]) == N.ERR_INVALID_ARG  # a plan of another (k, m)
    torch.cuda.synchronize()
    assert (dig.cpu().numpy() == SENT).all()
    assert (host(bad) == 0x0F0F).all() and (host(where) == 0x1111).all() and (host(flt) == 1).all()
    assert raw(enc, row, [0, 0, 0]) == N.HBEC_OK  # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert (host(bad) == np.array([0x0F0F | 0x3F, 0x0F0F, 0x0F0F | 0x3F], np.uint32)).all()


# ---- 7. counters ----

def test_stats_count_launches_and_chains():
    k, m, n = 4, 2, 6
    sizes = [5, 0, 70, 200, 0, 64]
    lay = Lay(k, m, sizes, False, seed=70)
    ne = len(sizes)
    t = lay.upload()
    plan = lay.plan(RS.New(k, m), t)
    dig, bad, where = u8(ne * n * 16), i32(ne), i32(ne)
    exp = dev8(md5_of(sizes, lay.at, lay.bufs, n))

    def delta(fn):
        a = B.hash_plan_stats()
        fn()
        torch.cuda.synchronize()
        b = B.hash_plan_stats()
        return {f: b[f] - a[f] for f in a}

    assert delta(lambda: plan.hash_mixed(None, digests=dig)) == {"kernel_launches": 1, "chains": 4 * n}
    sel = np.zeros((ne, n), np.uint8)
    sel[0, 2] = sel[1, 3] = sel[3, 0] = sel[3, 5] = 1  # entry 1 is empty: no chain
    assert delta(lambda: plan.hash_mixed(sel, expected=exp, bad=bad, where=where)) == {"kernel_launches": 2,
                                                                                      "chains": 3}
    dig.fill_(SENT)
    assert delta(lambda: plan.hash_mixed(np.zeros((ne, n)), digests=dig, bad=bad, where=where)) == {
        "kernel_launches": 0, "chains": 0}
    assert (dig.cpu().numpy() == SENT).all() and not host(bad).any() and not host(where).any()
    empty = B.StripePlan(RS.New(k, m), stripes=[])
    assert delta(lambda: empty.hash_mixed(None)) == {"kernel_launches": 0, "chains": 0}
