"""Every length, start residue and segment cut through the plan hash kernels:
md5_plan behind StripePlan.hash_mixed, md5_files behind StripePlan.hash_files,
and their `_rows` copies behind the same calls on shards= and files= plans.

Digest-exact: every digest slot of every call against hashlib.md5 of the bytes
that lie in the slots.  Digest, bad and where arrays start as sentinels or zeros
and are compared whole, so a write outside the selected shards of the examined
entries shows.  Every call runs three times: digests alone; with the true
digests as expected= (bad and where stay zero); with one bit flipped in every
selected slot, the bit walking over all 128 (bad is exactly the selection, where
exactly the rule of include/hbec.h).  The counters' delta of every call is the
model's.  Inputs are compared with their host image afterwards.

The cases, their placement for the three plan kinds and the model of the
kernels' schedule are tests/hash_sweep_cases.py; what they cover is asserted
without a GPU in tests/test_hash_sweep_cases.py.
"""
import hashlib

import numpy as np
import pytest
import torch

import hash_sweep_cases as M
import test_gpu_hash_plan as HP
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

pytestmark = pytest.mark.gpu

SENT = M.SENT
where_word, bits_of, u8, i32, host, dev8 = HP.where_word, HP.bits_of, HP.u8, HP.i32, HP.host, HP.dev8
KS = [(kind, k, m) for kind in M.KINDS for k, m in M.SHAPES]
IDS = [f"{kind}-{k}+{m}" for kind, k, m in KS]
assert M.D == HP.D


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield
    torch.cuda.synchronize()


def fill(call, kind, seed):
    """Host images of the placement's buffers: random bytes; in a shards placement the
    slack around the shards is M.SLACK."""
    at, lens = call.place(kind)
    rng = np.random.default_rng(seed)
    bufs = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    if kind == "shards":
        lo, hi = [[] for _ in lens], [[] for _ in lens]
        for e, s in enumerate(call.sizes):
            for b, o in at[e] or ():
                lo[b].append(o)
                hi[b].append(o + s)
        for b, n in enumerate(lens):
            edge = np.zeros(n + 1, np.int32)   # +1 where a shard starts, -1 behind it: no two overlap
            np.add.at(edge, np.asarray(lo[b], np.int64), 1)
            np.add.at(edge, np.asarray(hi[b], np.int64), -1)
            bufs[b][np.cumsum(edge[:-1]) == 0] = M.SLACK
    return bufs


def make_plan(call, kind, t):
    """A zero-length entry carries a row of zeros."""
    at, _ = call.place(kind)
    enc, n, k = RS.New(call.k, call.m), call.n, call.k
    P = [x.data_ptr() for x in t]
    assert all(p % 64 == 0 for p in P)        # an offset's residue is its address's
    rows = []
    for e, s in enumerate(call.sizes):
        a = at[e]
        if kind == "stripes":
            rows.append((P[0] + a[0][1], s) if s else (0, 0))
        elif kind == "objects":
            rows.append((P[0] + a[0][1], P[1] + a[k][1], s) if s else (0, 0, 0))
        else:
            rows.append(([P[b] + o for b, o in a], s) if s else ([0] * n, 0))
    return B.StripePlan(enc, **{kind: rows})


def delta(fn, call):
    a = fn()
    call()
    torch.cuda.synchronize()
    b = fn()
    return {x: b[x] - a[x] for x in a}


def flipped(ref, slots):
    """ref with one bit flipped in every slot of `slots`, the bit walking over all 128"""
    out = ref.copy()
    for q, (r, j) in enumerate(slots):
        out[r, j, (q % 128) // 8] ^= 1 << (q % 8)
    return out


def sweep(call, kind, seed):
    """The three runs of one call; fails naming the first wrong slots."""
    n, ne, nr = call.n, len(call.sizes), call.n_rows
    bufs = fill(call, kind, seed)
    t = [torch.from_numpy(x).cuda() for x in bufs]
    plan = make_plan(call, kind, t)
    chains = call.chains()
    live = [(r, j) for r, j in chains if call.examined(r)]
    raw = [x.tobytes() for x in bufs]
    ref = np.zeros((max(1, nr), n, 16), np.uint8)
    for r, j in chains:
        h = hashlib.md5()
        for b, o, ln in call.segs(kind, r, j):
            h.update(raw[b][o:o + ln])
        ref[r, j] = np.frombuffer(h.digest(), np.uint8)
    want_d = np.full_like(ref, SENT)
    sel_bits = np.zeros(max(1, nr), np.uint32)
    for r, j in live:
        want_d[r, j] = ref[r, j]
        sel_bits[r] |= 1 << j
    row_sel = [bits_of(call.row(r)) for r in range(nr)]
    want_w = np.zeros(max(1, ne), np.uint32)   # with every selected slot bad
    for r in range(nr):
        if call.total(r) and call.examined(r):
            for e in call.entries_of(r):
                if call.sizes[e] and call.passes(e):
                    want_w[e] = where_word(row_sel[r], int(sel_bits[r]))
    n_chains, n_segs = call.stats()
    want_stats = {"kernel_launches": 1 if chains else 0, "chains": n_chains}
    if call.files:
        want_stats["segments"] = n_segs
    stats = B.hash_files_stats if call.files else B.hash_plan_stats
    flt = None if call.flt is None else torch.from_numpy(np.asarray(call.flt, np.uint32).view(np.int32).copy()).cuda()
    select = None if call.select is None else np.asarray(call.select, np.uint8).reshape(nr, n)
    starts = np.asarray(call.starts, np.uint32) if call.files else None

    def run(**kw):
        if call.files:
            plan.hash_files(starts, select, filter=flt, filter_bits=call.fbits, **kw)
        else:
            plan.hash_mixed(select, filter=flt, filter_bits=call.fbits, **kw)

    def check_digests(dig, phase):
        got = dig.cpu().numpy().reshape(ref.shape)
        wrong = np.argwhere((got != want_d).any(axis=2))
        if len(wrong):
            r, j = (int(x) for x in wrong[0])
            state = "written but not selected or not examined" if (r, j) not in live else "wrong digest"
            what = call.describe(kind, r, j) if call.total(r) else f"{call.name} [{kind}] row {r} shard {j} (no byte)"
            pytest.fail(f"{phase}: {len(wrong)} slots differ; first: {state}: {what}: "
                        f"{bytes(got[r, j]).hex()} != {bytes(want_d[r, j]).hex()}")

    torch.cuda.synchronize()
    # 1. digests alone
    dig = u8(ref.size)
    assert delta(stats, lambda: run(digests=dig)) == want_stats, call.name
    check_digests(dig, "digests")
    # 2. the true digests as expected=: nothing is bad
    if chains:
        want_stats["kernel_launches"] = 2
    dig, bad, where = u8(ref.size), i32(max(1, nr)), i32(max(1, ne))
    assert delta(stats, lambda: run(digests=dig, expected=dev8(ref), bad=bad, where=where)) == want_stats, call.name
    check_digests(dig, "expected=true")
    assert not host(bad).any() and not host(where).any(), call.name
    # 3. one bit flipped in every selected slot
    bad, where = i32(max(1, nr)), i32(max(1, ne))
    exp = flipped(ref, chains)
    assert delta(stats, lambda: run(expected=dev8(exp), bad=bad, where=where)) == want_stats, call.name
    got_b, got_w = host(bad), host(where)
    for r in np.flatnonzero(got_b != sel_bits):
        j = int(got_b[r] ^ sel_bits[r]).bit_length() - 1
        pytest.fail(f"flipped: bad[{r}] = {int(got_b[r]):#x}, want {int(sel_bits[r]):#x}: "
                    f"{call.describe(kind, int(r), j) if call.total(int(r)) else call.name}")
    assert np.array_equal(got_w, want_w), (call.name, np.flatnonzero(got_w != want_w)[:6])
    if flt is not None:
        assert np.array_equal(host(flt), np.asarray(call.flt, np.uint32))
    for x, y in zip(t, bufs):
        assert np.array_equal(x.cpu().numpy(), y), call.name   # read only
    return len(live)


# ---- P. md5_plan and md5_plan_rows -----------------------------------------------------------
@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_p1_every_length_at_every_start_residue(kind, k, m):
    assert sweep(M.p1_call(k, m), kind, 1000 + k) == (16 * M.P_MAX + M.P1_EXTRA) * (k + m)


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_p2_what_one_wave_mixes(kind, k, m):
    for i, call in enumerate(M.p2_calls(k, m)):
        examined = sweep(call, kind, 2000 + 16 * k + i)
        assert (examined == 0) == (call.name == "P2.nothing_examined")


# ---- F. md5_files and md5_files_rows -----------------------------------------------------------
@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_f1_a_cut_in_every_slot_trip_and_offset(kind, k, m):
    assert sweep(M.f1_call(k, m), kind, 3000 + k) == 3 * M.SLOTS * 63 * (k + m)


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_f2_every_pair_of_shifts_across_a_boundary(kind, k, m):
    assert sweep(M.f2_call(k, m), kind, 4000 + k) == 7 * 16 * (k + m)


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_f3_spans_zero_length_entries_and_runs(kind, k, m):
    assert sweep(M.f3_call(k, m), kind, 5000 + k) > 0


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_f4_every_tail_over_every_span(kind, k, m):
    assert sweep(M.f4_call(k, m), kind, 6000 + k) > 0


@pytest.mark.parametrize("kind,k,m", KS, ids=IDS)
def test_f5_waves(kind, k, m):
    for i, call in enumerate(M.f5_calls(k, m)):
        assert sweep(call, kind, 7000 + 16 * k + i) > 0


@pytest.mark.parametrize("k,m", M.SHAPES, ids=["4+2", "8+3"])
def test_f6_files_plans_of_every_chunk_size(k, m):
    """files= plans: the library cuts the files into entries; the expected digest is
    hashlib's of each file's bytes as they lie, whatever the pieces."""
    n = k + m
    enc = RS.New(k, m)
    rng = np.random.default_rng(8000 + k)
    for chunk in M.F6_CHUNKS:
        lengths, cuts, offs, size = M.f6_layout(k, m, chunk)
        no, ne = len(lengths), sum(len(c) for c in cuts)
        buf = rng.integers(0, 256, size, dtype=np.uint8)
        t = torch.from_numpy(buf).cuda()
        assert t.data_ptr() % 64 == 0
        plan = B.StripePlan(enc, files=[([t.data_ptr() + o for o in offs[g]], lengths[g]) for g in range(no)],
                            chunk_size=chunk)
        starts = np.cumsum([0] + [len(c) for c in cuts])
        assert plan.object_start.tolist() == starts.tolist(), chunk
        raw = buf.tobytes()
        ref = np.zeros((no, n, 16), np.uint8)
        for g in range(no):
            for j in range(n):
                ref[g, j] = np.frombuffer(hashlib.md5(raw[offs[g][j]:offs[g][j] + sum(cuts[g])]).digest(), np.uint8)
        want_stats = {"kernel_launches": 1, "chains": no * n, "segments": ne * n}
        dig = u8(ref.size)
        assert delta(B.hash_files_stats, lambda: plan.hash_files(plan.object_start, None, digests=dig)) == want_stats
        got = dig.cpu().numpy().reshape(ref.shape)
        for g, j in np.argwhere((got != ref).any(axis=2))[:1]:
            s = M.Sched([(offs[g][j] + i * chunk, x) for i, x in enumerate(cuts[g])])
            pytest.fail(f"chunk_size {chunk}, {k}+{m}: content length {lengths[g]}, pieces {cuts[g]}, file {j}, "
                        f"start residue {offs[g][j] % 16}, first cut block {s.first_cut()}: "
                        f"{bytes(got[g, j]).hex()} != {bytes(ref[g, j]).hex()}")
        want_stats["kernel_launches"] = 2
        bad, where = i32(no), i32(ne)
        assert delta(B.hash_files_stats, lambda: plan.hash_files(plan.object_start, None, expected=dev8(ref), bad=bad,
                                                                 where=where)) == want_stats
        assert not host(bad).any() and not host(where).any(), chunk
        bad, where = i32(no), i32(ne)
        exp = flipped(ref, [(g, (j + chunk) % n) for g in range(no) for j in range(n)])
        assert delta(B.hash_files_stats, lambda: plan.hash_files(plan.object_start, None, expected=dev8(exp), bad=bad,
                                                                 where=where)) == want_stats
        assert host(bad).tolist() == [(1 << n) - 1] * no, chunk
        assert host(where).tolist() == [where_word((1 << n) - 1, (1 << n) - 1)] * ne, chunk
        assert np.array_equal(t.cpu().numpy(), buf), chunk


# ---- L. the bit count's upper word ---------------------------------------------------------------
@pytest.mark.slow
def test_l1_hash_files_bit_count_above_32_bits():
    """512 MiB + 1 through one md5_files lane: eight 64 MiB pieces of one buffer from
    different first bytes, then one byte.  The 1+1 entries overlap each other; the call
    only reads them, and only file 0 is selected."""
    rng = np.random.default_rng(90)
    buf = rng.integers(0, 256, M.L_BUFFER, dtype=np.uint8)
    t = torch.from_numpy(buf).cuda()
    P = t.data_ptr()
    assert P % 64 == 0
    stripes = [(P + o, M.L_PIECE) for o in M.L_OFFSETS] + [(P + M.L_LAST, 1)]
    plan = B.StripePlan(RS.New(1, 1), stripes=stripes)
    ref = hashlib.md5()   # fed piecewise instead of from a 512 MiB copy
    mv = memoryview(buf)
    for o in M.L_OFFSETS:
        ref.update(mv[o:o + M.L_PIECE])
    ref.update(mv[M.L_LAST:M.L_LAST + 1])
    want = np.frombuffer(ref.digest(), np.uint8)
    exp = np.zeros((1, 2, 16), np.uint8)
    exp[0, 0] = want
    dig, bad, where = u8(32), i32(1), i32(9)
    d = delta(B.hash_files_stats, lambda: plan.hash_files([0, 9], [[1, 0]], digests=dig, expected=dev8(exp), bad=bad,
                                                          where=where))
    assert d == {"kernel_launches": 2, "chains": 1, "segments": 9}
    got = dig.cpu().numpy().reshape(2, 16)
    assert bytes(got[0]).hex() == ref.hexdigest(), f"{M.L_TOTAL} bytes, bit count {M.L_TOTAL * 8:#x}"
    assert (got[1] == SENT).all() and not host(bad).any() and not host(where).any()
    assert np.array_equal(t.cpu().numpy(), buf)


@pytest.mark.slow
def test_l2_hash_mixed_bit_count_above_32_bits():
    """512 MiB + 1 through one md5_plan lane: shard 0 of one 1+1 entry, filled on the
    device from a 64 MiB host pool repeated."""
    rng = np.random.default_rng(91)
    pool = rng.integers(0, 256, M.L_PIECE, dtype=np.uint8)
    dpool = torch.from_numpy(pool).cuda()
    t = torch.zeros(M.L2_BASE + 2 * M.L_TOTAL + 64, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 64 == 0
    reps = len(M.L_OFFSETS)
    for i in range(reps):
        t[M.L2_BASE + i * M.L_PIECE:M.L2_BASE + (i + 1) * M.L_PIECE] = dpool
    t[M.L2_BASE + reps * M.L_PIECE] = int(pool[M.L_LAST])
    plan = B.StripePlan(RS.New(1, 1), stripes=[(t.data_ptr() + M.L2_BASE, M.L_TOTAL)])
    ref = hashlib.md5()
    for _ in range(reps):
        ref.update(memoryview(pool))
    ref.update(memoryview(pool)[M.L_LAST:M.L_LAST + 1])
    exp = np.zeros((1, 2, 16), np.uint8)
    exp[0, 0] = np.frombuffer(ref.digest(), np.uint8)
    dig, bad, where = u8(32), i32(1), i32(1)
    torch.cuda.synchronize()
    d = delta(B.hash_plan_stats, lambda: plan.hash_mixed([[1, 0]], digests=dig, expected=dev8(exp), bad=bad,
                                                         where=where))
    assert d == {"kernel_launches": 2, "chains": 1}
    got = dig.cpu().numpy().reshape(2, 16)
    assert bytes(got[0]).hex() == ref.hexdigest(), f"{M.L_TOTAL} bytes, bit count {M.L_TOTAL * 8:#x}"
    assert (got[1] == SENT).all() and not host(bad).any() and not host(where).any()
    for i in range(reps):   # read only
        assert torch.equal(t[M.L2_BASE + i * M.L_PIECE:M.L2_BASE + (i + 1) * M.L_PIECE], dpool)
    assert int(t[M.L2_BASE + reps * M.L_PIECE]) == int(pool[M.L_LAST]) and not int(t[:M.L2_BASE].max())
