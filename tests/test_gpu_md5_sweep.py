"""Every length, carry and alignment through the MD5 chain kernels (md5.hip:
md5_chains<ALIGNED, D>, md5_list<ALIGNED>) by way of every host entry that
launches them (shardhash.cpp): one-shot batches, streaming chains, device
lists, the host auditor pass and the encode + hash segment pipeline.

Digest-exact: every chain of every call against hashlib.md5 of the same host
bytes (oracle.shard_hash; parity against the C oracle).  Digest buffers are one
object-row longer than needed and start as sentinel bytes, and the whole buffer
is compared, so a digest written to another slot shows twice.  Inputs are
compared with their host image afterwards.  Which kernel ran is read from
shardhash.md5_route_stats() around every call and compared with the rule
restated in tests/md5_sweep_cases.py, which also holds the cases and whose
coverage tests/test_md5_sweep_cases.py asserts without a GPU.
"""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import md5_sweep_cases as M
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from hummingbird_amd import shardhash as H
from oracle import coracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KEYS = ("chains_aligned", "chains_unaligned", "list_aligned", "list_unaligned")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield
    torch.cuda.synchronize()


def stats():
    s = H.md5_route_stats()
    return tuple(s[k] for k in KEYS)


def delta(s0, s1):
    return tuple(b - a for a, b in zip(s0, s1))


def pool(size, seed):
    """(host bytes, the same on the device at a multiple of 64)"""
    host = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    assert dev.data_ptr() % 64 == 0
    return host, dev


def md5(mv, off, n):
    return bytes.fromhex(O.shard_hash(mv[off:off + n]))


def sentinel(*shape):
    return torch.full(shape, M.SENT, dtype=torch.uint8, device="cuda")


def digests_of(mv, starts, n, shape):
    """hashlib digests of the n bytes at every start, as uint8 [*shape, 16]"""
    return np.frombuffer(b"".join(md5(mv, s, n) for s in starts), np.uint8).reshape(*shape, 16)


def bad_slots(got, want):
    """index tuples of the first digest slots that differ"""
    return [tuple(int(x) for x in i) for i in np.argwhere((got != want).any(axis=-1))[:6]]


def unchanged(dev, host):
    return np.array_equal(dev.cpu().numpy(), host)


# ---- a. one-shot, unaligned kernel -------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 300), (301, 600), (601, 900)])
def test_a_oneshot_every_length_unaligned(lo, hi):
    host, dev = pool(M.A_POOL, 1)
    nv, no, lens = len(M.A_BASES), M.A_NOBJ, range(lo, hi + 1)
    views = [(dev.data_ptr() + b, M.A_STRIDE) for b in M.A_BASES]
    out = sentinel(len(lens), no + 1, nv, 16)
    s0 = stats()
    for i, n in enumerate(lens):
        H.md5_views(views, no, n, digests=out[i])
        s1 = stats()
        assert delta(s0, s1) == (0, 1, 0, 0), f"len {n}: launches {delta(s0, s1)}, want one md5_chains<false>"
        s0 = s1
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    mv = memoryview(host)
    want = np.full_like(got, M.SENT)
    for i, n in enumerate(lens):
        want[i, :no] = digests_of(mv, [b + o * M.A_STRIDE for o in range(no) for b in M.A_BASES], n, (no, nv))
    for i, o, v in bad_slots(got, want):
        b, r = M.blocks_rest(lens[i])
        pytest.fail(f"len {lens[i]} ({b} blocks + {r}), view {v}, object {o} "
                    f"(base residue {(M.A_BASES[v] + o * M.A_STRIDE) % 16}"
                    f"{', a slot past the last object' if o == no else ''}): "
                    f"{bytes(got[i, o, v]).hex()} != {bytes(want[i, o, v]).hex()}")
    assert unchanged(dev, host)


# ---- b. one-shot, aligned kernel ---------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0, 450), (451, 900)])
def test_b_oneshot_every_length_aligned(lo, hi):
    host, dev = pool(M.B_POOL, 2)
    nv, nmax, lens = len(M.B_BASES), max(M.B_NOBJS), range(lo, hi + 1)
    views = [(dev.data_ptr() + b, M.B_STRIDE) for b in M.B_BASES]
    out = sentinel(len(lens), nmax + 1, nv, 16)
    s0 = stats()
    for i, n in enumerate(lens):
        H.md5_views(views, M.b_nobj(n), n, digests=out[i])
        s1 = stats()
        assert delta(s0, s1) == (1, 0, 0, 0), f"len {n}: launches {delta(s0, s1)}, want one md5_chains<true>"
        s0 = s1
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    mv = memoryview(host)
    want = np.full_like(got, M.SENT)
    for i, n in enumerate(lens):
        no = M.b_nobj(n)
        want[i, :no] = digests_of(mv, [b + o * M.B_STRIDE for o in range(no) for b in M.B_BASES], n, (no, nv))
    for i, o, v in bad_slots(got, want):
        b, r = M.blocks_rest(lens[i])
        pytest.fail(f"len {lens[i]} ({b} blocks + {r}), {M.b_nobj(lens[i])} objects, view {v}, object {o} "
                    f"(base residue {(M.B_BASES[v] + o * M.B_STRIDE) % 64} mod 64): "
                    f"{bytes(got[i, o, v]).hex()} != {bytes(want[i, o, v]).hex()}")
    assert unchanged(dev, host)


# ---- c. view splitting -------------------------------------------------------------------
@pytest.mark.parametrize("n_obj", M.C_NOBJS)
@pytest.mark.parametrize("n_views", M.C_NVIEWS)
def test_c_oneshot_more_than_32_views(n_views, n_obj):
    offs, stride = M.c_layout(n_views)
    host, dev = pool(n_obj * stride + 16, 3 + n_views)
    views = [(dev.data_ptr() + o, stride) for o in offs]
    out = sentinel(len(M.C_LENGTHS), n_obj + 1, n_views, 16)
    for i, n in enumerate(M.C_LENGTHS):
        s0 = stats()
        H.md5_views(views, n_obj, n, digests=out[i])
        assert delta(s0, stats()) == (M.launches(n_views), 0, 0, 0), (n, n_views)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    mv = memoryview(host)
    want = np.full_like(got, M.SENT)
    for i, n in enumerate(M.C_LENGTHS):
        want[i, :n_obj] = digests_of(mv, [b + o * stride for o in range(n_obj) for b in offs], n, (n_obj, n_views))
    for i, o, v in bad_slots(got, want):
        pytest.fail(f"{n_views} views, {n_obj} objects, len {M.C_LENGTHS[i]}: view {v} (launch {v // 32}), "
                    f"object {o}: {bytes(got[i, o, v]).hex()} != {bytes(want[i, o, v]).hex()}")
    assert unchanged(dev, host)


@pytest.mark.parametrize("n_obj", M.C_NOBJS)
@pytest.mark.parametrize("n_views", M.C_NVIEWS)
def test_c_streaming_more_than_32_views(n_views, n_obj):
    offs, stride = M.c_layout(n_views)
    host, dev = pool(n_obj * stride + 16, 30 + n_views)
    out = sentinel(n_obj + 1, n_views, 16)
    ch = H.MD5Chains(n_views, n_obj)
    for u, total, n, aligned in M.c_stream_steps(n_views):
        s0 = stats()
        if u is None:
            ch.final(digests=out)
        else:
            ch.update([(dev.data_ptr() + o + total, stride) for o in offs], u)
        assert delta(s0, stats()) == ((n, 0, 0, 0) if aligned else (0, n, 0, 0)), (u, total, n_views)
    torch.cuda.synchronize()
    ch.close()
    got = out.cpu().numpy()
    want = np.full_like(got, M.SENT)
    want[:n_obj] = digests_of(memoryview(host), [b + o * stride for o in range(n_obj) for b in offs],
                              sum(M.C_UPDATES), (n_obj, n_views))
    for o, v in bad_slots(got, want):
        pytest.fail(f"{n_views} views, {n_obj} objects, updates {list(M.C_UPDATES)}: view {v} (launch {v // 32}), "
                    f"object {o}: {bytes(got[o, v]).hex()} != {bytes(want[o, v]).hex()}")
    assert unchanged(dev, host)


# ---- d. streaming carry ------------------------------------------------------------------
# (aligned kernel?, bytes carried?) a class's launches can show (md5_sweep_cases.d_offset)
D_COMBOS = {"A": {(True, False), (True, True), (False, True)},
            "U": {(True, False), (True, True)},
            "M": {(False, False), (False, True)}}


def run_chains(cls, chains):
    """Feed `chains` through one context at class `cls` placements, checking the
    kernel of every step and every digest; returns the (kernel, carry) combinations seen."""
    host, dev = pool(M.D_POOL, 40 + ord(cls))
    P = dev.data_ptr()
    no, nv = M.D_NOBJ, M.D_NVIEWS
    out = sentinel(len(chains), no + 1, nv, 16)
    parts = [[[] for _ in range(no * nv)] for _ in chains]  # per chain and (o, v): (offset, length) fed
    seen = set()
    ch = H.MD5Chains(nv, no)
    s0 = stats()
    for ci, ui, u, total, offs, n, aligned in M.d_steps(cls, chains):
        if ui is None:
            ch.final(digests=out[ci])
        else:
            ch.update([(P + o, M.D_STRIDE) for o in offs], u)
            for o in range(no):
                for v in range(nv):
                    parts[ci][o * nv + v].append((offs[v] + o * M.D_STRIDE, u))
        s1 = stats()
        assert delta(s0, s1) == ((n, 0, 0, 0) if aligned else (0, n, 0, 0)), \
            (f"class {cls}, chain {list(chains[ci])}, {'final' if ui is None else f'update {ui} of {u} bytes'}, "
             f"carry {total & 63}, base residues {[x % 16 for x in offs]}: launches {delta(s0, s1)}, "
             f"want {n} of md5_chains<{str(aligned).lower()}>")
        s0 = s1
        if n and ui is not None:
            seen.add((aligned, (total & 63) != 0))
    torch.cuda.synchronize()
    ch.close()
    got = out.cpu().numpy()
    raw = host.tobytes()
    want = np.full_like(got, M.SENT)
    for ci in range(len(chains)):
        msgs = [b"".join(raw[a:a + n] for a, n in p) for p in parts[ci]]
        want[ci, :no] = np.frombuffer(b"".join(bytes.fromhex(O.shard_hash(m)) for m in msgs),
                                      np.uint8).reshape(no, nv, 16)
    for ci, o, v in bad_slots(got, want):
        pairs = list(M.chain_pairs(chains[ci]))
        pytest.fail(f"class {cls}, chain {ci} updates {list(chains[ci])} (carry, carry + len: {pairs}), view {v}, "
                    f"object {o}{' (a slot past the last object)' if o == no else ''}, base residues "
                    f"{[a % 16 for a, _ in parts[ci][min(o, no - 1) * nv + v]]}: "
                    f"{bytes(got[ci, o, v]).hex()} != {bytes(want[ci, o, v]).hex()}")
    assert unchanged(dev, host)
    return seen


@pytest.mark.parametrize("cls", M.D_CLASSES)
def test_d_streaming_every_carry_and_length(cls):
    assert run_chains(cls, M.pair_chains()) == D_COMBOS[cls]


@pytest.mark.parametrize("cls", M.D_CLASSES)
def test_d_streaming_two_updates_within_a_block(cls):
    assert run_chains(cls, M.triple_chains()) == D_COMBOS[cls]


def test_d_streaming_edge_chains_and_all_four_routes():
    """Zero-length updates first and mid-chain, final() with no update, the
    context reused after every final(); over the three placements every kernel
    is seen with and without carried bytes."""
    seen = set()
    for cls in M.D_CLASSES:
        got = run_chains(cls, M.EDGE_CHAINS)
        assert got <= D_COMBOS[cls]
        seen |= got
    assert seen == {(True, True), (True, False), (False, True), (False, False)}
    # a fresh context per chain as well
    for chain in M.EDGE_CHAINS:
        run_chains("A", (chain,))


# ---- e. md5_list lane mixing -------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
def test_e_list_lane_mixing(aligned):
    for name, lens in M.list_cases():
        offs, size = M.list_offsets(lens, aligned)
        host, dev = pool(size, 50 + len(lens))
        n = len(lens)
        out = sentinel(n + 1, 16)
        s0 = stats()
        H.md5_list([(dev.data_ptr() + o, ln) for o, ln in zip(offs, lens)], digests=out)
        want_launch = (0, 0, 1, 0) if aligned else (0, 0, 0, 1)
        assert delta(s0, stats()) == want_launch, name
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        mv = memoryview(host)
        want = np.full_like(got, M.SENT)
        want[:n] = np.frombuffer(b"".join(md5(mv, o, ln) for o, ln in zip(offs, lens)), np.uint8).reshape(n, 16)
        order = sorted(range(n), key=lambda i: -lens[i])  # the host's lane order (stable, longest first)
        for (i,) in bad_slots(got, want):
            lane = order.index(i) if i < n else -1
            pytest.fail(f"{name} ({'aligned' if aligned else 'unaligned'}): buffer {i} of {n}, len "
                        f"{lens[i] if i < n else 'none: the slot past the last'}, address residue "
                        f"{offs[i] % 16 if i < n else '-'}, lane {lane % 64} of wave {lane // 64}, wave's longest "
                        f"{lens[order[lane // 64 * 64]] if i < n else '-'}: "
                        f"{bytes(got[i]).hex()} != {bytes(want[i]).hex()}")
        assert unchanged(dev, host), name


# ---- f. bit count above 32 bits ----------------------------------------------------------
@pytest.mark.slow
def test_f_bit_count_above_32_bits():
    """512 MiB + 1 through one chain: the only way to a non-zero upper word of
    the bit count.  Eight updates of one 64 MiB buffer from different first
    bytes, then one byte."""
    host, dev = pool(M.F_LEN + 64, 60)
    P = dev.data_ptr()
    out = sentinel(2, 1, 16)
    ch = H.MD5Chains(1, 1)
    ref = hashlib.md5()  # oracle.shard_hash's function, fed piecewise instead of from a 512 MiB copy
    mv = memoryview(host)
    for off in M.F_OFFSETS:
        s0 = stats()
        ch.update([(P + off, 0)], M.F_LEN)
        assert delta(s0, stats()) == ((1, 0, 0, 0) if off % 16 == 0 else (0, 1, 0, 0)), off
        ref.update(mv[off:off + M.F_LEN])
    ch.update([(P + 7, 0)], 1)
    ref.update(mv[7:8])
    ch.final(digests=out)
    torch.cuda.synchronize()
    ch.close()
    got = out.cpu().numpy()
    assert bytes(got[0, 0]).hex() == ref.hexdigest(), f"{M.F_TOTAL} bytes, bit count {M.F_TOTAL * 8:#x}"
    assert (got[1] == M.SENT).all()
    assert unchanged(dev, host)


# ---- g. segment pipeline -----------------------------------------------------------------
def encode_md5_case(k, m, S):
    no, n = M.G_NOBJ, k + m
    enc = RS.New(k, m)
    host = np.random.default_rng(S * 16 + k).integers(0, 256, (no, k * S), dtype=np.uint8)
    objs = torch.from_numpy(host).cuda()
    garbage = np.random.default_rng(S).integers(0, 256, (no + 1, m * S), dtype=np.uint8)
    par = torch.from_numpy(garbage).cuda()
    out = sentinel(no + 1, n, 16)
    views = B.shard_views(objs, k, S) + B.shard_views(par[:no], m, S)
    segs = M.segments(S, k)
    aligned = M.expect_aligned([b for b, _ in views], [s for _, s in views], 0)  # segments are 4 KiB multiples
    s0 = stats()
    H.encode_md5_views(enc, views, no, S, digests=out)
    d = delta(s0, stats())
    assert d == ((len(segs), 0, 0, 0) if aligned else (0, len(segs), 0, 0)), (k, m, S, segs)
    torch.cuda.synchronize()
    want_par, _ = CO.encode_batch(k, m, host)
    got_par = par.cpu().numpy()
    if not np.array_equal(got_par[:no], want_par):
        o, x = (int(i) for i in np.argwhere(got_par[:no] != want_par)[0])
        pytest.fail(f"{k}+{m} S {S} (segments {segs}): parity of object {o}, shard {k + x // S}, byte {x % S} "
                    f"(segment {x % S // segs[0]}): {got_par[o, x]:#x} != {want_par[o, x]:#x}")
    assert np.array_equal(got_par[no], garbage[no]), (k, m, S, "parity row past the last object written")
    got = out.cpu().numpy()
    want = np.full_like(got, M.SENT)
    for o in range(no):
        shards = [host[o, j * S:(j + 1) * S] for j in range(k)] + [want_par[o, r * S:(r + 1) * S] for r in range(m)]
        want[o] = np.frombuffer(b"".join(bytes.fromhex(O.shard_hash(x)) for x in shards), np.uint8).reshape(n, 16)
    for o, v in bad_slots(got, want):
        pytest.fail(f"{k}+{m} S {S} (segments {segs}, last ends {S % 64} past a block), object {o}, shard {v}"
                    f"{' (parity)' if v >= k else ''}, row stride residue {k * S % 16}: "
                    f"{bytes(got[o, v]).hex()} != {bytes(want[o, v]).hex()}")
    assert np.array_equal(objs.cpu().numpy(), host)


@pytest.mark.parametrize("k,m", M.G_PIPELINED)
def test_g_segment_pipeline(k, m):
    for S in M.G_SIZES:
        encode_md5_case(k, m, S)


def test_g_single_segment_above_four_data_shards():
    (k, m), sizes = M.G_SINGLE
    for S in sizes:
        encode_md5_case(k, m, S)


# ---- h. hbec_md5_host --------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in M.host_cases()])
def test_h_host_auditor_pass(name):
    lens = dict(M.host_cases())[name]
    n = len(lens)
    starts = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64) + 1)])  # a byte between neighbours
    host = np.random.default_rng(70 + n).integers(0, 256, int(starts[-1]) + 16, dtype=np.uint8)
    image = host.copy()
    base = host.ctypes.data
    ptrs = (C.c_void_p * n)(*[base + int(s) for s in starts[:n]])
    clens = (C.c_uint64 * n)(*lens)
    out = np.full((n + 1, 16), M.SENT, np.uint8)
    s0 = stats()
    RS.check(N.lib().hbec_md5_host(ptrs, clens, n, out.ctypes.data_as(C.POINTER(C.c_uint8))))
    assert delta(s0, stats()) == (0, 0, M.host_chunks(lens), 0), name
    mv = memoryview(image)
    want = np.full_like(out, M.SENT)
    want[:n] = np.frombuffer(b"".join(md5(mv, int(s), ln) for s, ln in zip(starts, lens)), np.uint8).reshape(n, 16)
    for (i,) in bad_slots(out, want):
        pytest.fail(f"{name}: buffer {i} of {n}, len {lens[i] if i < n else 'none: the slot past the last'}: "
                    f"{bytes(out[i]).hex()} != {bytes(want[i]).hex()}")
    assert np.array_equal(host, image)
