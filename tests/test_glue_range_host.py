"""The ranged glue calls without a device: the new symbols of libhbec.so, every
argument error of hbec_glue_plan_range and hbec_glue_plan_files_range with its
code, precedence and message keyword (all found before anything is queued), the
cut of an object's range into its entries' against oracle.ec_glue_range's
slicing, csrc/gluerange.h alone under AddressSanitizer + UBSan
(tests/native/gluerange_host.cpp, a stand-alone program that links no libhbec),
and the resources of the gf_range_plan instances from the library's code-object
metadata.

As in tests/test_glue_host.py, plans of zero-length entries need no device
memory, and the errors that need an entry with bytes in it are checked on shards
plans whose addresses are compared and never followed: `range_errors` returns
False where no device can keep their address rows, and
tests/test_gpu_glue_range_plan.py runs it again where one is."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_glue_host as GH
import test_kernel_resources as KR
import test_repair_mixed_host as RH
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS
from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "gluerange_host.cpp"
NEW = ["hbec_glue_plan_range", "hbec_glue_plan_files_range", "hbec_glue_range_stats", "hbec_glue_range_tile_bytes",
       "hbec_set_glue_range_chunk_tiles"]
K, M = GH.K, GH.M
U32P, U64P = GH.U32P, GH.U64P
FULL, LOST0, FEW, BASE, FAR = GH.FULL, GH.LOST0, GH.FEW, GH.BASE, GH.FAR


def test_new_symbols_are_exported_and_declared():
    lib = N.lib()
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS and f" {name}(" in header, name
        decl = header[:header.index(f" {name}(")]
        if "plan" in name:  # each entry's comment cites the reference
            comment = decl[decl.rindex("/*"):]
            assert "ecobj.go:207-267" in comment and "ecutils.go:134-186" in comment, name
    assert lib.hbec_version() == 2  # additive
    for name in ("glue_range_stats", "glue_range_tile_bytes", "set_glue_range_chunk_tiles"):
        assert hasattr(B, name), name
    assert hasattr(B.StripePlan, "glue_range") and hasattr(B.StripePlan, "glue_range_files")


@pytest.fixture(scope="module")
def range_host(tmp_path_factory):
    """tests/native/gluerange_host.cpp built with AddressSanitizer + UBSan: a program of its own."""
    text = SRC.read_text()
    assert "csrc/gluerange.h" in text and "hbec.h" not in text and "int main(" in text
    assert text.count("#include \"") == 1  # the header alone
    exe = tmp_path_factory.mktemp("gluerange_host") / "gluerange_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


def test_range_host_logic_under_sanitizers(range_host):
    out = subprocess.run([str(range_host)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = re.search(r"gluerange_host ok \((\d+) windows, (\d+) tiles, (\d+) blocks, (\d+) randoms, (\d+) cuts\)",
                    out.stdout)
    assert got, out.stdout
    # every (S, k, s, e) with S <= 40 and k <= 4: sum over S, k of k (k S + 1)(k S + 2) / 2 windows
    assert int(got.group(1)) == sum(k * (k * s + 1) * (k * s + 2) // 2 for s in range(1, 41) for k in range(1, 5))
    assert int(got.group(2)) > 1000000 and int(got.group(3)) > 100000
    assert int(got.group(4)) == 200000 and int(got.group(5)) > 100000


def _call(enc, plan, patterns, pattern_of, dsts=None, starts=None, lens=None, n_patterns=None, null=(), n=5):
    """hbec_glue_plan_range on host arrays."""
    pat = np.ascontiguousarray(patterns, dtype=np.uint8).reshape(-1, K + M)
    idx = np.ascontiguousarray(pattern_of, dtype=np.uint32)
    d = (C.c_void_p * max(1, n))(*[int(a) for a in (dsts if dsts is not None else [0] * n)])
    st, ln = np.zeros(max(1, n), np.uint64), np.zeros(max(1, n), np.uint64)
    if starts is not None:
        st[:n] = starts
    if lens is not None:
        ln[:n] = lens
    return N.lib().hbec_glue_plan_range(
        None if "codec" in null else enc.handle, None if "plan" in null else plan._h,
        None if "patterns" in null else pat.ctypes.data_as(N._U8P),
        pat.shape[0] if n_patterns is None else n_patterns, None if "pattern_of" in null else idx.ctypes.data_as(U32P),
        None if "dsts" in null else d, None if "starts" in null else st.ctypes.data_as(U64P),
        None if "lens" in null else ln.ctypes.data_as(U64P), None)


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_null_arguments(kind):
    enc = RS.New(K, M)
    plan = GH._plan(enc, kind=kind)
    for null in ("codec", "plan", "patterns", "pattern_of", "dsts", "starts", "lens"):
        assert _call(enc, plan, [LOST0], [0] * 5, null=(null,)) == N.ERR_INVALID_ARG, null
        assert "null" in N.last_error(), null
    empty = GH._plan(enc, 0, kind=kind)  # for a plan of no entries too
    for null in ("dsts", "starts", "lens"):
        assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32), null=(null,), n=0) == N.ERR_INVALID_ARG
    a = C.c_uint64()
    assert N.lib().hbec_glue_range_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert N.lib().hbec_glue_range_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert N.last_error()


def test_pattern_errors_are_those_of_reconstruct_with_their_precedence():
    enc = RS.New(K, M)
    plan = GH._plan(enc)
    other = GH._plan(RS.New(8, 3))
    assert _call(enc, other, [LOST0], [0] * 5) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    # reported before a bad pattern count or index, and before a bad range
    assert _call(enc, other, [LOST0], [7] * 5, lens=[9] * 5, n_patterns=0) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    assert _call(enc, plan, [LOST0], [0] * 5, n_patterns=0) == N.ERR_INVALID_ARG  # entries, no patterns
    assert "no patterns" in N.last_error()
    big = np.ones((65537, K + M), np.uint8)
    assert _call(enc, plan, big, [0] * 5) == N.ERR_INVALID_ARG
    assert "65536" in N.last_error()
    assert _call(enc, plan, big[:65536], [65535] * 5) == N.HBEC_OK  # the limit itself
    assert _call(enc, plan, [LOST0, FULL], [0, 1, 2, 0, 0]) == N.ERR_INVALID_ARG  # on a zero-length entry
    assert "index" in N.last_error() and "2" in N.last_error()
    assert _call(enc, plan, [LOST0, FEW], [0, 1, 0, 1, 0]) == N.ERR_TOO_FEW_SHARDS
    assert _call(enc, plan, [FULL, FEW], [0] * 5) == N.ERR_TOO_FEW_SHARDS  # listed, used by no entry
    assert "pattern 1" in N.last_error()
    assert _call(enc, plan, [FEW], [3] * 5) == N.ERR_TOO_FEW_SHARDS  # before a bad index
    # the pattern checks come before the range and destination checks
    assert _call(enc, plan, [FEW], [0] * 5, lens=[1] * 5) == N.ERR_TOO_FEW_SHARDS
    assert _call(enc, plan, [LOST0], [1] * 5, lens=[1] * 5) == N.ERR_INVALID_ARG
    assert "index" in N.last_error()
    assert _call(enc, plan, [LOST0], [0] * 5, lens=[1] * 5, null=("starts",)) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_range_past_the_entry_is_refused(kind):
    """starts[i] + lens[i] > k * S_i: a zero-length entry takes no byte, and the sum does not wrap."""
    enc = RS.New(K, M)
    plan = GH._plan(enc, kind=kind)
    s0 = B.glue_range_stats()
    for i in range(5):
        lens = [0] * 5
        lens[i] = 1
        assert _call(enc, plan, [FULL], [0] * 5, dsts=[FAR] * 5, lens=lens) == N.ERR_INVALID_ARG
        assert "starts + lens" in N.last_error() and f"entry {i}" in N.last_error()
    top = (1 << 64) - 1
    assert _call(enc, plan, [FULL], [0] * 5, dsts=[FAR] * 5, starts=[0, 0, top, 0, 0],
                 lens=[0, 0, 1, 0, 0]) == N.ERR_INVALID_ARG  # 2^64 - 1 + 1 is not 0
    assert "entry 2" in N.last_error()
    assert _call(enc, plan, [FULL], [0] * 5, dsts=[FAR] * 5, starts=[0, 2, 0, 0, 0],
                 lens=[0, top, 0, 0, 0]) == N.ERR_INVALID_ARG
    assert "entry 1" in N.last_error()
    # lens[i] = 0 skips the entry whatever its start and destination
    assert _call(enc, plan, [FULL], [0] * 5, dsts=[0, FAR, 0, 1, 0], starts=[7, top, 0, 1 << 40, 3]) == N.HBEC_OK
    assert B.glue_range_stats() == s0


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_nothing_to_do_is_ok_and_launches_nothing(kind):
    enc = RS.New(K, M)
    s0 = B.glue_range_stats()
    plan = GH._plan(enc, kind=kind)
    assert _call(enc, plan, [FULL], [0] * 5) == N.HBEC_OK
    assert _call(enc, plan, [LOST0], [0] * 5, dsts=[FAR] * 5) == N.HBEC_OK
    empty = GH._plan(enc, 0, kind=kind)
    assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32), n=0) == N.HBEC_OK
    assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32), n_patterns=0, n=0) == N.HBEC_OK
    # errors come first even when there is no work
    assert _call(enc, empty, [[1, 0, 0, 0, 0, 0]], np.zeros(0, np.uint32), n=0) == N.ERR_TOO_FEW_SHARDS
    B.set_glue_range_chunk_tiles(64)
    B.set_glue_range_chunk_tiles(0)
    assert B.glue_range_stats() == s0
    T = B.glue_range_tile_bytes()
    assert T > 0 and T % 16 == 0 and T == B.mixed_plan_tile_bytes() == B.glue_plan_tile_bytes()


def test_python_wrappers_check_shapes_before_a_stream_is_asked_for():
    enc = RS.New(K, M)
    plan = GH._plan(enc)
    ok = np.ones((5, K + M), np.uint8)
    with pytest.raises(ValueError):
        plan.glue_range(np.ones((4, K + M), np.uint8), [0] * 5, [0] * 5, [0] * 5)
    for bad in ((4, 5, 5), (5, 4, 5), (5, 5, 6)):
        with pytest.raises(ValueError):
            plan.glue_range(ok, *[[0] * x for x in bad])
    for kind in ("stripes", "objects", "shards"):
        with pytest.raises(ValueError, match="files"):
            GH._plan(enc, kind=kind).glue_range_files(ok, [], [], [])
    f = B.StripePlan(enc, files=[([0] * (K + M), 0)] * 3, chunk_size=4096)
    none = np.ones((0, K + M), np.uint8)
    for bad in ((2, 3, 3), (3, 2, 3), (3, 3, 4)):
        with pytest.raises(ValueError):
            f.glue_range_files(none, *[[0] * x for x in bad])
    s0 = B.glue_range_stats()
    f.glue_range_files(none, [0] * 3, [0] * 3, [0] * 3, stream=GH._NoStream())  # nothing to do: nothing queued
    plan.glue_range(ok, [0] * 5, [0] * 5, [0] * 5, stream=GH._NoStream())
    assert B.glue_range_stats() == s0


def _files_call(enc, plan, starts, n_objects, lengths, chunk, patterns, pattern_of, outs, r0, r1, null=()):
    st = np.ascontiguousarray(starts, dtype=np.uint32)
    ln = np.ascontiguousarray(lengths if len(lengths) else [0], dtype=np.uint64)
    pat = np.ascontiguousarray(patterns, dtype=np.uint8).reshape(-1, K + M)
    idx = np.ascontiguousarray(pattern_of if len(pattern_of) else [0], dtype=np.uint32)
    d = (C.c_void_p * max(1, len(outs)))(*[int(a) for a in outs])
    a0 = np.ascontiguousarray(r0 if len(r0) else [0], dtype=np.uint64)
    a1 = np.ascontiguousarray(r1 if len(r1) else [0], dtype=np.uint64)
    return N.lib().hbec_glue_plan_files_range(
        None if "codec" in null else enc.handle, None if "plan" in null else plan._h,
        None if "object_start" in null else st.ctypes.data_as(U32P), n_objects,
        None if "content_lengths" in null else ln.ctypes.data_as(U64P), chunk,
        None if "patterns" in null else pat.ctypes.data_as(N._U8P), pat.shape[0],
        None if "pattern_of" in null else idx.ctypes.data_as(U32P), None if "object_dsts" in null else d,
        None if "range_starts" in null else a0.ctypes.data_as(U64P),
        None if "range_ends" in null else a1.ctypes.data_as(U64P), None)


def test_files_range_argument_errors_on_empty_plans():
    enc = RS.New(K, M)
    s0 = B.glue_range_stats()
    f = B.StripePlan(enc, files=[([0] * (K + M), 0)] * 3, chunk_size=4096)
    args = (f.object_start, 3, [0, 0, 0], 4096, [FULL], [], [0, 0, 0], [0, 0, 0], [0, 0, 0])
    assert _files_call(enc, f, *args) == N.HBEC_OK
    for null in ("codec", "plan", "content_lengths", "patterns", "pattern_of", "object_dsts", "range_starts",
                 "range_ends"):
        assert _files_call(enc, f, *args, null=(null,)) == N.ERR_INVALID_ARG, null
        assert "null" in N.last_error(), null
    assert _files_call(RS.New(8, 3), f, *args) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    assert B.glue_range_stats() == s0


def range_errors():
    """The argument errors that need an entry with bytes in it.  Returns False
    where no plan with such an entry can be built (no device)."""
    enc = RS.New(K, M)
    S = 100
    row = [BASE + 3 * S * j for j in range(K + M)]  # shards 3 S apart
    plan = GH._shards_plan(enc, [row, [0] * (K + M), row], [S, 0, S])
    if plan is None:
        return False
    s0 = B.glue_range_stats()

    def call(dsts, starts, lens, pats=(FULL,), of=(0, 0, 0)):
        return _call(enc, plan, list(pats), list(of), dsts=dsts, starts=starts, lens=lens, n=3)

    # starts[i] + lens[i] > k S_i, before the entry's null destination and its overlap
    for st, ln in ((0, K * S + 1), (1, K * S), (K * S, 1), (K * S + 1, 1), ((1 << 64) - 1, 2)):
        assert call([0, 0, FAR], [st, 0, 0], [ln, 0, 1]) == N.ERR_INVALID_ARG, (st, ln)
        assert "starts + lens" in N.last_error() and "entry 0" in N.last_error()
        assert call([row[0], 0, FAR], [st, 0, 0], [ln, 0, 1]) == N.ERR_INVALID_ARG
        assert "starts + lens" in N.last_error()
    assert call([FAR, FAR, FAR], [0, 0, 0], [K * S, 1, 1]) == N.ERR_INVALID_ARG
    assert "starts + lens" in N.last_error() and "entry 1" in N.last_error()
    # entries are checked in order: entry 0's overlap before entry 2's range
    assert call([row[1], 0, FAR], [0, 0, K * S], [1, 0, 1]) == N.ERR_INVALID_ARG
    assert "overlaps" in N.last_error() and "entry 0" in N.last_error()
    # a null destination with a length (and none without), before that entry's overlap check can matter
    assert call([FAR, 0, 0], [K * S - 7, 0, K * S - 7], [7, 0, 7]) == N.ERR_INVALID_ARG
    assert "null destination" in N.last_error() and "entry 2" in N.last_error()
    # a destination over one of the entry's own shards, parity and missing ones too, wherever the range starts:
    # the destination holds lens bytes, not starts + lens
    for sh in range(K + M):
        for dst, ln in ((row[sh], 1), (row[sh] + S - 1, 1), (row[sh] - 5, 6), (row[sh] - 1, S)):
            for pats in ((FULL,), (LOST0,)):
                for st in (0, 3, K * S - ln):
                    assert call([FAR, 0, dst], [0, 0, st], [0, 0, ln], pats) == N.ERR_INVALID_ARG, (sh, dst, ln, st)
                    assert "overlaps" in N.last_error() and "entry 2" in N.last_error()
    # the pattern checks still come first
    assert call([row[0], 0, FAR], [0, 0, 0], [1, 0, 1], (FEW,)) == N.ERR_TOO_FEW_SHARDS
    assert B.glue_range_stats() == s0

    # files: hbec_glue_plan_files's checks, then the range, named by object
    chunk = 64
    L = 2 * K * chunk + 12  # stripes of 64, 64 and 3 bytes a shard
    files = [BASE + (1 << 20) * j for j in range(K + M)]
    f = B.StripePlan(enc, files=[(files, L), ([0] * (K + M), 0), (files, 5)], chunk_size=chunk)
    assert f.object_start.tolist() == [0, 3, 3, 4]
    good = (f.object_start, 3, [L, 0, 5], chunk, [FULL], [0] * 4, [FAR, 0, FAR + (1 << 20)], [3, 0, 1], [L, 0, 5])
    for bad_len, g in (([L + 1, 0, 5], 0), ([L - 8, 0, 5], 0), ([L, 1, 5], 1), ([L, 0, 9], 2), ([L, 0, 1 << 63], 2)):
        assert _files_call(enc, f, good[0], 3, bad_len, *good[3:]) == N.ERR_INVALID_ARG, bad_len
        assert f"object {g}" in N.last_error(), (bad_len, N.last_error())
    assert _files_call(enc, f, good[0], 3, good[2], 0, *good[4:]) == N.ERR_INVALID_ARG
    assert "chunk_size" in N.last_error()
    for starts, n_obj in (([1, 3, 3, 4], 3), ([0, 3, 2, 4], 3), ([0, 3, 3, 5], 3), ([0, 3, 3, 4], 0)):
        assert _files_call(enc, f, starts, n_obj, *good[2:]) == N.ERR_INVALID_ARG, starts
        assert "object" in N.last_error()
    for r0, r1, g in (([4, 0, 1], [3, 0, 5], 0), ([0, 0, 0], [L + 1, 0, 5], 0), ([0, 1, 0], [L, 1, 5], 1),
                      ([0, 0, 6], [L, 0, 5], 2), ([0, 0, 0], [L, 0, 6], 2), ([0, 0, 0], [L, 0, (1 << 64) - 1], 2)):
        assert _files_call(enc, f, *good[:7], r0, r1) == N.ERR_INVALID_ARG, (r0, r1)
        assert "range" in N.last_error() and f"object {g}" in N.last_error(), N.last_error()
    # an object's bad content length is reported before its bad range
    assert _files_call(enc, f, good[0], 3, [L, 0, 9], *good[3:7], [0, 0, 0], [L, 0, 77]) == N.ERR_INVALID_ARG
    assert "shard length mismatch (object 2" in N.last_error()
    # then it is the first call: its pattern and destination checks, on the entries the range reaches
    assert _files_call(enc, f, *good[:4], [FEW], *good[5:]) == N.ERR_TOO_FEW_SHARDS
    assert _files_call(enc, f, *good[:6], [0, 0, FAR], *good[7:]) == N.ERR_INVALID_ARG
    assert "null destination" in N.last_error() and "entry 0" in N.last_error()
    # a range that begins in the object's second stripe: entry 0 is skipped, entry 1 is the one named
    assert _files_call(enc, f, *good[:6], [0, 0, FAR], [K * chunk + 1, 0, 1], [L, 0, 5]) == N.ERR_INVALID_ARG
    assert "null destination" in N.last_error() and "entry 1" in N.last_error()
    assert _files_call(enc, f, *good[:6], [FAR, 0, files[5] + 1], *good[7:]) == N.ERR_INVALID_ARG  # object 2 is entry 3
    assert "overlaps" in N.last_error() and "entry 3" in N.last_error()
    # empty ranges ask for nothing, wherever they lie and whatever the destination
    assert _files_call(enc, f, *good[:6], [0, 0, 0], [0, 0, 5], [0, 0, 5]) == N.HBEC_OK
    assert _files_call(enc, f, *good[:6], [files[0], 0, files[1]], [L, 0, 2], [L, 0, 2]) == N.HBEC_OK
    assert B.glue_range_stats() == s0
    return True


def test_range_errors_where_a_plan_with_bytes_can_be_built():
    range_errors()


@pytest.mark.parametrize("k,chunk", [(1, 5), (3, 2), (4, 5), (8, 1)])
def test_files_cut_matches_the_oracles_slicing(k, chunk, range_host):
    """For objects around one, two and three stripes and every 0 <= start <= end <= L,
    the pieces csrc/gluerange.h cuts (printed by the stand-alone program), each
    taken from its entry's bytes and put at its destination offset, are what
    oracle.ec_glue_range returns for the object's shard files, which is obj[start:end]."""
    m = 2
    for L in (0, 1, k * chunk - 1, k * chunk, k * chunk + 1, 2 * k * chunk + 3, 3 * k * chunk + k):
        obj = bytes(np.asarray(O.object_bytes(900 + L, L), np.uint8)) if L else b""
        files = O.ec_split(k, m, obj, chunk)
        out = subprocess.run([str(range_host), "cuts", str(k), str(chunk), str(L)], capture_output=True, text=True,
                             env=RH.ENV, timeout=300)
        assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
        pieces = {}
        for line in out.stdout.split("\n"):
            if line:
                start, end, t, es, el, d = map(int, line.split())
                pieces.setdefault((start, end), []).append((t, es, el, d))
        # entry t's bytes are the object's from t k chunk on (tests/test_glue_host.py checks that cut)
        step = max(1, (L + 1) * (L + 2) // 2 // 400)  # the oracle on some 400 ranges, the slices on all
        for n, (start, end) in enumerate((a, b) for a in range(L + 1) for b in range(a, L + 1)):
            got = bytearray(end - start)
            filled = 0
            for t, es, el, d in pieces.get((start, end), []):
                entry = obj[t * k * chunk:(t + 1) * k * chunk]
                assert es + el <= len(entry)
                got[d:d + el] = entry[es:es + el]
                filled += el
            assert filled == end - start and bytes(got) == obj[start:end], (L, start, end)
            if n % step == 0 and end > start:
                assert O.ec_glue_range(k, m, files, chunk, L, start, end) == obj[start:end], (L, start, end)


def test_range_instances_use_no_scratch_and_no_lds():
    for fam in ("gf_range_plan", "gf_range_plan_rows"):
        found = KR.kernels(f"{fam}ILi")
        assert len(found) == 5, (fam, sorted(found))
        for r in range(5):
            assert any(f"{fam}ILi{r}E" in nm for nm in found), (fam, r)
        for nm, k in found.items():
            assert k[".private_segment_fixed_size"] == 0, nm
            assert k[".group_segment_fixed_size"] == 0, nm
            assert "gf_glue_planILi" not in nm and "gf_glue_plan_rowsILi" not in nm


def test_glue_plan_instances_are_still_five_each():
    for fam in ("gf_glue_plan", "gf_glue_plan_rows"):
        found = KR.kernels(f"{fam}ILi")
        assert len(found) == 5, (fam, sorted(found))
        for r in range(5):
            assert any(f"{fam}ILi{r}E" in nm for nm in found), (fam, r)
