"""The glue calls without a device: the new symbols of libhbec.so, every argument
error of hbec_glue_plan_mixed and hbec_glue_plan_files with its code, precedence
and message keyword (all found before anything is queued), the files cut against
the oracle's stripe sizes, csrc/glue.h alone under AddressSanitizer + UBSan
(tests/native/glue_host.cpp, a stand-alone program that links no libhbec), and the
resources of the gf_glue_plan instances from the library's code-object metadata.

Plans of zero-length entries need no device memory.  The errors that need an
entry with bytes in it (a null destination, a destination over an own shard, a
files length mismatch) are checked on shards plans whose addresses are compared
and never followed; such a plan keeps its address rows in device memory, so
where no device is present `destination_errors` has nothing to build them on
and tests/test_gpu_glue_plan.py runs it again where one is."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_kernel_resources as KR
import test_repair_mixed_host as RH
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import ecutils as E
from hummingbird_amd import reedsolomon as RS
from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "glue_host.cpp"
NEW = ["hbec_glue_plan_mixed", "hbec_glue_plan_files", "hbec_glue_plan_stats", "hbec_glue_plan_tile_bytes",
       "hbec_set_glue_plan_chunk_tiles"]
K, M = 4, 2
U32P = C.POINTER(C.c_uint32)
U64P = C.POINTER(C.c_uint64)
FULL = [1] * (K + M)
LOST0 = [0, 1, 1, 1, 1, 1]
FEW = [1, 1, 1, 0, 0, 0]
BASE = 0x7000_0000_0000  # addresses are compared here, never followed
FAR = 0x7100_0000_0000


def test_new_symbols_are_exported_and_declared():
    lib = N.lib()
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS and f" {name}(" in header, name
    assert "ecutils.go:134-186" in header
    assert lib.hbec_version() == 2  # additive
    for name in ("glue_plan_stats", "glue_plan_tile_bytes", "set_glue_plan_chunk_tiles"):
        assert hasattr(B, name), name
    assert hasattr(B.StripePlan, "glue_mixed") and hasattr(B.StripePlan, "glue_files")


@pytest.fixture(scope="module")
def glue_host(tmp_path_factory):
    """tests/native/glue_host.cpp built with AddressSanitizer + UBSan: a program of its own."""
    text = SRC.read_text()
    assert "csrc/glue.h" in text and "hbec.h" not in text and "int main(" in text
    exe = tmp_path_factory.mktemp("glue_host") / "glue_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


def test_glue_host_logic_under_sanitizers(glue_host):
    out = subprocess.run([str(glue_host)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = re.search(r"glue_host ok \((\d+) clamps, (\d+) tiles, (\d+) cuts, (\d+) pairs\)", out.stdout)
    assert got, out.stdout
    assert int(got.group(1)) == 200000 and int(got.group(2)) > 200000
    assert int(got.group(3)) > 3000 and int(got.group(4)) == 200000


def _plan(enc, n=5, kind="stripes"):
    if kind == "objects":
        return B.StripePlan(enc, objects=[(0, 0, 0)] * n)
    if kind == "shards":
        return B.StripePlan(enc, shards=[([0] * (enc.DataShards + enc.ParityShards), 0)] * n)
    return B.StripePlan(enc, stripes=[(0, 0)] * n)


def _call(enc, plan, patterns, pattern_of, dsts=None, lens=None, n_patterns=None, null=(), n=5):
    """hbec_glue_plan_mixed on host arrays."""
    pat = np.ascontiguousarray(patterns, dtype=np.uint8).reshape(-1, K + M)
    idx = np.ascontiguousarray(pattern_of, dtype=np.uint32)
    d = (C.c_void_p * max(1, n))(*[int(a) for a in (dsts if dsts is not None else [0] * n)])
    ln = np.zeros(max(1, n), np.uint64)
    if lens is not None:
        ln[:n] = lens
    return N.lib().hbec_glue_plan_mixed(
        None if "codec" in null else enc.handle, None if "plan" in null else plan._h,
        None if "patterns" in null else pat.ctypes.data_as(N._U8P),
        pat.shape[0] if n_patterns is None else n_patterns, None if "pattern_of" in null else idx.ctypes.data_as(U32P),
        None if "dsts" in null else d, None if "dst_lens" in null else ln.ctypes.data_as(U64P), None)


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_null_arguments(kind):
    enc = RS.New(K, M)
    plan = _plan(enc, kind=kind)
    for null in ("codec", "plan", "patterns", "pattern_of", "dsts", "dst_lens"):
        assert _call(enc, plan, [LOST0], [0] * 5, null=(null,)) == N.ERR_INVALID_ARG, null
        assert "null" in N.last_error(), null
    # for a plan of no entries too
    empty = _plan(enc, 0, kind=kind)
    for null in ("dsts", "dst_lens"):
        assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32), null=(null,), n=0) == N.ERR_INVALID_ARG
    a = C.c_uint64()
    assert N.lib().hbec_glue_plan_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert N.lib().hbec_glue_plan_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert N.last_error()


def test_pattern_errors_are_those_of_reconstruct_with_their_precedence():
    enc = RS.New(K, M)
    plan = _plan(enc)
    other = _plan(RS.New(8, 3))
    assert _call(enc, other, [LOST0], [0] * 5) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    # reported before a bad pattern count or index, and before a bad length
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
    assert _call(enc, plan, [LOST0], [0, 0, 0, 0, 0xFFFFFFFF]) == N.ERR_INVALID_ARG
    assert _call(enc, plan, [LOST0, FEW], [0, 1, 0, 1, 0]) == N.ERR_TOO_FEW_SHARDS
    assert _call(enc, plan, [FULL, FEW], [0] * 5) == N.ERR_TOO_FEW_SHARDS  # listed, used by no entry
    assert "pattern 1" in N.last_error()
    assert _call(enc, plan, [FEW], [3] * 5) == N.ERR_TOO_FEW_SHARDS  # before a bad index
    # the pattern checks come before the destination checks
    assert _call(enc, plan, [FEW], [0] * 5, lens=[1] * 5) == N.ERR_TOO_FEW_SHARDS
    assert _call(enc, plan, [LOST0], [1] * 5, lens=[1] * 5) == N.ERR_INVALID_ARG
    assert "index" in N.last_error()
    assert _call(enc, plan, [LOST0], [0] * 5, lens=[1] * 5, null=("dsts",)) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_length_past_the_entry_is_refused(kind):
    """dst_lens[i] > k * S_i: a zero-length entry takes no byte."""
    enc = RS.New(K, M)
    plan = _plan(enc, kind=kind)
    s0 = B.glue_plan_stats()
    for i in range(5):
        lens = [0] * 5
        lens[i] = 1
        assert _call(enc, plan, [FULL], [0] * 5, dsts=[FAR] * 5, lens=lens) == N.ERR_INVALID_ARG
        assert "dst_lens" in N.last_error() and f"entry {i}" in N.last_error()
    assert _call(enc, plan, [FULL], [0] * 5, dsts=[FAR] * 5, lens=[0, 0, 1 << 63, 0, 0]) == N.ERR_INVALID_ARG
    assert "entry 2" in N.last_error()
    assert B.glue_plan_stats() == s0


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_nothing_to_do_is_ok_and_launches_nothing(kind):
    enc = RS.New(K, M)
    s0 = B.glue_plan_stats()
    plan = _plan(enc, kind=kind)
    assert _call(enc, plan, [FULL], [0] * 5) == N.HBEC_OK
    assert _call(enc, plan, [LOST0], [0] * 5, dsts=[FAR] * 5) == N.HBEC_OK
    assert _call(enc, plan, [[1, 1, 1, 1, 0, 0], [0, 1, 1, 1, 0, 1]], [0, 1, 1, 0, 1]) == N.HBEC_OK
    empty = _plan(enc, 0, kind=kind)
    assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32), n=0) == N.HBEC_OK
    assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32), n_patterns=0, n=0) == N.HBEC_OK
    # errors come first even when there is no work
    assert _call(enc, empty, [[1, 0, 0, 0, 0, 0]], np.zeros(0, np.uint32), n=0) == N.ERR_TOO_FEW_SHARDS
    B.set_glue_plan_chunk_tiles(64)
    B.set_glue_plan_chunk_tiles(0)
    assert B.glue_plan_stats() == s0
    T = B.glue_plan_tile_bytes()
    assert T > 0 and T % 16 == 0 and T == B.mixed_plan_tile_bytes()


def test_python_wrappers_check_shapes_before_a_stream_is_asked_for():
    enc = RS.New(K, M)
    plan = _plan(enc)
    ok = np.ones((5, K + M), np.uint8)
    with pytest.raises(ValueError):
        plan.glue_mixed(np.ones((4, K + M), np.uint8), [0] * 5, [0] * 5)
    with pytest.raises(ValueError):
        plan.glue_mixed(np.ones((5, K + M + 1), np.uint8), [0] * 5, [0] * 5)
    with pytest.raises(ValueError):
        plan.glue_mixed(np.ones(5 * (K + M), np.uint8), [0] * 5, [0] * 5)
    with pytest.raises(ValueError):
        plan.glue_mixed(ok, [0] * 4, [0] * 5)
    with pytest.raises(ValueError):
        plan.glue_mixed(ok, [0] * 5, [0] * 6)
    # glue_files is for plans built from files= alone
    for kind in ("stripes", "objects", "shards"):
        with pytest.raises(ValueError, match="files"):
            _plan(enc, kind=kind).glue_files(ok, [])
    f = B.StripePlan(enc, files=[([0] * (K + M), 0)] * 3, chunk_size=4096)
    assert f._content_lengths == [0, 0, 0] and f._chunk_size == 4096
    with pytest.raises(ValueError):
        f.glue_files(np.ones((1, K + M), np.uint8), [0] * 3)  # no entries: present has no rows
    with pytest.raises(ValueError):
        f.glue_files(np.ones((0, K + M), np.uint8), [0] * 2)  # an address per object


def _files_call(enc, plan, starts, n_objects, lengths, chunk, patterns, pattern_of, outs, null=()):
    st = np.ascontiguousarray(starts, dtype=np.uint32)
    ln = np.ascontiguousarray(lengths if len(lengths) else [0], dtype=np.uint64)
    pat = np.ascontiguousarray(patterns, dtype=np.uint8).reshape(-1, K + M)
    idx = np.ascontiguousarray(pattern_of if len(pattern_of) else [0], dtype=np.uint32)
    d = (C.c_void_p * max(1, len(outs)))(*[int(a) for a in outs])
    return N.lib().hbec_glue_plan_files(
        None if "codec" in null else enc.handle, None if "plan" in null else plan._h,
        None if "object_start" in null else st.ctypes.data_as(U32P), n_objects,
        None if "content_lengths" in null else ln.ctypes.data_as(U64P), chunk,
        None if "patterns" in null else pat.ctypes.data_as(N._U8P), pat.shape[0],
        None if "pattern_of" in null else idx.ctypes.data_as(U32P), None if "object_dsts" in null else d, None)


def test_glue_files_argument_errors_on_empty_plans():
    enc = RS.New(K, M)
    s0 = B.glue_plan_stats()
    f = B.StripePlan(enc, files=[([0] * (K + M), 0)] * 3, chunk_size=4096)
    args = (f.object_start, 3, [0, 0, 0], 4096, [FULL], [], [0, 0, 0])
    assert _files_call(enc, f, *args) == N.HBEC_OK
    for null in ("codec", "plan", "content_lengths", "patterns", "pattern_of", "object_dsts"):
        assert _files_call(enc, f, *args, null=(null,)) == N.ERR_INVALID_ARG, null
        assert "null" in N.last_error(), null
    assert _files_call(RS.New(8, 3), f, *args) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    f.glue_files(np.ones((0, K + M), np.uint8), [0, 0, 0], stream=_NoStream())  # nothing to do: nothing queued
    assert B.glue_plan_stats() == s0


class _NoStream:
    """Stands in for a torch stream where nothing may be queued."""
    cuda_stream = 0


def _shards_plan(enc, rows, lens):
    """A shards plan over addresses that are never followed, or None where there
    is no device to keep its address rows on."""
    ptrs = (C.c_void_p * (len(rows) * (K + M)))(*[int(a) for row in rows for a in row])
    ln = np.ascontiguousarray(lens, dtype=np.uint64)
    h = C.c_void_p()
    rc = N.lib().hbec_plan_shards(enc.handle, ptrs, ln.ctypes.data_as(U64P), len(rows), C.byref(h))
    assert rc != N.ERR_INVALID_ARG, N.last_error()
    if rc != N.HBEC_OK:
        return None
    plan = B.StripePlan.__new__(B.StripePlan)
    plan.enc, plan._h, plan._n = enc, h, len(rows)
    return plan


def destination_errors():
    """The argument errors that need an entry with bytes in it.  Returns False
    where no plan with such an entry can be built (no device)."""
    enc = RS.New(K, M)
    S = 100
    row = [BASE + 3 * S * j for j in range(K + M)]  # shards 3 S apart
    plan = _shards_plan(enc, [row, [0] * (K + M), row], [S, 0, S])
    if plan is None:
        return False
    s0 = B.glue_plan_stats()

    def call(dsts, lens, pats=(FULL,), of=(0, 0, 0)):
        return _call(enc, plan, list(pats), list(of), dsts=dsts, lens=lens, n=3)

    # dst_lens[i] > k S_i
    assert call([FAR, 0, FAR], [K * S + 1, 0, 1]) == N.ERR_INVALID_ARG
    assert "dst_lens" in N.last_error() and "entry 0" in N.last_error()
    assert call([FAR, FAR, FAR], [K * S, 1, 1]) == N.ERR_INVALID_ARG
    assert "dst_lens" in N.last_error() and "entry 1" in N.last_error()
    # a null destination with a length (and none without)
    assert call([FAR, 0, 0], [K * S, 0, 7]) == N.ERR_INVALID_ARG
    assert "null destination" in N.last_error() and "entry 2" in N.last_error()
    # a destination over one of the entry's own shards, parity and missing ones too: one byte is enough
    for sh in range(K + M):
        for dst, ln in ((row[sh], 1), (row[sh] + S - 1, 1), (row[sh] - 5, 6), (row[sh] - 1, K * S)):
            for pats in ((FULL,), (LOST0,)):
                assert call([FAR, 0, dst], [0, 0, ln], pats) == N.ERR_INVALID_ARG, (sh, dst - row[sh], ln)
                assert "overlaps" in N.last_error() and "entry 2" in N.last_error()
    # the pattern checks still come first
    assert call([row[0], 0, FAR], [1, 0, 1], (FEW,)) == N.ERR_TOO_FEW_SHARDS
    # none of this launched anything
    assert B.glue_plan_stats() == s0

    # files: the entry lengths must be those of the content length, and the object is named
    chunk = 64
    L = 2 * K * chunk + 12  # stripes of 64, 64 and 3 bytes a shard
    files = [BASE + (1 << 20) * j for j in range(K + M)]
    f = B.StripePlan(enc, files=[(files, L), ([0] * (K + M), 0), (files, 5)], chunk_size=chunk)
    assert f.object_start.tolist() == [0, 3, 3, 4]
    good = (f.object_start, 3, [L, 0, 5], chunk, [FULL], [0] * 4, [FAR, 0, FAR + (1 << 20)])
    for bad_len, g in (([L + 1, 0, 5], 0), ([L - 8, 0, 5], 0), ([L + K * chunk, 0, 5], 0), ([L, 1, 5], 1),
                       ([L, 0, 9], 2), ([L, 0, 0], 2), ([L, 0, 1 << 63], 2)):
        assert _files_call(enc, f, good[0], 3, bad_len, *good[3:]) == N.ERR_INVALID_ARG, bad_len
        assert f"object {g}" in N.last_error(), (bad_len, N.last_error())
    assert _files_call(enc, f, good[0], 3, good[2], chunk // 2, *good[4:]) == N.ERR_INVALID_ARG
    assert "object 0" in N.last_error()
    assert _files_call(enc, f, good[0], 3, good[2], 0, *good[4:]) == N.ERR_INVALID_ARG
    assert "chunk_size" in N.last_error()
    # the object table is checked as hbec_hash_plan_files checks it
    for starts, n_obj in (([1, 3, 3, 4], 3), ([0, 3, 2, 4], 3), ([0, 3, 3, 5], 3), ([0, 3, 3, 4], 0)):
        assert _files_call(enc, f, starts, n_obj, *good[2:]) == N.ERR_INVALID_ARG, starts
        assert "object" in N.last_error()
    assert _files_call(enc, f, *good, null=("object_start",)) == N.ERR_INVALID_ARG
    # then it is the first call: its pattern and destination checks
    assert _files_call(enc, f, *good[:4], [FEW], *good[5:]) == N.ERR_TOO_FEW_SHARDS
    assert _files_call(enc, f, *good[:6], [0, 0, FAR]) == N.ERR_INVALID_ARG
    assert "null destination" in N.last_error() and "entry 0" in N.last_error()
    assert _files_call(enc, f, *good[:6], [FAR, 0, files[5] + 1]) == N.ERR_INVALID_ARG  # object 2 is entry 3
    assert "overlaps" in N.last_error() and "entry 3" in N.last_error()
    assert B.glue_plan_stats() == s0
    return True


def test_destination_errors_where_a_plan_with_bytes_can_be_built():
    destination_errors()


@pytest.mark.parametrize("chunk", [1, 5, 64])
@pytest.mark.parametrize("k", [1, 3, 4, 8])
def test_files_cut_matches_the_oracle(k, chunk, glue_host):
    """For every L in 0..3 k chunk + k the cut csrc/glue.h makes (printed by the
    stand-alone program) is the oracle's: entry t starts where the stripes before
    it end, holds min(k S_t, what is left) bytes with S_t from _stripe_sizes, and
    the pieces tile [0, L) exactly.  The library's own stripe arithmetic, which
    hbec_glue_plan_files checks the plan's entries against, agrees."""
    top = 3 * k * chunk + k
    out = subprocess.run([str(glue_host), "cuts", str(k), str(chunk), str(top)], capture_output=True, text=True,
                         env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = {}
    for line in out.stdout.split("\n"):
        if line:
            L, t, off, ln = map(int, line.split())
            got.setdefault(L, []).append((t, off, ln))
    for L in range(0, top + 1):
        sizes = O._stripe_sizes(k, chunk, L)
        assert E.ec_stripe_count(L, k, chunk) == len(sizes), L
        want, at = [], 0
        for t, s in enumerate(sizes):
            assert E.ec_stripe_shard_length(L, k, chunk, t) == s, (L, t)
            ln = min(k * s, L - at)  # ecutils.go:159-163: k shards of s bytes, cut at what is left
            assert 1 <= ln and k * s - ln < k
            want.append((t, at, ln))
            at += ln
        assert at == L
        assert got.get(L, []) == want, L
        assert all(off == t * k * chunk for t, off, _ in want)


def test_glue_instances_use_no_scratch_and_no_lds():
    for fam in ("gf_glue_plan", "gf_glue_plan_rows"):
        found = KR.kernels(f"{fam}ILi")
        assert len(found) == 5, (fam, sorted(found))
        for r in range(5):
            assert any(f"{fam}ILi{r}E" in nm for nm in found), (fam, r)
        for nm, k in found.items():
            assert k[".private_segment_fixed_size"] == 0, nm
            assert k[".group_segment_fixed_size"] == 0, nm
