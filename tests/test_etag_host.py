"""The ETag calls without a device: the new symbols of libhbec.so, every argument
error of hbec_etag_plan_mixed and hbec_etag_plan_files with its code, precedence
and message keyword (all found before anything is queued), csrc/etag.h alone
under AddressSanitizer + UBSan (tests/native/etag_host.cpp, a stand-alone
program that links no libhbec), and the resources of md5_etag and md5_etag_rows
from the library's code-object metadata.

As in tests/test_glue_host.py, plans of zero-length entries need no device
memory, and the errors that need an entry with bytes in it are checked on shards
plans whose addresses are compared and never followed: `length_errors` returns
False where no device can keep their address rows, and
tests/test_gpu_etag_plan.py runs it again where one is."""
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

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "etag_host.cpp"
NEW = ["hbec_etag_plan_mixed", "hbec_etag_plan_files", "hbec_etag_plan_stats"]
K, M = GH.K, GH.M
U32P, U64P = GH.U32P, GH.U64P
FULL, LOST0, FEW, BASE, FAR = GH.FULL, GH.LOST0, GH.FEW, GH.BASE, GH.FAR
DEV = 0x7200_0000_0000  # device pointers that are compared and never followed


def test_new_symbols_are_exported_and_declared():
    lib = N.lib()
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS and f" {name}(" in header, name
        if name != "hbec_etag_plan_stats":  # each entry point's comment cites the reference
            decl = header[:header.index(f" {name}(")]
            comment = decl[decl.rindex("/*"):]
            assert "ecengine.go:320-321" in comment and "ecutils.go:171-183" in comment, name
    assert lib.hbec_version() == 2  # additive
    assert hasattr(B, "etag_plan_stats")
    assert hasattr(B.StripePlan, "etag_mixed") and hasattr(B.StripePlan, "etag_files")
    assert set(B.etag_plan_stats()) == {"kernel_launches", "chains", "segments", "decoded_entries"}
    a = [C.c_uint64() for _ in range(4)]
    for null in range(4):
        args = [None if i == null else C.byref(a[i]) for i in range(4)]
        assert lib.hbec_etag_plan_stats(*args) == N.ERR_INVALID_ARG, null
        assert "null" in N.last_error()


def test_etag_host_logic_under_sanitizers(tmp_path):
    """tests/native/etag_host.cpp built with AddressSanitizer + UBSan: a program of its own."""
    text = SRC.read_text()
    assert "csrc/etag.h" in text and "hbec.h" not in text and "int main(" in text
    assert text.count("#include \"") == 1  # the header alone
    exe = tmp_path / "etag_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = re.search(r"etag_host ok \((\d+) walks, (\d+) segments, (\d+) chains, (\d+) big\)", out.stdout)
    assert got, out.stdout
    # every (k <= 4, S <= 40, len 0..k S, data mask), on slot and on row records
    assert int(got.group(1)) == sum(2 * (k * s + 1) * 2 ** k for k in range(1, 5) for s in range(1, 41))
    assert int(got.group(2)) > int(got.group(1)) and int(got.group(3)) > 500 and int(got.group(4)) == 36


def _call(enc, plan, patterns, pattern_of, lens=None, n_patterns=None, null=(), n=5, filt=None, expected=None,
          digests=DEV, bad=None):
    """hbec_etag_plan_mixed on host arrays and device pointers that are never followed."""
    pat = np.ascontiguousarray(patterns, dtype=np.uint8).reshape(-1, K + M)
    idx = np.ascontiguousarray(pattern_of, dtype=np.uint32)
    ln = np.zeros(max(1, n), np.uint64)
    if lens is not None:
        ln[:n] = lens
    return N.lib().hbec_etag_plan_mixed(
        None if "codec" in null else enc.handle, None if "plan" in null else plan._h,
        None if "patterns" in null else pat.ctypes.data_as(N._U8P),
        pat.shape[0] if n_patterns is None else n_patterns, None if "pattern_of" in null else idx.ctypes.data_as(U32P),
        None if "lens" in null else ln.ctypes.data_as(U64P), filt, 1, expected, digests, bad, None)


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_null_arguments(kind):
    enc = RS.New(K, M)
    plan = GH._plan(enc, kind=kind)
    for null in ("codec", "plan", "patterns", "pattern_of", "lens"):
        assert _call(enc, plan, [LOST0], [0] * 5, null=(null,)) == N.ERR_INVALID_ARG, null
        assert "null" in N.last_error(), null
    empty = GH._plan(enc, 0, kind=kind)  # for a plan of no entries too
    assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32), null=("lens",), n=0) == N.ERR_INVALID_ARG


def test_pattern_errors_are_those_of_glue_with_their_precedence():
    enc = RS.New(K, M)
    plan = GH._plan(enc)
    other = GH._plan(RS.New(8, 3))
    assert _call(enc, other, [LOST0], [0] * 5) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    # reported before a bad pattern count or index, a bad length and bad device pointers
    assert _call(enc, other, [LOST0], [7] * 5, lens=[9] * 5, n_patterns=0, expected=DEV) == N.ERR_INVALID_ARG
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
    # the pattern checks come before the length and device-pointer checks
    assert _call(enc, plan, [FEW], [0] * 5, lens=[1] * 5, expected=DEV) == N.ERR_TOO_FEW_SHARDS
    assert _call(enc, plan, [LOST0], [1] * 5, lens=[1] * 5, expected=DEV) == N.ERR_INVALID_ARG
    assert "index" in N.last_error()


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_device_pointer_errors_are_those_of_hash(kind):
    """Checked for any plan, an empty one too, before the lengths are looked at."""
    enc = RS.New(K, M)
    s0 = B.etag_plan_stats()
    for plan, of, n in ((GH._plan(enc, kind=kind), [0] * 5, 5), (GH._plan(enc, 0, kind=kind), np.zeros(0, np.uint32), 0)):
        assert _call(enc, plan, [FULL], of, n=n, expected=DEV + 64) == N.ERR_INVALID_ARG
        assert "d_expected needs d_bad" in N.last_error()
        assert _call(enc, plan, [FULL], of, n=n, expected=DEV + 64, bad=DEV + 128, filt=DEV + 128) == N.ERR_INVALID_ARG
        assert "distinct" in N.last_error()
        assert _call(enc, plan, [FULL], of, n=n, bad=DEV + 128, filt=DEV + 128) == N.ERR_INVALID_ARG
        for digests, expected in ((DEV + 1, None), (DEV + 2, None), (DEV, DEV + 67), (None, DEV + 65)):
            assert _call(enc, plan, [FULL], of, n=n, digests=digests, expected=expected, bad=DEV + 128) \
                == N.ERR_INVALID_ARG
            assert "aligned" in N.last_error()
        # d_expected without d_bad is reported before a misaligned buffer, and both before a bad length
        assert _call(enc, plan, [FULL], of, n=n, lens=[1] * n, digests=DEV + 1, expected=DEV) == N.ERR_INVALID_ARG
        assert "d_expected needs d_bad" in N.last_error()
        # a call with no chain accepts null device pointers, and any others
        assert _call(enc, plan, [FULL], of, n=n, digests=None) == N.HBEC_OK
        assert _call(enc, plan, [FULL], of, n=n, digests=DEV, expected=DEV + 64, bad=DEV + 128, filt=DEV + 256) \
            == N.HBEC_OK
    assert B.etag_plan_stats() == s0


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_length_past_the_entry_is_refused(kind):
    """lens[i] > k * S_i: a zero-length entry takes no byte."""
    enc = RS.New(K, M)
    plan = GH._plan(enc, kind=kind)
    s0 = B.etag_plan_stats()
    for i in range(5):
        lens = [0] * 5
        lens[i] = 1
        assert _call(enc, plan, [FULL], [0] * 5, lens=lens) == N.ERR_INVALID_ARG
        assert "lens exceeds" in N.last_error() and f"entry {i}" in N.last_error()
    assert _call(enc, plan, [FULL], [0] * 5, lens=[0, 0, (1 << 64) - 1, 0, 0], digests=None) == N.ERR_INVALID_ARG
    assert "entry 2" in N.last_error()
    assert B.etag_plan_stats() == s0


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_nothing_to_do_is_ok_and_launches_nothing(kind):
    enc = RS.New(K, M)
    s0 = B.etag_plan_stats()
    plan = GH._plan(enc, kind=kind)
    assert _call(enc, plan, [FULL], [0] * 5) == N.HBEC_OK
    assert _call(enc, plan, [LOST0], [0] * 5, digests=None) == N.HBEC_OK
    assert _call(enc, plan, [[1, 1, 1, 1, 0, 0], [0, 1, 1, 1, 0, 1]], [0, 1, 1, 0, 1]) == N.HBEC_OK
    empty = GH._plan(enc, 0, kind=kind)
    assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32), n=0, digests=None) == N.HBEC_OK
    assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32), n_patterns=0, n=0) == N.HBEC_OK
    # errors come first even when there is no work
    assert _call(enc, empty, [[1, 0, 0, 0, 0, 0]], np.zeros(0, np.uint32), n=0) == N.ERR_TOO_FEW_SHARDS
    assert B.etag_plan_stats() == s0


def test_python_wrappers_check_shapes_before_a_stream_is_asked_for():
    enc = RS.New(K, M)
    plan = GH._plan(enc)
    ok = np.ones((5, K + M), np.uint8)
    for present in (np.ones((4, K + M), np.uint8), np.ones((5, K + M + 1), np.uint8), np.ones(5 * (K + M), np.uint8)):
        with pytest.raises(ValueError):
            plan.etag_mixed(present, [0] * 5)
    for lens in ([0] * 4, [0] * 6):
        with pytest.raises(ValueError):
            plan.etag_mixed(ok, lens)
    for kind in ("stripes", "objects", "shards"):
        with pytest.raises(ValueError, match="files"):
            GH._plan(enc, kind=kind).etag_files(ok)
    f = B.StripePlan(enc, files=[([0] * (K + M), 0)] * 3, chunk_size=4096)
    none = np.ones((0, K + M), np.uint8)
    with pytest.raises(ValueError):
        f.etag_files(np.ones((1, K + M), np.uint8))
    s0 = B.etag_plan_stats()
    f.etag_files(none, stream=GH._NoStream())  # nothing to do: nothing queued
    f.etag_files(None, stream=GH._NoStream())
    plan.etag_mixed(ok, [0] * 5, stream=GH._NoStream())
    plan.etag_mixed(None, [0] * 5, stream=GH._NoStream())
    assert B.etag_plan_stats() == s0


def _files_call(enc, plan, starts, n_objects, lengths, chunk, patterns, pattern_of, null=(), filt=None, expected=None,
                digests=DEV, bad=None):
    st = np.ascontiguousarray(starts, dtype=np.uint32)
    ln = np.ascontiguousarray(lengths if len(lengths) else [0], dtype=np.uint64)
    pat = np.ascontiguousarray(patterns, dtype=np.uint8).reshape(-1, K + M)
    idx = np.ascontiguousarray(pattern_of if len(pattern_of) else [0], dtype=np.uint32)
    return N.lib().hbec_etag_plan_files(
        None if "codec" in null else enc.handle, None if "plan" in null else plan._h,
        None if "object_start" in null else st.ctypes.data_as(U32P), n_objects,
        None if "content_lengths" in null else ln.ctypes.data_as(U64P), chunk,
        None if "patterns" in null else pat.ctypes.data_as(N._U8P), pat.shape[0],
        None if "pattern_of" in null else idx.ctypes.data_as(U32P), filt, 1, expected, digests, bad, None)


def test_files_argument_errors_on_empty_plans():
    enc = RS.New(K, M)
    s0 = B.etag_plan_stats()
    f = B.StripePlan(enc, files=[([0] * (K + M), 0)] * 3, chunk_size=4096)
    args = (f.object_start, 3, [0, 0, 0], 4096, [FULL], [])
    assert _files_call(enc, f, *args) == N.HBEC_OK
    assert _files_call(enc, f, *args, digests=None) == N.HBEC_OK
    for null in ("codec", "plan", "content_lengths", "patterns", "pattern_of"):
        assert _files_call(enc, f, *args, null=(null,)) == N.ERR_INVALID_ARG, null
        assert "null" in N.last_error(), null
    assert _files_call(RS.New(8, 3), f, *args) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    assert _files_call(enc, f, *args, expected=DEV) == N.ERR_INVALID_ARG
    assert "d_expected needs d_bad" in N.last_error()
    assert _files_call(enc, f, *args[:4], [FEW], []) == N.ERR_TOO_FEW_SHARDS
    assert B.etag_plan_stats() == s0


def length_errors():
    """The argument errors that need an entry with bytes in it.  Returns False
    where no plan with such an entry can be built (no device)."""
    enc = RS.New(K, M)
    S = 100
    row = [BASE + 3 * S * j for j in range(K + M)]  # shards 3 S apart
    plan = GH._shards_plan(enc, [row, [0] * (K + M), row], [S, 0, S])
    if plan is None:
        return False
    s0 = B.etag_plan_stats()

    def call(lens, pats=(FULL,), of=(0, 0, 0), **kw):
        return _call(enc, plan, list(pats), list(of), lens=lens, n=3, **kw)

    for lens, i in (([K * S + 1, 0, 0], 0), ([K * S, 1, 0], 1), ([K * S, 0, (1 << 64) - 1], 2), ([0, 0, K * S + 1], 2)):
        assert call(lens) == N.ERR_INVALID_ARG, lens
        assert "lens exceeds" in N.last_error() and f"entry {i}" in N.last_error()
    # a call with a chain needs somewhere to put or to find its digests; reported after a bad length
    assert call([K * S, 0, 1], digests=None) == N.ERR_INVALID_ARG
    assert "neither" in N.last_error()
    assert call([K * S + 1, 0, 1], digests=None) == N.ERR_INVALID_ARG
    assert "lens exceeds" in N.last_error()
    # the pattern and device-pointer checks still come first
    assert call([K * S + 1, 0, 0], (FEW,)) == N.ERR_TOO_FEW_SHARDS
    assert call([K * S + 1, 0, 0], expected=DEV) == N.ERR_INVALID_ARG
    assert "d_expected needs d_bad" in N.last_error()
    assert call([K * S + 1, 0, 0], digests=DEV + 2) == N.ERR_INVALID_ARG
    assert "aligned" in N.last_error()
    assert B.etag_plan_stats() == s0

    # files: hbec_glue_plan_files's checks and messages, named by object, then the call's own
    chunk = 64
    L = 2 * K * chunk + 12  # stripes of 64, 64 and 3 bytes a shard
    files = [BASE + (1 << 20) * j for j in range(K + M)]
    f = B.StripePlan(enc, files=[(files, L), ([0] * (K + M), 0), (files, 5)], chunk_size=chunk)
    assert f.object_start.tolist() == [0, 3, 3, 4]
    good = (f.object_start, 3, [L, 0, 5], chunk, [FULL], [0] * 4)
    for bad_len, g in (([L + 1, 0, 5], 0), ([L - 8, 0, 5], 0), ([L, 1, 5], 1), ([L, 0, 9], 2), ([L, 0, 1 << 63], 2)):
        assert _files_call(enc, f, good[0], 3, bad_len, *good[3:]) == N.ERR_INVALID_ARG, bad_len
        assert f"object {g}" in N.last_error(), (bad_len, N.last_error())
    assert _files_call(enc, f, good[0], 3, [L, 0, 9], *good[3:]) == N.ERR_INVALID_ARG
    assert "shard length mismatch (object 2" in N.last_error()
    assert _files_call(enc, f, good[0], 3, good[2], 0, *good[4:]) == N.ERR_INVALID_ARG
    assert "chunk_size" in N.last_error()
    for starts, n_obj in (([1, 3, 3, 4], 3), ([0, 3, 2, 4], 3), ([0, 3, 3, 5], 3), ([0, 3, 3, 4], 0)):
        assert _files_call(enc, f, starts, n_obj, *good[2:]) == N.ERR_INVALID_ARG, starts
        assert "object" in N.last_error()
    assert _files_call(enc, f, *good, null=("object_start",)) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    # the object table before the patterns, the patterns before the device pointers
    assert _files_call(enc, f, good[0], 3, [L, 0, 9], chunk, [FEW], [0] * 4) == N.ERR_INVALID_ARG
    assert _files_call(enc, f, *good[:4], [FEW], [0] * 4, expected=DEV) == N.ERR_TOO_FEW_SHARDS
    assert _files_call(enc, f, *good, expected=DEV) == N.ERR_INVALID_ARG
    assert "d_expected needs d_bad" in N.last_error()
    assert _files_call(enc, f, *good, digests=None) == N.ERR_INVALID_ARG
    assert "neither" in N.last_error()
    assert B.etag_plan_stats() == s0
    return True


def test_length_errors_where_a_plan_with_bytes_can_be_built():
    length_errors()


def test_chain_kernels_use_no_scratch_and_no_lds():
    found = KR.kernels("md5_etag")
    assert len(found) == 2, sorted(found)
    assert any("8md5_etagE" in nm for nm in found) and any("13md5_etag_rowsE" in nm for nm in found)
    for nm, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, nm
        assert k[".group_segment_fixed_size"] == 0, nm
        assert k[".vgpr_count"] <= 128, (nm, k[".vgpr_count"])  # four waves a SIMD, as md5_files
