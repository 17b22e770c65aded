"""The split calls without a device: the new symbols of libhbec.so, every argument
error of hbec_split_plan and hbec_split_plan_files with its code, precedence and
message keyword (all found before anything is queued), the length rule against
the oracle's ecShardLength and stripe sizes, csrc/splitplan.h alone under
AddressSanitizer + UBSan (tests/native/split_host.cpp, a stand-alone program
that links no libhbec), and the resources of the gf_split_plan instances from the
library's code-object metadata.

Plans of zero-length entries need no device memory.  The errors that need an
entry with bytes in it (a wrong length for a real shard length, a null source,
a source over an own shard, a files length mismatch) are checked on shards
plans whose addresses are compared and never followed; such a plan keeps its
address rows in device memory, so where no device is present `source_errors`
has nothing to build them on and tests/test_gpu_split_plan.py runs it again
where one is."""
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
from hummingbird_amd import ecutils as E
from hummingbird_amd import reedsolomon as RS
from oracle import oracle as O

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "split_host.cpp"
NEW = ["hbec_split_plan", "hbec_split_plan_files", "hbec_split_plan_stats", "hbec_split_plan_tile_bytes",
       "hbec_set_split_plan_chunk_tiles"]
K, M = 4, 2
U32P = C.POINTER(C.c_uint32)
U64P = C.POINTER(C.c_uint64)
BASE = 0x7000_0000_0000  # addresses are compared here, never followed
FAR = 0x7100_0000_0000


def test_new_symbols_are_exported_and_declared():
    lib = N.lib()
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS and f" {name}(" in header, name
        # each declaration cites ecSplit's lines in the comment right above it
        above = header[:header.index(f" {name}(")]
        assert "ecutils.go:26-72" in above[above.rindex("/*"):], name
    assert lib.hbec_version() == 2  # additive
    for name in ("split_plan_stats", "split_plan_tile_bytes", "set_split_plan_chunk_tiles"):
        assert hasattr(B, name), name
    assert hasattr(B.StripePlan, "split") and hasattr(B.StripePlan, "split_files")


@pytest.fixture(scope="module")
def split_host(tmp_path_factory):
    """tests/native/split_host.cpp built with AddressSanitizer + UBSan: a program of its own."""
    text = SRC.read_text()
    assert "csrc/splitplan.h" in text and "hbec.h" not in text and "int main(" in text
    header = (ROOT / "hummingbird_amd" / "csrc" / "splitplan.h").read_text()
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', header) == ["stdint.h", "glue.h"]  # neither HIP nor the library
    exe = tmp_path_factory.mktemp("split_host") / "split_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return exe


def test_split_host_logic_under_sanitizers(split_host):
    out = subprocess.run([str(split_host)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = re.search(r"split_host ok \((\d+) rules, (\d+) tiles, (\d+) cuts\)", out.stdout)
    assert got, out.stdout
    assert int(got.group(1)) == 200000 and int(got.group(2)) > 200000 and int(got.group(3)) > 3000


@pytest.mark.parametrize("chunk", [1, 5, 64])
@pytest.mark.parametrize("k", [1, 3, 4, 8, 12])
def test_length_rule_matches_the_oracle(k, chunk, split_host):
    """For every L in 0..3 k chunk + k: the piece of every entry (printed by the
    stand-alone program) has the oracle's ecShardLength, which is the oracle's
    stripe size of that entry, and the rule accepts it; the pieces tile [0, L)."""
    top = 3 * k * chunk + k
    out = subprocess.run([str(split_host), "lens", str(k), str(chunk), str(top)], capture_output=True, text=True,
                         env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = {}
    for line in out.stdout.split("\n"):
        if line:
            L, t, off, ln, s, ok = map(int, line.split())
            got.setdefault(L, []).append((t, off, ln, s, ok))
    for L in range(0, top + 1):
        sizes = O._stripe_sizes(k, chunk, L)
        assert E.ec_stripe_count(L, k, chunk) == len(sizes), L
        want, at = [], 0
        for t, s in enumerate(sizes):
            ln = min(k * chunk, L - at)  # ecutils.go:40-45: k chunk_size bytes, or what is left
            assert O.ec_shard_length(ln, k) == s, (L, t)
            want.append((t, at, ln, s, 1))
            at += ln
        assert at == L
        assert got.get(L, []) == want, L
    assert O.ec_shard_length(0, k) == 0 and O.ec_shard_length(1, k) == 1


def _plan(enc, n=5, kind="stripes"):
    if kind == "objects":
        return B.StripePlan(enc, objects=[(0, 0, 0)] * n)
    if kind == "shards":
        return B.StripePlan(enc, shards=[([0] * (enc.DataShards + enc.ParityShards), 0)] * n)
    return B.StripePlan(enc, stripes=[(0, 0)] * n)


def _call(enc, plan, srcs=None, lens=None, null=(), n=5):
    """hbec_split_plan on host arrays."""
    d = (C.c_void_p * max(1, n))(*[int(a) for a in (srcs if srcs is not None else [0] * n)])
    ln = np.zeros(max(1, n), np.uint64)
    if lens is not None:
        ln[:n] = lens
    return N.lib().hbec_split_plan(
        None if "codec" in null else enc.handle, None if "plan" in null else plan._h,
        None if "srcs" in null else d, None if "src_lens" in null else ln.ctypes.data_as(U64P), None)


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_null_arguments(kind):
    enc = RS.New(K, M)
    plan = _plan(enc, kind=kind)
    for null in ("codec", "plan", "srcs", "src_lens"):
        assert _call(enc, plan, null=(null,)) == N.ERR_INVALID_ARG, null
        assert "null" in N.last_error(), null
    empty = _plan(enc, 0, kind=kind)  # for a plan of no entries too
    for null in ("srcs", "src_lens"):
        assert _call(enc, empty, null=(null,), n=0) == N.ERR_INVALID_ARG
    a = C.c_uint64()
    assert N.lib().hbec_split_plan_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert N.lib().hbec_split_plan_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert N.last_error()


def test_another_shape_is_refused_before_the_lengths():
    enc = RS.New(K, M)
    other = _plan(RS.New(8, 3))
    assert _call(enc, other) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    assert _call(enc, other, srcs=[FAR] * 5, lens=[9] * 5) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    assert _call(enc, _plan(RS.New(K, 0)), srcs=[FAR] * 5) == N.ERR_INVALID_ARG  # m counts too
    assert "(k, m)" in N.last_error()
    # a null array is reported before the shape
    assert _call(enc, other, null=("srcs",)) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_bytes_for_a_zero_length_entry_are_refused(kind):
    """ecShardLength(len) > 0 = S: a zero-length entry takes no byte, and the length
    is looked at before the source (a null one here)."""
    enc = RS.New(K, M)
    plan = _plan(enc, kind=kind)
    s0 = B.split_plan_stats()
    for i in range(5):
        lens = [0] * 5
        lens[i] = 1
        for srcs in ([FAR] * 5, [0] * 5):
            assert _call(enc, plan, srcs=srcs, lens=lens) == N.ERR_INVALID_ARG
            assert "src_lens" in N.last_error() and f"entry {i}" in N.last_error()
    assert _call(enc, plan, srcs=[FAR] * 5, lens=[0, 0, 1 << 63, 0, 7]) == N.ERR_INVALID_ARG
    assert "entry 2" in N.last_error()  # the first bad entry is named
    assert B.split_plan_stats() == s0


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
@pytest.mark.parametrize("m", [0, 2])
def test_nothing_to_do_is_ok_and_launches_nothing(kind, m):
    enc = RS.New(K, m)
    s0 = B.split_plan_stats()
    plan = _plan(enc, kind=kind)
    assert _call(enc, plan) == N.HBEC_OK
    assert _call(enc, plan, srcs=[FAR] * 5) == N.HBEC_OK  # sources without lengths are not looked at
    empty = _plan(enc, 0, kind=kind)
    assert _call(enc, empty, n=0) == N.HBEC_OK
    B.set_split_plan_chunk_tiles(64)
    B.set_split_plan_chunk_tiles(0)
    assert B.split_plan_stats() == s0
    T = B.split_plan_tile_bytes()
    assert T > 0 and T % 16 == 0 and T == B.mixed_plan_tile_bytes()


def test_python_wrappers_check_shapes_before_a_stream_is_asked_for():
    enc = RS.New(K, M)
    plan = _plan(enc)
    with pytest.raises(ValueError):
        plan.split([0] * 4, [0] * 5)
    with pytest.raises(ValueError):
        plan.split([0] * 5, [0] * 6)
    plan.split([0] * 5, [0] * 5, stream=GH._NoStream())  # nothing to do: nothing queued
    for kind in ("stripes", "objects", "shards"):  # split_files is for plans built from files= alone
        with pytest.raises(ValueError, match="files"):
            _plan(enc, kind=kind).split_files([])
    f = B.StripePlan(enc, files=[([0] * (K + M), 0)] * 3, chunk_size=4096)
    with pytest.raises(ValueError):
        f.split_files([0] * 2)  # an address per object
    with pytest.raises(RS.ErrInvalidArg, match="src_lens"):
        plan.split([FAR] * 5, [0, 0, 3, 0, 0], stream=GH._NoStream())


def _files_call(enc, plan, starts, n_objects, lengths, chunk, srcs, null=()):
    st = np.ascontiguousarray(starts, dtype=np.uint32)
    ln = np.ascontiguousarray(lengths if len(lengths) else [0], dtype=np.uint64)
    d = (C.c_void_p * max(1, len(srcs)))(*[int(a) for a in srcs])
    return N.lib().hbec_split_plan_files(
        None if "codec" in null else enc.handle, None if "plan" in null else plan._h,
        None if "object_start" in null else st.ctypes.data_as(U32P), n_objects,
        None if "content_lengths" in null else ln.ctypes.data_as(U64P), chunk,
        None if "object_srcs" in null else d, None)


def test_split_files_argument_errors_on_empty_plans():
    enc = RS.New(K, M)
    s0 = B.split_plan_stats()
    f = B.StripePlan(enc, files=[([0] * (K + M), 0)] * 3, chunk_size=4096)
    args = (f.object_start, 3, [0, 0, 0], 4096, [0, 0, 0])
    assert _files_call(enc, f, *args) == N.HBEC_OK
    for null in ("codec", "plan", "content_lengths", "object_srcs"):
        assert _files_call(enc, f, *args, null=(null,)) == N.ERR_INVALID_ARG, null
        assert "null" in N.last_error(), null
    assert _files_call(RS.New(8, 3), f, *args) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    f.split_files([0, 0, 0], stream=GH._NoStream())  # nothing to do: nothing queued
    assert B.split_plan_stats() == s0


def source_errors():
    """The argument errors that need an entry with bytes in it.  Returns False
    where no plan with such an entry can be built (no device)."""
    enc = RS.New(K, M)
    S = 100
    row = [BASE + 3 * S * j for j in range(K + M)]  # shards 3 S apart
    plan = GH._shards_plan(enc, [row, [0] * (K + M), row], [S, 0, S])
    if plan is None:
        return False
    s0 = B.split_plan_stats()

    def call(srcs, lens):
        return _call(enc, plan, srcs=srcs, lens=lens, n=3)

    # every length but k S - k + 1 .. k S is refused, and the entry named
    for ln in (1, S, K * S - K, K * S + 1, 1 << 63):
        assert call([FAR, 0, FAR], [K * S, 0, ln]) == N.ERR_INVALID_ARG, ln
        assert "src_lens" in N.last_error() and "entry 2" in N.last_error()
    assert call([FAR, FAR, FAR], [K * S, 1, 1]) == N.ERR_INVALID_ARG
    assert "src_lens" in N.last_error() and "entry 1" in N.last_error()
    # the length is looked at before the source: null and overlapping ones here
    assert call([0, 0, row[0]], [K * S + 1, 0, K * S]) == N.ERR_INVALID_ARG
    assert "src_lens" in N.last_error() and "entry 0" in N.last_error()
    # a null source with a length (and none without)
    for pad in range(K):
        assert call([FAR, 0, 0], [K * S, 0, K * S - pad]) == N.ERR_INVALID_ARG
        assert "null source" in N.last_error() and "entry 2" in N.last_error()
    # a null source is reported before an overlap of a later entry, and an entry's own before its overlap
    assert call([0, 0, row[0]], [K * S, 0, K * S]) == N.ERR_INVALID_ARG
    assert "null source" in N.last_error() and "entry 0" in N.last_error()
    # a source over one of the entry's own shards, parity too: one byte is enough
    ln = K * S - 1
    for sh in range(K + M):
        for src in (row[sh] - ln + 1, row[sh] + S - 1, row[sh] - 5, row[sh]):
            assert call([FAR, 0, src], [0, 0, ln]) == N.ERR_INVALID_ARG, (sh, src - row[sh])
            assert "overlaps" in N.last_error() and "entry 2" in N.last_error()
    # none of this launched anything
    assert B.split_plan_stats() == s0

    # files: the entry lengths must be those of the content length, and the object is named
    chunk = 64
    L = 2 * K * chunk + 12  # stripes of 64, 64 and 3 bytes a shard
    files = [BASE + (1 << 20) * j for j in range(K + M)]
    f = B.StripePlan(enc, files=[(files, L), ([0] * (K + M), 0), (files, 5)], chunk_size=chunk)
    assert f.object_start.tolist() == [0, 3, 3, 4]
    good = (f.object_start, 3, [L, 0, 5], chunk, [FAR, 0, FAR + (1 << 20)])
    for bad_len, g in (([L + 1, 0, 5], 0), ([L - 8, 0, 5], 0), ([L + K * chunk, 0, 5], 0), ([L, 1, 5], 1),
                       ([L, 0, 9], 2), ([L, 0, 0], 2), ([L, 0, 1 << 63], 2)):
        assert _files_call(enc, f, good[0], 3, bad_len, *good[3:]) == N.ERR_INVALID_ARG, bad_len
        assert f"object {g}" in N.last_error(), (bad_len, N.last_error())
    assert _files_call(enc, f, good[0], 3, good[2], chunk // 2, good[4]) == N.ERR_INVALID_ARG
    assert "object 0" in N.last_error()
    assert _files_call(enc, f, good[0], 3, good[2], 0, good[4]) == N.ERR_INVALID_ARG
    assert "chunk_size" in N.last_error()
    # the object table is checked as hbec_hash_plan_files checks it
    for starts, n_obj in (([1, 3, 3, 4], 3), ([0, 3, 2, 4], 3), ([0, 3, 3, 5], 3), ([0, 3, 3, 4], 0)):
        assert _files_call(enc, f, starts, n_obj, *good[2:]) == N.ERR_INVALID_ARG, starts
        assert "object" in N.last_error()
    assert _files_call(enc, f, *good, null=("object_start",)) == N.ERR_INVALID_ARG
    # then it is the first call: its source checks, by entry
    assert _files_call(enc, f, *good[:4], [0, 0, FAR]) == N.ERR_INVALID_ARG
    assert "null source" in N.last_error() and "entry 0" in N.last_error()
    assert _files_call(enc, f, *good[:4], [FAR, 0, files[5] + 1]) == N.ERR_INVALID_ARG  # object 2 is entry 3
    assert "overlaps" in N.last_error() and "entry 3" in N.last_error()
    # object 0's second piece starts k chunk bytes into it: placed so that it is the first to reach a file
    assert _files_call(enc, f, *good[:4], [files[3] + chunk - K * chunk - K * chunk + 1, 0, FAR]) == N.ERR_INVALID_ARG
    assert "overlaps shard 3" in N.last_error() and "entry 1" in N.last_error()
    assert B.split_plan_stats() == s0
    return True


def test_source_errors_where_a_plan_with_bytes_can_be_built():
    source_errors()


def test_split_instances_use_no_scratch_and_no_lds():
    for fam in ("gf_split_plan", "gf_split_plan_rows"):
        found = KR.kernels(f"{fam}ILi")
        assert len(found) == 5, (fam, sorted(found))
        for r in range(5):
            assert any(f"{fam}ILi{r}E" in nm for nm in found), (fam, r)
        for nm, k in found.items():
            assert k[".private_segment_fixed_size"] == 0, nm
            assert k[".group_segment_fixed_size"] == 0, nm
