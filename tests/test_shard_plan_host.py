"""Shards plans without a device: the new symbols of libhbec.so, every argument
error of hbec_plan_shards and hbec_plan_files (all found before the first device
call), ecSplit's stripe arithmetic against the oracle, csrc/shardplan.h alone
under AddressSanitizer + UBSan (tests/native/shard_plan_host.cpp, a stand-alone
program that links no libhbec), and the resources of the `_rows` kernels and of
their twins from the library's code-object metadata.

The twins' figures on the commit before the `_rows` kernels were added are in
tests/golden/shard_plan_kernel_resources.json: adding the new instances must not
have moved a register of an existing one."""
import ctypes as C
import json
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
SRC = ROOT / "tests" / "native" / "shard_plan_host.cpp"
GOLDEN = ROOT / "tests" / "golden" / "shard_plan_kernel_resources.json"
NEW = ["hbec_plan_shards", "hbec_plan_files", "hbec_ec_stripe_count", "hbec_ec_stripe_shard_length"]
K, M = 4, 2
U64P = C.POINTER(C.c_uint64)
U32P = C.POINTER(C.c_uint32)
BASE = 0x7000_0000_0000  # addresses are compared and sorted here, never followed


def test_new_symbols_are_exported_and_declared():
    lib = N.lib()
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS and f" {name}(" in header, name
    assert "hbec_file_object" in header
    assert lib.hbec_version() == 2  # additive
    assert hasattr(E, "ec_stripe_count") and hasattr(E, "ec_stripe_shard_length")


def test_shard_plan_host_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "shard_plan_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = re.search(r"shard_plan_host ok \((\d+) rows, (\d+) lengths\)", out.stdout)
    assert got, out.stdout
    assert int(got.group(1)) == 200000 and int(got.group(2)) > 10000


def _plan_shards(enc, rows, lens, n_entries=None, null=()):
    """hbec_plan_shards on host arrays; returns (rc, handle)."""
    rows = [int(a) for row in rows for a in row]
    ptrs = (C.c_void_p * max(1, len(rows)))(*rows)
    ln = np.ascontiguousarray(lens if len(lens) else [0], dtype=np.uint64)
    h = C.c_void_p()
    rc = N.lib().hbec_plan_shards(
        None if "codec" in null else enc.handle, None if "shards" in null else ptrs,
        None if "lens" in null else ln.ctypes.data_as(U64P), len(lens) if n_entries is None else n_entries,
        None if "out" in null else C.byref(h))
    return rc, h


def _free(h):
    if h:
        N.lib().hbec_plan_free(h)


def _row(S, order=None, gap=0):
    """k+m shards of S bytes back to back (ranges touch), or `gap` bytes apart, in `order`."""
    order = list(range(K + M)) if order is None else order
    row = [0] * (K + M)
    for pos, sh in enumerate(order):
        row[sh] = BASE + pos * (S + gap)
    return row


def test_plan_shards_argument_errors_need_no_device():
    enc = RS.New(K, M)
    good = [_row(100)]
    for null in ("codec", "shards", "lens", "out"):
        rc, h = _plan_shards(enc, good, [0], null=(null,))
        assert rc == N.ERR_INVALID_ARG, null
        assert not h
    # null arrays are refused for no entries too
    assert _plan_shards(enc, [], [], null=("shards",))[0] == N.ERR_INVALID_ARG
    assert _plan_shards(enc, [], [], null=("lens",))[0] == N.ERR_INVALID_ARG
    # 2^32 entries or more: refused before the arrays are read
    assert _plan_shards(enc, good, [0], n_entries=1 << 32)[0] == N.ERR_INVALID_ARG
    # a null shard pointer counts only where shard_len > 0
    for sh in range(K + M):
        row = _row(64)
        row[sh] = 0
        rc, h = _plan_shards(enc, [_row(64), row], [0, 64])
        assert rc == N.ERR_INVALID_ARG and not h, sh
        assert "null shard pointer" in N.last_error() and "entry 1" in N.last_error()
        rc, h = _plan_shards(enc, [row, row], [0, 0])
        assert rc == N.HBEC_OK and h
        _free(h)
    # overlap inside an entry: equal addresses, one byte shared, one shard inside another's range
    S = 100
    for a, b in ((0, 1), (0, K + M - 1), (K - 1, K), (2, 5)):
        for delta in (0, 1, S - 1, -(S - 1)):
            row = _row(S, gap=3 * S)
            row[b] = row[a] + delta
            rc, h = _plan_shards(enc, [row], [S])
            assert rc == N.ERR_INVALID_ARG and not h, (a, b, delta)
            assert "overlap" in N.last_error()
    # the same row is fine for an entry of no bytes, and overlap ACROSS entries is the caller's business:
    # it passes the check (what follows needs a device, so without one the code is the device's)
    rc, h = _plan_shards(enc, [_row(S), _row(S)], [0, 0])
    assert rc == N.HBEC_OK and h
    _free(h)


@pytest.mark.parametrize("order", [None, [5, 0, 3, 1, 4, 2]])
def test_adjacent_shards_pass_the_overlap_check(order):
    """Ranges that touch do not overlap: the checks pass and the build goes on to the
    device.  With a GPU it succeeds (no address is followed at build time); without
    one it fails there, with the device's code and not HBEC_ERR_INVALID_ARG."""
    enc = RS.New(K, M)
    for S in (1, 16, 17, 4097):
        rc, h = _plan_shards(enc, [_row(S, order), _row(S, order)], [S, S])
        assert rc != N.ERR_INVALID_ARG, (S, N.last_error())
        assert (rc == N.HBEC_OK) == bool(h)
        _free(h)


def _plan_files(enc, objects, chunk, null=(), n_objects=None):
    n = enc.DataShards + enc.ParityShards
    objs = (N.FileObject * max(1, len(objects)))()
    keep = []
    for i, (files, length) in enumerate(objects):
        if files is not None:
            arr = (C.c_void_p * n)(*[int(f) for f in files])
            keep.append(arr)
            objs[i].files = C.cast(arr, C.POINTER(C.c_void_p))
        objs[i].content_length = length
    starts = np.full(len(objects) + 1, 0xFFFFFFFF, np.uint32)
    h = C.c_void_p()
    rc = N.lib().hbec_plan_files(
        None if "codec" in null else enc.handle, None if "objects" in null else objs,
        len(objects) if n_objects is None else n_objects, chunk,
        None if "starts" in null else starts.ctypes.data_as(U32P), None if "out" in null else C.byref(h))
    return rc, h, starts


def test_plan_files_argument_errors_need_no_device():
    enc = RS.New(K, M)
    files = [BASE + j * (1 << 30) for j in range(K + M)]
    for null in ("codec", "objects", "starts", "out"):
        rc, h, _ = _plan_files(enc, [(files, 0)], 1024, null=(null,))
        assert rc == N.ERR_INVALID_ARG and not h, null
    assert _plan_files(enc, [(files, 10)], 0)[0] == N.ERR_INVALID_ARG  # chunk_size = 0
    assert "chunk_size" in N.last_error()
    # more than 2^32 - 1 entries: counted before anything is built
    rc, h, _ = _plan_files(enc, [(files, (1 << 31) * K)] * 2, 1)
    assert rc == N.ERR_INVALID_ARG and not h and "entries" in N.last_error()
    # a null file pointer counts only in an object with bytes
    for j in range(K + M):
        f = list(files)
        f[j] = 0
        rc, h, _ = _plan_files(enc, [(files, 0), (f, 1)], 1024)
        assert rc == N.ERR_INVALID_ARG and not h and "object 1" in N.last_error(), j
    assert _plan_files(enc, [(None, 1)], 1024)[0] == N.ERR_INVALID_ARG
    # files of one object that overlap
    f = list(files)
    f[3] = f[2] + 5
    assert _plan_files(enc, [(f, 1000)], 64)[0] == N.ERR_INVALID_ARG
    assert "overlap" in N.last_error()
    # zero-length objects have no entries: nothing for a device to do
    f0 = [0] * (K + M)
    rc, h, starts = _plan_files(enc, [(f0, 0), (None, 0), (files, 0)], 1024)
    assert rc == N.HBEC_OK and h
    assert starts.tolist() == [0, 0, 0, 0]
    nt, fb, sb, tb = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7), C.c_int(7)
    assert N.lib().hbec_plan_info(h, C.byref(nt), C.byref(tb), C.byref(fb), C.byref(sb)) == N.HBEC_OK
    assert (nt.value, tb.value, fb.value, sb.value) == (0, 0, 0, 0)
    _free(h)
    rc, h, starts = _plan_files(enc, [], 1024)
    assert rc == N.HBEC_OK and h and starts.tolist() == [0]
    _free(h)


def test_python_wrapper_without_device():
    enc = RS.New(K, M)
    p = B.StripePlan(enc, shards=[([0] * (K + M), 0)] * 3)
    assert p.info() == {"n_tiles": 0, "tile_bytes": 0, "n_fallback": 0, "shard_bytes": 0}
    # the uniform calls take it; with nothing but zero-length entries none launches anything
    lib = N.lib()
    mask = (C.c_uint8 * (K + M))(*([1] * K + [0] * M))
    assert lib.hbec_encode_plan(enc.handle, p._h, None) == N.HBEC_OK
    assert lib.hbec_reconstruct_plan(enc.handle, p._h, mask, 0, None) == N.HBEC_OK
    assert lib.hbec_verify_plan(enc.handle, p._h, C.c_void_p(16), None) == N.HBEC_OK
    assert lib.hbec_encode_plan(RS.New(8, 3).handle, p._h, None) == N.ERR_INVALID_ARG  # another (k, m)
    f = B.StripePlan(enc, files=[([0] * (K + M), 0)] * 2, chunk_size=4096)
    assert f.object_start.dtype == np.uint32 and f.object_start.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        B.StripePlan(enc, files=[([0] * (K + M), 0)])  # no chunk_size
    with pytest.raises(ValueError):
        B.StripePlan(enc, shards=[([0] * K, 0)])  # not k+m addresses
    with pytest.raises(ValueError):
        B.StripePlan(enc, shards=[], stripes=[])
    with pytest.raises(RS.ErrInvalidArg):
        B.StripePlan(enc, shards=[([0] * (K + M), 5)])


def _go_shard_length(L, k, chunk, done):
    """ecutils.go:85-92, literally."""
    expected = chunk
    if L - done < chunk * k:
        expected = (L - done) // k
        if (L - done) % k != 0:
            expected += 1
    return expected


@pytest.mark.parametrize("chunk", [1, 5, 1024])
@pytest.mark.parametrize("k", [1, 3, 4, 8])
def test_stripe_arithmetic_matches_ec_split(k, chunk, monkeypatch):
    cuts = []
    real = O.Encoder.encode

    def counting(self, shards):
        cuts.append(len(shards[0]))
        return real(self, shards)

    monkeypatch.setattr(O.Encoder, "encode", counting)
    lib = N.lib()
    n, s = C.c_uint64(), C.c_uint64()
    data = bytes(3 * k * chunk + k)
    for L in range(0, 3 * k * chunk + k + 1):
        assert lib.hbec_ec_stripe_count(L, k, chunk, C.byref(n)) == N.HBEC_OK
        del cuts[:]
        files = O.ec_split(k, 0, data[:L], chunk)  # the stripes it cuts, one encode each
        assert n.value == len(cuts), L
        total, done = 0, 0
        for t in range(n.value):
            assert lib.hbec_ec_stripe_shard_length(L, k, chunk, t, C.byref(s)) == N.HBEC_OK
            assert s.value == _go_shard_length(L, k, chunk, done) == cuts[t], (L, t)
            total += s.value
            done += min(k * chunk, L - done)
        assert total == O.ec_shard_length(L, k) == len(files[0]) == E.ec_shard_length(L, k), L
        assert lib.hbec_ec_stripe_shard_length(L, k, chunk, n.value, C.byref(s)) == N.ERR_INVALID_ARG
    assert E.ec_stripe_count(2 * k * chunk + 1, k, chunk) == 3
    assert E.ec_stripe_shard_length(2 * k * chunk + 1, k, chunk, 2) == 1


def test_stripe_arithmetic_argument_errors():
    lib = N.lib()
    n = C.c_uint64(99)
    assert lib.hbec_ec_stripe_count(10, 4, 4, None) == N.ERR_INVALID_ARG
    assert lib.hbec_ec_stripe_count(10, 0, 4, C.byref(n)) == N.ERR_INVALID_ARG
    assert lib.hbec_ec_stripe_count(10, 4, 0, C.byref(n)) == N.ERR_INVALID_ARG
    assert lib.hbec_ec_stripe_shard_length(10, 4, 4, 0, None) == N.ERR_INVALID_ARG
    assert lib.hbec_ec_stripe_shard_length(10, -1, 4, 0, C.byref(n)) == N.ERR_INVALID_ARG
    assert lib.hbec_ec_stripe_shard_length(0, 4, 4, 0, C.byref(n)) == N.ERR_INVALID_ARG  # no stripes
    assert lib.hbec_ec_stripe_count(-5, 4, 4, C.byref(n)) == N.HBEC_OK and n.value == 0
    with pytest.raises(RS.ErrInvalidArg):
        E.ec_stripe_shard_length(16, 4, 4, 1)


# ---- kernel resources ----

FAMILIES = ("gf_mixed_plan", "gf_verify_mixed_plan", "gf_repair_mixed_plan", "gf_heal_mixed_plan",
            "gf_locate_mixed_plan", "md5_plan", "md5_files")


@pytest.fixture(scope="module")
def kernels():
    return KR.kernels("")


def _figures(k):
    return {"vgpr": k[".vgpr_count"], "sgpr": k[".sgpr_count"], "scratch": k[".private_segment_fixed_size"],
            "lds": k[".group_segment_fixed_size"]}


def _waves_per_simd(k):
    """512 registers per lane and SIMD, allocated 8 at a time, at most 8 waves."""
    regs = k[".vgpr_count"] + k.get(".agpr_count", 0)
    return min(8, 512 // (8 * ((regs + 7) // 8)))


def _mangled(family, rows):
    name = family + ("_rows" if rows else "")
    return f"_ZN4hbec{len(name)}{name}"


def test_existing_instances_kept_their_registers(kernels):
    want = json.loads(GOLDEN.read_text())
    assert len(want) == 5 * 4 + 2
    for fam in FAMILIES:
        assert any(n.startswith(_mangled(fam, False)) for n in want), fam
    for name, fig in want.items():
        assert name in kernels, f"{name} is gone"
        assert _figures(kernels[name]) == fig, name


def test_rows_instances_against_their_twins(kernels):
    seen = 0
    for fam in FAMILIES:
        old, new = _mangled(fam, False), _mangled(fam, True)
        twins = {n: k for n, k in kernels.items() if n.startswith(old) and not n.startswith(new)}
        rows = {n: k for n, k in kernels.items() if n.startswith(new)}
        assert len(twins) == len(rows) == (1 if fam.startswith("md5") else 4), fam
        for n, k in rows.items():
            twin = twins[old + n[len(new):]]  # same template arguments, same parameters
            if twin[".private_segment_fixed_size"] == 0:
                assert k[".private_segment_fixed_size"] == 0, n
            if twin[".group_segment_fixed_size"] == 0:
                assert k[".group_segment_fixed_size"] == 0, n
            assert _waves_per_simd(k) == _waves_per_simd(twin), (n, k[".vgpr_count"], twin[".vgpr_count"])
            seen += 1
    assert seen == 22
