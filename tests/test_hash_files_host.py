"""The shard-file hash call's host side, without a device: csrc/hashfiles.h's
inline logic (the check of the object table, the chain list a call builds, the
object of every entry) through a stand-alone C++ program
(tests/native/hash_files_host.cpp) under AddressSanitizer + UBSan, the new
symbols of libhbec.so, every argument error a plan of zero-length entries can
provoke, the Python wrapper's shape checks, and the resources of md5_files and
hash_files_where from the library's code-object metadata.

The program is compiled with the host compiler and run directly; it links no
libhbec and touches no device."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_repair_mixed_host as RH
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "hash_files_host.cpp"
NEW = ["hbec_hash_plan_files", "hbec_hash_files_stats"]
K, M = 4, 2
U32P = C.POINTER(C.c_uint32)


def test_hash_files_host_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "hash_files_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{RH.ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = re.search(r"hash_files_host ok \((\d+) tables, (\d+) chains, (\d+) segments\)", out.stdout)
    assert got, out.stdout
    tables, chains, segments = map(int, got.groups())
    assert tables > 200 and chains > 1000 and segments > chains  # objects of several pieces were walked


def test_new_symbols_are_exported_and_declared():
    lib = N.lib()
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS and f" {name}(" in header, name
    a, b = C.c_uint64(), C.c_uint64()
    assert lib.hbec_hash_files_stats(None, C.byref(a), C.byref(b)) == N.ERR_INVALID_ARG
    assert lib.hbec_hash_files_stats(C.byref(a), None, C.byref(b)) == N.ERR_INVALID_ARG
    assert lib.hbec_hash_files_stats(C.byref(a), C.byref(b), None) == N.ERR_INVALID_ARG
    assert set(B.hash_files_stats()) == {"kernel_launches", "chains", "segments"}
    assert hasattr(B.StripePlan, "hash_files")


def _call(enc, plan, starts, select, select_of, n_objects=None, n_select=None, flt=None, bits=1, expected=None,
          digests=None, bad=None, where=None, n=K + M):
    st = np.ascontiguousarray(starts, dtype=np.uint32)
    sel = np.ascontiguousarray(select, dtype=np.uint8).reshape(-1)
    idx = np.ascontiguousarray(select_of, dtype=np.uint32)
    ptr = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    return N.lib().hbec_hash_plan_files(
        enc.handle if enc is not None else None, plan._h if plan is not None else None,
        st.ctypes.data_as(U32P) if st.size else None, max(0, len(st) - 1) if n_objects is None else n_objects,
        sel.ctypes.data_as(N._U8P) if sel.size else None, len(sel) // n if n_select is None else n_select,
        idx.ctypes.data_as(U32P) if idx.size else None, ptr(flt), bits, ptr(expected), ptr(digests), ptr(bad),
        ptr(where), None)


def test_argument_errors_need_no_device():
    """Pointers are only compared and tested for alignment here, never followed:
    every error is found before anything is queued or written."""
    enc, other = RS.New(K, M), RS.New(8, 3)
    plan = B.StripePlan(enc, stripes=[(0, 0)] * 5)  # zero-length entries: nothing to hash
    objs = B.StripePlan(enc, objects=[(0, 0, 0)] * 5)
    ones = [1] * (K + M)
    st, idx = [0, 2, 2, 5], [0, 0, 0]
    D, E, BAD, W, F = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000  # stand-ins for device buffers
    before = B.hash_files_stats()
    for p in (plan, objs):
        assert _call(enc, p, st, ones, idx, digests=D) == N.HBEC_OK
        assert _call(enc, p, [0, 5], ones, [0], digests=D) == N.HBEC_OK
        assert _call(enc, p, st, ones, idx, expected=E, bad=BAD, where=W, flt=F, digests=D) == N.HBEC_OK
        assert _call(enc, p, st, [0] * (K + M), idx, digests=D) == N.HBEC_OK  # a row may select nothing
        bad_calls = [
            _call(None, p, st, ones, idx, digests=D),
            _call(enc, None, st, ones, idx, digests=D),
            _call(other, p, st, [1] * 11, idx, digests=D, n_select=1),  # a plan of another (k, m)
            _call(enc, p, [], ones, idx, digests=D, n_objects=3),  # null object_start
            _call(enc, p, st, ones, idx, digests=D, n_objects=0),
            _call(enc, p, [1, 2, 2, 5], ones, idx, digests=D),  # does not start at 0
            _call(enc, p, [0, 3, 2, 5], ones, idx, digests=D),  # decreases
            _call(enc, p, [0, 2, 6, 5], ones, idx, digests=D),  # decreases at the end
            _call(enc, p, [0, 2, 2, 4], ones, idx, digests=D),  # ends short of the entry count
            _call(enc, p, [0, 2, 2, 6], ones, idx, digests=D),  # ends past it
            _call(enc, p, st, [], idx, digests=D, n_select=1),  # null select
            _call(enc, p, st, ones, [], digests=D),  # null select_of
            _call(enc, p, st, ones, idx, digests=D, n_select=0),
            _call(enc, p, st, ones, idx, digests=D, n_select=65537),
            _call(enc, p, st, ones, [0, 1, 0], digests=D),  # index >= n_select, on an object with no entries
            _call(enc, p, st, ones, idx),  # neither digests nor expected
            _call(enc, p, st, ones, idx, digests=D, bad=None, where=W),  # where without bad
            _call(enc, p, st, ones, idx, expected=E),  # expected without bad
            _call(enc, p, st, ones, idx, digests=D, bad=BAD, where=BAD),
            _call(enc, p, st, ones, idx, digests=D, bad=BAD, flt=BAD),
            _call(enc, p, st, ones, idx, digests=D, bad=BAD, where=W, flt=W),
            _call(enc, p, st, ones, idx, digests=D + 2),
            _call(enc, p, st, ones, idx, digests=D, expected=E + 1, bad=BAD),
        ]
        assert bad_calls == [N.ERR_INVALID_ARG] * len(bad_calls), bad_calls
    # expected needs one bit per shard: k + m <= 32
    wide = RS.New(28, 8)
    wplan = B.StripePlan(wide, stripes=[(0, 0)] * 2)
    w1 = [1] * 36
    assert _call(wide, wplan, [0, 2], w1, [0], expected=E, bad=BAD, n=36) == N.ERR_INVALID_ARG
    assert _call(wide, wplan, [0, 2], w1, [0], digests=D, n=36) == N.HBEC_OK
    # a plan with no entries accepts null arrays and null device pointers
    empty = B.StripePlan(enc, stripes=[])
    assert _call(enc, empty, [], [], [], n_objects=0, n_select=0) == N.HBEC_OK
    assert _call(enc, empty, [0], [], [], n_select=0) == N.HBEC_OK
    assert B.hash_files_stats() == before  # nothing was launched or listed


def test_python_wrapper_checks_its_arrays():
    enc = RS.New(K, M)
    plan = B.StripePlan(enc, stripes=[(0, 0)] * 3)
    with pytest.raises(ValueError):
        plan.hash_files([0, 1, 3], np.ones((3, K + M)))  # a row per object, not per entry
    with pytest.raises(ValueError):
        plan.hash_files([0, 1, 3], np.ones((2, K + M + 1)))
    with pytest.raises(ValueError):
        plan.hash_files([[0, 3]])
    with pytest.raises(ValueError):
        plan.hash_files([])
    with pytest.raises(ValueError):
        plan.hash_files([0.0, 3.0])
    with pytest.raises(ValueError):
        plan.hash_files([0, -1, 3])


def test_md5_files_uses_no_scratch_and_no_lds():
    import test_kernel_resources as KR

    ks = {**KR.kernels("9md5_filesE"), **KR.kernels("16hash_files_whereE")}
    files = [k for nm, k in ks.items() if "9md5_filesE" in nm]
    where = [k for nm, k in ks.items() if "16hash_files_whereE" in nm]
    assert len(files) == 1 and len(where) == 1, sorted(ks)
    for k in files + where:
        assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, k[".name"]
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k[".name"]
    # md5_plan's bound: the same two load groups in flight, plus two cursors
    assert all(k[".vgpr_count"] <= 128 for k in files), [k[".vgpr_count"] for k in files]
