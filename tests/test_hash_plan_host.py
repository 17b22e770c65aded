"""The hash call's host side, without a device: csrc/hashplan.h's inline logic
(the where word of every selection and bad-shard set, the chain list a call
builds) through a stand-alone C++ program (tests/native/hash_plan_host.cpp)
under AddressSanitizer + UBSan, the new symbols of libhbec.so, every argument
error a plan of zero-length entries can provoke, and the resources of md5_plan
from the library's code-object metadata.

The program is compiled with the host compiler and run directly; it links no
libhbec and touches no device."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_repair_mixed_host as RH
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "hash_plan_host.cpp"
NEW = ["hbec_hash_plan_mixed", "hbec_hash_plan_stats"]
K, M = 4, 2


def test_hash_host_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "hash_plan_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{RH.ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    # every (selection, subset of it): 3^n pairs of 4+2 and 8+3
    assert f"hash_plan_host ok ({3 ** 6 + 3 ** 11} words, " in out.stdout


def test_new_symbols_are_exported_and_declared():
    lib = N.lib()
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS and f" {name}(" in header, name
    a = C.c_uint64()
    assert lib.hbec_hash_plan_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert lib.hbec_hash_plan_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert set(B.hash_plan_stats()) == {"kernel_launches", "chains"}
    assert hasattr(B.StripePlan, "hash_mixed")


def _call(enc, plan, select, select_of, n_select=None, flt=None, bits=1, expected=None, digests=None, bad=None,
          where=None):
    sel = np.ascontiguousarray(select, dtype=np.uint8).reshape(-1)
    idx = np.ascontiguousarray(select_of, dtype=np.uint32)
    ptr = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    return N.lib().hbec_hash_plan_mixed(
        enc.handle if enc is not None else None, plan._h if plan is not None else None,
        sel.ctypes.data_as(N._U8P) if sel.size else None, len(sel) // (K + M) if n_select is None else n_select,
        idx.ctypes.data_as(C.POINTER(C.c_uint32)) if idx.size else None, ptr(flt), bits, ptr(expected), ptr(digests),
        ptr(bad), ptr(where), None)


def test_argument_errors_need_no_device():
    """Pointers are only compared and tested for alignment here, never followed:
    every error is found before anything is queued or written."""
    enc, other = RS.New(K, M), RS.New(8, 3)
    plan = B.StripePlan(enc, stripes=[(0, 0)] * 5)  # zero-length entries: nothing to hash
    objs = B.StripePlan(enc, objects=[(0, 0, 0)] * 5)
    ones, idx = [1] * (K + M), [0] * 5
    D, E, BAD, W, F = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000  # stand-ins for device buffers
    before = B.hash_plan_stats()
    for p in (plan, objs):
        assert _call(enc, p, ones, idx, digests=D) == N.HBEC_OK
        assert _call(enc, p, ones, idx, expected=E, bad=BAD, where=W, flt=F, digests=D) == N.HBEC_OK
        assert _call(enc, p, [0] * (K + M), idx, digests=D) == N.HBEC_OK  # a row may select nothing
        bad_calls = [
            _call(None, p, ones, idx, digests=D),
            _call(enc, None, ones, idx, digests=D),
            _call(other, p, [1] * 11, idx, digests=D, n_select=1),  # a plan of another (k, m)
            _call(enc, p, [], idx, digests=D),  # null select
            _call(enc, p, ones, [], digests=D, n_select=1),  # null select_of
            _call(enc, p, ones, idx, digests=D, n_select=0),
            _call(enc, p, ones, idx, digests=D, n_select=65537),
            _call(enc, p, ones, [0, 0, 1, 0, 0], digests=D),  # index >= n_select, on a zero-length entry
            _call(enc, p, ones, idx),  # neither digests nor expected
            _call(enc, p, ones, idx, digests=D, bad=None, where=W),  # where without bad
            _call(enc, p, ones, idx, expected=E),  # expected without bad
            _call(enc, p, ones, idx, digests=D, bad=BAD, where=BAD),
            _call(enc, p, ones, idx, digests=D, bad=BAD, flt=BAD),
            _call(enc, p, ones, idx, digests=D, bad=BAD, where=W, flt=W),
            _call(enc, p, ones, idx, digests=D + 2),
            _call(enc, p, ones, idx, digests=D, expected=E + 1, bad=BAD),
        ]
        assert bad_calls == [N.ERR_INVALID_ARG] * len(bad_calls), bad_calls
    # expected needs one bit per shard: k + m <= 32
    wide = RS.New(28, 8)
    wplan = B.StripePlan(wide, stripes=[(0, 0)] * 2)
    sel = np.ones(36, np.uint8)
    i2 = np.zeros(2, np.uint32)
    call = lambda **kw: N.lib().hbec_hash_plan_mixed(  # noqa: E731
        wide.handle, wplan._h, sel.ctypes.data_as(N._U8P), 1, i2.ctypes.data_as(C.POINTER(C.c_uint32)), None, 1,
        kw.get("expected"), kw.get("digests"), kw.get("bad"), None, None)
    assert call(expected=C.c_void_p(E), bad=C.c_void_p(BAD)) == N.ERR_INVALID_ARG
    assert call(digests=C.c_void_p(D)) == N.HBEC_OK
    # a plan with no entries accepts null arrays and null device pointers
    empty = B.StripePlan(enc, stripes=[])
    assert _call(enc, empty, [], [], n_select=0) == N.HBEC_OK
    assert B.hash_plan_stats() == before  # nothing was launched or listed


def test_python_wrapper_checks_its_arrays():
    enc = RS.New(K, M)
    plan = B.StripePlan(enc, stripes=[(0, 0)] * 3)
    with pytest.raises(ValueError):
        plan.hash_mixed(np.ones((2, K + M)))
    with pytest.raises(ValueError):
        plan.hash_mixed(np.ones((3, K + M + 1)))


def test_md5_plan_uses_no_scratch_and_no_lds():
    import test_kernel_resources as KR

    ks = {**KR.kernels("8md5_planE"), **KR.kernels("10hash_whereE")}
    plan = [k for nm, k in ks.items() if "8md5_planE" in nm]
    where = [k for nm, k in ks.items() if "10hash_whereE" in nm]
    assert len(plan) >= 1 and len(where) == 1, sorted(ks)
    for k in plan + where:
        assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, k[".name"]
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k[".name"]
    # two load groups of 17 dwords per block in flight beside the block being compressed
    assert all(k[".vgpr_count"] <= 128 for k in plan), [k[".vgpr_count"] for k in plan]
