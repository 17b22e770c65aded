"""The locate call's host side, without a device: hbec_locate_decode over every
class of word, the per-byte rule loc_classify and the rest of csrc/locate.h's
inline logic through a stand-alone C++ program (tests/native/locate_host.cpp)
under AddressSanitizer + UBSan, and the new symbols of libhbec.so.  The program
is compiled with the host compiler and run directly; it links no libhbec and
touches no device."""
import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from hummingbird_amd import _native as N
from hummingbird_amd import batch as B

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "locate_host.cpp"
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
NEW = ["hbec_locate_plan_mixed", "hbec_locate_decode", "hbec_locate_plan_stats", "hbec_locate_plan_tile_bytes",
       "hbec_set_locate_plan_chunk_tiles"]


def host_compiler():
    for c in (str(ROCM / "lib" / "llvm" / "bin" / "clang++"), "clang++", "g++", "c++"):
        w = c if os.path.isabs(c) and os.path.exists(c) else shutil.which(c)
        if w:
            return w
    raise AssertionError("no host C++ compiler found")


def test_locate_host_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "locate_host"
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "locate_host ok" in out.stdout


def test_new_symbols_are_exported_and_declared():
    lib = N.lib()
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS and f" {name}(" in header, name
    assert lib.hbec_locate_plan_tile_bytes() == lib.hbec_verify_mixed_plan_tile_bytes() == 4 * 992
    assert B.locate_plan_tile_bytes() == 4 * 992
    a = C.c_uint64()
    assert lib.hbec_locate_plan_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert lib.hbec_locate_plan_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert set(B.locate_plan_stats()) == {"kernel_launches", "skipped_entries"}
    # null arguments are found before the plan is looked at
    pat = (C.c_uint8 * 6)(1, 1, 1, 1, 1, 1)
    idx = (C.c_uint32 * 1)(0)
    assert lib.hbec_locate_plan_mixed(None, None, pat, 1, idx, None, None, None) == N.ERR_INVALID_ARG
    assert (N.LOC_BAD, N.LOC_SKIPPED, N.LOC_NOTHING) == (1 << 31, 1 << 30, 1 << 29)


def test_locate_plan_instances_use_no_scratch_and_no_lds():
    """RMAX = 1..4: the cold path selects accumulators with a chain on a uniform
    counter, so nothing is indexed in private memory, and it must not cost the
    hot path a wave: each instance stays in the occupancy step of its Verify
    twin (96 / 116 / 134 / 152 VGPRs: 5 / 4 / 3 / 3 waves per SIMD)."""
    import test_kernel_resources as KR

    found = KR.kernels("gf_locate_mixed_planILi")
    assert len(found) == 4, sorted(found)
    step = {1: 96, 2: 128, 3: 168, 4: 168}  # the largest allocation with Verify's waves per SIMD
    for r in range(1, 5):
        (k,) = [k for nm, k in found.items() if f"gf_locate_mixed_planILi{r}E" in nm]
        assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, r
        assert k[".vgpr_spill_count"] == 0, r
        assert k[".vgpr_count"] <= step[r], (r, k[".vgpr_count"])


def decode(k, m, present, where):
    p = np.ascontiguousarray(present, np.uint8)
    return N.lib().hbec_locate_decode(k, m, p.ctypes.data_as(N._U8P), where)


def test_locate_decode_every_class_of_word():
    full = [1] * 6
    assert decode(4, 2, full, 0) == N.LOC_CLEAN == -1
    for j in range(6):
        assert decode(4, 2, full, N.LOC_BAD | (0x3F & ~(1 << j))) == j
    assert decode(4, 2, full, N.LOC_BAD) == N.LOC_AMBIGUOUS == -2  # one check only: nothing ruled out
    assert decode(4, 2, full, N.LOC_BAD | 0x03) == N.LOC_AMBIGUOUS
    assert decode(4, 2, full, N.LOC_BAD | 0x3F) == N.LOC_MULTIPLE == -3
    assert decode(4, 2, full, N.LOC_SKIPPED) == N.LOC_UNCHECKED == -4
    assert decode(4, 2, full, N.LOC_NOTHING) == N.LOC_UNCHECKED
    assert decode(4, 2, full, N.LOC_BAD | N.LOC_SKIPPED | 0x3E) == N.LOC_UNCHECKED
    # a missing shard is no candidate: shards 0 1 3 4 5 present, 0 1 4 5 ruled out
    lost = [1, 1, 0, 7, 255, 1]
    assert decode(4, 2, lost, N.LOC_BAD | 0x33) == 3
    assert decode(4, 2, lost, N.LOC_BAD | 0x3B) == N.LOC_MULTIPLE
    # 5 of 6 present and nothing ruled out (r = 1)
    assert decode(4, 2, lost, N.LOC_BAD) == N.LOC_AMBIGUOUS
    assert decode(12, 4, [1] * 16, N.LOC_BAD | 0x7FFF) == 15
    assert decode(12, 4, [1] * 16, N.LOC_BAD | 0xFFFE) == 0
    assert N.lib().hbec_locate_decode(4, 2, None, 0) == N.ERR_INVALID_ARG
    assert decode(0, 2, full, 0) == N.ERR_INVALID_ARG
    assert decode(4, -1, full, 0) == N.ERR_INVALID_ARG


def test_batch_locate_decode_takes_arrays():
    where = np.array([0, N.LOC_BAD | 0x3E, N.LOC_BAD | 0x3F, N.LOC_BAD, N.LOC_NOTHING, N.LOC_SKIPPED,
                      N.LOC_BAD | 0x1F], np.uint32)
    got = B.locate_decode(4, 2, None, where)
    assert got.tolist() == [N.LOC_CLEAN, 0, N.LOC_MULTIPLE, N.LOC_AMBIGUOUS, N.LOC_UNCHECKED, N.LOC_UNCHECKED, 5]
    # int32 words (a torch.int32 tensor's view of the same bits) decode alike
    assert B.locate_decode(4, 2, None, where.view(np.int32)).tolist() == got.tolist()
    present = np.ones((7, 6), np.uint8)
    present[6, 5] = 0  # the only shard left is missing: nobody
    assert B.locate_decode(4, 2, present, where)[6] == N.LOC_MULTIPLE
    with pytest.raises(ValueError):
        B.locate_decode(4, 2, np.ones((3, 6), np.uint8), where)
    with pytest.raises(ValueError):
        B.locate_decode(4, 2, np.ones((7, 5), np.uint8), where)
