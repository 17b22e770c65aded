"""hbec_glue_plan_range_checked without a device, in the manner of tests/test_glue_checked_host.py."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import test_kernel_resources as KR
import test_repair_mixed_host as RH
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "gluerangecheck_host.cpp"
K, M = 4, 2


def test_new_symbols_are_exported_declared_and_cited():
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in ("hbec_glue_plan_range_checked", "hbec_glue_plan_files_range_checked", "hbec_glue_range_checked_stats",
                 "hbec_glue_range_checked_tile_bytes", "hbec_set_glue_range_checked_chunk_tiles"):
        assert hasattr(N.lib(), name) and name in N.SYMBOLS and f" {name}(" in header, name
        above = header[:header.index(f" {name}(")]
        assert "ecobj.go:207-267" in above[above.rindex("/*"):] and "ecobj.go:173-203" in above[above.rindex("/*"):], name
    above = header[:header.index(" hbec_glue_plan_range_checked(")]
    assert "hbec_etag_plan_mixed) is what catches it" in above[above.rindex("/*"):]  # the r = 2 caveat
    assert B.glue_range_checked_tile_bytes() == B.glue_range_tile_bytes() == B.glue_checked_tile_bytes()
    assert hasattr(B.StripePlan, "glue_range_checked") and hasattr(B.StripePlan, "glue_range_files_checked")


def test_byte_mask_over_the_examined_positions_under_sanitizers(tmp_path):
    text = SRC.read_text()
    assert "csrc/gluerangecheck.h" in text and "hbec.h" not in text and "int main(" in text
    for h in ("gluerangecheck.h", "gluerange.h"):  # both compile without HIP
        inc = re.findall(r'#include\s+[<"]([^>"]+)[>"]', (ROOT / "hummingbird_amd" / "csrc" / h).read_text())
        assert not [x for x in inc if "hip" in x], h
    exe = tmp_path / "gluerangecheck_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = re.search(r"gluerangecheck_host ok \((\d+) masks\)", out.stdout)
    # every (S, k, s <= e) and every dword below S + 16
    assert got and int(got.group(1)) == sum((k * s + 1) * (k * s + 2) // 2 * ((s + 19) // 4)
                                            for s in range(1, 41) for k in range(1, 5)), out.stdout


def test_argument_errors_and_their_precedence():
    enc = RS.New(K, M)
    plan, s0 = B.StripePlan(enc, stripes=[(0, 0)] * 5), B.glue_range_checked_stats()
    pat, of = np.ones((1, K + M), np.uint8), (C.c_uint32 * 5)()
    d, st, ln, fixed = (C.c_void_p * 5)(), (C.c_uint64 * 5)(), (C.c_uint64 * 5)(), (C.c_uint32 * 5)()
    good = [enc.handle, plan._h, pat.ctypes.data_as(N._U8P), 1, of, d, st, ln, fixed]
    call, other = N.lib().hbec_glue_plan_range_checked, RS.New(8, 3)
    for i in (0, 1, 2, 4, 5, 6, 7, 8):  # a null codec, plan, patterns, pattern_of, dsts, starts, lens, d_fixed
        assert call(*good[:i], None, *good[i + 1:], None) == N.ERR_INVALID_ARG
        assert "null" in N.last_error(), i
    assert call(other.handle, *good[1:], None) == N.ERR_INVALID_ARG and "(k, m)" in N.last_error()
    assert call(*good[:3], 0, *good[4:], None) == N.ERR_INVALID_ARG and "no patterns" in N.last_error()
    few = np.array([[1, 1, 1, 0, 0, 0]], np.uint8)
    assert call(*good[:2], few.ctypes.data_as(N._U8P), *good[3:8], None, None) == N.ERR_TOO_FEW_SHARDS
    of[3], ln[0] = 1, 7  # the pattern index comes before the ranges, the ranges before d_fixed
    assert call(*good[:8], None, None) == N.ERR_INVALID_ARG
    assert "out of range" in N.last_error() and "stripe 3" in N.last_error()
    of[3] = 0
    assert call(*good[:8], None, None) == N.ERR_INVALID_ARG
    assert "starts + lens exceeds" in N.last_error() and "entry 0" in N.last_error()
    ln[0], st[0] = 0, (1 << 64) - 1  # lens = 0 skips the entry whatever its start
    assert call(*good, None) == N.HBEC_OK  # nothing asked for: nothing queued
    files = N.lib().hbec_glue_plan_files_range_checked
    f = B.StripePlan(enc, files=[([0] * (K + M), 0)] * 3, chunk_size=4096)
    start = np.ascontiguousarray(f.object_start, np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
    fgood = [enc.handle, f._h, start, 3, ln, 4096, good[2], 1, of, d, ln, ln, fixed]
    assert files(*fgood, None) == N.HBEC_OK
    for i in (0, 1, 4, 6, 8, 9, 10, 11):  # hbec_glue_plan_files_range's null arguments
        assert files(*fgood[:i], None, *fgood[i + 1:], None) == N.ERR_INVALID_ARG and "null" in N.last_error(), i
    assert files(other.handle, *fgood[1:], None) == N.ERR_INVALID_ARG and "(k, m)" in N.last_error()
    a = C.c_uint64()
    assert N.lib().hbec_glue_range_checked_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert B.glue_range_checked_stats() == s0 and not any(fixed)


def test_both_kernel_families_use_no_scratch_and_no_lds():
    for fam in ("gf_range_checked", "gf_range_checked_rows"):
        found = KR.kernels(f"{fam}ILi")
        assert sorted(nm[nm.index("ILi") + 3] for nm in found) == list("01234"), (fam, sorted(found))
        for nm, k in found.items():
            assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, nm
