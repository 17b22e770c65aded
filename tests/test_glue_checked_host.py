"""hbec_glue_plan_checked without a device, in the manner of tests/test_split_select_host.py."""
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
SRC = ROOT / "tests" / "native" / "gluecheck_host.cpp"
K, M = 4, 2


def test_new_symbols_are_exported_declared_and_cited():
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in ("hbec_glue_plan_checked", "hbec_glue_plan_files_checked", "hbec_glue_checked_stats",
                 "hbec_glue_checked_tile_bytes", "hbec_set_glue_checked_chunk_tiles"):
        assert hasattr(N.lib(), name) and name in N.SYMBOLS and f" {name}(" in header, name
        above = header[:header.index(f" {name}(")]
        assert "ecobj.go:173-203" in above[above.rindex("/*"):], name
    assert "main.go:233-241" in header and "hbec_etag_plan_mixed) is what catches it" in header  # the r = 2 caveat
    assert B.glue_checked_tile_bytes() == B.glue_plan_tile_bytes()


def test_record_builder_under_sanitizers(tmp_path):
    assert "csrc/gluecheck.h" in SRC.read_text() and "hbec.h" not in SRC.read_text()
    header = (ROOT / "hummingbird_amd" / "csrc" / "gluecheck.h").read_text()
    assert not [h for h in re.findall(r'#include\s+[<"]([^>"]+)[>"]', header) if "hip" in h]
    exe = tmp_path / "gluecheck_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = re.search(r"gluecheck_host ok \((\d+) records\)", out.stdout)
    assert got and int(got.group(1)) == 22 + 16 + 300 + 300, out.stdout


def test_argument_errors_and_their_precedence():
    enc = RS.New(K, M)
    plan, s0 = B.StripePlan(enc, stripes=[(0, 0)] * 5), B.glue_checked_stats()
    pat, of = np.ones((1, K + M), np.uint8), (C.c_uint32 * 5)()
    d, ln, fixed = (C.c_void_p * 5)(), (C.c_uint64 * 5)(), (C.c_uint32 * 5)()
    good = [enc.handle, plan._h, pat.ctypes.data_as(N._U8P), 1, of, d, ln, fixed]
    for i in (0, 1, 2, 4, 5, 6, 7):  # a null codec, plan, patterns, pattern_of, dsts, dst_lens, d_fixed
        assert N.lib().hbec_glue_plan_checked(*good[:i], None, *good[i + 1:], None) == N.ERR_INVALID_ARG
        assert "null" in N.last_error(), i
    of[3], ln[0] = 1, 7  # the pattern index comes before the lengths, the lengths before d_fixed
    assert N.lib().hbec_glue_plan_checked(*good[:7], None, None) == N.ERR_INVALID_ARG
    assert "out of range" in N.last_error() and "stripe 3" in N.last_error()
    of[3] = 0
    assert N.lib().hbec_glue_plan_checked(*good[:7], None, None) == N.ERR_INVALID_ARG
    assert "dst_lens exceeds" in N.last_error() and "entry 0" in N.last_error()
    ln[0] = 0
    assert N.lib().hbec_glue_plan_checked(*good, None) == N.HBEC_OK  # nothing asked for: nothing queued
    assert N.lib().hbec_glue_plan_files_checked(enc.handle, plan._h, of, 5, ln, 0, good[2], 1, of, d, fixed,
                                                None) == N.ERR_INVALID_ARG  # chunk_size 0
    assert B.glue_checked_stats() == s0 and not any(fixed)


def test_both_kernel_families_use_no_scratch_and_no_lds():
    for fam in ("gf_glue_checked", "gf_glue_checked_rows"):
        found = KR.kernels(f"{fam}ILi")
        assert sorted(nm[nm.index("ILi") + 3] for nm in found) == list("01234"), (fam, sorted(found))
        for nm, k in found.items():
            assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, nm
