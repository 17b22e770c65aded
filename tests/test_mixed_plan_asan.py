"""The mixed plan reconstruct's host side under AddressSanitizer + UBSan: a
stand-alone C++ program (tests/native/mixed_plan_asan.cpp, built by build.py
build_asan() against the host-sanitized libhbec) routes edge-case shard
lengths to records and tiles, builds pattern records, and walks every argument
check of hbec_reconstruct_plan_mixed.  CPU only; no device is touched."""
import os
import subprocess

import pytest

from hummingbird_amd import build as Bd

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:protect_shadow_gap=0:abort_on_error=0",
           UBSAN_OPTIONS="print_stacktrace=1")


def test_mixed_plan_host_side_under_sanitizers():
    if not Bd.ASAN_MIXED_PLAN_EXE.exists():
        pytest.skip("sanitizer build missing: run __graft_entry__.build()")
    out = subprocess.run([str(Bd.ASAN_MIXED_PLAN_EXE)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "mixed_plan_asan ok" in out.stdout
