"""The plan Verify's host side under AddressSanitizer + UBSan: a stand-alone
C++ program (tests/native/verify_plan_asan.cpp, built by build.py
build_asan() against the host-sanitized libhbec) builds Verify records and
flag indices for edge-case shard lengths and walks every argument check of
hbec_verify_plan / hbec_verify_host.  CPU only; no device is touched."""
import os
import subprocess

import pytest

from hummingbird_amd import build as Bd

ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:protect_shadow_gap=0:abort_on_error=0",
           UBSAN_OPTIONS="print_stacktrace=1")


def test_verify_plan_host_side_under_sanitizers():
    if not Bd.ASAN_VERIFY_EXE.exists():
        pytest.skip("sanitizer build missing: run __graft_entry__.build()")
    out = subprocess.run([str(Bd.ASAN_VERIFY_EXE)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "verify_plan_asan ok" in out.stdout
