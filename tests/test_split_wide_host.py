"""csrc/splitwide.h's host logic as a stand-alone C++ program under ASan + UBSan, run
directly; and the resources of every gf_split_wide_plan instance from the metadata."""
import subprocess
from pathlib import Path

import pytest

import test_kernel_resources as KR
from test_repair_mixed_host import ENV, ROCM, host_compiler

SRC = Path(__file__).resolve().parent / "native" / "split_wide_host.cpp"


def test_split_wide_host_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "split_wide_host"
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "split_wide_host ok (16 records, 180 cuts)" in out.stdout  # (k, m) pairs; legal lengths


def test_split_wide_instances_fit_three_waves_without_scratch_or_lds():
    """M = 1..4, plain and ROWS, all at prefetch depth two: three waves per SIMD at least."""
    if not KR.LIB.exists():
        pytest.skip("libhbec.so not built")
    if not KR._readelf():
        pytest.skip("llvm-readelf not found")
    found = KR.kernels("gf_split_wide_planILi")
    assert len(found) == 8, sorted(found)
    for nm, k in found.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, nm
        assert k[".vgpr_count"] <= 168, (nm, k[".vgpr_count"])
