"""csrc/gluewide.h's inline host logic, without a device: a stand-alone C++ program
(tests/native/glue_wide_host.cpp) under AddressSanitizer + UBSan, run directly; and
the resources of every gf_glue_wide_plan instance from the library's code-object
metadata."""
import subprocess
from pathlib import Path

import pytest

import test_kernel_resources as KR
from test_repair_mixed_host import ENV, ROCM, host_compiler

SRC = Path(__file__).resolve().parent / "native" / "glue_wide_host.cpp"


def test_glue_wide_host_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "glue_wide_host"
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    # r = 0..4 at k = 12, 13, 32 and r = 0, 1 at k = 1; 4 shard lengths x 6 missing sets x 5 cuts x 3 offsets
    assert "glue_wide_host ok (17 records, 360 words)" in out.stdout


def test_glue_wide_instances_fit_three_waves_without_scratch_or_lds():
    """RMAX = 0..4, for record plans and for shards plans: no private memory, no LDS,
    and at most 168 VGPRs, three waves per SIMD, the step gf_repair_wide_plan<4> is on."""
    if not KR.LIB.exists():
        pytest.skip("libhbec.so not built")
    if not KR._readelf():
        pytest.skip("llvm-readelf not found")
    found = KR.kernels("gf_glue_wide_planILi")
    assert len(found) == 10, sorted(found)
    for nm, k in found.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, nm
        assert k[".vgpr_count"] <= 168, (nm, k[".vgpr_count"])
