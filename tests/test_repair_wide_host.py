"""csrc/repairwide.h's inline host logic, without a device: a stand-alone C++ program
(tests/native/repair_wide_host.cpp) under AddressSanitizer + UBSan, run directly."""
import subprocess
from pathlib import Path

from test_repair_mixed_host import ENV, ROCM, host_compiler

SRC = Path(__file__).resolve().parent / "native" / "repair_wide_host.cpp"


def test_repair_wide_host_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "repair_wide_host"
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    # the 14 (r_o, r_c) pairs at k = 12, 13, 32 and the 8 with r_o <= 1 at k = 1
    assert "repair_wide_host ok (50 records)" in out.stdout
