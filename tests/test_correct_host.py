"""The correct call's host side, without a device: csrc/correct.h's inline logic
through a stand-alone C++ program (tests/native/correct_host.cpp) compiled with
the host compiler under AddressSanitizer + UBSan and run directly (it links no
libhbec)."""
import subprocess
from pathlib import Path

from test_locate_host import ENV, ROCM, host_compiler

SRC = Path(__file__).resolve().parent / "native" / "correct_host.cpp"


def test_correct_host_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "correct_host"
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0 and "correct_host ok" in out.stdout, (out.stdout + out.stderr)[-4000:]
