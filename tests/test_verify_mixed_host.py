"""The degraded plan Verify's host logic under AddressSanitizer + UBSan: a
stand-alone C++ program (tests/native/verify_mixed_host.cpp) over the inline
functions of csrc/vmixed.h — shard selection per mask, record words, word
packing, routing of sizes and shapes.  The test compiles it with the host
compiler and runs it directly; it links no libhbec and touches no device."""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "verify_mixed_host.cpp"
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def host_compiler():
    for c in (str(ROCM / "lib" / "llvm" / "bin" / "clang++"), "clang++", "g++", "c++"):
        w = c if os.path.isabs(c) and os.path.exists(c) else shutil.which(c)
        if w:
            return w
    raise AssertionError("no host C++ compiler found")


def test_verify_mixed_host_logic_under_sanitizers(tmp_path):
    exe = tmp_path / "verify_mixed_host"
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall","-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "verify_mixed_host ok" in out.stdout
