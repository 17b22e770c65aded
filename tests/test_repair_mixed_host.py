"""The repair call's host side, without a device: csrc/repair.h's inline logic
(per-entry words for every (r_o, r_c), pattern records, routing) through a
stand-alone C++ program (tests/native/repair_host.cpp) under AddressSanitizer +
UBSan, the new symbols of libhbec.so, and the resources of every
gf_repair_mixed_plan instance from the library's code-object metadata.

The program is compiled with the host compiler and run directly; it links no
libhbec and touches no device.  What hbec_decode_rows and hbec_check_rows answer
for every mask of 4+2 and 8+3 (both host-only calls) is written to a file the
program reads, so the record layout is checked against the library's own rows."""
import ctypes as C
import itertools
import os
import shutil
import subprocess
from pathlib import Path

from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "repair_host.cpp"
ROCM = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
NEW = ["hbec_repair_plan_mixed", "hbec_repair_plan_stats", "hbec_repair_plan_tile_bytes",
       "hbec_set_repair_plan_chunk_tiles"]


def host_compiler():
    for c in (str(ROCM / "lib" / "llvm" / "bin" / "clang++"), "clang++", "g++", "c++"):
        w = c if os.path.isabs(c) and os.path.exists(c) else shutil.which(c)
        if w:
            return w
    raise AssertionError("no host C++ compiler found")


def library_rows():
    """One line per (mask, data_only) of 4+2 and 8+3 with at least k present."""
    lines = []
    for k, m in ((4, 2), (8, 3)):
        enc, n = RS.New(k, m), k + m
        for lost_n in range(m + 1):
            for lost in itertools.combinations(range(n), lost_n):
                mask = [0 if i in lost else 1 for i in range(n)]
                surv, chk, crows = enc.check_rows(mask)
                for data_only in (0, 1):
                    outs, orows = [], []
                    if lost and not (data_only and all(mask[:k])):  # Reconstruct's early return
                        dsurv, outs, orows = enc.DecodeRows(mask, bool(data_only))
                        assert dsurv == surv
                        orows = orows.reshape(-1).tolist()
                    f = [k, m, data_only, *mask, *surv, len(outs), *outs, *orows, len(chk), *chk,
                         *crows.reshape(-1).tolist()]
                    lines.append(" ".join(str(int(x)) for x in f))
    return lines


def test_repair_host_logic_under_sanitizers(tmp_path):
    assert all(hasattr(N.lib(), name) for name in NEW)
    lines = library_rows()
    assert len(lines) == 2 * (22 + 232)
    rows = tmp_path / "rows.txt"
    rows.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "repair_host"
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe), str(rows)], capture_output=True, text=True, env=ENV, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert f"repair_host ok ({len(lines)} masks)" in out.stdout


def test_new_symbols_are_exported_and_declared():
    lib = N.lib()
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS and f" {name}(" in header, name
    assert lib.hbec_version() == 2
    assert lib.hbec_repair_plan_tile_bytes() == lib.hbec_mixed_plan_tile_bytes() == 4 * 992
    assert B.repair_plan_tile_bytes() == 4 * 992
    a = C.c_uint64()
    assert lib.hbec_repair_plan_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert lib.hbec_repair_plan_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert set(B.repair_plan_stats()) == {"kernel_launches", "per_stripe_calls"}
    # null arguments are found before the plan is looked at
    pat = (C.c_uint8 * 6)(1, 1, 1, 1, 1, 1)
    idx = (C.c_uint32 * 1)(0)
    assert lib.hbec_repair_plan_mixed(None, None, pat, 1, idx, 0, None, None) == N.ERR_INVALID_ARG
    B.set_repair_plan_chunk_tiles(3)
    B.set_repair_plan_chunk_tiles(0)


def test_repair_plan_instances_use_no_scratch_and_no_lds():
    """RMAX = 1..4: no private memory (nothing is indexed at run time: a tile
    per (r_o, r_c) pair), no LDS, no spilled VGPR, and no instance below the
    occupancy step of its gf_verify_mixed_plan twin (5 / 4 / 3 / 3 waves per
    SIMD: at most 96 / 128 / 168 / 168 VGPRs)."""
    import test_kernel_resources as KR

    found = KR.kernels("gf_repair_mixed_planILi")
    assert len(found) == 4, sorted(found)
    step = {1: 96, 2: 128, 3: 168, 4: 168}
    for r in range(1, 5):
        (k,) = [k for nm, k in found.items() if f"gf_repair_mixed_planILi{r}E" in nm]
        assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, r
        assert k[".vgpr_spill_count"] == 0, r
        assert k[".vgpr_count"] <= step[r], (r, k[".vgpr_count"])
