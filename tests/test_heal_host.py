"""The heal call's host side, without a device: csrc/heal.h's inline logic (the
rule that turns a locate word into the shard to rewrite, the records and tables
staged per call, routing) through a stand-alone C++ program
(tests/native/heal_host.cpp) under AddressSanitizer + UBSan, the new symbols of
libhbec.so, and the resources of every gf_heal_mixed_plan instance from the
library's code-object metadata.

The program is compiled with the host compiler and run directly; it links no
libhbec and touches no device.  What hbec_decode_rows and hbec_check_rows answer
for every mask of 4+2 and 8+3 with something missing (both host-only calls) is
written to a file the program reads, so every staged record of a mask with one
shard left out is checked against the library's own rows of that mask."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np

import test_repair_mixed_host as RH
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "heal_host.cpp"
NEW = ["hbec_heal_plan_mixed", "hbec_heal_plan_stats", "hbec_heal_plan_tile_bytes",
       "hbec_set_heal_plan_chunk_tiles"]


def library_rows():
    """One line per mask of 4+2 and 8+3 with at least k present and something
    missing: what a repair of that mask (no data_only) rebuilds and checks."""
    lines = []
    for k, m in ((4, 2), (8, 3)):
        enc, n = RS.New(k, m), k + m
        for lost_n in range(1, m + 1):
            for lost in itertools.combinations(range(n), lost_n):
                mask = [0 if i in lost else 1 for i in range(n)]
                surv, chk, crows = enc.check_rows(mask)
                dsurv, outs, orows = enc.DecodeRows(mask, False)
                assert dsurv == surv and sorted(outs) == list(lost)
                f = [k, m, 0, *mask, *surv, len(outs), *outs, *orows.reshape(-1).tolist(), len(chk), *chk,
                     *crows.reshape(-1).tolist()]
                lines.append(" ".join(str(int(x)) for x in f))
    return lines


def test_heal_host_logic_under_sanitizers(tmp_path):
    assert all(hasattr(N.lib(), name) for name in NEW)
    lines = library_rows()
    assert len(lines) == 21 + 231
    rows = tmp_path / "rows.txt"
    rows.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "heal_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{RH.ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe), str(rows)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    # every (mask, present j) of a mask with at least k + 1 present: 6 + 6 * 5 at 4+2, 11 + 11 * 10 + 55 * 9
    # at 8+3 (the mask the program lists twice has exactly k present: no record)
    words = (22 + 232) * 8 * 65536
    pairs = (6 + 6 * 5) + (11 + 11 * 10 + 55 * 9)
    assert f"heal_host ok ({words} words, {pairs} records of a mask with one shard left out)" in out.stdout


def test_pick_is_locate_decode_through_the_library():
    """The same rule through the exported hbec_locate_decode, sampled: the C++
    program checks it exhaustively against the inline function behind it."""
    rng = np.random.default_rng(5)
    for k, m in ((4, 2), (8, 3), (12, 4)):
        n = k + m
        for _ in range(300):
            present = (rng.random(n) < 0.85).astype(np.uint8)
            bits = int(sum(int(b) << i for i, b in enumerate(present)))
            where = int(rng.integers(0, 1 << 16)) | (N.LOC_BAD if rng.random() < 0.8 else 0)
            if rng.random() < 0.1:
                where |= int(rng.choice([N.LOC_SKIPPED, N.LOC_NOTHING]))
            d = int(B.locate_decode(k, m, present, np.array([where], np.uint32))[0])
            examined = bool(where & N.LOC_BAD) and not where & (N.LOC_SKIPPED | N.LOC_NOTHING)
            cand = bits & ~where & 0xFFFF
            pick = cand.bit_length() - 1 if bin(cand).count("1") == 1 else -1
            if d >= 0:
                assert examined and pick == d
            elif d in (N.LOC_AMBIGUOUS, N.LOC_MULTIPLE):
                assert examined and pick == -1
            else:
                assert not examined


def test_new_symbols_are_exported_and_declared():
    lib = N.lib()
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in N.SYMBOLS and f" {name}(" in header, name
    assert "#define HBEC_HEAL_DONE 4u" in header and "#define HBEC_HEAL_UNNAMED 8u" in header
    assert (N.HEAL_DONE, N.HEAL_UNNAMED) == (4, 8)
    assert lib.hbec_version() == 2
    assert lib.hbec_heal_plan_tile_bytes() == lib.hbec_repair_plan_tile_bytes() == 4 * 992
    assert B.heal_plan_tile_bytes() == 4 * 992
    a = C.c_uint64()
    assert lib.hbec_heal_plan_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert lib.hbec_heal_plan_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert set(B.heal_plan_stats()) == {"kernel_launches", "skipped_entries"}
    # null arguments are found before the plan is looked at
    pat = (C.c_uint8 * 6)(1, 1, 1, 1, 1, 1)
    idx = (C.c_uint32 * 1)(0)
    assert lib.hbec_heal_plan_mixed(None, None, pat, 1, idx, None, None, None) == N.ERR_INVALID_ARG
    B.set_heal_plan_chunk_tiles(3)
    B.set_heal_plan_chunk_tiles(0)
    assert hasattr(B.StripePlan, "heal_mixed")


def waves_per_simd(vgprs):
    """gfx950: 512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves."""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def test_heal_plan_instances_use_no_scratch_and_no_lds_and_keep_repairs_occupancy():
    """RMAX = 1..4: no private memory, no LDS, no spilled VGPR, and as many
    waves per SIMD as the gf_repair_mixed_plan instance of the same RMAX
    (5 / 4 / 3 / 3)."""
    import test_kernel_resources as KR

    heal, repair = KR.kernels("gf_heal_mixed_planILi"), KR.kernels("gf_repair_mixed_planILi")
    assert len(heal) == 4 and len(repair) == 4, (sorted(heal), sorted(repair))
    for r in range(1, 5):
        (h,) = [k for nm, k in heal.items() if f"gf_heal_mixed_planILi{r}E" in nm]
        (p,) = [k for nm, k in repair.items() if f"gf_repair_mixed_planILi{r}E" in nm]
        assert h[".private_segment_fixed_size"] == 0 and h[".group_segment_fixed_size"] == 0, r
        assert h[".vgpr_spill_count"] == 0, r
        assert waves_per_simd(h[".vgpr_count"]) >= waves_per_simd(p[".vgpr_count"]), (r, h[".vgpr_count"],
                                                                                     p[".vgpr_count"])
    assert [waves_per_simd(k[".vgpr_count"]) for _, k in sorted(repair.items())] == [5, 4, 3, 3]
