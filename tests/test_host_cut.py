"""The host path's cutting rules, without a device: csrc/hostcut.h (the ring's
pieces and chunks, the chunks of a staged Verify, the records of a zero-copy
slot, the stripe classifier and its two policies) through a stand-alone C++
program (tests/native/host_cut.cpp) under AddressSanitizer + UBSan.

The program is compiled with the host compiler and run directly; it links no
libhbec and touches no device.  Its capacities are a few KiB, so every seam of
the rules is a few hundred bytes away, and the number of cases it reports is
restated here from its case lists: a loop that silently ran short fails."""
import subprocess
from pathlib import Path

import test_repair_mixed_host as RH

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "host_cut.cpp"


def expected_cases():
    cap = 4096
    # ring: every shard length 0 .. 3 W + 17 of four shapes; three exact fills and three groups of refusals
    ring = sum(3 * ((min(cap // k, cap // r) // 16) * 16) + 18 for k, r in ((4, 2), (3, 5), (10, 4), (1, 1))) + 6
    # plain fills: tile totals 1..40 in three patterns, aligned once and unaligned with edges on and off;
    # five runs of edge-only stripes, edges on and off
    plain = 40 * 3 * (1 + 2) + 5 * 2
    # hashing fills, both record kinds: 600 lengths at two arena sizes, two arena-closing lists, one run of
    # edge-only stripes, 30 random lists at two record capacities
    md5 = 2 * (600 * 2 + 2 + 1 + 30 * 2)
    # verify: every shard length 1 .. 3 W + 17 for k + m = 6, 3 and 4; records bound, bytes bound, refusal
    verify = sum(3 * ((cap // n // 16) * 16) + 17 for n in (6, 3, 4)) + 3
    # classifier: 13 stripes and the plain policy, any alignment off and on; five hashing-policy cases
    classifier = 2 * (13 + 1) + 5
    return ring + plain + md5 + verify + classifier


def test_host_cut_rules_under_sanitizers(tmp_path):
    exe = tmp_path / "host_cut"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           f"-I{RH.ROCM / 'include'}", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert f"host_cut ok ({expected_cases()} cases)" in out.stdout, out.stdout[-400:]
