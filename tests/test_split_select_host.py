"""The split calls with a writers mask without a device, in the manner of
tests/test_split_host.py.  `source_errors` needs a device for its plans:
tests/test_gpu_split_select.py runs it."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import test_glue_host as GH
import test_kernel_resources as KR
import test_repair_mixed_host as RH
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "tests" / "native" / "splitselect_host.cpp"
K, M = 4, 2
BASE, FAR = 0x7000_0000_0000, 0x7100_0000_0000  # addresses are compared here, never followed


def test_new_symbols_are_exported_and_declared():
    header = (ROOT / "include" / "hbec.h").read_text()
    for name in ("hbec_split_plan_select", "hbec_split_plan_files_select", "hbec_split_select_stats"):
        assert hasattr(N.lib(), name) and name in N.SYMBOLS and f" {name}(" in header, name
        above = header[:header.index(f" {name}(")]
        assert "ecutils.go:26-72" in above[above.rindex("/*"):] and "line 63" in above[above.rindex("/*"):], name


def test_record_builder_under_sanitizers(tmp_path):
    assert "csrc/splitselect.h" in SRC.read_text() and "hbec.h" not in SRC.read_text()
    header = (ROOT / "hummingbird_amd" / "csrc" / "splitselect.h").read_text()
    assert not [h for h in re.findall(r'#include\s+[<"]([^>"]+)[>"]', header) if "hip" in h]
    exe = tmp_path / "splitselect_host"
    cmd = [RH.host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", str(SRC), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=RH.ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    got = re.search(r"splitselect_host ok \((\d+) records, (\d+) walks\)", out.stdout)
    assert got and int(got.group(1)) == 64 + 32 + 16 + 600 and int(got.group(2)) > 30000, out.stdout


@pytest.mark.parametrize("kind", ["stripes", "objects", "shards"])
def test_argument_errors_and_their_precedence(kind):
    entry = {"stripes": (0, 0), "objects": (0, 0, 0), "shards": ([0] * (K + M), 0)}[kind]
    enc = RS.New(K, M)
    plan, sel = B.StripePlan(enc, **{kind: [entry] * 5}), np.ones((5, K + M), np.uint8)
    s0 = (B.split_select_stats(), B.split_plan_stats())
    d, ln, of = (C.c_void_p * 5)(), (C.c_uint64 * 5)(), (C.c_uint32 * 5)()
    good = [enc.handle, plan._h, d, ln, sel.ctypes.data_as(N._U8P), of, 1]
    for i in range(6):  # a null codec, plan, srcs, src_lens, patterns, pattern_of
        assert N.lib().hbec_split_plan_select(*good[:i], None, *good[i + 1:], None) == N.ERR_INVALID_ARG
        assert "null" in N.last_error(), i
    for n_patterns, word in ((65537, "65536"), (0, "no patterns")):
        assert N.lib().hbec_split_plan_select(*good[:6], n_patterns, None) == N.ERR_INVALID_ARG
        assert word in N.last_error()
    of[3] = 1  # the index of every entry is checked, zero-length ones too, and before the lengths
    ln[0] = 7
    assert N.lib().hbec_split_plan_select(*good, None) == N.ERR_INVALID_ARG
    assert "out of range" in N.last_error() and "stripe 3" in N.last_error()
    other = B.StripePlan(RS.New(8, 3), stripes=[(0, 0)] * 5)  # another shape: before the masks and the lengths
    assert N.lib().hbec_split_plan_select(enc.handle, other._h, *good[2:], None) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    for rows in (sel, 0 * sel):  # bytes for a zero-length entry: refused whatever its mask, before its null source
        with pytest.raises(RS.ErrInvalidArg, match="src_lens.*entry 2"):
            plan.split_select([0] * 5, [0, 0, 5, 0, 0], rows, stream=GH._NoStream())
    with pytest.raises(ValueError, match="files"):
        plan.split_files_select([], sel[:4])
    plan.split_select([FAR] * 5, [0] * 5, sel, stream=GH._NoStream())  # nothing given: nothing queued
    assert (B.split_select_stats(), B.split_plan_stats()) == s0  # nothing launched or counted


def source_errors():
    """The argument errors that need an entry with bytes in it.  False: no device for the plans' rows."""
    enc, S = RS.New(K, M), 100
    row = [BASE + 3 * S * j for j in range(K + M)]  # shards 3 S apart
    plan = GH._shards_plan(enc, [row, [0] * (K + M), row], [S, 0, S])
    if plan is None:
        return False
    s0, ln, eye = B.split_select_stats(), K * S - 1, np.eye(K + M, dtype=np.uint8)

    def fails(word, srcs, lens, masks, p=plan):
        with pytest.raises(RS.ErrInvalidArg, match=word):
            p.split_select(srcs, lens, np.array(masks, np.uint8), stream=GH._NoStream())

    for mask in (eye[0] + 1, eye[0] * 0, eye[0]):  # the length rule holds whatever the mask
        for bad in (K * S - K, K * S + 1):
            fails("src_lens.*entry 2", [FAR, 0, FAR], [K * S, 0, bad], [eye[0] + 1, eye[0], mask])
    fails("null source.*entry 2", [FAR, 0, 0], [K * S, 0, ln], [eye[0] + 1, eye[0], eye[3]])
    plan.split_select([0, 0, 0], [K * S, 0, ln], 0 * eye[:3], stream=GH._NoStream())
    # over a shard: refused only where it is selected; over unselected ones or touching: entry 2's null source
    for sh in (0, K - 1, K + M - 1):
        for over, touch in ((row[sh] - ln + 1, row[sh] - ln), (row[sh] + S - 1, row[sh] + S)):
            fails(f"overlaps selected shard {sh}.*entry 0", [over, 0, 0], [ln, 0, K * S], [eye[sh], eye[0], eye[0] + 1])
            fails("null source.*entry 2", [over, 0, 0], [ln, 0, K * S], [eye[(sh + 3) % (K + M)], eye[0], eye[0] + 1])
            fails("null source.*entry 2", [touch, 0, 0], [ln, 0, K * S], [eye[sh], eye[0], eye[0] + 1])
    # files, a mask per entry: object 0's second stripe over its shard 3; a null source at the first selected entry
    chunk, files = 64, [BASE + (1 << 20) * j for j in range(K + M)]
    f = B.StripePlan(enc, files=[(files, 2 * K * chunk + 12), ([0] * (K + M), 0), (files, 5)], chunk_size=chunk)
    over = [files[3] + chunk - 2 * K * chunk + 1, 0, FAR]
    with pytest.raises(RS.ErrInvalidArg, match="overlaps selected shard 3.*entry 1"):
        f.split_files_select(over, [eye[0] * 0, eye[3], eye[0] + 1, eye[0] + 1], stream=GH._NoStream())
    with pytest.raises(RS.ErrInvalidArg, match="null source.*entry 2"):
        f.split_files_select([0, 0, FAR], [eye[0] * 0, eye[0] * 0, eye[2], eye[0] + 1], stream=GH._NoStream())
    assert B.split_select_stats() == s0  # none of this launched anything
    return True


def test_select_instances_use_no_scratch_and_no_lds():
    for fam in ("gf_split_select_plan", "gf_split_select_plan_rows"):
        found = KR.kernels(f"{fam}ILi")
        assert sorted(nm[nm.index("ILi") + 3] for nm in found) == list("01234"), (fam, sorted(found))
        for nm, k in found.items():
            assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, nm
