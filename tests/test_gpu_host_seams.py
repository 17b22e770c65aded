"""Seams of the host path (csrc/hostpath.cpp) byte for byte: hbec_encode_host,
hbec_reconstruct_host and hbec_encode_host_md5 where the code cuts, packs,
rotates and flushes.  At the default 64 MiB staging slot a test moves hundreds
of MB to cross one seam and never reuses a slot, so every mode runs
tests/host_seams_child.py in a fresh process with HBEC_HOST_SLOT_MB=1 and
HBEC_HASH_ARENA_MB=1 (a ring reads its capacities when it is made):

  pieces              stripes wider than a slot, cut into column pieces, at
                      every length around one, two and three piece widths
  chunks              a chunk filled exactly to the IN slot, more chunks than
                      2 kSlots, and a chunk closed by its tile records
  zerocopy            pinned stripes that end on, straddle and span record
                      slots; accumulate passes over PCIe
  zerocopy-unaligned  likewise through the odd-shard records, with runs of
                      stripes that have edge records only
  md5-ring            hash arenas filled, flushed and reused by the staging
                      ring; a stripe at the slot bound; one over it refused
  md5-pinned          every instance of the mirrored stripes kernel (48:
                      K 1..8 x R 1..3, first and accumulate pass), arena
                      switching, and the unaligned twin
  mixed               pinned-aligned, pinned-unaligned, pageable and empty
                      stripes in one call

The child compares whole backing buffers (sentinel bytes around every stripe
included) with the oracle image after every call and every digest with
hashlib, restates the cutting rules and checks hbec_host_run_stats,
hbec_stripes_kernel_stats and hbec_host_md5_stats against them; it reports
what it found as one JSON line, asserted here.  The time limit only guards
against a hang.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

CHILD = Path(__file__).resolve().parent / "host_seams_child.py"
K_SLOTS = 3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield


def run(mode):
    env = dict(os.environ, HBEC_HOST_SLOT_MB="1", HBEC_HASH_ARENA_MB="1")
    p = subprocess.run([sys.executable, str(CHILD), mode], env=env, capture_output=True, text=True, timeout=120)
    lines = p.stdout.strip().splitlines()
    assert lines, p.stdout + p.stderr
    try:
        res = json.loads(lines[-1])
    except ValueError:
        pytest.fail(f"{mode}: no result line\n{p.stdout}{p.stderr}")
    assert res["mode"] == mode and res["errors"] == [] and p.returncode == 0, (res["errors"], p.stderr[-2000:])
    assert res["caps"] == {"in_cap": 1 << 20, "tile_cap": 2048, "arena": 2 << 20}
    print("HOST-SEAMS", mode, json.dumps(res["cases"]))
    return res["cases"]


def test_pieces():
    cases = run("pieces")
    assert [c["shape"] for c in cases] == ["4+2", "3+5", "10+4"]
    W = cases[0]["W"]
    assert W == (1 << 20) // 4 and cases[1]["W"] == ((1 << 20) // 5) // 16 * 16 and cases[2]["W"] == ((1 << 20) // 10) // 16 * 16
    assert cases[0]["lengths"] == [W - 16, W - 1, W, W + 1, W + 15, W + 16, W + 17, 2 * W, 2 * W + 1, 3 * W + 1024 + 5]
    # 4+2 encode: 1 1 1 2 2 2 2 2 3 4 pieces of the wide stripes and one per short stripe
    assert cases[0]["ops"][0]["pieces"] == 20 + 10
    assert [len(c["ops"]) for c in cases] == [4, 4, 4]


def test_chunks():
    a, b = run("chunks")
    assert a["case"] == "bytes" and all(o["chunks"] == 2 * K_SLOTS + 2 for o in a["ops"])
    assert b["case"] == "tile_cap" and b["stripes"] >= 2049 and all(o["chunks"] == 2 for o in b["ops"])


def test_zerocopy():
    a, b = run("zerocopy")
    assert a["slots"] >= K_SLOTS + 2 and a["pinned_bytes"] < 48 << 20 and len(a["ops"]) == 2
    assert b["shape"] == "11+3" and len(b["ops"]) == 4


def test_zerocopy_unaligned():
    (a,) = run("zerocopy-unaligned")
    assert min(a["slots"]) >= K_SLOTS + 2 and a["tiny"] > 4 * 2047 and len(a["ops"]) == 2


def test_md5_ring():
    (a,) = run("md5-ring")
    assert a["counters"]["arena_flushes"] >= 5 and a["counters"]["md5_ring"] == 1


def test_md5_pinned():
    inst, arenas, odd = run("md5-pinned")
    assert inst["mirror"] == 24 and inst["mirror_accumulate"] == 24
    assert arenas["counters"]["arena_flushes"] >= 5 and odd["counters"]["arena_flushes"] >= 5


def test_mixed():
    (a,) = run("mixed")
    assert [o["op"] for o in a["ops"]] == ["encode", "reconstruct[0, 6]"]
    assert {w for _, w in a["specs"]} == {"pin", "pinodd", "page"} and any(s == 0 for s, _ in a["specs"])
