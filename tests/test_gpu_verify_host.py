"""hbec_verify_host / Encoder.VerifyStripes: Verify of stripes in host memory,
pageable (staged through the ring, one copy per stripe) and pinned
(HostBuffer: read in place over PCIe), with exact flags; and a stripe larger
than a ring slot, cut into column pieces (a fresh child process with
HBEC_HOST_SLOT_MB=1, run as `python tests/test_gpu_verify_host.py`)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))

from hummingbird_amd import batch as B  # noqa: E402
from hummingbird_amd import reedsolomon as RS  # noqa: E402
from oracle import coracle as CO  # noqa: E402

pytestmark = pytest.mark.gpu

N_STRIPES = 200


def sizes_for(k, m, seed):
    T = B.verify_plan_tile_bytes(k)
    A = 1024 * (4 // k if k <= 4 else 1)
    rng = np.random.default_rng(seed)
    s = [1, 3, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, T - 1, T, T + 1, 2 * T - 1, 2 * T + 17, A, A + 16, 3 * A]
    s += [int(x) for x in rng.integers(1, 300_000, 40)]
    s += [int(x) for x in rng.integers(1, 3000, N_STRIPES - len(s) - 4)]
    s = [s[i] for i in rng.permutation(len(s))]
    for at in (0, 50, 120, len(s) + 3):  # zero-length stripes
        s.insert(min(at, len(s)), 0)
    assert len(s) == N_STRIPES
    return s


def codewords(k, m, sizes, seed):
    """One uint8 array with every stripe ((k+m) S bytes, parity from the oracle) at an odd offset."""
    rng = np.random.default_rng(seed)
    rows = CO.build_matrix(k, m)[k:]
    offs, pos = [], 0
    for s in sizes:
        pos += 1 + int(rng.integers(0, 13))
        if pos % 16 == 0:
            pos += 3
        offs.append(pos)
        pos += (k + m) * s
    buf = rng.integers(0, 256, pos + 9, dtype=np.uint8)
    for s, o in zip(sizes, offs):
        if s:
            par = CO.apply(rows, [buf[o + j * s:o + (j + 1) * s] for j in range(k)])
            for r in range(m):
                buf[o + (k + r) * s:o + (k + r + 1) * s] = par[r]
    return buf, offs


def flip_some(k, m, sizes, offs, buf):
    T = B.verify_plan_tile_bytes(k)
    live = [e for e, s in enumerate(sizes) if s]
    bad = []
    for q, e in enumerate(live[::3]):
        s = sizes[e]
        cand = [0, 1, 15, 16, s - 17, s - 16, s - 1, T - 1, T, T + 1, s // 2]
        p = min(max(cand[q % len(cand)], 0), s - 1)
        buf[offs[e] + (q % (k + m)) * s + p] ^= 0xA7
        bad.append(e)
    return bad


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_exact_flags_pageable_and_pinned(k, m, pinned):
    sizes = sizes_for(k, m, 3 * k + m)
    clean, offs = codewords(k, m, sizes, k)
    enc = RS.New(k, m)
    hb = None
    if pinned:
        hb = RS.HostBuffer(clean.size)
        assert RS.host_device_addr(hb.array) != 0
        buf = hb.array
        buf[:] = clean
    else:
        buf = clean.copy()
    stripes = [buf[o:o + (k + m) * s] for s, o in zip(sizes, offs)]
    s0 = B.verify_plan_stats()
    assert not enc.VerifyStripes(stripes).any()  # oracle codewords: all False
    bad = flip_some(k, m, sizes, offs, buf)
    keep = np.array(buf, copy=True)
    got = enc.VerifyStripes(stripes)
    s1 = B.verify_plan_stats()
    assert got.dtype == bool and np.nonzero(got)[0].tolist() == bad
    assert np.array_equal(buf, keep)  # read-only
    assert s1["per_stripe_calls"] == s0["per_stripe_calls"] and s1["plan_launches"] > s0["plan_launches"]
    del stripes, buf
    if hb is not None:
        hb.free()


def test_other_shape_host_stripes():
    """16+4 is outside the plan kernels: one verify call per stripe, same flags."""
    k, m = 16, 4
    sizes = [1, 17, 0, 4096, 1985, 33, 50_001, 16, 777]
    buf, offs = codewords(k, m, sizes, 2)
    buf[offs[4] + 19 * sizes[4] + sizes[4] - 1] ^= 1
    buf[offs[7] + 3] ^= 0x80
    got = RS.New(k, m).VerifyStripes([buf[o:o + (k + m) * s] for s, o in zip(sizes, offs)])
    assert np.nonzero(got)[0].tolist() == [4, 7]


def _child():
    """HBEC_HOST_SLOT_MB=1: a 4+2 stripe of 1.2 MB is cut into column pieces; a
    flip in the last piece (and one in the first, in another stripe) is flagged
    exactly, between stripes that fit."""
    k, m = 4, 2
    slot = int(os.environ["HBEC_HOST_SLOT_MB"]) << 20
    big = slot // (k + m) + 25_001  # (k+m) S > one slot
    sizes = [1000, big, 33, big + 7, 0, 5000]
    buf, offs = codewords(k, m, sizes, 9)
    enc = RS.New(k, m)
    stripes = [buf[o:o + (k + m) * s] for s, o in zip(sizes, offs)]
    res = {"clean": enc.VerifyStripes(stripes).tolist()}
    buf[offs[1] + 5 * big + big - 3] ^= 0x10   # last piece of stripe 1, last parity shard
    buf[offs[3] + 2 * (big + 7) + 11] ^= 0x01  # first piece of stripe 3, a data shard
    res["flags"] = enc.VerifyStripes(stripes).tolist()
    res["pieces"] = -(-big // ((slot // (k + m)) // 16 * 16))
    print(json.dumps(res))


def test_stripe_larger_than_a_ring_slot_is_cut_into_pieces():
    env = dict(os.environ, HBEC_HOST_SLOT_MB="1")
    p = subprocess.run([sys.executable, str(Path(__file__).resolve())], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["pieces"] >= 2
    assert res["clean"] == [False] * 6
    assert res["flags"] == [False, True, False, True, False, False]


if __name__ == "__main__":
    _child()
