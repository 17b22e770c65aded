"""bench.py end to end on one GPU at a reduced size: the JSON line the driver
parses carries the metric, a roofline with the dominant kernel and fresh (or
explicitly stale) traffic, and with --full every BASELINE-config leg with its
parity flag; a plain run stops at the headline, and --dump-outputs writes the
last step's parity and rebuilt shards."""
import json

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu

FULL_LEGS = ("config5", "small_objects", "config4", "odd_objects", "random_objects", "mid_objects", "host_path")


def test_bench_line_small(capsys):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    rc = bench.main(["--full", "--steps", "3", "--warmup", "1", "--objects", "128", "--config5-objects", "512",
                     "--no-cpu-baseline", "--no-host-path", "--settle-ms", "5"])
    out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert rc == 0 and len(out) == 1
    d = json.loads(out[0])
    assert d["metric"] == bench.METRIC and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["parity_ok"] and d["value"] > 0 and d["settle_steps"] >= 1
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == bench.HBM_PEAK_GBS and 0 < r["frac"] < 1
    assert r["kernel"] == bench.KERNEL_NAME
    assert (r["traffic"] is None) == (r["traffic_note"] is not None)
    assert d["config5"]["parity_ok"] and d["config5"]["objects"] == 512
    assert d["config4"]["parity_ok"] and 0 < d["config4"]["frac"] < 1
    assert all(sh["parity_ok"] for sh in d["small_objects"]["shapes"])
    assert d["odd_objects"]["parity_ok"] and d["odd_objects"]["shard_bytes"] % 16 != 0
    assert all(0 < d["odd_objects"][op]["frac"] < 1 for op in ("encode", "reconstruct", "verify"))


def test_bench_plain_run_and_dump(capsys, tmp_path):
    """Without --full the line is the headline alone; --dump-outputs writes
    the parity the oracle computes for the same objects and the erased data
    shards, and a second run with the same arguments writes the same files."""
    from oracle import coracle as CO

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    n, k, m = 48, 4, 2  # 48 x 512 KiB parity = 24 MiB > DUMP_MAX_ELEMS: the sampled path
    s = bench.MiB // k
    got = []
    for name in ("a", "b"):
        rc = bench.main(["--steps", "2", "--warmup", "1", "--objects", str(n), "--settle-ms", "5",
                         "--dump-outputs", str(tmp_path / name)])
        out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        assert rc == 0 and len(out) == 1
        d = json.loads(out[0])
        assert d["steps"] == 2 and d["warmup"] == 1 and d["parity_ok"] and d["value"] > 0
        assert d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
        assert d["ms_per_step"] > 0 and d["cpu_baseline"] is None
        assert not [leg for leg in FULL_LEGS if leg in d]
        assert sorted(p.name for p in (tmp_path / name).iterdir()) == ["parity.npy", "rebuilt.npy"]
        got.append({x: np.load(tmp_path / name / f"{x}.npy") for x in ("parity", "rebuilt")})
    host = CO.fill_objects(0, n, bench.MiB)
    want_par, _ = CO.encode_batch(k, m, host, threads=CO.cpu_threads())
    want = {"parity": want_par, "rebuilt": host[:, :2 * s]}
    for i, x in enumerate(("parity", "rebuilt")):
        a = got[0][x]
        assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_ELEMS,)
        assert np.array_equal(a, got[1][x])
        idx = np.sort(np.random.default_rng(bench.DUMP_SEED + i).integers(0, want[x].size, bench.DUMP_MAX_ELEMS,
                                                                          dtype=np.int64))
        assert np.array_equal(a, want[x].reshape(-1)[idx].astype(np.float32))
