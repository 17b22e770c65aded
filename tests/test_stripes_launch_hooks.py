"""Argument handling of the test hook hbec_set_stripes_grid_cap and of the
counters hbec_stripes_kernel_stats and hbec_host_run_stats (CPU only: they set
or read process-wide values and touch no device)."""
import ctypes as C

import pytest

from hummingbird_amd import _native as N
from hummingbird_amd import batch as B


@pytest.fixture(autouse=True)
def _restore():
    yield
    B.set_stripes_grid_cap(0)


def test_grid_cap_bounds():
    L = N.lib()
    for cap in (1, 3, 1 << 20, 0):
        assert L.hbec_set_stripes_grid_cap(cap) == 0
        B.set_stripes_grid_cap(cap)
    assert L.hbec_set_stripes_grid_cap(-1) == N.ERR_INVALID_ARG
    assert "negative" in N.last_error()
    with pytest.raises(Exception):
        B.set_stripes_grid_cap(-5)
    assert L.hbec_set_stripes_grid_cap(0) == 0


def test_stripes_kernel_stats_answers_without_a_device():
    L = N.lib()
    v = [C.c_uint64(1 << 40) for _ in range(5)]
    assert L.hbec_stripes_kernel_stats(None, None, None, None, None) == 0
    for i in range(5):
        args = [None] * 5
        args[i] = C.byref(v[i])
        assert L.hbec_stripes_kernel_stats(*args) == 0
    s = B.stripes_kernel_stats()
    assert list(s) == ["plain", "split", "accumulate", "mirror", "mirror_accumulate"]
    assert [x.value for x in v] == list(s.values())  # nothing was coded in between


def test_host_run_stats_answers_without_a_device():
    L = N.lib()
    v = [C.c_uint64(1 << 40) for _ in range(4)]
    assert L.hbec_host_run_stats(None, None, None, None) == 0
    for i in range(4):
        args = [None] * 4
        args[i] = C.byref(v[i])
        assert L.hbec_host_run_stats(*args) == 0
    s = B.host_run_stats()
    assert list(s) == ["ring_chunks", "ring_pieces", "zc_record_slots", "arena_flushes"]
    assert [x.value for x in v] == list(s.values())
