"""hbec_reconstruct_plan_mixed without a GPU: every argument check answers
before anything is queued, with the codes, precedence and message keywords of
hbec_reconstruct_batch_mixed (tests/test_mixed_host.py); a call with nothing to
rebuild is a no-op; and every shipped gf_mixed_plan instance (R = 1..4) runs
without scratch memory.  The plans here are built from zero-length entries
only, which need no device memory."""
import ctypes as C

import numpy as np
import pytest

import test_kernel_resources as KR
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS

K, M = 4, 2
U32P = C.POINTER(C.c_uint32)
FULL = [1] * (K + M)
LOST0 = [0, 1, 1, 1, 1, 1]
FEW = [1, 1, 1, 0, 0, 0]


def _plan(enc, n=5, objects=False):
    if objects:
        return B.StripePlan(enc, objects=[(0, 0, 0)] * n)
    return B.StripePlan(enc, stripes=[(0, 0)] * n)


def _call(enc, plan, patterns, pattern_of, data_only=0, n_patterns=None):
    pat = np.ascontiguousarray(patterns, dtype=np.uint8).reshape(-1, K + M)
    idx = np.ascontiguousarray(pattern_of, dtype=np.uint32)
    return N.lib().hbec_reconstruct_plan_mixed(
        enc.handle, plan._h, pat.ctypes.data_as(N._U8P), pat.shape[0] if n_patterns is None else n_patterns,
        idx.ctypes.data_as(U32P), data_only, None)


@pytest.mark.parametrize("objects", [False, True])
def test_null_arguments(objects):
    enc = RS.New(K, M)
    plan = _plan(enc, objects=objects)
    L = N.lib()
    pat = (C.c_uint8 * (K + M))(*LOST0)
    idx = (C.c_uint32 * 5)()
    assert L.hbec_reconstruct_plan_mixed(None, plan._h, pat, 1, idx, 0, None) == N.ERR_INVALID_ARG
    assert N.last_error()
    assert L.hbec_reconstruct_plan_mixed(enc.handle, None, pat, 1, idx, 0, None) == N.ERR_INVALID_ARG
    assert L.hbec_reconstruct_plan_mixed(enc.handle, plan._h, None, 1, idx, 0, None) == N.ERR_INVALID_ARG
    assert L.hbec_reconstruct_plan_mixed(enc.handle, plan._h, pat, 1, None, 0, None) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    a = C.c_uint64()
    assert L.hbec_mixed_plan_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert L.hbec_mixed_plan_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert N.last_error()


def test_plan_of_another_shape():
    enc = RS.New(K, M)
    plan = _plan(RS.New(8, 3))
    assert _call(enc, plan, [LOST0], [0] * 5) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()
    # precedence: reported before a bad pattern count or index
    assert _call(enc, plan, [LOST0], [7] * 5, n_patterns=0) == N.ERR_INVALID_ARG
    assert "(k, m)" in N.last_error()


def test_pattern_count_and_index_errors():
    enc = RS.New(K, M)
    plan = _plan(enc)
    assert _call(enc, plan, [LOST0], [0] * 5, n_patterns=0) == N.ERR_INVALID_ARG  # entries, no patterns
    assert N.last_error()
    big = np.ones((65537, K + M), np.uint8)
    assert _call(enc, plan, big, [0] * 5) == N.ERR_INVALID_ARG
    assert "65536" in N.last_error()
    assert _call(enc, plan, big[:65536], [65535] * 5) == N.HBEC_OK  # the limit itself; nothing missing
    # an index == n_patterns, on a zero-length entry (all of them are)
    assert _call(enc, plan, [LOST0, FULL], [0, 1, 2, 0, 0]) == N.ERR_INVALID_ARG
    assert "index" in N.last_error() and "2" in N.last_error()
    assert _call(enc, plan, [LOST0], [0, 0, 0, 0, 0xFFFFFFFF]) == N.ERR_INVALID_ARG


def test_too_few_shards_in_any_listed_pattern():
    enc = RS.New(K, M)
    plan = _plan(enc)
    assert _call(enc, plan, [LOST0, FEW], [0, 1, 0, 1, 0]) == N.ERR_TOO_FEW_SHARDS
    assert N.last_error()
    # listed but used by no entry: still an error
    assert _call(enc, plan, [FULL, FEW], [0] * 5) == N.ERR_TOO_FEW_SHARDS
    assert "pattern 1" in N.last_error()
    # with data_only a pattern still needs k shards
    assert _call(enc, plan, [FEW], [0] * 5, data_only=1) == N.ERR_TOO_FEW_SHARDS
    # precedence, as hbec_reconstruct_batch_mixed: before a bad index
    assert _call(enc, plan, [FEW], [3] * 5) == N.ERR_TOO_FEW_SHARDS


@pytest.mark.parametrize("objects", [False, True])
def test_nothing_to_do_is_ok_and_launches_nothing(objects):
    enc = RS.New(K, M)
    s0 = B.mixed_plan_stats()
    plan = _plan(enc, objects=objects)
    assert _call(enc, plan, [FULL], [0] * 5) == N.HBEC_OK
    assert _call(enc, plan, [LOST0], [0] * 5) == N.HBEC_OK  # zero-length entries: nothing to rebuild
    assert _call(enc, plan, [[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 0, 1]], [0, 1, 1, 0, 1], data_only=1) == N.HBEC_OK
    empty = _plan(enc, 0, objects=objects)
    assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32)) == N.HBEC_OK
    assert _call(enc, empty, [LOST0], np.zeros(0, np.uint32), n_patterns=0) == N.HBEC_OK
    # errors come first even when there is no work
    assert _call(enc, empty, [[1, 0, 0, 0, 0, 0]], np.zeros(0, np.uint32)) == N.ERR_TOO_FEW_SHARDS
    with pytest.raises(ValueError):  # the shape is checked before a stream is asked for
        plan.reconstruct_mixed(np.ones((4, K + M), np.uint8))
    with pytest.raises(ValueError):
        plan.reconstruct_mixed(np.ones((5, K + M + 1), np.uint8))
    with pytest.raises(ValueError):
        plan.reconstruct_mixed(np.ones(5 * (K + M), np.uint8))
    assert B.mixed_plan_stats() == s0


def test_chunk_hook_stats_and_tile_bytes_answer():
    a = B.mixed_plan_stats()
    B.set_mixed_plan_chunk_tiles(64)
    B.set_mixed_plan_chunk_tiles(0)
    assert B.mixed_plan_stats() == a  # nothing was launched here
    T = B.mixed_plan_tile_bytes()
    assert T > 0 and T % 16 == 0


def test_mixed_plan_instances_use_no_scratch():
    """R = 1..4 (K is a run-time argument): bases, indices and tables come
    through scalar loads, nothing is indexed in private memory."""
    found = KR.kernels("gf_mixed_planILi")
    assert len(found) == 4, sorted(found)
    for r in range(1, 5):
        assert any(f"gf_mixed_planILi{r}E" in nm for nm in found), r
    bad = {nm: k[".private_segment_fixed_size"] for nm, k in found.items() if k[".private_segment_fixed_size"] != 0}
    assert not bad, bad
    lds = {nm: k[".group_segment_fixed_size"] for nm, k in found.items() if k[".group_segment_fixed_size"] != 0}
    assert not lds, lds
