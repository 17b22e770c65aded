"""hbec_reconstruct_batch_mixed without a GPU: every argument check answers
before anything is queued (as hbec_reconstruct_batch's do), a batch with
nothing to rebuild is a no-op, and every shipped gf_apply_mixed instance
(K = 1..8 x R = 1..4) runs without scratch memory."""
import ctypes as C

import numpy as np
import pytest

import test_kernel_resources as KR
from hummingbird_amd import _native as N
from hummingbird_amd import reedsolomon as RS

K, M = 4, 2
U32P = C.POINTER(C.c_uint32)


def _views(base=4096, n=K + M):
    v = (N.View * n)()
    for i in range(n):
        v[i].base = base + i * 64
        v[i].obj_stride = 1024
    return v


def _call(enc, views, patterns, pattern_of, n_objects=None, shard_len=64, data_only=0, n_patterns=None):
    pat = np.ascontiguousarray(patterns, dtype=np.uint8).reshape(-1, K + M)
    idx = np.ascontiguousarray(pattern_of, dtype=np.uint32)
    return N.lib().hbec_reconstruct_batch_mixed(
        enc.handle, views, pat.ctypes.data_as(N._U8P), pat.shape[0] if n_patterns is None else n_patterns,
        idx.ctypes.data_as(U32P), idx.size if n_objects is None else n_objects, shard_len, data_only, None)


FULL = [1] * (K + M)
LOST0 = [0, 1, 1, 1, 1, 1]


def test_null_arguments():
    enc = RS.New(K, M)
    L = N.lib()
    pat = (C.c_uint8 * (K + M))(*LOST0)
    idx = (C.c_uint32 * 1)(0)
    v = _views()
    assert L.hbec_reconstruct_batch_mixed(None, v, pat, 1, idx, 1, 64, 0, None) == N.ERR_INVALID_ARG
    assert N.last_error()
    assert L.hbec_reconstruct_batch_mixed(enc.handle, None, pat, 1, idx, 1, 64, 0, None) == N.ERR_INVALID_ARG
    assert L.hbec_reconstruct_batch_mixed(enc.handle, v, None, 1, idx, 1, 64, 0, None) == N.ERR_INVALID_ARG
    assert L.hbec_reconstruct_batch_mixed(enc.handle, v, pat, 1, None, 1, 64, 0, None) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    a = C.c_uint64()
    assert L.hbec_mixed_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert L.hbec_mixed_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert N.last_error()
    b, c = C.c_uint64(), C.c_uint64()
    assert L.hbec_mixed_walk_stats(None, C.byref(b), C.byref(c)) == N.ERR_INVALID_ARG
    assert L.hbec_mixed_walk_stats(C.byref(a), None, C.byref(c)) == N.ERR_INVALID_ARG
    assert L.hbec_mixed_walk_stats(C.byref(a), C.byref(b), None) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    assert L.hbec_mixed_walk_stats(C.byref(a), C.byref(b), C.byref(c)) == N.HBEC_OK


def test_pattern_count_and_index_errors():
    enc = RS.New(K, M)
    v = _views()
    assert _call(enc, v, [LOST0], [0], n_patterns=0) == N.ERR_INVALID_ARG  # objects, no patterns
    assert N.last_error()
    big = np.ones((65537, K + M), np.uint8)
    assert _call(enc, v, big, [0]) == N.ERR_INVALID_ARG
    assert "65536" in N.last_error()
    assert _call(enc, v, big[:65536], [65535]) == N.HBEC_OK  # the limit itself; nothing missing
    assert _call(enc, v, [LOST0, FULL], [0, 1, 2]) == N.ERR_INVALID_ARG  # index == n_patterns
    assert "object 2" in N.last_error()
    assert _call(enc, v, [LOST0], [0xFFFFFFFF]) == N.ERR_INVALID_ARG


def test_too_few_shards_in_any_listed_pattern():
    enc = RS.New(K, M)
    v = _views()
    few = [1, 1, 1, 0, 0, 0]
    assert _call(enc, v, [LOST0, few], [0, 1]) == N.ERR_TOO_FEW_SHARDS
    assert N.last_error()
    # listed but used by no object: still an error
    assert _call(enc, v, [FULL, few], [0, 0]) == N.ERR_TOO_FEW_SHARDS
    assert "pattern 1" in N.last_error()
    # with data_only a pattern still needs k shards
    assert _call(enc, v, [few], [0], data_only=1) == N.ERR_TOO_FEW_SHARDS


def test_null_view_base():
    enc = RS.New(K, M)
    v = _views()
    v[0].base = None  # shard 0 is an output of LOST0
    assert _call(enc, v, [LOST0], [0]) == N.ERR_INVALID_ARG
    assert "view" in N.last_error()
    v = _views()
    v[2].base = None  # a survivor
    assert _call(enc, v, [LOST0], [0]) == N.ERR_INVALID_ARG
    # precedence: a bad index is reported although a view is null too
    assert _call(enc, v, [LOST0], [3]) == N.ERR_INVALID_ARG
    assert "index" in N.last_error()


def test_nothing_to_do_is_ok():
    enc = RS.New(K, M)
    v = _views()
    assert _call(enc, v, [FULL], [0] * 7) == N.HBEC_OK  # all present
    assert _call(enc, v, [[1, 1, 1, 1, 0, 0], [1, 1, 1, 1, 0, 1]], [0, 1, 1], data_only=1) == N.HBEC_OK
    assert _call(enc, v, [LOST0], [0], n_objects=0) == N.HBEC_OK
    assert _call(enc, v, [LOST0], [0], shard_len=0) == N.HBEC_OK
    assert _call(enc, v, [LOST0], np.zeros(0, np.uint32), n_patterns=0) == N.HBEC_OK
    # errors come first even when there is no work
    assert _call(enc, v, [LOST0], [1], shard_len=0) == N.ERR_INVALID_ARG
    assert _call(enc, v, [[1, 0, 0, 0, 0, 0]], [0], n_objects=0) == N.ERR_TOO_FEW_SHARDS


def test_chunk_hook_and_stats_answer():
    L = N.lib()
    a, b = C.c_uint64(), C.c_uint64()
    assert L.hbec_mixed_stats(C.byref(a), C.byref(b)) == N.HBEC_OK
    assert L.hbec_set_mixed_chunk_tiles(64) == N.HBEC_OK
    assert L.hbec_set_mixed_chunk_tiles(0) == N.HBEC_OK
    a2, b2 = C.c_uint64(), C.c_uint64()
    assert L.hbec_mixed_stats(C.byref(a2), C.byref(b2)) == N.HBEC_OK
    assert (a2.value, b2.value) == (a.value, b.value)  # nothing was launched here


def test_mixed_instances_use_no_scratch():
    """K = 1..8 x R = 1..4: the tables of the largest instances (8+3: 120
    words, 8+4: 160) stay in registers."""
    found = KR.kernels("gf_apply_mixedILi")
    assert len(found) >= 32, sorted(found)
    for kk in range(1, 9):
        for r in range(1, 5):
            assert any(f"gf_apply_mixedILi{kk}ELi{r}E" in nm for nm in found), (kk, r)
    bad = {nm: k[".private_segment_fixed_size"] for nm, k in found.items() if k[".private_segment_fixed_size"] != 0}
    assert not bad, bad
    lds = {nm: k[".group_segment_fixed_size"] for nm, k in found.items() if k[".group_segment_fixed_size"] != 0}
    assert not lds, lds
