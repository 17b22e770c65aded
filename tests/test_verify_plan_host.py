"""hbec_verify_plan / hbec_verify_host without a GPU: every argument check
answers before anything is queued and without touching a device (a plan of
zero-length stripes is built on the host alone), m = 0 and all-empty inputs are
no-ops, and every shipped plan Verify kernel runs without scratch memory."""
import ctypes as C

import numpy as np
import pytest

import test_kernel_resources as KR
from hummingbird_amd import _native as N
from hummingbird_amd import batch as B
from hummingbird_amd import reedsolomon as RS


def _empty_plan(enc, n=3, objects=False):
    """A plan of n zero-length stripes: no device memory, no launch."""
    h = C.c_void_p()
    if objects:
        arr = (N.Object * n)()
        assert N.lib().hbec_plan_objects(enc.handle, arr, n, C.byref(h)) == N.HBEC_OK
    else:
        arr = (N.Stripe * n)()
        assert N.lib().hbec_plan_stripes(enc.handle, arr, n, C.byref(h)) == N.HBEC_OK
    return h


def test_verify_plan_argument_errors_need_no_device():
    L = N.lib()
    enc, other = RS.New(4, 2), RS.New(8, 3)
    flags = (C.c_uint32 * 3)(7, 7, 7)
    for objects in (False, True):
        h = _empty_plan(enc, 3, objects)
        assert L.hbec_verify_plan(None, h, flags, None) == N.ERR_INVALID_ARG
        assert "null" in N.last_error()
        assert L.hbec_verify_plan(enc.handle, None, flags, None) == N.ERR_INVALID_ARG
        assert L.hbec_verify_plan(enc.handle, h, None, None) == N.ERR_INVALID_ARG  # 3 entries, no flags
        assert L.hbec_verify_plan(other.handle, h, flags, None) == N.ERR_INVALID_ARG
        assert "(k, m)" in N.last_error()
        L.hbec_plan_free(h)
    # no stripes at all: d_flags may be NULL
    h = _empty_plan(enc, 0)
    assert L.hbec_verify_plan(enc.handle, h, None, None) == N.HBEC_OK
    L.hbec_plan_free(h)
    assert list(flags) == [7, 7, 7]


def test_verify_plan_of_zero_length_stripes_leaves_flags():
    L = N.lib()
    enc = RS.New(4, 2)
    flags = (C.c_uint32 * 3)(5, 0, 2)  # host memory: a call that touched it on a device would fault
    for objects in (False, True):
        h = _empty_plan(enc, 3, objects)
        assert L.hbec_verify_plan(enc.handle, h, flags, None) == N.HBEC_OK
        L.hbec_plan_free(h)
    assert list(flags) == [5, 0, 2]


def test_verify_plan_without_parity_is_ok():
    L = N.lib()
    enc = RS.New(4, 0)
    h = _empty_plan(enc, 2)
    flags = (C.c_uint32 * 2)(1, 0)
    assert L.hbec_verify_plan(enc.handle, h, flags, None) == N.HBEC_OK
    assert list(flags) == [1, 0]
    L.hbec_plan_free(h)
    # m = 0 answers before the stripes are looked at
    st = (N.Stripe * 1)()
    st[0].base, st[0].shard_len = 4096, 64
    out = (C.c_uint8 * 1)(9)
    assert L.hbec_verify_host(enc.handle, st, 1, out) == N.HBEC_OK
    assert out[0] == 0


def test_verify_host_argument_errors_need_no_device():
    L = N.lib()
    enc = RS.New(4, 2)
    st = (N.Stripe * 2)()
    out = (C.c_uint8 * 2)(9, 9)
    assert L.hbec_verify_host(None, st, 2, out) == N.ERR_INVALID_ARG
    assert L.hbec_verify_host(enc.handle, None, 2, out) == N.ERR_INVALID_ARG
    assert L.hbec_verify_host(enc.handle, st, 2, None) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    st[1].base, st[1].shard_len = None, 16
    assert L.hbec_verify_host(enc.handle, st, 2, out) == N.ERR_INVALID_ARG
    assert "base" in N.last_error()
    assert list(out) == [9, 9]  # errors leave the flags alone
    assert L.hbec_verify_host(enc.handle, None, 0, None) == N.HBEC_OK
    # only zero-length stripes: flags 0, no device
    st[1].shard_len = 0
    assert L.hbec_verify_host(enc.handle, st, 2, out) == N.HBEC_OK
    assert list(out) == [0, 0]
    assert enc.VerifyStripes([np.zeros(0, np.uint8)] * 3).tolist() == [False] * 3
    assert enc.VerifyStripes([]).tolist() == []


def test_stats_and_tile_bytes_answer():
    L = N.lib()
    a = C.c_uint64()
    assert L.hbec_verify_plan_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert L.hbec_verify_plan_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert L.hbec_verify_route_stats(None) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    r0 = B.verify_route_stats()
    assert list(r0) == ["packed", "pipe", "records", "odd", "wide", "unaligned", "scratch"]
    assert B.verify_route_stats() == r0  # nothing was verified here
    assert L.hbec_apply_route_stats(None) == N.ERR_INVALID_ARG
    assert "null" in N.last_error()
    a0 = B.apply_route_stats()
    assert list(a0) == ["packed", "vec", "odd", "unaligned", "wide"]
    assert B.apply_route_stats() == a0  # nothing was coded here
    s0 = B.verify_plan_stats()
    assert set(s0) == {"plan_launches", "per_stripe_calls"}
    assert B.verify_plan_stats() == s0  # nothing was launched here
    t = B.verify_plan_tile_bytes(8)
    assert t > 0 and t % 16 == 0 and t == B.verify_plan_tile_bytes(4)


def test_plan_verify_kernels_use_no_scratch():
    """gf_verify_tiles K = 1..8 x R = 1..4 and gf_verify_recs / its tail R =
    1..4: no private segment; only gf_verify_recs uses LDS (its tables, < 1 KiB)."""
    found = {**KR.kernels("gf_verify_tiles"), **KR.kernels("gf_verify_recs")}
    for kk in range(1, 9):
        for r in range(1, 5):
            assert any(f"gf_verify_tilesILi{kk}ELi{r}E" in nm for nm in found), (kk, r)
    for r in range(1, 5):
        assert any(f"gf_verify_recsILi{r}E" in nm for nm in found), r
        assert any(f"gf_verify_recs_tailILi{r}E" in nm for nm in found), r
    bad = {nm: k[".private_segment_fixed_size"] for nm, k in found.items() if k[".private_segment_fixed_size"] != 0}
    assert not bad, bad
    lds = {nm: k[".group_segment_fixed_size"] for nm, k in found.items()
           if k[".group_segment_fixed_size"] != 0 and "gf_verify_recsILi" not in nm}
    assert not lds, lds
    assert all(k[".group_segment_fixed_size"] <= 1024 for k in found.values())
