"""hbec_check_rows: what the degraded Verify (hbec_verify_plan_mixed) checks for
one present mask.  The survivors are the first k present shards, the checked
shards the other present ones, and the row of a checked shard c is the Lagrange
basis over the survivor points evaluated at c (oracle/lagrange.py), which never
inverts a matrix.  CPU only: no device is touched."""
import ctypes as C
import itertools

import numpy as np
import pytest

from hummingbird_amd import _native as N
from hummingbird_amd import reedsolomon as RS
from oracle import lagrange as LG

U32P = C.POINTER(C.c_uint32)


def masks(k, m, max_lost):
    n = k + m
    for lost_n in range(0, max_lost + 1):
        for lost in itertools.combinations(range(n), lost_n):
            yield [0 if i in lost else 1 for i in range(n)]


@pytest.mark.parametrize("k,m,max_lost", [(4, 2, 2), (8, 3, 3), (10, 4, 2), (12, 4, 2), (17, 3, 0)])
def test_rows_are_the_lagrange_rows_over_the_first_k_present(k, m, max_lost):
    enc = RS.New(k, m)
    seen = 0
    for mask in masks(k, m, max_lost):
        here = [i for i in range(k + m) if mask[i]]
        surv, checked, rows = enc.check_rows(mask)
        assert surv == here[:k]
        assert checked == here[k:]
        assert all(c >= k for c in checked)  # a present data shard is always a survivor
        assert rows.shape == (len(checked), k)
        for c, row in zip(checked, rows):
            assert row.tolist() == LG.lagrange_row(surv, c), (mask, c)
            assert row.all(), (mask, c)  # c is no survivor point: every survivor counts
        seen += 1
    assert seen == sum(len(list(itertools.combinations(range(k + m), q))) for q in range(max_lost + 1))


@pytest.mark.parametrize("k,m", [(4, 2), (8, 3), (12, 4), (17, 3)])
def test_all_present_rows_are_the_parity_rows(k, m):
    enc = RS.New(k, m)
    mat = (C.c_uint8 * ((k + m) * k))()
    assert N.lib().hbec_matrix(enc.handle, mat) == N.HBEC_OK
    parity = np.frombuffer(bytes(mat), np.uint8).reshape(k + m, k)[k:]
    surv, checked, rows = enc.check_rows([1] * (k + m))
    assert surv == list(range(k)) and checked == list(range(k, k + m))
    assert np.array_equal(rows, parity)


@pytest.mark.parametrize("k,m", [(4, 2), (8, 3)])
def test_exactly_k_present_checks_nothing(k, m):
    enc = RS.New(k, m)
    for lost in itertools.combinations(range(k + m), m):
        mask = [0 if i in lost else 1 for i in range(k + m)]
        surv, checked, rows = enc.check_rows(mask)
        assert surv == [i for i in range(k + m) if mask[i]] and checked == [] and rows.shape == (0, k)


def test_too_few_shards_and_null_arguments():
    enc = RS.New(4, 2)
    with pytest.raises(RS.ErrTooFewShards):
        enc.check_rows([1, 1, 1, 0, 0, 0])
    with pytest.raises(RS.ErrTooFewShards):
        enc.check_rows([0] * 6)
    L = N.lib()
    p = (C.c_uint8 * 6)(1, 1, 1, 1, 1, 1)
    sv, ck, nc, rows = (C.c_int * 4)(), (C.c_int * 2)(), C.c_int(), (C.c_uint8 * 8)()
    good = [enc.handle, p, sv, ck, C.byref(nc), rows]
    assert L.hbec_check_rows(*good) == N.HBEC_OK and nc.value == 2
    for i in range(len(good)):
        args = list(good)
        args[i] = None
        assert L.hbec_check_rows(*args) == N.ERR_INVALID_ARG, i


def test_verify_plan_mixed_null_arguments_need_no_plan():
    enc = RS.New(4, 2)
    L = N.lib()
    pat = (C.c_uint8 * 6)(1, 1, 1, 1, 1, 1)
    idx = (C.c_uint32 * 1)(0)
    flags = (C.c_uint32 * 1)(0)  # never written: every call fails its argument check
    fake_plan = C.c_void_p(0)
    assert L.hbec_verify_plan_mixed(None, fake_plan, pat, 1, idx, flags, None) == N.ERR_INVALID_ARG
    assert L.hbec_verify_plan_mixed(enc.handle, None, pat, 1, idx, flags, None) == N.ERR_INVALID_ARG
    a = C.c_uint64()
    assert L.hbec_verify_mixed_plan_stats(None, C.byref(a)) == N.ERR_INVALID_ARG
    assert L.hbec_verify_mixed_plan_stats(C.byref(a), None) == N.ERR_INVALID_ARG
    assert L.hbec_verify_mixed_plan_tile_bytes() == L.hbec_mixed_plan_tile_bytes()


def test_verify_plan_mixed_arguments_on_a_plan_of_zero_length_entries():
    """Zero-length entries are planned on the host alone, so every argument
    check answers without a device, and a valid call queues nothing."""
    from hummingbird_amd import batch as B

    enc, other = RS.New(4, 2), RS.New(8, 3)
    L = N.lib()
    pats = np.array([[0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0]], np.uint8)
    idx = np.array([0, 1, 0], np.uint32)
    bad = np.array([0, 1, 2], np.uint32)
    flags = (C.c_uint32 * 3)(0, 0, 0)  # host memory: no flag of a zero-length entry is ever touched

    def call(e, plan, p, n_p, i, f):
        return L.hbec_verify_plan_mixed(e.handle, plan._h, None if p is None else p.ctypes.data_as(N._U8P), n_p,
                                        None if i is None else i.ctypes.data_as(U32P), f, None)

    for plan in (B.StripePlan(enc, stripes=[(0, 0)] * 3), B.StripePlan(enc, objects=[(0, 0, 0)] * 3)):
        assert call(enc, plan, None, 2, idx, flags) == N.ERR_INVALID_ARG
        assert call(enc, plan, pats, 2, None, flags) == N.ERR_INVALID_ARG
        assert call(enc, plan, pats, 2, idx, None) == N.ERR_INVALID_ARG  # entries, no flags
        assert call(other, plan, pats, 2, idx, flags) == N.ERR_INVALID_ARG
        assert call(enc, plan, pats, 0, idx, flags) == N.ERR_INVALID_ARG
        assert call(enc, plan, pats, 65537, idx, flags) == N.ERR_INVALID_ARG
        assert call(enc, plan, pats, 2, bad, flags) == N.ERR_INVALID_ARG and "index" in N.last_error()
        assert call(enc, plan, pats, 3, idx, flags) == N.ERR_TOO_FEW_SHARDS  # listed, unused
        assert call(enc, plan, pats, 2, idx, flags) == N.HBEC_OK
        assert list(flags) == [0, 0, 0]
    empty = B.StripePlan(enc, stripes=[])
    assert call(enc, empty, pats, 1, idx, None) == N.HBEC_OK
    assert call(enc, empty, pats, 0, idx, None) == N.HBEC_OK


def test_verify_mixed_plan_instances_use_no_scratch_and_no_lds():
    """RMAX = 1..4 (K is a run-time argument): bases, indices and tables come
    through scalar loads, nothing is indexed in private memory."""
    import test_kernel_resources as KR

    found = KR.kernels("gf_verify_mixed_planILi")
    assert len(found) == 4, sorted(found)
    for r in range(1, 5):
        assert any(f"gf_verify_mixed_planILi{r}E" in nm for nm in found), r
    for nm, k in found.items():
        assert k[".private_segment_fixed_size"] == 0 and k[".group_segment_fixed_size"] == 0, nm
        assert k[".vgpr_count"] <= 168, (nm, k[".vgpr_count"])  # three waves per SIMD at the least
