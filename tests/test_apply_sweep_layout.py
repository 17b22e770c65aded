"""The coverage the encode / reconstruct sweep claims, checked on the layouts
themselves (tests/apply_sweep_layout.py), and the sweep's checker on images a
numpy oracle produced: no GPU."""
import numpy as np
import pytest

import apply_sweep_layout as L
from oracle import coracle as CO

SHAPES = [(4, 2), (11, 4)]


@pytest.fixture(scope="module", params=["stripes", "objects"])
def lay(request):
    return L.Layout(4, 2, request.param)


def residues(lay):
    return lay.S % 16, lay.a % 16, lay.b % 16


def test_smax_is_two_tiles_and_368():
    assert L.SMAX == 2 * 2016 + 368 == 4400 and L.BANDS[-1][1] == L.SMAX and L.BANDS[0][0] == 161


def test_c1_every_length_occurs(lay):
    per = 1 if lay.layout == "stripes" else 4
    assert np.array_equal(np.bincount(lay.S, minlength=L.SMAX + 1)[1:], np.full(L.SMAX, per))
    assert lay.S.min() == 1 and lay.S.max() == L.SMAX


def test_c2_stripes_every_length_and_base_residue_in_each_band():
    lay = L.Layout(4, 2, "stripes")
    s, a, _ = residues(lay)
    assert np.array_equal(a, (lay.S >> 4) & 15)
    for lo, hi in L.BANDS:
        band = (lay.S >= lo) & (lay.S <= hi)
        assert len(set(zip(s[band].tolist(), a[band].tolist()))) == 256, (lo, hi)


def test_c3_objects_every_triple_and_every_pair_in_each_band():
    lay = L.Layout(4, 2, "objects")
    s, a, b = residues(lay)
    big = lay.S > 160
    assert len(set(zip(s[big].tolist(), a[big].tolist(), b[big].tolist()))) == 4096
    for lo, hi in L.BANDS:
        band = (lay.S >= lo) & (lay.S <= hi)
        assert len(set(zip(s[band].tolist(), a[band].tolist()))) == 256, (lo, hi)
        assert len(set(zip(s[band].tolist(), b[band].tolist()))) == 256, (lo, hi)


@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("layout", ["stripes", "objects"])
def test_c4_regions_disjoint_inside_and_sentinels_elsewhere(k, m, layout):
    lay = L.Layout(k, m, layout, smax=700)
    want = lay.expected()
    lost = L.mixed_losses(k, m, lay.n)[0]
    init = lay.initial(want, lost)
    assert [w.size for w in want] == lay.sizes
    for buf, (start, size, ent, first) in enumerate(lay.regions):
        assert np.all(np.diff(start) > 0) and start[0] >= L.GAP
        assert np.all(start[1:] - (start[:-1] + size[:-1]) >= L.GAP)  # disjoint, a gap between entries
        assert start[-1] + size[-1] + L.GAP <= lay.sizes[buf]
        cover = np.zeros(lay.sizes[buf], bool)
        for s0, n in zip(start.tolist(), size.tolist()):
            cover[s0:s0 + n] = True
        assert np.all(want[buf][~cover] == L.FILL) and np.all(init[buf][~cover] == L.FILL)
        # the initial image differs from the expected one inside lost shards only
        assert np.all(cover[init[buf] != want[buf]])
    # every shard of every entry inside its buffer, and where shard() says
    for e in (0, lay.n // 2, lay.n - 1):
        for i in range(k + m):
            buf, off = lay.shard(e, i)
            S = int(lay.S[e])
            assert 0 <= off and off + S <= lay.sizes[buf]
            assert np.array_equal(want[buf][off:off + S], L.pool(k, m)[i, lay.col[e]:lay.col[e] + S])
            assert lay.locate(buf, off) == (e, i, 0) and lay.locate(buf, off + S - 1) == (e, i, S - 1)
            if lost[e, i]:
                assert np.all(init[buf][off:off + S] == L.GARBLE)
    assert len(lay.entries([1 << 20, 1 << 24])) == lay.n


def test_pool_columns_are_oracle_codewords():
    k, m = 4, 2
    cw = L.pool(k, m)
    data = [cw[j, 12345:12345 + 999] for j in range(k)]
    par = CO.apply(CO.build_matrix(k, m)[k:], data, impl=CO.SCALAR)
    for r in range(m):
        assert np.array_equal(par[r], cw[k + r, 12345:12345 + 999])


def numpy_reconstruct(lay, imgs, lost):
    """Rebuild the lost shards of every entry from the first k present ones
    with the oracle's matrix inverse (what the GPU calls are asked to do)."""
    k, m = lay.k, lay.m
    M = CO.build_matrix(k, m)
    for e in range(lay.n):
        miss = np.nonzero(lost[e])[0].tolist()
        if not miss:
            continue
        S = int(lay.S[e])
        surv = [i for i in range(k + m) if i not in miss][:k]
        ins = []
        for i in surv:
            buf, off = lay.shard(e, i)
            ins.append(imgs[buf][off:off + S].copy())
        inv = CO.invert(M[surv])
        data = CO.apply(inv, ins)
        for i in miss:
            out = data[i] if i < k else CO.apply(M[i:i + 1], data)[0]
            buf, off = lay.shard(e, i)
            imgs[buf][off:off + S] = out


@pytest.mark.parametrize("layout", ["stripes", "objects"])
def test_checker_passes_an_oracle_image_and_reports_planted_bytes(layout):
    k, m = 4, 2
    lay = L.Layout(k, m, layout, smax=300)
    want = lay.expected()
    lost, which, P = L.mixed_losses(k, m, lay.n)
    assert set(which.tolist()) == set(range(P)) and set(lost.sum(1).tolist()) == {1, 2}
    got = lay.initial(want, lost)
    assert lay.mismatches(got, want)  # garbled: reported
    numpy_reconstruct(lay, got, lost)
    assert lay.mismatches(got, want) == []
    # one wrong byte in a shard
    e = lay.n - 7
    buf, off = lay.shard(e, k + 1)
    got[buf][off + 33] ^= 0x10
    assert lay.mismatches(got, want) == [(buf, e, k + 1, 33, int(want[buf][off + 33]) ^ 0x10, int(want[buf][off + 33]))]
    got[buf][off + 33] ^= 0x10
    # one changed sentinel byte: 2 bytes past the end of entry e's last shard in that buffer
    end = off + int(lay.S[e])
    assert got[buf][end + 2] == L.FILL
    got[buf][end + 2] = 0
    assert lay.mismatches(got, want) == [(buf, e, -1, 2, 0, L.FILL)]
    got[buf][end + 2] = L.FILL
    # and one before the first entry
    got[0][1] = 7
    assert lay.mismatches(got, want) == [(0, -1, -1, 1, 7, L.FILL)]


def test_single_patterns_and_mixed_losses():
    for k, m in [(4, 2), (2, 4), (8, 3), (12, 4), (24, 4)]:
        one, mix, par = L.single_patterns(k, m)
        assert len(one) == 1 and one[0] < k
        assert len(mix) == min(m, 4) and min(mix) < k <= max(mix) and len(set(mix)) == len(mix)
        assert par == list(range(k, k + m))
        lost, which, P = L.mixed_losses(k, m, L.SMAX)
        assert P == len(L.loss_patterns(k, m)) and set(lost.sum(1).tolist()) == set(range(1, m + 1))
        assert lost.sum(1).max() <= m
        if P <= L.SMAX:
            assert set(which.tolist()) == set(range(P))
    assert len(L.loss_patterns(12, 4)) == 2516
