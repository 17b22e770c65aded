"""Byte-exact sweep of the 16-B-aligned strided apply kernels of
csrc/kernels.hip: gf_apply_packed<K,R>, gf_apply_vec_pipe2<K,R>,
gf_apply_vec_pipe<K,R>, gf_apply_vec<K,R> and gf_apply_vec_stream<R>, one
case per kernel instance (tests/vec_sweep_cases.py; what its cases cover is
asserted in tests/test_vec_sweep_cases.py).

This family is what bench.py measures, and a wrong byte from it is silent data
loss.  What varies inside the kernels is a function of S mod tile, the tiles
per object, the tile count of the launch against the waves of the grid, and
for the packed kernel the elements per object against the tile: full or
partial last tile, the clamp of the loads to the last 16 B, the masked store,
the stand-in tile of a wave past the end, gf_apply_vec_pipe2's groups and
runs, the packed kernel's per-lane (object, offset), the read-back of an
accumulate pass.  Every length of an instance runs twice through
batch.apply_views, once as a single block of 4 waves over 3..6 objects and
once on an uncapped grid over 2, every third length with its inputs and
outputs in two arrays of different pitch.

One device buffer per instance holds a region per call, filled with
fill_splitmix (pads and the canaries between regions included), outputs
garbled.  hbec_vec_kernel_stats is read around every call: the launches must
be the ones the restated rule names, kernel by kernel.  Expected bytes are
the oracle's (coracle.apply_batch over the same views of a host copy taken
before the calls); the whole buffer is compared, so inputs, pads and canaries
must be unchanged.  No tolerance, no sampling.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from hummingbird_amd import batch as B
from oracle import coracle as CO

import vec_sweep_cases as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)
    yield


@pytest.fixture(autouse=True)
def _hooks():
    yield
    B.set_vec_grid_cap(0)
    B.set_vec_chunk_tiles(0)
    B.set_force_stream(False)


def describe(inst, reg, off):
    """where byte `off` of the buffer lies in region `reg`"""
    c = reg.case
    for what, views in (("input", reg.in_views), ("output", reg.out_views)):
        for i, (base, stride) in enumerate(views):
            o, w = divmod(off - base, stride)
            if off >= base and o < c.n and w < c.S:
                return f"{what} shard row {i} object {o} offset {w}"
    return "outside every shard (row pad)"


def fail_at(inst, regs, got, want):
    bad = np.flatnonzero(got != want)
    off = int(bad[0])
    T = V.tile_bytes(inst)
    reg = next((r for r in regs if r.begin <= off < r.end), None)
    if reg is None:
        nxt = next((r for r in regs if r.begin > off), None)
        where = f"canary before the region of {nxt.case}" if nxt else "canary after the last region"
    else:
        c = reg.case
        where = (f"S={c.S} ({c.S // T} tiles + {c.S % T}) n={c.n} cap={c.cap} "
                 f"{'two arrays' if c.split else 'one array'}: {describe(inst, reg, off)}")
    pytest.fail(f"{inst.name} ({inst.rows} x {inst.cols}): {bad.size} bytes differ; first at buffer offset {off}: "
                f"{where}; got {int(got[off])} want {int(want[off])}")


@pytest.mark.parametrize("inst", V.INSTANCES, ids=[i.name for i in V.INSTANCES])
def test_every_length_of_the_instance(inst):
    regs, size = V.layout(inst)
    coeffs = V.coeffs(inst)
    buf = torch.empty(size, dtype=torch.uint8, device="cuda")
    base = buf.data_ptr()
    assert base % 128 == 0  # so offsets mod 128 are address residues
    B.fill_splitmix(buf.view(1, size), size, first=len(inst.name) * 1000 + inst.rows * 100 + inst.cols)
    for r in regs:
        off, stride = r.out_views[0]
        buf.as_strided((r.case.n, inst.rows * r.case.S), (stride, 1), off).fill_(V.GARBLE)
    want = buf.cpu().numpy()  # synchronises; the oracle writes its outputs into this copy

    B.set_force_stream(inst.force)
    cap = None
    for r in regs:
        c = r.case
        if c.cap != cap:
            cap = c.cap
            B.set_vec_grid_cap(cap)
        s0 = B.vec_kernel_stats()
        B.apply_views(inst.rows, inst.cols, coeffs, [(base + o, s) for o, s in r.in_views],
                      [(base + o, s) for o, s in r.out_views], c.n, c.S)
        s1 = B.vec_kernel_stats()
        delta = {k: s1[k] - s0[k] for k in s0}
        assert delta == V.launches(inst.rows, inst.cols, c.S, inst.force), (inst.name, c, delta)
    torch.cuda.synchronize()

    hbase = want.ctypes.data

    def oracle(r):
        CO.apply_batch(coeffs, [(hbase + o, s) for o, s in r.in_views], [(hbase + o, s) for o, s in r.out_views],
                       r.case.n, r.case.S)

    with ThreadPoolExecutor(CO.cpu_threads()) as ex:
        list(ex.map(oracle, regs))
    got = buf.cpu().numpy()
    if not np.array_equal(got, want):
        fail_at(inst, regs, got, want)
    # the expected image is not the garbled one it started from: the oracle wrote its outputs
    o, S = regs[-1].out_views[0][0], regs[-1].case.S
    assert (want[o:o + S] != V.GARBLE).any()


@pytest.mark.parametrize("kernel,K,R,S,chunk,n,launches", V.CUTS,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[6]}-launches" for c in V.CUTS])
def test_cut_launches_code_the_same_bytes(kernel, K, R, S, chunk, n, launches):
    """set_vec_chunk_tiles cuts a batch into launches of whole objects, each
    with its bases moved to its first object: the bytes are those of the one
    launch."""
    inst = V.Instance(f"cut-{kernel}", kernel, K, R, R, K, False)
    coeffs = V.coeffs(inst)
    pitch = (K + R) * S + V.ROW_PAD
    buf = torch.empty((n, pitch), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(buf, pitch, first=S + n)
    buf[:, K * S:(K + R) * S] = V.GARBLE
    start = buf.clone()
    base = buf.data_ptr()
    iv = [(base + j * S, pitch) for j in range(K)]
    ov = [(base + (K + r) * S, pitch) for r in range(R)]

    def run(tiles):
        buf.copy_(start)
        B.set_vec_chunk_tiles(tiles)
        s0 = B.vec_kernel_stats()
        B.apply_views(R, K, coeffs, iv, ov, n, S)
        s1 = B.vec_kernel_stats()
        torch.cuda.synchronize()
        return buf.clone(), {k: s1[k] - s0[k] for k in s0 if s1[k] != s0[k]}

    whole, d0 = run(0)
    assert d0 == {kernel: 1}, d0
    cut, d1 = run(chunk)
    assert d1 == {kernel: launches} and V.cut_launches(kernel, K, S, chunk, n) == launches, d1
    assert torch.equal(cut, whole)
    assert torch.equal(whole[:, :K * S], start[:, :K * S]) and torch.equal(whole[:, (K + R) * S:], start[:, (K + R) * S:])
    want = start.cpu().numpy()
    h = want.ctypes.data
    CO.apply_batch(coeffs, [(h + j * S, pitch) for j in range(K)], [(h + (K + r) * S, pitch) for r in range(R)], n, S)
    assert np.array_equal(whole.cpu().numpy(), want)
