"""Cases of the aligned apply sweep (tests/test_gpu_vec_sweep.py): which kernel
instance a call has to run, at which shard lengths and object counts, and
where its shards lie.  Plain Python, no torch, no numpy;
tests/test_vec_sweep_cases.py asserts what these cases cover on a machine
without a GPU.

The family is the 16-B-aligned strided apply of csrc/kernels.hip:
gf_apply_packed<K,R>, gf_apply_vec_pipe2<K,R>, gf_apply_vec_pipe<K,R>,
gf_apply_vec<K,R> and gf_apply_vec_stream<R>.  Every call is
batch.apply_views(rows, cols, coeffs, ...) over views whose bases, strides and
shard length are multiples of 16.

The rules restated here are the library's (hbec.cpp apply_views, kernels.hip
launch_vec / is_packed_shape), written out a second time; only the thresholds
are read from csrc/tuning.h.  A call is cut into row passes of 4 and, inside
each, column passes of 16; a column pass after the first accumulates.  A pass
of K inputs and R rows over shards of S bytes runs

  * gf_apply_packed   K <= 8, R <= 3, not accumulating, 16 <= S < packed_limit(K)
                      (4096 for K = 1, 2048 for K = 2..4, HBEC_PACKED_MAX_BIG
                      for K = 5..8); a tile is packed_u(K) x 64 elements of
                      16 B running across the objects of the launch;
  * gf_apply_vec_pipe2 / gf_apply_vec_pipe   K <= 4 / 5 <= K <= 8, R <= 3, not
                      accumulating, S >= pipe_u(K) KiB (one tile);
  * gf_apply_vec      K <= 8, R <= 3 otherwise, which with the packed kernel
                      below the pipelined ones leaves the accumulate pass of a
                      call with 17..24 inputs; tile_kib(K) KiB per tile;
  * gf_apply_vec_stream   K >= 9, R = 4, or any shape under
                      set_force_stream(True); 4 KiB per tile.

Calls of 5..12 inputs leave the family for the record kernels from
HBEC_REC_ROUTE_MIN_S (5..8) / HBEC_REC_ROUTE_MIN_S_BIG (9..12) bytes on; every
case here stays below.  All these kernels run 4 waves per block, one tile per
wave at a time, so under a grid cap of one block the launch's tile count mod 4
decides whether the last row of tiles is full.
"""
import random
import re
from collections import Counter, namedtuple
from functools import lru_cache
from pathlib import Path

_T = (Path(__file__).resolve().parents[1] / "hummingbird_amd" / "csrc" / "tuning.h").read_text()


def _tune(name):
    return int(re.search(rf"#define {name} (\d+)", _T).group(1))


PACKED_MAX_BIG = _tune("HBEC_PACKED_MAX_BIG")
PACKED_U_BIG = _tune("HBEC_PACKED_U_BIG")
PIPE_U_BIG = _tune("HBEC_PIPE_U_BIG")
PIPE_V2_MAXK = _tune("HBEC_PIPE_V2_MAXK")
TILE_KIB = (_tune("HBEC_TILE_SMALL"), _tune("HBEC_TILE_MID"), _tune("HBEC_TILE_BIG"))
REC_MIN_S = _tune("HBEC_REC_ROUTE_MIN_S")
REC_MIN_S_BIG = _tune("HBEC_REC_ROUTE_MIN_S_BIG")
WAVES = _tune("HBEC_PIPE_BLOCK") // 64     # waves per block, 4 in every kernel of the family
MAX_K, MAX_R = 16, 4                        # kernels.h kMaxK, kMaxR: inputs / rows per pass
STREAM_TILE = 4096
KERNELS = ("packed", "pipe2", "pipe", "vec", "stream")
TAIL = 368                                  # bytes past two tiles, as in the other sweeps
ROW_PAD = 48                                # bytes of an object row past its shards
SPLIT_PAD = 80                              # likewise for the output array of a two-array case
CANARY = 64                                 # bytes between regions that nothing may write
GARBLE = 0xC5


# ---- the route rule ----------------------------------------------------------------------

def pipe_u(k):
    return 4 // k if k <= 4 else (PIPE_U_BIG if k <= 8 else 1)


def tile_kib(k):
    return TILE_KIB[0] if k <= 2 else (TILE_KIB[1] if k <= 4 else TILE_KIB[2])


def packed_u(k):
    return PACKED_U_BIG if k > 4 else pipe_u(k)


def packed_tile_elems(k):
    return packed_u(k) * 64


def packed_limit(k):
    """shards shorter than this take the packed kernel (K <= 8, R <= 3)"""
    return PACKED_MAX_BIG if k > 4 else max(pipe_u(k) * 1024, 2048)


def pass_kernel(K, R, S, accumulate, force_stream=False):
    """(kernel, tile bytes) of one pass"""
    unrolled = K <= 8 and R <= 3 and not force_stream
    if unrolled and not accumulate and 16 <= S < packed_limit(K):
        return "packed", packed_tile_elems(K) * 16
    if not unrolled:
        return "stream", STREAM_TILE
    if not accumulate and S >= pipe_u(K) * 1024:
        return ("pipe2" if K <= PIPE_V2_MAXK else "pipe"), pipe_u(K) * 1024
    return "vec", tile_kib(K) * 1024


def passes(rows, cols, S, force_stream=False):
    """The launches of one apply_views call in order: (kernel, K, R, accumulate, tile bytes)"""
    out = []
    for r0 in range(0, rows, MAX_R):
        R = min(MAX_R, rows - r0)
        for c0 in range(0, cols, MAX_K):
            K = min(MAX_K, cols - c0)
            kern, tile = pass_kernel(K, R, S, c0 > 0, force_stream)
            out.append((kern, K, R, c0 > 0, tile))
    return out


def launches(rows, cols, S, force_stream=False):
    """what hbec_vec_kernel_stats has to gain over one call (launch hooks at 0: one launch per pass)"""
    c = Counter(p[0] for p in passes(rows, cols, S, force_stream))
    return {k: c.get(k, 0) for k in KERNELS}


def below_records(cols, S):
    """the call cannot leave for the record kernels (hbec.cpp rec_route), whatever its alignment"""
    if not 5 <= cols <= 12:
        return True
    return S < (REC_MIN_S_BIG if cols > 8 else REC_MIN_S)


# ---- instances ---------------------------------------------------------------------------

# kernel: the one the instance is there for; (K, R): that kernel's pass; (rows, cols): the call
Instance = namedtuple("Instance", "name kernel K R rows cols force")


def _instances():
    out = []
    for K in range(1, 9):
        for R in range(1, 4):
            out.append(Instance(f"packed-{K}x{R}", "packed", K, R, R, K, False))
    for K in range(1, 5):
        for R in range(1, 4):
            out.append(Instance(f"pipe2-{K}x{R}", "pipe2", K, R, R, K, False))
    for K in range(5, 9):
        for R in range(1, 4):
            out.append(Instance(f"pipe-{K}x{R}", "pipe", K, R, R, K, False))
    for K in range(1, 9):
        for R in range(1, 4):
            out.append(Instance(f"vec-{K}x{R}", "vec", K, R, R, 16 + K, False))
    for K in (1, 4, 8):
        out.append(Instance(f"stream-r4-{K}x4", "stream", K, 4, 4, K, False))
    for K in (9, 13, 16):
        for R in range(1, 5):
            out.append(Instance(f"stream-{K}x{R}", "stream", K, R, R, K, False))
    for cols in (25, 32):
        for R in (2, 4):
            out.append(Instance(f"stream-acc-{cols}x{R}", "stream", cols - 16, R, R, cols, False))
    for rows in (5, 7):
        out.append(Instance(f"stream-rows-4x{rows}", "stream", 4, 4, rows, 4, False))
    for K, R in ((4, 2), (8, 3)):
        out.append(Instance(f"stream-forced-{K}x{R}", "stream", K, R, R, K, True))
    return tuple(out)


INSTANCES = _instances()


def tile_bytes(inst):
    """T of the instance's kernel (packed: the bytes of one tile's elements)"""
    return {"packed": packed_tile_elems(inst.K) * 16, "pipe2": pipe_u(inst.K) * 1024, "pipe": pipe_u(inst.K) * 1024,
            "vec": tile_kib(inst.K) * 1024, "stream": STREAM_TILE}[inst.kernel]


@lru_cache(maxsize=None)
def lengths(inst):
    T = tile_bytes(inst)
    if inst.kernel == "packed":
        lim = packed_limit(inst.K)
        if inst.K <= 4:
            return tuple(range(16, lim, 16))
        # q KiB + 16 at q = 32 is the limit itself (the pipelined kernel's first length, swept
        # there): only lengths below it can be packed
        s = set(range(16, 4401, 16))
        s |= {q * 1024 + d for q in range(5, 33) for d in (-16, 0, 16)}
        s |= {(lim - 1) // 16 * 16 - 16 * i for i in range(3)}
        return tuple(sorted(x for x in s if x < lim))
    lo = {"pipe2": packed_limit(inst.K), "pipe": PACKED_MAX_BIG}.get(inst.kernel, 16)
    top = lo + (T if inst.kernel == "pipe" else 2 * T) + TAIL
    return tuple(range(lo, top + 1, 16))


# a case: S bytes per shard, n objects, grid cap (0 = none), two arrays?
Case = namedtuple("Case", "S n cap split")


@lru_cache(maxsize=None)
def cases(inst):
    """Every length twice: one block (cap 1) over 3..6 objects (pipe: 2..3), and
    an uncapped grid over 2; every third length with inputs and outputs in two
    arrays of different pitch.  The capped cases come first, so the cap is set
    twice per instance.  Packed instances add two long walks under cap 1."""
    ls = lengths(inst)
    capped = [Case(S, (2 + i % 2) if inst.kernel == "pipe" else (3 + i % 4), 1, i % 3 == 2)
              for i, S in enumerate(ls)]
    if inst.kernel == "packed":
        te = packed_tile_elems(inst.K)
        # spo = 3: the first whole object past 9 tiles (9 te + 1 is no multiple of 3): a tenth
        # tile of one object; spo = 80: 5 tiles exactly
        capped.append(Case(48, -(-(9 * te + 1) // 3), 1, False))
        capped.append(Case(1280, 5 * te // 80, 1, True))
    return tuple(capped + [Case(S, 2, 0, i % 3 == 2) for i, S in enumerate(ls)])


def n_tiles(inst, case):
    """tiles of the launch of the instance's kernel"""
    if inst.kernel == "packed":
        return -(-(case.n * (case.S // 16)) // packed_tile_elems(inst.K))
    return case.n * -(-case.S // tile_bytes(inst))


# ---- coefficients ------------------------------------------------------------------------

@lru_cache(maxsize=None)
def coeffs(inst):
    """rows x cols, seeded by the instance: a 0 and a 1 somewhere (a 1 alone in
    a matrix of two entries, neither in a single one, where they would make the
    call a fill or a copy) and no two rows equal."""
    rng = random.Random(f"vec-sweep-{inst.name}")
    while True:
        m = [[rng.randrange(2, 256) for _ in range(inst.cols)] for _ in range(inst.rows)]
        cells = [(r, c) for r in range(inst.rows) for c in range(inst.cols)]
        rng.shuffle(cells)
        if len(cells) >= 2:
            m[cells[0][0]][cells[0][1]] = 1
        if len(cells) >= 3:
            m[cells[1][0]][cells[1][1]] = 0
        if len({tuple(r) for r in m}) == inst.rows:
            return tuple(tuple(r) for r in m)


# ---- layout ------------------------------------------------------------------------------

# views are (offset, object stride) from the buffer's base; begin..end is the region
Region = namedtuple("Region", "case begin end in_views out_views")


def layout(inst):
    """One buffer for all cases of an instance: (regions, bytes).  An object row is
    its cols + rows shards back to back and ROW_PAD bytes; a two-array case has
    an array of input rows (ROW_PAD) and one of output rows (SPLIT_PAD), CANARY
    bytes apart.  CANARY bytes or more separate regions and close the buffer."""
    regs, pos = [], 0
    for i, c in enumerate(cases(inst)):
        # at least CANARY bytes on, at the next base whose 16-B residue of a 128-B line is this
        # case's: the residues step with the lengths and drift by one every 8, so every object
        # count and array form meets every residue
        pos += CANARY
        pos += (16 * ((i + i // 8) % 8) - pos) % 128
        begin = pos
        if c.split:
            pin, pout = inst.cols * c.S + ROW_PAD, inst.rows * c.S + SPLIT_PAD
            iv = [(pos + j * c.S, pin) for j in range(inst.cols)]
            pos += c.n * pin + CANARY
            ov = [(pos + r * c.S, pout) for r in range(inst.rows)]
            pos += c.n * pout
        else:
            pitch = (inst.cols + inst.rows) * c.S + ROW_PAD
            iv = [(pos + j * c.S, pitch) for j in range(inst.cols)]
            ov = [(pos + (inst.cols + r) * c.S, pitch) for r in range(inst.rows)]
            pos += c.n * pitch
        regs.append(Region(c, begin, pos, tuple(iv), tuple(ov)))
    return regs, pos + CANARY


# ---- launches cut by set_vec_chunk_tiles -------------------------------------------------

# (kernel, K, R, S, chunk tiles, objects, launches): whole objects per launch, as
# hbec.cpp objs_per_launch / packed_objs_per_launch cut them
CUTS = (
    ("packed", 4, 2, 1008, 4, 8, 2),     # 4 tiles x 64 elements / 63 per object: 4 objects per launch
    ("packed", 4, 2, 1008, 4, 9, 3),
    ("pipe", 8, 3, 32864, 22, 4, 2),     # 11 tiles per object: 2 objects per launch
    ("pipe", 8, 3, 32864, 22, 5, 3),
)


def cut_launches(kernel, K, S, chunk_tiles, n):
    if kernel == "packed":
        per = max(1, chunk_tiles * packed_tile_elems(K) // (S // 16))
    else:
        per = max(1, chunk_tiles // -(-S // (pipe_u(K) * 1024)))
    return -(-n // per)
