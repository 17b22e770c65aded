"""Cases of the tiled stripes sweep (tests/test_gpu_stripes_sweep.py) and of the
pinned hash mode of the host seams (tests/host_seams_child.py): which instance
of gf_apply_stripes<K, R, SPLIT, ACC, MIRROR> a call has to launch, over which
shard lengths, in which tile order.  Plain Python, no torch, no numpy;
tests/test_stripes_sweep_cases.py asserts what these cases cover on a machine
without a GPU.

The rules restated here are the library's (plan.cpp launch_stripe_passes,
hbec_plan_stripes / hbec_plan_objects; stripes.hip), written out a second
time; only the thresholds are read from csrc/tuning.h.

  * A call of K_all inputs and R_all outputs is cut into row passes of 3 and,
    inside each, column passes of 8; a column pass after the first accumulates
    (ACC).  Every pass of an object plan is SPLIT, and object plans stay on
    the tiled kernel only for k <= 8, so they never accumulate.  The hashing
    host call on pinned stripes runs the same passes MIRRORed.
  * The tile is stripes_u(min(k, 8)) KiB of shard column: 4096 B for k = 1,
    2048 B for k = 2, 1024 B otherwise; an entry of S bytes per shard is
    ceil(S / T) tiles, the last of `valid` = S - T (tiles - 1) bytes.
  * Aligned entries of 5 <= k <= 12 leave for the record kernels from
    HBEC_REC_ROUTE_MIN_S (k <= 8, unless base and length are whole 128-B
    lines) / HBEC_REC_ROUTE_MIN_S_BIG (k >= 9) bytes per shard on.
  * A block is 4 waves, wave w of block b starts at tile 4 b + w and steps by
    4 x grid: tile t is stored at iteration t div (4 x grid).  Under a grid cap
    of one block, row t div 4 of a plan's tile list is one iteration; row 0 is
    loaded by the prologue, the last row is stored by the epilogue, and when
    n_tiles % 4 != 0 the waves past the end of the last row hold stand-ins.
"""
import random
import re
from collections import Counter, namedtuple
from functools import lru_cache
from pathlib import Path

_T = (Path(__file__).resolve().parents[1] / "hummingbird_amd" / "csrc" / "tuning.h").read_text()


def _tune(name):
    return int(re.search(rf"#define {name} (\d+)", _T).group(1))


REC_MIN_S = _tune("HBEC_REC_ROUTE_MIN_S")
REC_MIN_S_BIG = _tune("HBEC_REC_ROUTE_MIN_S_BIG")
MAX_K, MAX_R = 8, 3            # kernels.h kStripeMaxK; rows per pass (plan.cpp launch_stripe_passes)
WAVES = 4                      # waves per block (kBlockThreads / 64)
TAIL = 368                     # bytes past two tiles, as in the other sweeps
GAP = 48                       # sentinel bytes after every entry
FILLER = 16                    # shard length of a filler entry: one tile of 16 valid bytes
VARIANTS = ("plain", "split", "accumulate", "mirror", "mirror_accumulate")


# ---- the pass rule -----------------------------------------------------------------------

def tile_bytes(k):
    kk = min(k, MAX_K)
    return 4096 if kk == 1 else (2048 if kk == 2 else 1024)


def passes(k_all, r_all, objects=False, mirror=False):
    """The launches of one call in order: (variant, K, R)"""
    if objects and (k_all > MAX_K or mirror):
        raise ValueError("object plans take <= 8 inputs per pass and are never mirrored")
    out = []
    for r0 in range(0, r_all, MAX_R):
        R = min(MAX_R, r_all - r0)
        for c0 in range(0, k_all, MAX_K):
            K = min(MAX_K, k_all - c0)
            if mirror:
                v = "mirror_accumulate" if c0 else "mirror"
            else:
                v = "accumulate" if c0 else ("split" if objects else "plain")
            out.append((v, K, R))
    return out


def launches(k_all, r_all, objects=False, mirror=False):
    """what hbec_stripes_kernel_stats has to gain over one launch_stripe_passes"""
    c = Counter(p[0] for p in passes(k_all, r_all, objects, mirror))
    return {v: c.get(v, 0) for v in VARIANTS}


def on_records(k, S, line=False):
    """an aligned entry the plan hands to the record kernels (m = 3..5: k r <= 24 for k <= 8)"""
    if not 5 <= k <= 12:
        return False
    return S >= REC_MIN_S_BIG if k > 8 else (S >= REC_MIN_S and not line)


def tiles_of(S, T):
    """`valid` of every tile of one entry"""
    n = -(-S // T)
    return [T] * (n - 1) + [S - T * (n - 1)]


# ---- plans -------------------------------------------------------------------------------

Plan = namedtuple("Plan", "k m layout spot")


def seams(k):
    T = tile_bytes(k)
    return (16, T - 16, T, T + 16, 2 * T, 2 * T + TAIL)


def _plans():
    out = [Plan(k, 3, "stripes", False) for k in range(1, 17)]
    out += [Plan(k, 3, "objects", False) for k in range(1, 9)]
    # row passes of 3 + 1 and 3 + 2; three column passes (8 + 8 + 1, 8 + 8 + 8)
    out += [Plan(4, 4, "stripes", True), Plan(4, 4, "objects", True), Plan(3, 5, "stripes", True),
            Plan(3, 5, "objects", True), Plan(17, 3, "stripes", True), Plan(24, 4, "stripes", True)]
    return tuple(out)


PLANS = _plans()


def plan_id(p):
    return f"{p.k}+{p.m}-{p.layout}" + ("-seams" if p.spot else "")


@lru_cache(maxsize=None)
def lengths(p):
    """the swept shard lengths of a plan (boundary entries and fillers apart)"""
    T = tile_bytes(p.k)
    return seams(p.k) if p.spot else tuple(range(16, 2 * T + TAIL + 1, 16))


def boundary(p):
    """two entries at the record-route threshold: 16 below (tiled) and the threshold (records)"""
    if p.spot or not 5 <= p.k <= 12:
        return ()
    thr = REC_MIN_S_BIG if p.k > 8 else REC_MIN_S
    return (thr - 16, thr)


def lost_patterns(p):
    """(name, lost shards) of the four operations; encode 'loses' every parity shard"""
    k, m = p.k, p.m
    three = sorted({0, k - 1, k})[:min(m, 3)]
    return (("encode", tuple(range(k, k + m))), ("rec-data", (0,)), ("rec-data-parity", (0, k)),
            ("rec-three", tuple(three)))


def op_passes(p, lost):
    """the launches of one operation over the plan's tile list"""
    return passes(p.k, len(lost), p.layout == "objects")


def op_launches(p, lost):
    return launches(p.k, len(lost), p.layout == "objects")


# ---- entry orders ------------------------------------------------------------------------

# name; cap-1 encode only (a rotation); entries in order, fillers included
Order = namedtuple("Order", "name rotation entries")


def rotations_needed(T):
    """rows of 4 single-tile entries that hold every valid value 16..T once"""
    return T // 16 // WAVES


def _rotation_share(p):
    """The rotations this plan runs.  The plans of one tile size share them: the
    14 + 6 full plans of T = 1024 take one each (16 needed), k = 2 and k = 1
    have two plans each and take half of their 32 / 64."""
    if p.spot:
        return ()
    T = tile_bytes(p.k)
    mates = [q for q in PLANS if not q.spot and tile_bytes(q.k) == T]
    i, n = mates.index(p), len(mates)
    return tuple(j for j in range(rotations_needed(T)) if j % n == i)


def _wave_neighbours_differ(vals, T):
    """tiles t and t + 4 (one wave's consecutive tiles under one block) differ in valid, whole tiles apart"""
    return all(a != b or a == T for a, b in zip(vals, vals[WAVES:]))


def valids(p, entries):
    """`valid` of every tile of the plan's tile list, in order"""
    T = tile_bytes(p.k)
    out = []
    for S in entries:
        if not on_records(p.k, S):
            out += tiles_of(S, T)
    return out


def _with_fillers(p, entries, residue, at):
    """insert 0..3 filler entries at index `at` so that n_tiles % 4 == residue"""
    n = len(valids(p, entries))
    fill = (residue - n) % WAVES
    return tuple(entries[:at]) + (FILLER,) * fill + tuple(entries[at:])


def residue_of(p, order_name):
    """n_tiles % 4 assigned to an order of a plan: the two full orders of the plans walk 0..3"""
    if order_name.startswith("rot"):
        return 0  # a whole last row: four valid values meet the epilogue
    i = PLANS.index(p)
    return (i + (2 if order_name == "shuffle" else 0) + i // 4) % WAVES


@lru_cache(maxsize=None)
def orders(p):
    T = tile_bytes(p.k)
    base = list(lengths(p)) + list(boundary(p))
    out = [Order("ascending", False, _with_fillers(p, base, residue_of(p, "ascending"), len(base)))]
    for seed in range(1000):
        sh = base[:]
        random.Random(f"stripes-sweep-{plan_id(p)}-{seed}").shuffle(sh)
        ent = _with_fillers(p, sh, residue_of(p, "shuffle"), len(sh))
        if _wave_neighbours_differ(valids(p, ent), T):
            break
    else:
        raise AssertionError("no shuffle with differing wave neighbours")
    out.append(Order("shuffle", False, ent))
    nrot = rotations_needed(T)
    for j in _rotation_share(p):
        head = [16 * (WAVES * j + 1 + i) for i in range(WAVES)]
        tail = [16 * (WAVES * ((j + nrot // 2) % nrot) + 1 + i) for i in range(WAVES)]
        mid = [S for S in base if S not in head and S not in tail]
        random.Random(f"stripes-sweep-rot-{plan_id(p)}-{j}").shuffle(mid)
        ent = _with_fillers(p, head + mid + tail, 0, len(head) + len(mid) // 2)
        out.append(Order(f"rot{j}", True, ent))
    return tuple(out)


def n_tiles(p, order):
    return len(valids(p, order.entries))


def n_records(p, order):
    return sum(on_records(p.k, S) for S in order.entries)


def rows_seen(p, order):
    """(first row, middle rows, last row) of valid values under a cap of one block"""
    v = valids(p, order.entries)
    last = (len(v) - 1) // WAVES * WAVES
    return v[:WAVES], v[WAVES:last], v[last:]


# ---- pinned hash cases (host seams, mode md5-pinned) ----------------------------------------

HashCase = namedtuple("HashCase", "k m lengths")
HASH_CASES = tuple(HashCase(k, m, seams(k)) for k in range(1, 17) for m in range(1, 4))


def hash_passes(c):
    return passes(c.k, c.m, mirror=True)


def hash_launches(c):
    """per record slot of an hbec_encode_host_md5 call on pinned 16-B-aligned stripes"""
    return launches(c.k, c.m, mirror=True)
