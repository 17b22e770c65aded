"""Cases of the MD5 chain sweep (tests/test_gpu_md5_sweep.py): what is hashed,
where it lies and which kernel has to take it.  Plain Python, no torch, no
numpy; tests/test_md5_sweep_cases.py asserts what these inputs cover on a
machine without a GPU.

Every placement is an offset into a pool of random bytes whose device address
is a multiple of 64, so an offset's residue is the address's.  The kernels only
read, so views of one call may overlap in the pool; what matters is that every
chain starts somewhere else.

The rules restated here are the host code's (shardhash.cpp), written out a
second time: expect_aligned is md5_step's choice of kernel, segments is
md5_segment's cut of a shard into encode + hash segments (n = 8 for k <= 4:
floor(S / 8) rounded up to 4 KiB, at least 16 KiB; one segment above), and
host_chunks is hbec_md5_host's packing of buffers into staging slots.
"""
from functools import lru_cache

SENT = 0xA5                 # digest slots nothing may write
LENGTHS = range(0, 901)     # block counts 0..14, every rest 0..63 at each
VIEWS_PER_LAUNCH = 32


def expect_aligned(bases, strides, total):
    """md5_step: the 16-B-load kernel runs when the first whole block of every
    view (base + 64 - carried bytes; base itself with nothing carried) and
    every object stride are multiples of 16."""
    carry = total & 63
    first = 64 - carry if carry else 0
    return all((b + first) % 16 == 0 and s % 16 == 0 for b, s in zip(bases, strides))


def launches(n_views):
    return -(-n_views // VIEWS_PER_LAUNCH)


def blocks_rest(length, carry=0):
    """(whole blocks, bytes left) of carry + length pending bytes"""
    return divmod(carry + length, 64)


# ---- a. one-shot, unaligned kernel -------------------------------------------------------
A_NOBJ = 65
A_STRIDE = 977                                   # = 1 mod 16: object o of view v at residue v + o
A_BASES = [64 + 1009 * v for v in range(16)]     # 1009 = 1 mod 16: view v at residue v
A_POOL = A_BASES[-1] + (A_NOBJ - 1) * A_STRIDE + LENGTHS[-1] + 16

# ---- b. one-shot, aligned kernel ---------------------------------------------------------
B_NOBJS = (1, 63, 64, 65, 129)
B_STRIDE = 976                                   # 61 * 16: a multiple of 16, 16 mod 64
B_BASES = [0, 64 * 50 + 16, 64 * 101 + 48]       # residues 0, 16, 48 mod 64
B_POOL = B_BASES[-1] + (max(B_NOBJS) - 1) * B_STRIDE + LENGTHS[-1] + 16


def b_nobj(length):
    return B_NOBJS[length % len(B_NOBJS)]


# ---- c. view splitting -------------------------------------------------------------------
C_NVIEWS = (32, 33, 64, 65)
C_NOBJS = (1, 65)
C_LENGTHS = (0, 55, 56, 64, 200)
C_UPDATES = (37, 100, 0, 64)
C_PITCH = 208                                    # bytes between the views of an object, 13 * 16


def c_layout(n_views):
    """(view offsets, object stride): contiguous rows of n_views slots of C_PITCH bytes"""
    return [v * C_PITCH for v in range(n_views)], n_views * C_PITCH


def c_stream_steps(n_views):
    """Per step of the streaming case, update after update and then final():
    (length or None for final, bytes before it, launches, aligned kernel?)."""
    offs, stride = c_layout(n_views)
    steps, total, started = [], 0, False
    for u in C_UPDATES:
        n = 0 if (u == 0 and started) else launches(n_views)
        steps.append((u, total, n, expect_aligned([o + total for o in offs], [stride] * n_views, total)))
        started = True
        total += u
    steps.append((None, total, launches(n_views), expect_aligned([0] * n_views, [0] * n_views, total)))
    return steps


# ---- d. streaming carry ------------------------------------------------------------------
D_NOBJ = 2
D_NVIEWS = 2
D_TMAX = 320                                     # carry + len up to five blocks
D_STRIDE = 336                                   # 21 * 16, at least the longest update
D_SLOTS = 509
D_POOL = 16 * D_SLOTS + 16 + (D_NOBJ - 1) * D_STRIDE + D_TMAX + 16
D_MAX_UPDATES = 8
D_CLASSES = ("A", "U", "M")


def d_offset(cls, carry, idx, view):
    """Pool offset of view `view` of the idx-th update of a run, `carry` bytes
    pending.  A: a multiple of 16, so the kernel follows the carry.  U: carry
    mod 16, so base + 64 - carry is a multiple of 16 and the 16-B-load kernel
    runs from an address that is none (unless carry is 0 mod 16).  M: 1..15
    past that, so no step is ever aligned (the only way to the bytewise kernel
    with nothing carried, which neither A nor U reaches)."""
    res = {"A": 0, "U": carry % 16, "M": (carry + 1 + idx % 15) % 16}[cls]
    return 16 * ((idx * 37 + 11 * view) % D_SLOTS) + res


def chain_pairs(chain):
    """(carry, carry + len) before each update of a chain"""
    total = 0
    for u in chain:
        yield total & 63, (total & 63) + u
        total += u


def all_pairs():
    return {(c, t) for c in range(64) for t in range(c, D_TMAX + 1)}


@lru_cache(maxsize=None)
def pair_chains():
    """Chains of at most D_MAX_UPDATES updates in which every (carry 0..63,
    carry + len carry..320) occurs: a chain starts with `c` bytes (the pair
    (0, c)) and every further update is a pair at the carry the one before
    left, chosen to land where most pairs are still open."""
    left = [[[] for _ in range(64)] for _ in range(64)]   # [carry][carry after] -> open t
    count = [0] * 64
    for c in range(64):
        for t in range(D_TMAX, c - 1, -1):
            left[c][t & 63].append(t)
            count[c] += 1

    def take(c):
        nc = max((x for x in range(64) if left[c][x]), key=lambda x: (count[x], -x))
        count[c] -= 1
        return left[c][nc].pop()

    chains = []
    while any(count):
        c = max(range(64), key=lambda x: (count[x], -x))
        ups = []
        if c:
            ups.append(c)
            if c in left[0][c]:
                left[0][c].remove(c)
                count[0] -= 1
        carry = c
        while len(ups) < D_MAX_UPDATES and count[carry]:
            t = take(carry)
            ups.append(t - carry)
            carry = t & 63
        chains.append(tuple(ups))
    return tuple(chains)


def all_triples():
    return {(c, l1, s - c - l1) for s in (62, 63, 64, 65) for c in range(1, s - 1) for l1 in range(1, s - c)}


@lru_cache(maxsize=None)
def triple_chains():
    """c bytes, then two updates that together end at 62..65 pending bytes:
    the tail is carried twice without a block between (rewritten in place)."""
    return tuple(sorted(all_triples()))


# zero-length first update, zero-length update mid-chain, final() with no
# update at all, short and whole-block single updates; every run keeps one
# context across its chains, so each chain but the first reuses it after final()
EDGE_CHAINS = ((), (0,), (0, 5, 70), (0, 0, 64), (5, 0, 70), (64, 0, 1), (63, 0, 0, 1), (1,), (64,), (),
               (37, 100, 0, 64), (55,), (56,), (9, 47), (9, 46))


def d_steps(cls, chains):
    """The launches of a run of chains through one context, in order:
    (chain index, update index or None for final, length, bytes before,
    view offsets, launches 0/1, aligned kernel?)."""
    out, idx = [], 0
    for ci, chain in enumerate(chains):
        total, started = 0, False
        for ui, u in enumerate(chain):
            offs = [d_offset(cls, total & 63, idx, v) for v in range(D_NVIEWS)]
            idx += 1
            n = 0 if (u == 0 and started) else 1
            out.append((ci, ui, u, total, offs, n, expect_aligned(offs, [D_STRIDE] * D_NVIEWS, total)))
            started = True
            total += u
        out.append((ci, None, 0, total, [0] * D_NVIEWS, 1, expect_aligned([0] * D_NVIEWS, [0] * D_NVIEWS, total)))
    return out


# ---- e. md5_list lane mixing -------------------------------------------------------------
E_LONG = 5000


def list_cases():
    """(name, lengths) of every md5_list call"""
    cases = [("every_length", list(LENGTHS)),
             ("long_first", [E_LONG] + list(range(63))),
             ("long_last", list(range(63)) + [E_LONG])]
    for n in (1, 63, 64, 65, 129):
        cases.append((f"n{n}", [(i * 131 + 7 * n) % 700 for i in range(n)]))
    cases.append(("all_empty", [0] * 65))
    return cases


def list_offsets(lens, aligned):
    """(offsets, pool bytes): buffer i at a multiple of 16, or at residue 1 + i mod 15"""
    offs, pos = [], 0
    for i, n in enumerate(lens):
        pos = (pos + 15) // 16 * 16 + (0 if aligned else 1 + i % 15)
        offs.append(pos)
        pos += n + 3
    return offs, pos + 16


# ---- f. bit count above 32 bits ----------------------------------------------------------
F_LEN = 64 << 20
F_OFFSETS = (0, 16, 5, 32, 48, 1, 64, 33)       # first byte of each 64 MiB update in the buffer
F_TOTAL = len(F_OFFSETS) * F_LEN + 1

# ---- g. segment pipeline -----------------------------------------------------------------
G_NOBJ = 3
G_PIPELINED = ((4, 2), (3, 2), (2, 1), (1, 1))
G_SIZES = (16383, 16384, 16385, 16384 + 55, 16384 + 56, 16384 + 64, 20479, 32768, 32769, 49153, 131072, 131073,
           135169, 139263)
G_SINGLE = ((8, 3), (16385, 40001))


def segments(S, k):
    """md5_segment and hbec_encode_md5_batch's loop: the segment lengths of a shard"""
    if k > 4:
        return [S]
    seg = max((S // 8 + 4095) & ~4095, 16384)
    return [min(seg, S - off) for off in range(0, S, seg)]


# ---- h. hbec_md5_host --------------------------------------------------------------------
H_SLOT = 64 << 20
H_RECS = 65536


def host_cases():
    return [("every_length", list(LENGTHS)),
            ("records", [i % 41 for i in range(65541)]),
            ("slot_bytes", [(1 << 20) - i % 16 for i in range(70)] + [(i * 53) % 300 for i in range(40)])]


def host_chunks(lens):
    """hbec_md5_host: buffers longest first, a chunk closes when the slot's
    bytes (16-B-rounded buffers) or its records are used up"""
    chunks, used, recs = 0, 0, 0
    for n in sorted(lens, reverse=True):
        sz = (n + 15) & ~15
        if chunks == 0 or used + sz > H_SLOT or recs >= H_RECS:
            chunks, used, recs = chunks + 1, 0, 0
        used += sz
        recs += 1
    return chunks
