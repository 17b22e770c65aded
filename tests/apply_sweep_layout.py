"""Layouts of the encode / reconstruct sweep (tests/test_gpu_apply_sweep.py):
for (k, m, layout) the plan entries of every shard length 1..SMAX at every
alignment class, the buffer sizes, the sentinel-filled initial images and the
expected images, whose shard bytes all come from the oracle (coracle
build_matrix / apply).  numpy only; tests/test_apply_sweep_layout.py checks
the coverage conditions and the checker on a machine without a GPU.

stripes: one buffer, one entry per length, shard i of an entry at base + i S,
  base mod 16 = (S >> 4) & 15, at least 5 sentinel bytes between entries.
objects: data and parity regions in two buffers, four entries per length; with
  q = S >> 4 and e = 0..3 the data base is (q + 4 e) & 15 mod 16 and the parity
  base ((q >> 4) + 4 e + (q & 15) (2 e + 1)) & 15.

The codeword of an entry is a window of S columns of one pool codeword
((k+m) x POOL bytes, parity rows = oracle apply of the oracle matrix over
seeded random data rows): GF(2^8) coding is column by column, so every window
of a codeword is a codeword.
"""
from functools import lru_cache
from itertools import combinations

import numpy as np

from oracle import coracle as CO

# 2 T + 368 for the largest apply tile span, T = 2016 B: two 63-column windows
# with carry (odd_impl.h; the bit-plane span (64 * 2 - 1) * 16 = 2032 of
# HBEC_ODD_BP_U = 2 is a Verify / record-list span of the same order: 2 * 2032 + 64 < 4400)
TILE = 2016
SMAX = 2 * TILE + 368
BANDS = ((161, 1100), (1101, 2200), (2201, SMAX))
FILL = 0xA5    # bytes that belong to no shard
GARBLE = 0x5A  # shards an operation has to write
POOL = 1 << 20
GAP = 5


@lru_cache(maxsize=4)
def pool(k, m):
    """(k+m) x POOL bytes, every column a codeword: read-only."""
    data = np.random.default_rng(9000 + 100 * k + m).integers(0, 256, (k, POOL), dtype=np.uint8)
    par = CO.apply(CO.build_matrix(k, m)[k:], [data[j] for j in range(k)])
    cw = np.concatenate([data, np.stack(par)])
    cw.setflags(write=False)
    return cw


def stripes_residue(S):
    return (S >> 4) & 15


def objects_residues(S, e):
    q = S >> 4
    return (q + 4 * e) & 15, ((q >> 4) + 4 * e + (q & 15) * (2 * e + 1)) & 15


def _place(pos, residue):
    """The first offset >= pos + GAP with the wanted residue mod 16."""
    pos += GAP
    return pos + (residue - pos) % 16


class Layout:
    """S[e]: shard length of entry e; col[e]: its first pool column;
    a[e], b[e]: offset of its data shards (buffer 0) and of its parity shards
    (buffer 0 for stripes: a + k S; buffer 1 for objects); sizes: buffer bytes."""

    def __init__(self, k, m, layout, smax=SMAX, smin=1):
        assert layout in ("stripes", "objects")
        self.k, self.m, self.layout = k, m, layout
        per = 1 if layout == "stripes" else 4
        S, a, b = [], [], []
        p0 = p1 = 0
        for s in range(smin, smax + 1):
            for e in range(per):
                S.append(s)
                if layout == "stripes":
                    p0 = _place(p0, stripes_residue(s))
                    a.append(p0)
                    b.append(p0 + k * s)
                    p0 += (k + m) * s
                else:
                    rd, rp = objects_residues(s, e)
                    p0 = _place(p0, rd)
                    p1 = _place(p1, rp)
                    a.append(p0)
                    b.append(p1)
                    p0 += k * s
                    p1 += m * s
        self.S = np.array(S, np.int64)
        self.a = np.array(a, np.int64)
        self.b = np.array(b, np.int64)
        self.n = self.S.size
        self.sizes = [p0 + 11] if layout == "stripes" else [p0 + 11, p1 + 11]
        self.col = (np.arange(self.n, dtype=np.int64) * 40503 + 7 * self.S) % (POOL - smax)
        # written regions per buffer, in address order: (start, bytes, entry, first shard)
        if layout == "stripes":
            self.regions = [(self.a, (k + m) * self.S, np.arange(self.n), np.zeros(self.n, np.int64))]
        else:
            self.regions = [(self.a, k * self.S, np.arange(self.n), np.zeros(self.n, np.int64)),
                            (self.b, m * self.S, np.arange(self.n), np.full(self.n, k, np.int64))]

    def shard(self, e, i):
        """(buffer, offset) of shard i of entry e"""
        S = int(self.S[e])
        if i < self.k:
            return 0, int(self.a[e]) + i * S
        return (0 if self.layout == "stripes" else 1), int(self.b[e]) + (i - self.k) * S

    def entries(self, addrs):
        """The plan's entry list for buffers at device addresses `addrs`."""
        if self.layout == "stripes":
            return [(addrs[0] + int(a), int(s)) for a, s in zip(self.a, self.S)]
        return [(addrs[0] + int(a), addrs[1] + int(b), int(s)) for a, b, s in zip(self.a, self.b, self.S)]

    def expected(self):
        """The images after any operation: sentinel bytes and oracle codewords."""
        cw = pool(self.k, self.m)
        k, m = self.k, self.m
        imgs = [np.full(n, FILL, np.uint8) for n in self.sizes]
        par = imgs[-1]
        for e in range(self.n):
            S, c, a, b = int(self.S[e]), int(self.col[e]), int(self.a[e]), int(self.b[e])
            imgs[0][a:a + k * S].reshape(k, S)[:] = cw[:k, c:c + S]
            par[b:b + m * S].reshape(m, S)[:] = cw[k:, c:c + S]
        return imgs

    def initial(self, want, lost):
        """Copies of the expected images with the lost shards garbled.  lost:
        shard indices (every entry), or a bool array [entries, k+m]."""
        imgs = [w.copy() for w in want]
        lost = np.asarray(lost)
        for e in range(self.n):
            S = int(self.S[e])
            for i in (lost if lost.ndim == 1 else np.nonzero(lost[e])[0]):
                buf, off = self.shard(e, int(i))
                imgs[buf][off:off + S] = GARBLE
        return imgs

    def locate(self, buf, off):
        """(entry, shard, position) of byte `off` of buffer `buf`; a sentinel
        byte is (the entry whose region precedes it or -1, -1, bytes past that
        region's end or the offset itself)."""
        start, size, ent, first = self.regions[buf]
        i = int(np.searchsorted(start, off, side="right")) - 1
        if i < 0:
            return -1, -1, int(off)
        rel = int(off - start[i])
        if rel < size[i]:
            S = int(self.S[ent[i]])
            return int(ent[i]), int(first[i]) + rel // S, rel % S
        return int(ent[i]), -1, rel - int(size[i])

    def mismatches(self, got, want, limit=12):
        """[(buffer, entry, shard, position, got, want)] of the first `limit`
        differing bytes per buffer, whole buffers compared; [] when equal."""
        out = []
        for buf, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and g.dtype == np.uint8
            if np.array_equal(g, w):
                continue
            for off in np.nonzero(g != w)[0][:limit]:
                out.append((buf,) + self.locate(buf, int(off)) + (int(g[off]), int(w[off])))
        return out


def loss_patterns(k, m):
    """Every set of 1..m lost shards of k+m, by size then lexicographic."""
    return [c for r in range(1, m + 1) for c in combinations(range(k + m), r)]


def single_patterns(k, m):
    """The three erasure patterns of the single-pattern reconstructs: one data
    shard; min(m, 4) shards, data and parity mixed; all parity."""
    n = min(m, 4)
    mixed = [1] + ([k - 1] if n >= 3 and k - 1 > 1 else [])
    mixed += list(range(k + m - 1, k - 1, -1))[:n - len(mixed)]
    assert len(mixed) == n and (n == 1 or (min(mixed) < k <= max(mixed)))
    return [[k // 2], sorted(mixed), list(range(k, k + m))]


def mixed_losses(k, m, n):
    """bool [n, k+m]: entry e loses pattern (e * step) % P of the P loss
    patterns, step coprime to P (every pattern used when n >= P)."""
    pats = loss_patterns(k, m)
    P = len(pats)
    step = next(s for s in range(max(1, P // 3) | 1, 2 * P + 3, 2) if np.gcd(s, P) == 1)
    lost = np.zeros((n, k + m), bool)
    which = (np.arange(n, dtype=np.int64) * step) % P
    for e in range(n):
        lost[e, list(pats[which[e]])] = True
    return lost, which, P
