// gluerange.h — any byte range of a plan's entries from their shards
// (hbec_glue_plan_range, hbec_glue_plan_files_range): ecObject.CopyRange's decode
// (ecobj.go:207-267) over ecGlue's layout (ecutils.go:134-186) for a batch.
// Entry i's D_i = data shard 0 || ... || data shard k-1 (glue.h); the call
// writes D_i[s, e) to dsts[i], e = s + lens[i].
//
// Here: the arithmetic of the call, the host's and the kernel's.  The window of
// each data shard, the shard positions anyone wants, which tiles of the
// {entry, tile} list are live and which of those must be decoded, which bytes of
// a 16-B destination block a lane owns, and how an object's range is cut into
// its entries'.  Everything is inline and needs neither HIP nor the library's
// headers, so it compiles alone (tests/native/gluerange_host.cpp); under hipcc
// the functions are __host__ __device__ and gluerange_tile.h / gluerange.hip run
// this text, they do not restate it.
//
// Unless said otherwise a function expects S > 0 and s <= e <= k S with k S
// below 2^64 (shards lie in memory); hbec_glue_plan_range checks the range
// first (gr_range_ok).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HBEC_GR_FN __host__ __device__ inline
#else
#define HBEC_GR_FN inline
#endif

namespace hbec {

// Shard positions [lo, hi); empty when lo >= hi.
struct GrWin {
    uint64_t lo, hi;
};

HBEC_GR_FN bool gr_empty(GrWin w) { return w.lo >= w.hi; }

// [lo, hi) and [p0, p1) share a position.
HBEC_GR_FN bool gr_meets(GrWin w, uint64_t p0, uint64_t p1) { return w.lo < w.hi && w.lo < p1 && p0 < w.hi; }

// The window of data shard j: the positions of it inside D[s, e),
// [clamp(s - j S, 0, S), clamp(e - j S, 0, S)).
HBEC_GR_FN GrWin gr_window(uint64_t S, uint64_t s, uint64_t e, uint64_t j) {
    const uint64_t off = j * S;
    GrWin w;
    w.lo = s <= off ? 0u : (s - off < S ? s - off : S);
    w.hi = e <= off ? 0u : (e - off < S ? e - off : S);
    return w;
}

// Where position 0 of data shard j would land: dst - s + j S, modulo 2^64 (it
// may lie below dst).  Position p of the shard lands at gr_base + p.
HBEC_GR_FN uint64_t gr_base(uint64_t dst, uint64_t S, uint64_t s, uint64_t j) { return dst - s + j * S; }

// P, the shard positions with a wanted byte in some data shard, as at most two
// intervals, a before b: one when the range lies in one shard; [0, e - j1 S) and
// [s - j0 S, S) when it crosses one junction and its two parts do not meet;
// [0, S) otherwise.
struct GrSpan {
    GrWin a, b;
};

HBEC_GR_FN GrSpan gr_positions(uint64_t S, uint64_t s, uint64_t e) {
    GrSpan p;
    p.a.lo = p.a.hi = p.b.lo = p.b.hi = 0u;
    if (S == 0u || s >= e) return p;
    const uint64_t j0 = s / S, j1 = (e - 1u) / S;
    const uint64_t ps = s - j0 * S, pe = e - j1 * S;  // ps in [0, S), pe in (0, S]
    if (j0 == j1) {
        p.a.lo = ps, p.a.hi = pe;
    } else if (j1 == j0 + 1u && pe < ps) {
        p.a.hi = pe;
        p.b.lo = ps, p.b.hi = S;
    } else {
        p.a.hi = S;
    }
    return p;
}

// The tile of shard positions [p0, p1) is live: it holds a position of P.  A
// dead tile loads no shard byte.
HBEC_GR_FN bool gr_tile_live(GrSpan p, uint64_t p0, uint64_t p1) { return gr_meets(p.a, p0, p1) || gr_meets(p.b, p0, p1); }

// Present data shard j is read by a gather tile [p0, p1): its window meets it.
HBEC_GR_FN bool gr_shard_in_tile(uint64_t S, uint64_t s, uint64_t e, uint64_t j, uint64_t p0, uint64_t p1) {
    return gr_meets(gr_window(S, s, e, j), p0, p1);
}

// The tile [p0, p1) must be decoded: one of the entry's r missing data shards
// (their indices a byte each in `lost`, lowest first, as the pattern record
// packs them) has a wanted position in it.  Every other live tile is a gather.
HBEC_GR_FN bool gr_tile_coded(uint64_t S, uint64_t s, uint64_t e, uint64_t p0, uint64_t p1, uint32_t lost, int r) {
    for (int q = 0; q < r; ++q)
        if (gr_shard_in_tile(S, s, e, (lost >> (8 * q)) & 0xFFu, p0, p1)) return true;
    return false;
}

// The bytes [*b0, *b1) of the 16-B block at shard positions [q, q + 16) that
// lie inside the window; false when none does.  All sixteen: the block is
// stored whole.  Fewer: they go bytewise, for the others may be another wave's
// (the next shard's head, the previous one's tail, or outside the destination).
HBEC_GR_FN bool gr_block_bytes(GrWin w, uint64_t q, uint32_t* b0, uint32_t* b1) {
    if (!(w.lo < w.hi && q < w.hi && w.lo < q + 16u)) return false;
    *b0 = w.lo > q ? (uint32_t)(w.lo - q) : 0u;
    *b1 = w.hi - q < 16u ? (uint32_t)(w.hi - q) : 16u;
    return true;
}

// The head of a 64-lane window whose first column is `col`: with the output's
// blocks starting e (0..15) bytes into a column, positions [col, col + e) belong
// to the last block of the window before.  That window stores for this shard
// only if it holds a wanted position, which it does exactly when lo < col; so
// where lo >= col the window's first lane writes those of them that are wanted,
// bytes [*b0, *b1) of its column, bytewise.
HBEC_GR_FN bool gr_head_bytes(GrWin w, uint64_t col, uint32_t e, uint32_t* b0, uint32_t* b1) {
    if (!(w.lo < w.hi && w.lo >= col && w.lo - col < e)) return false;
    *b0 = (uint32_t)(w.lo - col);
    *b1 = w.hi - col < e ? (uint32_t)(w.hi - col) : e;
    return true;
}

// s + len <= k S, without overflow (any values).
inline bool gr_range_ok(uint64_t s, uint64_t len, uint64_t k, uint64_t S) {
    return (unsigned __int128)s + len <= (unsigned __int128)k * S;
}

// The part of an object's range [start, end) that falls into the entry holding
// object bytes [off, off + len) (glue.h glue_files_cut): where it starts in the
// entry, how long it is (0: the entry is outside the range), and how far into
// the range's destination it goes.
inline void gr_files_cut(uint64_t off, uint64_t len, uint64_t start, uint64_t end, uint64_t* entry_start,
                         uint64_t* entry_len, uint64_t* dst_off) {
    const unsigned __int128 top = (unsigned __int128)off + len;
    const uint64_t lo = start > off ? start : off;
    const uint64_t hi = (unsigned __int128)end < top ? end : (uint64_t)top;
    *entry_start = *entry_len = *dst_off = 0u;
    if (lo >= hi) return;
    *entry_start = lo - off;
    *entry_len = hi - lo;
    *dst_off = lo - start;
}

struct MRec;
struct MTile;
// Tiles [0, n_tiles) of `tiles`: glues the range of every tile whose entry's
// word is not kGlueSkip (glue.h; r <= rmax, the largest count of missing data
// shards in the call, 0..kMaxR).  ranges: per source entry {address, start,
// length}, 64 bits each, low word first.  rows: the records are a shards
// plan's.  stream: a hipStream_t; returns a hipError_t (both as plain types, so
// this header stays free of HIP).
int launch_glue_range(int k, int rmax, const MRec* recs, const MTile* tiles, uint32_t n_tiles, const uint32_t* words,
                      const uint32_t* ranges, const uint32_t* pats, int cus, void* stream, bool rows);

}  // namespace hbec
