// glue.h — the object bytes of a plan's entries from their shards
// (hbec_glue_plan_mixed, hbec_glue_plan_files): ecGlue's loop (ecutils.go:134-186)
// over a batch.  Per stripe ecGlue runs ReconstructData and writes data shards
// 0..k-1 back to back, cut at the object's remaining length; here entry i's
// D_i = data shard 0 || ... || data shard k-1 goes to dsts[i], its first
// dst_lens[i] bytes.
//
// Here: the host arithmetic of the call.  How much of each data shard is
// written, which tiles of the {entry, tile} list have anything to do, how an
// object of a files plan is cut into its entries' destinations, and whether a
// destination overlaps a shard.  Everything is inline and needs neither HIP nor
// a device, so it compiles alone (tests/native/glue_host.cpp).  The kernels are
// gf_glue_plan and gf_glue_plan_rows (glue.hip, glue_tile.h).
#pragma once
#include <stdint.h>

#include "shardplan.h"

namespace hbec {

// Per-call word of a source entry: (r << kMPatShift) | record offset as in
// mixedplan.h, r = 0 included (a healthy entry is gathered through its record's
// survivor list); this word says the entry is not the kernel's (zero length,
// nothing asked for, or the per-entry route).  Its r reads as 15: no instance's.
constexpr uint32_t kGlueSkip = 0xFFFFFFFFu;

// Bytes of data shard j (S bytes long) inside the first `len` bytes of D:
// clamp(len - j S, 0, S).
inline uint64_t glue_valid(uint64_t len, uint64_t j, uint64_t S) {
    const unsigned __int128 off = (unsigned __int128)j * S;
    if ((unsigned __int128)len <= off) return 0;
    const unsigned __int128 left = (unsigned __int128)len - off;
    return left < S ? (uint64_t)left : S;
}

// Shard positions a call reads and writes: [0, min(S, len)) of every shard it
// touches at all (data shard 0 is the longest written).
inline uint64_t glue_span(uint64_t S, uint64_t len) { return len < S ? len : S; }

// Tile ti (shard positions from ti * tile_bytes) has something to do.
inline bool glue_tile_needed(uint64_t S, uint64_t len, uint64_t ti, uint64_t tile_bytes) {
    return (unsigned __int128)ti * tile_bytes < glue_span(S, len);
}

// Entry t of an object of L bytes cut k * chunk bytes at a time (t below
// ec_stripe_count): where its bytes start in the object and how many they are,
// min(k S_t, L - t k chunk).  The cuts tile [0, L) in order.
inline void glue_files_cut(uint64_t L, uint64_t k, uint64_t chunk, uint64_t t, uint64_t* off, uint64_t* len) {
    const unsigned __int128 full = (unsigned __int128)k * chunk;
    const unsigned __int128 at = full * t;
    const unsigned __int128 left = (unsigned __int128)L - at;
    *off = (uint64_t)at;
    *len = (uint64_t)(left < full ? left : full);
}

// [dst, dst + len) and [shard, shard + S) share a byte (ranges that touch do not;
// an empty range shares none).
inline bool glue_overlaps(uint64_t dst, uint64_t len, uint64_t shard, uint64_t S) {
    if (len == 0 || S == 0) return false;
    return (unsigned __int128)dst < (unsigned __int128)shard + S && (unsigned __int128)shard < (unsigned __int128)dst + len;
}

struct MRec;
struct MTile;
// Tiles [0, n_tiles) of `tiles`: glues every tile whose entry's word is not
// kGlueSkip (r <= rmax, the largest count of missing data shards in the call,
// 0..kMaxR).  dsts: per source entry {address lo, hi, length lo, hi}.  rows: the
// records are a shards plan's.  stream: a hipStream_t; returns a hipError_t
// (both as plain types, so this header stays free of HIP).
int launch_glue_plan(int k, int rmax, const MRec* recs, const MTile* tiles, uint32_t n_tiles, const uint32_t* words,
                     const uint32_t* dsts, const uint32_t* pats, int cus, void* stream, bool rows);

}  // namespace hbec
