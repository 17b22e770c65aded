// splitplan.h — the k + m shards of a plan's entries from their object bytes
// (hbec_split_plan, hbec_split_plan_files): ecSplit's loop (ecutils.go:26-72)
// over a batch.  Per stripe ecSplit reads k * S bytes of the object, zero-pads
// the last stripe to a multiple of k (:51-54), cuts it into k data shards and
// encodes m parity shards; here entry i's piece O_i = [srcs[i], srcs[i] +
// src_lens[i]) becomes data shard j = O_i[j S, (j + 1) S) with zeros past the
// piece's end, and parity shard r = row k + r of the coding matrix over them.
// It is the inverse of glue.h's call.
//
// Here: the host arithmetic of the call.  Which lengths a piece may have for a
// shard length, how many bytes of each data shard come from the piece, which
// tiles of the {entry, tile} list have work, and (from glue.h) how an object of
// a files plan is cut into its entries' pieces and whether a piece overlaps a
// shard.  Everything is inline and needs neither HIP nor a device, so it
// compiles alone (tests/native/split_host.cpp).  The kernels are gf_split_plan
// and gf_split_plan_rows (splitplan.hip, split_tile.h).
#pragma once
#include <stdint.h>

#include "glue.h"

namespace hbec {

// Per-call word of a source entry: (m << kMPatShift) | record offset as in
// mixedplan.h; this word says the entry is not the kernel's (zero length, no
// piece given, or the per-entry route).  Its r reads as 15: no instance's.
constexpr uint32_t kSplitSkip = 0xFFFFFFFFu;

// ecShardLength (ecutils.go:85-92) of a piece of len bytes: ceil(len / k).
inline uint64_t split_shard_length(uint64_t len, uint64_t k) { return len / k + (len % k ? 1u : 0u); }

// A piece of len > 0 bytes fills shards of S bytes: k S - k < len <= k S.
inline bool split_len_ok(uint64_t len, uint64_t k, uint64_t S) { return len > 0 && split_shard_length(len, k) == S; }

// ecSplit's pad: the zero bytes that end the k data shards of a piece that
// passed split_len_ok, 0..k-1 of them.
inline uint64_t split_pad(uint64_t len, uint64_t k, uint64_t S) {
    return (uint64_t)((unsigned __int128)k * S - len);
}

// Bytes of data shard j that come from the piece, clamp(len - j S, 0, S); the
// rest of the shard, split_pad at most in all, is zero.  With len < k a whole
// trailing shard is pad.
inline uint64_t split_valid(uint64_t len, uint64_t j, uint64_t S) { return glue_valid(len, j, S); }

// Every shard is written whole, so every tile of [0, S) has work.
inline uint64_t split_tiles(uint64_t S, uint64_t tile_bytes) { return S / tile_bytes + (S % tile_bytes ? 1u : 0u); }
inline bool split_tile_needed(uint64_t S, uint64_t ti, uint64_t tile_bytes) {
    return (unsigned __int128)ti * tile_bytes < S;
}

struct MRec;
struct MTile;
// Tiles [0, n_tiles) of `tiles`: splits every tile whose entry's word is not
// kSplitSkip.  m: the parity count, 0..kMaxR (0: a scatter).  srcs: per source
// entry {address lo, hi, length lo, hi}.  rows: the records are a shards
// plan's.  stream: a hipStream_t; returns a hipError_t (both as plain types,
// so this header stays free of HIP).
int launch_split_plan(int k, int m, const MRec* recs, const MTile* tiles, uint32_t n_tiles, const uint32_t* words,
                      const uint32_t* srcs, const uint32_t* pats, int cus, void* stream, bool rows);

}  // namespace hbec
