// gluewide.h — hbec_glue_plan_mixed's contract for wide stripes, 1 <= k <= 32
// with 1 <= m <= 4, in one launch (hbec_glue_plan_wide, hbec_glue_plan_files_wide):
// ecGlue's loop (ecutils.go:134-186) over a batch of 16+4, 17+3, 20+4 stripes and
// their like, which hbec_glue_plan_mixed glues one entry at a time above k = 12.
//
// Here: the pattern records and the per-entry words of gf_glue_wide_plan
// (gluewide.hip).  Both are repairwide.h's: 32 survivor bytes, the rows word
// naming the missing data shards, the tables of row q x survivor j at word
// kRwHdr + 5 (j R + q) (rw_pattern with no checked rows), one stride per call,
// the record named by its position.  The {entry, tile} list is that call's too
// (rw_build), the destinations glue.h's.  Everything inline here needs no device,
// so it compiles alone (tests/native/glue_wide_host.cpp).
#pragma once
#include <stdint.h>

#include "glue.h"
#include "repairwide.h"

namespace hbec {

// Words between two records of a call whose largest count of rebuilt data shards
// is rmax (0: headers alone).
inline uint32_t gw_stride(int k, int rmax) { return rw_record_words(k, rmax); }

// The gather record, of kRwHdr words (zeroed): survivors 0..k-1, no rows, no
// tables.  Every entry with nothing to rebuild names it, whatever its mask.
inline void gw_gather_pattern(uint32_t* p, int k) {
    for (int j = 0; j < k; ++j) p[j / 4] |= (uint32_t)j << (8 * (j % 4));
}

// The record of a mask with r >= 1 missing data shards `outs` (ascending), whose
// r x k decode rows over `survivors` are `rows`.
inline void gw_pattern(uint32_t* p, int k, const int* survivors, const int* outs, int r, const uint8_t* rows) {
    rw_pattern(p, k, survivors, outs, r, rows, nullptr, 0, nullptr);
}

// No missing data shard of the entry has a byte inside the first `len` bytes of
// D (glue_valid == 0 for each): nothing is decoded, and the data shards with a
// byte wanted are all present.  A ranged GET that ends before the lost shard then
// reads the ceil(len / S) shards it wants and not all k survivors.
inline bool gw_gathers(uint64_t S, uint64_t len, const int* outs, int r) {
    for (int q = 0; q < r; ++q)
        if (glue_valid(len, (uint64_t)outs[q], S)) return false;
    return true;
}

// Per-call word of a source entry with shards of S bytes, of which `len` bytes
// of D are asked for: 0 when the entry is not the kernel's (zero length, nothing
// asked for); rw_word(0, 0, gather) when nothing has to be decoded; else
// rw_word(r, 0, rec), rec its mask's record.
inline uint32_t gw_word(uint64_t S, uint64_t len, const int* outs, int r, uint32_t rec, uint32_t gather) {
    if (S == 0 || len == 0) return 0u;
    if (gw_gathers(S, len, outs, r)) return rw_word(0, 0, gather);
    return rw_word(r, 0, rec);
}

// Tiles [0, n_tiles) of `tiles`: glues every tile whose entry's word is not 0 and
// has something to do (glue_tile_needed).  rmax: the largest r among the words,
// 0..kMaxR.  pats: the call's records, `stride` words apart; dsts: per source
// entry {address lo, hi, length lo, hi}.  rows: the records are a shards plan's.
// stream: a hipStream_t; returns a hipError_t (plain types, as glue.h's).
int launch_glue_wide_plan(int k, int rmax, uint32_t stride, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                          const uint32_t* words, const uint32_t* dsts, const uint32_t* pats, int cus, void* stream,
                          bool rows);

}  // namespace hbec
