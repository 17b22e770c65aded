// splitwide.h — hbec_split_plan's contract for wide stripes, 1 <= k <= 32 with
// 1 <= m <= 4, in one launch (hbec_split_plan_wide, hbec_split_plan_files_wide):
// ecSplit's loop (ecutils.go:26-72) over a batch of 16+4, 17+3, 20+4 stripes and
// their like, which hbec_split_plan cuts and codes one entry at a time above
// k = 12.
//
// Here: the one pattern record of a call, the per-entry word and the cut of an
// entry's k virtual inputs into the three phases of gf_split_wide_plan's tile
// (splitwide.hip).  The record and the word are repairwide.h's (rw_pattern with
// survivors 0..k-1, the parity shards as outputs and no checked rows; rw_word),
// the {entry, tile} list is that call's too (rw_build), the sources splitplan.h's.
// Everything inline here needs no device, so it compiles alone
// (tests/native/split_wide_host.cpp); the kernel calls sw_cut itself.
#pragma once
#include <stdint.h>

#include "repairwide.h"
#include "splitplan.h"

#ifdef __HIP__
#define HBEC_SW_HD __host__ __device__
#else
#define HBEC_SW_HD
#endif

namespace hbec {

// The record of a call, of rw_record_words(k, m) zeroed words: data shards
// 0..k-1 in, parity shards k..k+m-1 out, `rows` the m x k encode rows (rows
// k..k+m-1 of the coding matrix).  The tables of row q x input j lie at word
// kRwHdr + 5 (j m + q).
inline void sw_pattern(uint32_t* p, int k, int m, const uint8_t* rows) {
    int data[kRwMaxK], par[kMaxR];
    for (int j = 0; j < k; ++j) data[j] = j;
    for (int r = 0; r < m; ++r) par[r] = k + r;
    rw_pattern(p, k, data, par, m, rows, nullptr, 0, nullptr);
}

// Per-call word of a source entry with shards of S bytes given a piece of `len`
// bytes: 0 when the entry is not the kernel's (zero length, or no piece given),
// else rw_word(m, 0, 0): m rows to code, none checked, the call's one record.
inline uint32_t sw_word(int m, uint64_t S, uint64_t len) { return S == 0 || len == 0 ? 0u : rw_word(m, 0, 0); }

// The k virtual inputs of a piece that passed split_len_ok, in three runs.
// V_j = clamp(len - j S, 0, S) never rises in j and at most one input has
// 0 < V_j < S, so:
//   inputs [0, whole)          V_j = S: loaded and stored as they are,
//   input whole, if partial    V_j = partial in (0, S): loaded clamped, padded,
//   inputs [pad_from, k)       V_j = 0: ecSplit's pad alone, zero stores.
// pad_from = whole + (partial > 0).  No division: whole >= k - ceil(k / S), so the
// walk down from k is one step wherever S >= k.
struct SwCut {
    uint32_t whole, partial, pad_from;
};
HBEC_SW_HD inline SwCut sw_cut(uint64_t len, uint32_t S, uint32_t k) {
    uint32_t jf = k;
    uint64_t off = (uint64_t)k * S;  // k <= 32, S < 2^31
    while (off > len) {
        off -= S;
        --jf;
    }
    const uint32_t v = jf < k ? (uint32_t)(len - off) : 0u;  // < S: (jf + 1) S > len
    return SwCut{jf, v, jf + (v > 0u ? 1u : 0u)};
}

// Tiles [0, n_tiles) of `tiles`: splits every tile whose entry's word is not 0.
// m: the parity count, 1..kMaxR.  pats: the call's record; srcs: per source entry
// {address lo, hi, length lo, hi}.  rows: the records are a shards plan's.
// stream: a hipStream_t; returns a hipError_t (plain types, as splitplan.h's).
int launch_split_wide_plan(int k, int m, const MRec* recs, const MTile* tiles, uint32_t n_tiles, const uint32_t* words,
                           const uint32_t* srcs, const uint32_t* pats, int cus, void* stream, bool rows);

}  // namespace hbec
