// repairwide.h — hbec_repair_plan_mixed's contract for wide stripes, 1 <= k <= 32
// with 1 <= m <= 4, in one launch (hbec_repair_plan_wide): the pattern records
// and per-call words of gf_repair_wide_plan (repairwide.hip) and the {entry,
// tile} list of a plan whose k the mixed family's list does not take.  The device
// records (MRec) and the list (MTile) are the mixed plan reconstruct's
// (mixedplan.h).  Everything inline here needs no device, so it compiles alone
// (tests/native/repair_wide_host.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "mixedplan.h"

namespace hbec {

constexpr int kRwMaxK = 32;
inline bool rw_shape(int k, int m) { return k >= 1 && k <= kRwMaxK && m >= 1 && m <= kMaxR; }

// One pattern record, as words: the k survivor shard indices, a byte each, in
// words 0..7 (survivor j in word j / 4, bits 8 (j % 4)); the shard indices of
// its A = r_o + r_c rows in word kRwRowsWord, the rebuilt shards' first, then
// the checked ones'; the v_perm tables of row q x survivor j (gf256.h
// perm_table) at word kRwHdr + 5 (j A + q): the kernel reads the A rows of one
// input together.  kRwHdr keeps the tables 16-B aligned.
constexpr uint32_t kRwSurvWords = kRwMaxK / 4;
constexpr uint32_t kRwRowsWord = kRwSurvWords;
constexpr uint32_t kRwHdr = 12;
inline uint32_t rw_record_words(int k, int a) { return (kRwHdr + 5u * (uint32_t)(k * a) + 3u) & ~3u; }

// The records of one call have one stride, rw_record_words(k, the call's largest
// A) (32+4 with four rows: 2608 B), and are named by their position: 65536 of
// the longest are 2^25.4 16-B units, which no offset field beside two counts
// holds.  Per-call word of a source entry: kRwLive | r_o << kRwOutShift | r_c <<
// kRwChkShift | record position.  r_c == 0 says that exactly k shards are present
// (flag bit 1); with r_o == 0 too the entry has no record and the position is
// not looked at.  0: no tiles in this call (zero-length).
constexpr uint32_t kRwLive = 1u << 31;
constexpr uint32_t kRwOutShift = 19;
constexpr uint32_t kRwChkShift = 16;
constexpr uint32_t kRwPatMask = 0xFFFFu;
inline uint32_t rw_word(int r_out, int r_chk, uint32_t pat) {
    return kRwLive | ((uint32_t)r_out << kRwOutShift) | ((uint32_t)r_chk << kRwChkShift) | (pat & kRwPatMask);
}
inline uint32_t rw_word_out(uint32_t w) { return (w >> kRwOutShift) & 7u; }
inline uint32_t rw_word_chk(uint32_t w) { return (w >> kRwChkShift) & 7u; }
inline uint32_t rw_word_pat(uint32_t w) { return w & kRwPatMask; }

// Fill the record at p (rw_record_words(k, >= r_out + r_chk) zeroed words) of a
// mask with r_out + r_chk >= 1 rows: out_rows is r_out x k (the decode rows),
// chk_rows r_chk x k (row q rebuilds checked[q] from the survivors).
inline void rw_pattern(uint32_t* p, int k, const int* survivors, const int* outs, int r_out, const uint8_t* out_rows,
                       const int* checked, int r_chk, const uint8_t* chk_rows) {
    const int a = r_out + r_chk;
    for (int j = 0; j < k; ++j) p[j / 4] |= (uint32_t)survivors[j] << (8 * (j % 4));
    for (int q = 0; q < a; ++q) {
        const int shard = q < r_out ? outs[q] : checked[q - r_out];
        const uint8_t* row = q < r_out ? out_rows + (size_t)q * k : chk_rows + (size_t)(q - r_out) * k;
        p[kRwRowsWord] |= (uint32_t)shard << (8 * q);
        for (int j = 0; j < k; ++j) perm_table(row[j], p + kRwHdr + 5 * (j * a + q));
    }
}

// mp_build for a plan whose (k, m) the mixed family does not take: every
// non-empty entry gets a record and its tiles (the caller has refused shards
// longer than kPos32MaxShard).  false: too many tiles (>= 2^31).
inline bool rw_build(MixedPlanRecs& o, const std::vector<MSrc>& src, uint32_t tile_bytes) {
    o.recs.assign(src.size(), MRec{0, 0, 0, 0});
    for (size_t i = 0; i < src.size(); ++i) {
        const MSrc& s = src[i];
        if (s.shard_len == 0 || !pos32_shard(s.shard_len)) continue;
        o.recs[i] = MRec{s.a, s.b, (uint32_t)s.shard_len, 0};
        const uint64_t nt = (s.shard_len + tile_bytes - 1) / tile_bytes;
        if (o.tiles.size() + nt >= (1ull << 31)) return false;
        for (uint64_t t = 0; t < nt; ++t) o.tiles.push_back(MTile{(uint32_t)i, (uint32_t)t});
    }
    return true;
}

// Tiles [0, n_tiles) of `tiles`: every tile whose entry's word has 1..a rows in
// total (a >= 1: the largest total in the call) rebuilds its r_o outputs and ORs
// 1 into flags[entry] when one of its r_c checked shards differs from what the
// survivors imply; tile 0 of an entry whose word has r_c == 0 ORs 2.  pats: the
// call's records, `stride` words apart.  rows: the records are a shards plan's.
hipError_t launch_repair_wide_plan(int k, int a, uint32_t stride, const MRec* recs, const MTile* tiles,
                                   uint32_t n_tiles, const uint32_t* words, const uint32_t* pats, uint32_t* flags,
                                   int cus, hipStream_t stream, bool rows = false);

}  // namespace hbec
