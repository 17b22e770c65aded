// heal.h — rebuild the shard hbec_locate_plan_mixed named, on the same plan and
// without a host trip (hbec_heal_plan_mixed): the rule that turns an entry's
// locate word into the shard to rewrite, the tables gf_heal_mixed_plan
// (heal.hip) chooses an entry's pattern record from, and the routing of a
// plan's source entries to it.  The device records and the static {entry, tile}
// list are the mixed plan reconstruct's (mixedplan.h); a pattern record and its
// word are the repair call's (repair.h), one per (mask p, present shard j of p)
// for the mask p \ {j}.  Everything inline here needs no device, so it compiles
// alone (tests/native/heal_host.cpp).
#pragma once
#include <stdint.h>

#include <map>
#include <vector>

#include "locate.h"
#include "repair.h"

namespace hbec {

// Flag bits of the call beside the repair call's 1 and 2 (include/hbec.h HBEC_HEAL_*).
constexpr uint32_t kHealDone = 4u;     // the named shard and the missing ones were rewritten
constexpr uint32_t kHealUnnamed = 8u;  // kLocBad, examined, but no single present shard named

// Per-call index of a source entry with no tiles in the call (zero-length, or
// the other route); every other entry carries the index of its mask's row in
// the two tables below.
constexpr uint32_t kHealNone = 0xFFFFFFFFu;
constexpr int kHealRow = 16;  // words of a mask's row of the word table: one per shard

// Is the entry one locate examined and found inconsistent?  Words that are 0,
// that say kLocSkipped or kLocNothing, or that hold only bits of the caller's
// own are none of the call's business (loc_decode: kLocClean, kLocUnchecked).
__host__ __device__ inline bool heal_examined(uint32_t where) {
    return (where & kLocBad) != 0u && (where & (kLocSkipped | kLocNothing)) == 0u;
}

// The shard a word names under a mask (bit i: shard i present): the single
// present shard not ruled out, or -1 (none left, or two or more).  For an
// examined word this is loc_decode's answer when that is >= 0.
__host__ __device__ inline int heal_pick(uint32_t present_bits, uint32_t where) {
    const uint32_t cand = present_bits & ~where & kLocRuledMask;
    return __builtin_popcount(cand) == 1 ? __builtin_ctz(cand) : -1;
}

inline uint32_t heal_mask_bits(int n, const uint8_t* mask) {
    uint32_t bits = 0;
    for (int i = 0; i < n && i < kHealRow; ++i) bits |= mask[i] ? 1u << i : 0u;
    return bits;
}

// Where a source entry of shard length S goes: the repair call's rule, since
// the tile list is shared.  kVmOther entries have no per-stripe fallback here,
// as in locate: they are left alone and counted.
inline VmRoute heal_route(int k, int m, uint64_t shard_len) { return rp_route(k, m, shard_len); }

// What a call's masks need on the device.  stage = [records | words | present]:
//   records  one rp_pattern record per distinct mask p \ {j} (equal masks share one)
//   words    kHealRow per listed mask: rp_word of p \ {j} at [row][j] for every
//            present j that leaves at least k present, 0 everywhere else
//   present  one word per listed mask: its present bits
// It depends on (k, m) and the listed masks alone, so a plan keeps it from call
// to call; the index of every source entry's mask in the list travels per call.
// Offsets below are in words; index_at is the end.
struct HealStage {
    std::vector<uint32_t> stage;
    size_t words_at = 0, present_at = 0, index_at = 0;
    uint32_t n_rows = 0;
    std::map<uint32_t, uint32_t> rec_of;  // cleared mask bits -> its word
    bool overflow = false;                // a record past rp_word's 22-bit offset
};

// rows_of(mask, survivors, outs, &n_out, out_rows, checked, &n_chk, chk_rows): the
// library's hbec_decode_rows and hbec_check_rows on one mask of n shards (at
// least k present, at least one missing); false on failure.  Called once per
// distinct cleared mask.
template <typename RowsOf>
inline bool heal_add_mask(HealStage& h, std::vector<uint32_t>& words, int k, int m, uint32_t bits,
                          RowsOf&& rows_of) {
    const int n = k + m;
    const size_t row = words.size();
    words.resize(row + kHealRow, 0u);
    if (__builtin_popcount(bits) <= k) return true;  // no shard can be left out
    std::vector<uint8_t> mask((size_t)n), orows((size_t)n * k), crows((size_t)n * k);
    std::vector<int> surv((size_t)k), outs((size_t)n), chk((size_t)n);
    for (int j = 0; j < n; ++j) {
        if (!((bits >> j) & 1u)) continue;
        const uint32_t cleared = bits & ~(1u << j);
        auto it = h.rec_of.find(cleared);
        if (it == h.rec_of.end()) {
            for (int i = 0; i < n; ++i) mask[i] = (uint8_t)((cleared >> i) & 1u);
            int n_out = 0, n_chk = 0;
            if (!rows_of(mask.data(), surv.data(), outs.data(), &n_out, orows.data(), chk.data(), &n_chk,
                         crows.data()))
                return false;
            if (n_out < 1 || n_out + n_chk != m) return false;
            const uint32_t rec = rp_pattern(h.stage, k, surv.data(), outs.data(), n_out, orows.data(), chk.data(),
                                            n_chk, crows.data());
            if (rec >= kRpNothing) {
                h.overflow = true;
                return false;
            }
            it = h.rec_of.emplace(cleared, rp_word(n_out, n_chk, rec)).first;
        }
        words[row + j] = it->second;
    }
    return true;
}

// Records and tables of the listed masks (bits[0..n_rows)), in that order.
// false: rows_of failed, or (h.overflow) a record would start past rp_word's
// 22-bit offset.
template <typename RowsOf>
inline bool heal_build(HealStage& h, int k, int m, const std::vector<uint32_t>& bits, RowsOf&& rows_of) {
    std::vector<uint32_t> words;
    for (uint32_t b : bits)
        if (!heal_add_mask(h, words, k, m, b, rows_of)) return false;
    h.n_rows = (uint32_t)bits.size();
    h.words_at = h.stage.size();
    h.stage.insert(h.stage.end(), words.begin(), words.end());
    h.present_at = h.stage.size();
    h.stage.insert(h.stage.end(), bits.begin(), bits.end());
    h.index_at = h.stage.size();
    return true;
}

// Tiles [0, n_tiles) of `tiles`, instance r = m.  For every tile whose entry has
// an index (not kHealNone) and an examined word: with a named shard j whose
// word heal_word[index][j] is not 0, the tile of that record runs (outputs
// written, flags[entry] |= 1 on a disagreeing checked shard) and tile 0 ORs
// kHealDone, and 2 when nothing is checked; otherwise nothing of the entry is
// loaded and tile 0 ORs kHealUnnamed.
// rows: the records are a shards plan's (a = the entry's address row, shardplan.h).
hipError_t launch_heal_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                  const uint32_t* index_of, const uint32_t* heal_word,
                                  const uint32_t* present_bits, const uint32_t* pats, const uint32_t* where,
                                  uint32_t* flags, int cus, hipStream_t stream, bool rows = false);

}  // namespace hbec
