// correct.h — correct the corrupt bytes of a plan column by column
// (hbec_correct_plan_mixed): the output word, the per-byte rule as a reference
// function, the pattern record and the routing of a plan's source entries to
// gf_correct_mixed_plan (correct.hip).  The device records, the static
// {entry, tile} list and the per-call words are the degraded Verify's
// (vmixed.h, mixedplan.h), as for locate (locate.h).  Everything inline here
// needs no device, so it compiles alone (tests/native/correct_host.cpp).
//
// The rule.  locate.h derives it: with r >= 2 checked shards a non-zero
// syndrome s[0..r) is a multiple of at most one column of [rows | I], and that
// column's shard is the position's candidate.  Locate keeps only who is NOT the
// candidate.  Here the candidate and the multiple are kept: e = s[q] for checked
// shard q (the one non-zero component), e = s[0] / rows[0][t] for survivor t
// (all components non-zero and proportional to column t), and shard[x] ^= e
// makes the position consistent.  A syndrome that is a multiple of no column
// (two bad bytes in the column with r >= 3; anything non-zero with r = 1) has
// no candidate and the position is left as it is.
//
// The caveat is locate's: at r = 2 the code has distance 3, and two bad bytes
// in one column can produce the syndrome of a third shard.  That column is then
// "corrected" into a consistent but wrong codeword; only a check outside the
// code (the object's ETag, etag.h) catches it.  With r >= 3 any three columns
// are independent, so a column with two bad bytes never finds a candidate.
#pragma once
#include <stdint.h>

#include <vector>

#include "gf256.h"
#include "locate.h"
#include "vmixed.h"

namespace hbec {

// The word of one source entry (include/hbec.h HBEC_COR_*).
constexpr uint32_t kCorBad = 1u << 31;      // some compared byte was inconsistent
constexpr uint32_t kCorSkipped = 1u << 30;  // the other route: not examined
constexpr uint32_t kCorNothing = 1u << 29;  // exactly k present: nothing to check
constexpr uint32_t kCorLeft = 1u << 28;     // some inconsistent position was left as it is
constexpr uint32_t kCorShardMask = 0xFFFFu; // bit j: shard j had a byte corrected

// What one byte position with syndrome s[0..r) asks for (rows: r x k, row q
// rebuilds checked[q] from the survivors): the shard to XOR *err into, or -1
// when the position is consistent (*err = 0) or has no candidate (*err = 0 too;
// the caller tells the two apart by the syndrome).
inline int cor_classify(int k, int r, const uint8_t* rows, const uint8_t* s, const int* survivors,
                        const int* checked, uint8_t* err) {
    const Field& F = field();
    *err = 0;
    int nz = 0, at = -1;
    for (int q = 0; q < r; ++q)
        if (s[q]) {
            ++nz;
            at = q;
        }
    if (nz == 0 || r < 2) return -1;
    if (nz == 1) {
        *err = s[at];
        return checked[at];
    }
    if (nz != r) return -1;
    int found = -1;
    for (int t = 0; t < k; ++t) {
        bool prop = true;
        for (int q = 1; q < r && prop; ++q) prop = F.mul(s[q], rows[t]) == F.mul(s[0], rows[(size_t)q * k + t]);
        if (!prop) continue;
        if (found >= 0) return -1;  // cannot happen: the columns are pairwise independent
        found = t;
    }
    if (found < 0) return -1;
    *err = F.div(s[0], rows[found]);
    return survivors[found];
}

// Where a source entry goes: locate's rule, since the tile list is shared.
// kVmOther entries have no per-stripe fallback here: kCorSkipped.
inline VmRoute cor_route(int k, int m, uint64_t shard_len) { return loc_route(k, m, shard_len); }

// Words of a record of r checked shards before its inverse tables: mp_pattern_words(k, r),
// spelt out so that the kernel calls the same function (cor_pattern appends there).
__host__ __device__ inline uint32_t cor_inverse_at(int k, int r) {
    return (kMPatHdr + 5u * (uint32_t)(k * r) + 3u) & ~3u;
}
inline uint32_t cor_pattern_words(int k, int r) { return cor_inverse_at(k, r) + ((5u * (uint32_t)k + 3u) & ~3u); }

// The record of one mask with r >= 1 checked shards: the degraded Verify's,
// word for word, then perm_table(1 / rows[0][t]) for t = 0..k-1 at word
// cor_inverse_at(k, r) + 5 t, padded to 16 B.  Returns its offset in 16-B units.
inline uint32_t cor_pattern(std::vector<uint32_t>& buf, int k, const int* survivors, const int* checked, int r,
                            const uint8_t* rows) {
    const uint32_t rec = vm_pattern(buf, k, survivors, checked, r, rows);
    const size_t at = (size_t)rec * 4u + cor_inverse_at(k, r);
    buf.resize((size_t)rec * 4u + cor_pattern_words(k, r), 0u);  // Verify's record ends at or before `at`
    for (int t = 0; t < k; ++t) perm_table(field().div(1, rows[t]), buf.data() + at + 5 * t);
    return rec;
}
// 1 / rows[0][t] read back from a record of r checked shards (perm_table's word
// 0 holds c * {0, 1, 2, 3}: byte 1 is c itself)
inline uint8_t cor_pattern_inverse(const uint32_t* p, int k, int r, int t) {
    return (uint8_t)(p[cor_inverse_at(k, r) + 5 * t] >> 8);
}

// Tiles [0, n_tiles) of `tiles`: every tile whose entry passes the filter
// (flags == nullptr, or flags[entry] & 1) and whose word has 1..r checked shards
// (r >= 1: the largest count in the call) is compared; where it is inconsistent
// every position with a candidate has that shard's byte corrected in place, and
// fixed[entry] |= kCorBad | corrected shards | kCorLeft if a position was left.
// Tile 0 of an entry whose word is kVmNothing ORs kCorNothing, filtered or not.
// pats: cor_pattern records.
// rows: the records are a shards plan's (a = the entry's address row, shardplan.h).
hipError_t launch_correct_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                     const uint32_t* pat_of, const uint32_t* pats, const uint32_t* flags,
                                     uint32_t* fixed, int cus, hipStream_t stream, bool rows = false);

}  // namespace hbec
