// locate.h — which shard of an inconsistent stripe is the corrupt one
// (hbec_locate_plan_mixed): the output word, the per-byte rule as a reference
// function, the decode of a word, the pattern record and the routing of a
// plan's source entries to gf_locate_mixed_plan (locate.hip).  The device
// records, the static {entry, tile} list and the per-call words are the
// degraded Verify's (vmixed.h, mixedplan.h).  Everything inline here needs no
// device, so it compiles alone (tests/native/locate_host.cpp).
//
// The rule.  A mask with k survivors and r checked shards gives every byte
// position a syndrome s[0..r): s[q] = stored[checked q] ^ sum_t rows[q][t] *
// survivor t, zero everywhere on a clean stripe.  One corrupt shard with error
// byte e leaves a multiple of its column of [rows | I]: e * unit_q for checked
// shard q, e * (rows[0][t], ..., rows[r-1][t]) for survivor t.  Every rows[q][t]
// is non-zero and with r >= 2 the k + r columns are pairwise independent (any
// k shards of the code determine the rest), so a non-zero syndrome is a multiple
// of at most one column: that shard is the position's candidate, and every other
// present shard is ruled out as the single cause.  With r = 1 every column is a
// non-zero scalar: nothing can be ruled out.
#pragma once
#include <stdint.h>

#include <vector>

#include "gf256.h"
#include "vmixed.h"

namespace hbec {

// The word of one source entry (include/hbec.h HBEC_LOC_*).
constexpr uint32_t kLocBad = 1u << 31;      // some compared byte is inconsistent
constexpr uint32_t kLocSkipped = 1u << 30;  // the other route: not examined
constexpr uint32_t kLocNothing = 1u << 29;  // exactly k present: nothing to check
constexpr uint32_t kLocRuledMask = 0xFFFFu; // bit j: present shard j alone does not explain some position

constexpr int kLocClean = -1, kLocAmbiguous = -2, kLocMultiple = -3, kLocUnchecked = -4;

// bit i for every shard the mask reads or checks
inline uint32_t loc_present_bits(int k, const int* survivors, int r, const int* checked) {
    uint32_t bits = 0;
    for (int t = 0; t < k; ++t) bits |= 1u << survivors[t];
    for (int q = 0; q < r; ++q) bits |= 1u << checked[q];
    return bits;
}

// What one byte position with syndrome s[0..r) ORs into its entry's word
// (rows: r x k, row q rebuilds checked[q] from the survivors): 0 when the
// position is consistent, else kLocBad and, with r >= 2, every present shard
// but the position's candidate.
inline uint32_t loc_classify(int k, int r, const uint8_t* rows, const uint8_t* s, uint32_t present_bits,
                             const int* survivors, const int* checked) {
    const Field& F = field();
    int nz = 0, at = -1;
    for (int q = 0; q < r; ++q)
        if (s[q]) {
            ++nz;
            at = q;
        }
    if (nz == 0) return 0u;
    if (r < 2) return kLocBad;
    uint32_t cand = 0u;
    if (nz == 1) {
        cand = 1u << checked[at];
    } else if (nz == r) {
        for (int t = 0; t < k; ++t) {
            bool prop = true;
            for (int q = 1; q < r && prop; ++q)
                prop = F.mul(s[q], rows[t]) == F.mul(s[0], rows[(size_t)q * k + t]);
            if (prop) cand |= 1u << survivors[t];
        }
    }
    return kLocBad | (present_bits & ~cand & kLocRuledMask);
}

// The shard a word names (hbec_locate_decode): the single present shard not
// ruled out, or kLocClean / kLocAmbiguous / kLocMultiple / kLocUnchecked.
inline int loc_decode(int k, int m, const uint8_t* present, uint32_t where) {
    if (where == 0u) return kLocClean;
    if (where & (kLocSkipped | kLocNothing)) return kLocUnchecked;
    if (!(where & kLocBad)) return kLocClean;  // bits of the caller's own
    int found = -1, n_left = 0;
    for (int i = 0; i < k + m && i < 16; ++i)
        if (present[i] && !((where >> i) & 1u)) {
            found = i;
            ++n_left;
        }
    return n_left == 1 ? found : (n_left == 0 ? kLocMultiple : kLocAmbiguous);
}

// Where a source entry goes: the degraded Verify's rule, since the tile list is
// shared.  kVmOther entries have no per-stripe fallback here: kLocSkipped.
inline VmRoute loc_route(int k, int m, uint64_t shard_len) { return vm_route(k, m, shard_len); }

// The record of one mask with r >= 1 checked shards is the degraded Verify's,
// word for word.  The raw coefficient the proportionality test needs is in it
// already: perm_table's word 0 holds c * {0, 1, 2, 3}, so byte 1 is c itself.
inline uint32_t loc_pattern(std::vector<uint32_t>& buf, int k, const int* survivors, const int* checked, int r,
                            const uint8_t* rows) {
    return vm_pattern(buf, k, survivors, checked, r, rows);
}
// rows[q][t] read back from a record of r checked shards
inline uint8_t loc_pattern_coef(const uint32_t* p, int r, int t, int q) {
    return (uint8_t)(p[kMPatHdr + 5 * (t * r + q)] >> 8);
}

// Tiles [0, n_tiles) of `tiles`: every tile whose entry passes the filter
// (flags == nullptr, or flags[entry] & 1) and whose word has 1..r checked shards
// (r >= 1: the largest count in the call) is compared, and classified where it
// is inconsistent: where[entry] |= kLocBad | ruled-out shards.  Tile 0 of an
// entry whose word is kVmNothing ORs kLocNothing, filtered or not.
// rows: the records are a shards plan's (a = the entry's address row, shardplan.h).
hipError_t launch_locate_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                    const uint32_t* pat_of, const uint32_t* pats, const uint32_t* flags,
                                    uint32_t* where, int cus, hipStream_t stream, bool rows = false);

}  // namespace hbec
