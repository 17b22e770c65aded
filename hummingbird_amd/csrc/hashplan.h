// hashplan.h — ShardHash over a plan (hbec_hash_plan_mixed): the MD5 of the
// selected shards of every examined entry, compared with the stored ShardHashes
// on the device, and the result in hbec_locate_plan_mixed's word format.  The
// reference audits a shard by re-hashing it against the hash IndexDB holds
// (objectserver/auditor.go:100-156, indexdb.go:746-753): a shard whose hash
// differs is the corrupt one, whatever the number of surplus shards.
//
// Here: the device record of a source entry, the per-call chain list and its
// builder, and the rule that turns an entry's bad-shard bits into its where
// word.  The kernels are md5_plan and hash_where (hashplan.hip).  Everything
// inline here needs no device, so it compiles alone (tests/native/hash_plan_host.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "locate.h"

namespace hbec {

// Device record of one source entry (every entry has one): shard j is at
// (j < k ? a + j len : b + (j - k) len), MSrc's rule, with the length in 64 bits.
struct HRec {
    uint64_t a, b, len;
    uint32_t route;  // VmRoute of loc_route: what the entry's where word may say
    uint32_t pad_;
};

// One chain of a call: shard `shard` of source entry `entry`.
struct HChain {
    uint32_t entry, shard;
};

// The where word of an examined, non-empty entry from its selected-shard bits
// and its bad-shard bits: what the call ORs into d_where.  On the kernel route
// of loc_route a clean entry adds nothing, one bad shard j rules out every
// other selected shard (loc_decode under the selection names j), two or more
// rule out all of them (kLocMultiple; d_bad still says which).  The other route
// says kLocSkipped, as locate does.
__host__ __device__ inline uint32_t hash_where_word(uint32_t sel, uint32_t bad, uint32_t route) {
    if (route == (uint32_t)kVmSkip) return 0u;
    if (route != (uint32_t)kVmKernel) return kLocSkipped;
    if (bad == 0u) return 0u;
    const bool one = (bad & (bad - 1u)) == 0u;
    return kLocBad | ((one ? sel & ~bad : sel) & kLocRuledMask);
}

// bit j (j < 32) for every selected shard of a selection row of n bytes
inline uint32_t hash_select_bits(int n, const uint8_t* row) {
    uint32_t bits = 0;
    for (int j = 0; j < n && j < 32; ++j) bits |= row[j] ? 1u << j : 0u;
    return bits;
}

// The non-empty source entries, longest shard first (equal lengths in source
// order): built once per plan.  A call lists its chains in this order, so the
// 64 lanes of a wave run similar trip counts.
inline void hash_order(const std::vector<MSrc>& src, std::vector<uint32_t>& order) {
    order.clear();
    for (size_t i = 0; i < src.size(); ++i)
        if (src[i].shard_len) order.push_back((uint32_t)i);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t x, uint32_t y) { return src[x].shard_len > src[y].shard_len; });
}

// The chain list of one call: every selected shard of every non-empty entry,
// each once, entries in `order`.  select: n_select rows of n bytes; select_of:
// one row index per source entry (already checked against n_select).
inline void hash_chains(const std::vector<uint32_t>& order, int n, const uint8_t* select, uint32_t n_select,
                        const uint32_t* select_of, std::vector<HChain>& chains) {
    // the selected shards of every row, once: [at[p], at[p + 1]) of `shards`
    std::vector<uint32_t> at((size_t)n_select + 1, 0u), shards;
    for (uint32_t p = 0; p < n_select; ++p) {
        for (int j = 0; j < n; ++j)
            if (select[(size_t)p * n + j]) shards.push_back((uint32_t)j);
        at[p + 1] = (uint32_t)shards.size();
    }
    chains.clear();
    for (uint32_t e : order) {
        const uint32_t p = select_of[e];
        for (uint32_t q = at[p]; q < at[p + 1]; ++q) chains.push_back(HChain{e, shards[q]});
    }
}

// Chains [0, n_chains) of `chains`, one lane each: the MD5 of the chain's shard
// when its entry passes the filter (filter == nullptr, or filter[entry] &
// filter_bits); digest to digests + (entry n + shard) 16 when digests is given;
// bad[entry] |= 1 << shard when expected is given and differs there.
// rows: the records are a shards plan's (a = the entry's address row, shardplan.h).
hipError_t launch_md5_plan(const HRec* recs, const HChain* chains, uint64_t n_chains, int k, int n,
                           const uint32_t* filter, uint32_t filter_bits, const uint8_t* expected, uint8_t* digests,
                           uint32_t* bad, hipStream_t stream, bool rows = false);
// One thread per source entry, after md5_plan on the same stream: where[i] |=
// hash_where_word(sel[i], bad[i], route) for the examined non-empty entries on
// the kernel route, kLocSkipped for every non-empty entry on the other.
hipError_t launch_hash_where(const HRec* recs, uint32_t n_src, const uint32_t* sel, const uint32_t* filter,
                             uint32_t filter_bits, const uint32_t* bad, uint32_t* where, hipStream_t stream);

}  // namespace hbec
