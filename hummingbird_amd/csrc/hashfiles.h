// hashfiles.h — ShardHash of multi-stripe shard FILES over a plan
// (hbec_hash_plan_files).  The reference's ShardHash is the MD5 of the whole
// shard file, and ecSplit appends shard j of every stripe to writer j
// (ecutils.go:38-70): the file is shard j of each of the object's stripes, back
// to back.  An object is a run of the plan's source entries, and chain (g, j)
// is shard j of each of them in order, hashed as one stream with one pad.
//
// Here: the check of the caller's object table, the per-call chain list, the
// object index of every entry and the selection bits of every object.  The
// kernels are md5_files and hash_files_where (hashfiles.hip); the entry records
// and the where word are hashplan.h's.  Everything inline here needs no device,
// so it compiles alone (tests/native/hash_files_host.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "hashplan.h"

namespace hbec {

// One chain of a call: shard file `shard` of object `object`.
struct FChain {
    uint32_t object, shard;
};

// What is wrong with an object table of n_objects + 1 words over n_src entries
// (n_src > 0), or nullptr: it starts at 0, never decreases and ends at n_src.
inline const char* files_check_objects(const uint32_t* object_start, uint32_t n_objects, uint64_t n_src) {
    if (!object_start) return "null object_start";
    if (n_objects == 0) return "entries but no objects";
    if (object_start[0] != 0) return "object_start[0] is not 0";
    for (uint32_t g = 0; g < n_objects; ++g)
        if (object_start[g + 1] < object_start[g]) return "object_start decreases";
    if (object_start[n_objects] != n_src) return "object_start does not end at the plan's entry count";
    return nullptr;
}

// The object of every source entry (object_start already checked).
inline void files_entry_objects(const uint32_t* object_start, uint32_t n_objects, std::vector<uint32_t>& object_of) {
    object_of.assign(object_start[n_objects], 0u);
    for (uint32_t g = 0; g < n_objects; ++g)
        for (uint32_t i = object_start[g]; i < object_start[g + 1]; ++i) object_of[i] = g;
}

// The chain list of one call: every selected shard file of every object with a
// byte in it, each once, objects by total file length, longest first (equal
// totals in object order): the 64 lanes of a wave run similar trip counts,
// hash_order's reason.  The total is 64-bit.  select / select_of as hash_chains,
// one row index per OBJECT (already checked against n_select).  Returns the
// segments the chains walk: non-empty entries of an object, once per chain.
inline uint64_t files_chains(const std::vector<MSrc>& src, const uint32_t* object_start, uint32_t n_objects, int n,
                             const uint8_t* select, uint32_t n_select, const uint32_t* select_of,
                             std::vector<FChain>& chains) {
    std::vector<uint64_t> total(n_objects, 0u);
    std::vector<uint32_t> pieces(n_objects, 0u), order;
    for (uint32_t g = 0; g < n_objects; ++g) {
        for (uint32_t i = object_start[g]; i < object_start[g + 1]; ++i) {
            total[g] += src[i].shard_len;
            pieces[g] += src[i].shard_len != 0;
        }
        if (total[g]) order.push_back(g);
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return total[x] > total[y]; });
    // the selected shards of every row, once: [at[p], at[p + 1]) of `shards`
    std::vector<uint32_t> at((size_t)n_select + 1, 0u), shards;
    for (uint32_t p = 0; p < n_select; ++p) {
        for (int j = 0; j < n; ++j)
            if (select[(size_t)p * n + j]) shards.push_back((uint32_t)j);
        at[p + 1] = (uint32_t)shards.size();
    }
    chains.clear();
    uint64_t segments = 0;
    for (uint32_t g : order) {
        const uint32_t p = select_of[g];
        for (uint32_t q = at[p]; q < at[p + 1]; ++q) chains.push_back(FChain{g, shards[q]});
        segments += (uint64_t)(at[p + 1] - at[p]) * pieces[g];
    }
    return segments;
}

// Chains [0, n_chains) of `chains`, one lane each: the MD5 of shard `shard` of
// the entries [object_start[g], object_start[g + 1]) back to back, when any of
// them passes the filter (filter == nullptr, or filter[entry] & filter_bits);
// digest to digests + (g n + shard) 16 when digests is given; bad[g] |=
// 1 << shard when expected is given and differs there.
// rows: the records are a shards plan's (a = the entry's address row, shardplan.h).
hipError_t launch_md5_files(const HRec* recs, const uint32_t* object_start, const FChain* chains, uint64_t n_chains,
                            int k, int n, const uint32_t* filter, uint32_t filter_bits, const uint8_t* expected,
                            uint8_t* digests, uint32_t* bad, hipStream_t stream, bool rows = false);
// One thread per source entry, after md5_files on the same stream: with g =
// object_of[i], where[i] |= hash_where_word(sel[g], bad[g], route) for the
// non-empty entries on the kernel route that pass the filter themselves,
// kLocSkipped for every non-empty entry on the other.
hipError_t launch_hash_files_where(const HRec* recs, uint32_t n_src, const uint32_t* object_of, const uint32_t* sel,
                                   const uint32_t* filter, uint32_t filter_bits, const uint32_t* bad, uint32_t* where,
                                   hipStream_t stream);

}  // namespace hbec
