// shardplan.h — plans whose entries name every shard (hbec_plan_shards,
// hbec_plan_files).  klauspost's boundary is [][]byte, every shard its own
// slice, and ecSplit writes an object of more than k chunk_size bytes as k + m
// shard FILES, file j being shard j of every stripe appended
// (ecutils.go:38-70): neither is one base with the shards back to back.
//
// Such a plan reuses the records of the other two kinds.  MSrc, MRec and HRec
// keep {a, b, shard_len}; `a` is the device address of the entry's row of k + m
// 64-bit shard addresses in the plan's table and b is 0.  The kernels that hold
// the address rule have a `_rows` instance that reads the row instead
// (shard_rows.h; md5_plan_rows and md5_files_rows read it per lane).  The table
// is n (k + m) words, rows in entry order.
//
// Here: the checks of an entry's row and ecSplit's stripe arithmetic.  Everything
// is inline and needs no device, so it compiles alone
// (tests/native/shard_plan_host.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace hbec {

// What is wrong with the n shard addresses of one entry of shard_len > 0 bytes,
// or nullptr: none is null, and no two byte ranges [addr, addr + shard_len)
// overlap (ranges that touch do not).  `tmp` is scratch, reused entry after entry.
inline const char* shards_check_row(const uint64_t* row, int n, uint64_t shard_len, std::vector<uint64_t>& tmp) {
    tmp.assign(row, row + n);
    for (int i = 0; i < n; ++i)
        if (tmp[i] == 0) return "null shard pointer in an entry with shard_len > 0";
    std::sort(tmp.begin(), tmp.end());
    for (int i = 0; i + 1 < n; ++i)
        if (tmp[i + 1] - tmp[i] < shard_len) return "two shards of one entry overlap";
    return nullptr;
}

// ecSplit's loop (ecutils.go:38-58): stripes of an object of `length` bytes cut
// k chunk_size bytes at a time; nothing is written for length <= 0.  k, chunk >= 1.
inline uint64_t ec_stripe_count(int64_t length, int64_t k, int64_t chunk) {
    if (length <= 0) return 0;
    const unsigned __int128 full = (unsigned __int128)(uint64_t)k * (uint64_t)chunk;
    return (uint64_t)(((unsigned __int128)(uint64_t)length + full - 1) / full);
}

// Shard length of stripe t < ec_stripe_count: chunk_size while k chunk_size bytes
// or more remain, else the remaining bytes over k, rounded up (ecutils.go:85-92).
inline uint64_t ec_stripe_shard_length(int64_t length, int64_t k, int64_t chunk, uint64_t t) {
    const unsigned __int128 full = (unsigned __int128)(uint64_t)k * (uint64_t)chunk;
    const unsigned __int128 left = (unsigned __int128)(uint64_t)length - full * t;
    if (left >= full) return (uint64_t)chunk;
    return (uint64_t)((left + (uint64_t)k - 1) / (uint64_t)k);
}

}  // namespace hbec
