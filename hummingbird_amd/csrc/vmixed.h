// vmixed.h — Verify over a plan with a present mask per stripe
// (hbec_verify_plan_mixed): which shards a mask reads and checks, the per-call
// words of gf_verify_mixed_plan (vmixed.hip) and the routing of a plan's source
// entries to it.  The device records, the static {entry, tile} list and the
// pattern records are the mixed plan reconstruct's (mixedplan.h), with a
// record's "outputs" read as the shards that are checked.  Everything inline
// here needs no device, so it compiles alone (tests/native/verify_mixed_host.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "mixedplan.h"

namespace hbec {

// The shards one present mask (n = k + m bytes, non-zero = present) reads:
// survivors = the first k present in index order (Reconstruct's rule), checked
// = every other present shard (always parity indices: a present data shard is
// among the first k present).  false: fewer than k present.
inline bool vm_select(int k, int n, const uint8_t* present, int* survivors, int* checked, int* n_checked) {
    int ns = 0, nc = 0;
    for (int i = 0; i < n; ++i) {
        if (!present[i]) continue;
        if (ns < k)
            survivors[ns++] = i;
        else
            checked[nc++] = i;
    }
    *n_checked = nc;
    return ns == k;
}

// Per-call word of a source entry, as gf_mixed_plan's: (r << kMPatShift) |
// record offset in 16-B units, r the number of checked shards.  An entry with
// exactly k present has nothing to check and no record: kVmNothing (r = 0 with
// every offset bit set; no record starts there, mixed_plan_asan.cpp).  0: no
// tiles (zero-length, or the other route).
constexpr uint32_t kVmNothing = kMPatMask;
inline uint32_t vm_word(int r, uint32_t rec) { return r > 0 ? ((uint32_t)r << kMPatShift) | rec : kVmNothing; }
inline uint32_t vm_word_r(uint32_t w) { return w >> kMPatShift; }
inline uint32_t vm_word_rec(uint32_t w) { return w & kMPatMask; }

// Where a source entry of shard length S goes: mp_build's rule.
enum VmRoute { kVmSkip = 0, kVmKernel = 1, kVmOther = 2 };
inline VmRoute vm_route(int k, int m, uint64_t shard_len) {
    if (shard_len == 0) return kVmSkip;
    return mp_fast_shape(k, m) && pos32_shard(shard_len) ? kVmKernel : kVmOther;
}

// Append the record of one mask with r >= 1 checked shards (rows: r x k, row q
// rebuilds checked[q] from the survivors); returns its offset in 16-B units.
inline uint32_t vm_pattern(std::vector<uint32_t>& buf, int k, const int* survivors, const int* checked, int r,
                           const uint8_t* rows) {
    return mp_pattern(buf, k, survivors, checked, r, rows);
}

// Tiles [0, n_tiles) of `tiles`: every tile whose entry's word has 1..r checked
// shards (r >= 1: the largest count in the call) is compared and ORs 1 into
// flags[entry] on a mismatch; tile 0 of an entry whose word is kVmNothing ORs 2.
// rows: the records are a shards plan's (a = the entry's address row, shardplan.h).
hipError_t launch_verify_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                    const uint32_t* pat_of, const uint32_t* pats, uint32_t* flags, int cus,
                                    hipStream_t stream, bool rows = false);
// the other route: *flag |= 1 when x[0, n) != y[0, n);  *flag |= bits
hipError_t launch_vm_compare(const void* x, const void* y, uint64_t n, uint32_t* flag, int cus, hipStream_t stream);
hipError_t launch_vm_or(uint32_t* flag, uint32_t bits, hipStream_t stream);

}  // namespace hbec
