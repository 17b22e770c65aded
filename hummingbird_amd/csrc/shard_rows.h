// shard_rows.h — where shard i of a plan entry is, for the kernels of the mixed
// family (mixedplan.hip, vmixed.hip, repair_tile.h, locate.hip).  Device code only.
//
// A stripe or object plan's record says it with two bases: shard i is at
// (i < k ? a + i S : b + (i - k) S).  A shards plan (hbec_plan_shards,
// hbec_plan_files) names every shard: `a` is the device address of the entry's
// row of k + m 64-bit shard addresses and b is 0 (shardplan.h).  shard_at<ROWS>
// is the one place the tiles hold either rule.  With ROWS = false it is the text
// the tiles had, and the record kernels compile to what they were; the `_rows`
// kernels instantiate the tiles with true.
//
// The row index is wave-uniform and the address space constant, so a row load
// is a scalar load of 8 bytes.  It is issued where the address is asked for: the
// checked and rebuilt shards' ahead of the tile's first vector load, a
// survivor's one input ahead of its use, beside the scalar loads of that input's
// tables.  Reading the whole row into registers where the record is read was
// tried first: 16 addresses are 32 SGPRs, the larger twins already hold 94 to 106,
// and every such instance spilled (280 to 288 B of scratch).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hbec {

typedef __attribute__((address_space(4))) const uint64_t row_u64_c;

template <bool ROWS>
__device__ __forceinline__ uint64_t shard_at(uint64_t a, uint64_t b, uint64_t S, uint32_t k, uint32_t i) {
    if constexpr (ROWS) return reinterpret_cast<row_u64_c*>(a)[i];
    return i < k ? a + (uint64_t)i * S : b + (uint64_t)(i - k) * S;
}

}  // namespace hbec
