// mixedplan.hip — reconstruct over a plan with an erasure pattern per stripe
// (hbec_reconstruct_plan_mixed): a repair sweep over whatever the failed disk
// held, objects of any sizes (S = ceil(len / k) is a multiple of 16 for 1
// size in 16, ecutils.go:14-24) that lost different shards (shard i of a
// partition's objects lives on ring.GetNodes(partition)[i], ecobj.go:348-357).
//
// gf_mixed_plan<R> walks the plan's static {entry, tile} list grid-stride.
// For each tile a wave reads, through wave-uniform indices on read-only
// __restrict__ arguments (scalar loads):
//   the list entry        -> the source entry and the tile's shard position,
//   pat_of[entry]         -> this call's pattern record and its output count
//                            (0: nothing to rebuild, the tile is skipped),
//   recs[entry]           -> the two bases and S,
//   pats + record offset  -> the K survivor and R output shard indices (a byte
//                            each, in 4 words) and, per input, its R tables.
// The tile itself is gf_apply_unaligned's (unaligned_tile.h): any base, any S,
// 16-B-aligned accesses only, loads clamped inside their shard, bytewise head
// and tail, never a byte stored outside [shard, shard + S).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "kernels.h"
#include "mixedplan.h"
#include "planwalk.h"
#include "shard_rows.h"
#include "unaligned_tile.h"

namespace hbec {

// One tile of a stripe whose pattern has R outputs.  Every capture is a value
// in SGPRs: a reference capture would put the record in private memory and
// select between addresses.  ROWS: the entry names every shard (shard_rows.h).
template <int R, bool ROWS = false>
__device__ __forceinline__ void mixed_plan_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0,
                                                const uint32_t* __restrict__ p, uint32_t lane) {
    const uint64_t s_lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);  // survivors 0..7
    const uint32_t s_hi = p[2], so = p[3];
    const uint32_t k = (uint32_t)K;
    unaligned_tile<R>(
        K, S, p0, false, lane,
        [=](int j) {
            const uint32_t i = (j < 8 ? (uint32_t)(s_lo >> (8 * j)) : s_hi >> (8 * (j - 8))) & 0xFFu;
            return shard_at<ROWS>(a, b, S, k, i);
        },
        [=](int r) {
            const uint32_t i = (so >> (8 * r)) & 0xFFu;
            return shard_at<ROWS>(a, b, S, k, i);
        },
        [=](int r, int j) { return p + kMPatHdr + 5 * (j * R + r); });
}

// RMAX: the largest output count among the call's patterns.  One launch codes
// every tile, whatever its stripe's count (a wave-uniform branch to the tile
// of that count): with one launch per count, each skipping the other counts'
// tiles, a wave's share of coded tiles was binomial and the launch waited for
// the unluckiest wave (4096 stripes 4+2, random patterns: 0.75 ms against
// 0.67 ms for the same patterns sorted into runs).
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_mixed_plan(const MRec* __restrict__ recs,
                                                               const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                               const uint32_t* __restrict__ pat_of,
                                                               const uint32_t* __restrict__ pats, int K) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = pat_of[e.rec];
        const uint32_t r = w >> kMPatShift;  // wave-uniform
        if (r == 0u || r > (uint32_t)RMAX) continue;  // nothing to rebuild
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t* p = pats + (size_t)(w & kMPatMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        if (r == 1u) mixed_plan_tile<1>(K, a, b, S, p0, p, lane);
        if constexpr (RMAX >= 2)
            if (r == 2u) mixed_plan_tile<2>(K, a, b, S, p0, p, lane);
        if constexpr (RMAX >= 3)
            if (r == 3u) mixed_plan_tile<3>(K, a, b, S, p0, p, lane);
        if constexpr (RMAX >= 4)
            if (r == 4u) mixed_plan_tile<4>(K, a, b, S, p0, p, lane);
    }
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of shard
// addresses (shard_rows.h).  The text is gf_mixed_plan's, word for word, with the
// tiles' ROWS flag set.  It is not shared through a function: wrapping the walk
// moved the register counts of existing instances (gf_heal_mixed_plan<4> from 161
// to 152 VGPRs, md5_plan from 92 to 96), and those are pinned.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_mixed_plan_rows(const MRec* __restrict__ recs,
                                                                    const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                                    const uint32_t* __restrict__ pat_of,
                                                                    const uint32_t* __restrict__ pats, int K) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = pat_of[e.rec];
        const uint32_t r = w >> kMPatShift;  // wave-uniform
        if (r == 0u || r > (uint32_t)RMAX) continue;  // nothing to rebuild
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t* p = pats + (size_t)(w & kMPatMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        if (r == 1u) mixed_plan_tile<1, true>(K, a, b, S, p0, p, lane);
        if constexpr (RMAX >= 2)
            if (r == 2u) mixed_plan_tile<2, true>(K, a, b, S, p0, p, lane);
        if constexpr (RMAX >= 3)
            if (r == 3u) mixed_plan_tile<3, true>(K, a, b, S, p0, p, lane);
        if constexpr (RMAX >= 4)
            if (r == 4u) mixed_plan_tile<4, true>(K, a, b, S, p0, p, lane);
    }
}

static const void* mixed_plan_kernel(int r, bool rows) {
    if (rows) {
        switch (r) {
            case 1: return reinterpret_cast<const void*>(&gf_mixed_plan_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_mixed_plan_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_mixed_plan_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_mixed_plan_rows<4>);
        }
        return nullptr;
    }
    switch (r) {
        case 1: return reinterpret_cast<const void*>(&gf_mixed_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_mixed_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_mixed_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_mixed_plan<4>);
    }
    return nullptr;
}

// the tile of every kernel that walks the list (planwalk.h): its one definition
uint32_t mixed_plan_tile_bytes() { return (uint32_t)kUnalignedU * kUnalignedWindow; }

hipError_t launch_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                             const uint32_t* pat_of, const uint32_t* pats, int cus, hipStream_t stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = mixed_plan_kernel(r, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &pat_of, &pats, &k};
    return launch_plan_walk(fn, fn ? &occ[rows][r] : nullptr, k, n_tiles, cus, args, stream);
}

}  // namespace hbec
