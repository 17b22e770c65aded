// splitplan.hip — the k + m shards of a plan's entries from their object bytes
// (hbec_split_plan, hbec_split_plan_files): ecSplit's loop (ecutils.go:26-72)
// for a batch whose objects are in device memory.
//
// gf_split_plan<M> walks the plan's static {entry, tile} list grid-stride, as
// gf_glue_plan does (glue.hip), one wave per tile.  For each tile a wave reads,
// through wave-uniform indices on read-only __restrict__ arguments (scalar
// loads):
//   the list entry        -> the source entry and the tile's shard position,
//   words[entry]          -> the call's pattern record and its parity count
//                            (kSplitSkip: not this kernel's),
//   srcs + 4 entry        -> the piece's address and length, 64 bits each,
//   recs[entry]           -> the two bases (or the address row) and S,
//   pats + record offset  -> per data shard, the tables of the m parity rows.
// Every tile of the list has work: all k + m shards are written whole.  The
// tile is split_tile.h's.  A call has one pattern, the codec's encode rows, so
// an instance codes the tile of its own M and no other.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "kernels.h"
#include "mixedplan.h"
#include "planwalk.h"
#include "split_tile.h"
#include "splitplan.h"

namespace hbec {

static_assert(kUnalignedU % 2 == 0, "the four-parity tile is coded as two halves");

// The tile of one list entry (split_tile.h), for the two walks below.  M = 4 is
// coded as two halves of kUnalignedU / 2 windows, as glue's r = 4 is and for its
// reason (glue_tile.h).  M = 2 and 3 in halves take half the VGPRs or fewer and
// were measured 1.4 to 4 % slower than in one piece.
template <int M, bool ROWS>
__device__ __forceinline__ void split_walk_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0, uint64_t src,
                                                uint64_t len, const uint32_t* __restrict__ p, uint32_t lane) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    if constexpr (M < 4) {
        split_tile<M, ROWS>(K, a, b, S, p0, src, len, p, lane);
    } else {
        split_tile<M, ROWS, kUnalignedU / 2>(K, a, b, S, p0, src, len, p, lane);
        if (p0 + T / 2u < S) split_tile<M, ROWS, kUnalignedU / 2>(K, a, b, S, p0 + T / 2u, src, len, p, lane);
    }
}

template <int M>
__global__ __launch_bounds__(kBlockThreads) void gf_split_plan(const MRec* __restrict__ recs,
                                                               const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                               const uint32_t* __restrict__ words,
                                                               const uint32_t* __restrict__ srcs,
                                                               const uint32_t* __restrict__ pats, int K) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = words[e.rec];
        if ((w >> kMPatShift) != (uint32_t)M) continue;  // wave-uniform; kSplitSkip reads as 15
        const uint32_t* sl = srcs + (size_t)e.rec * 4u;
        const uint64_t src = (uint64_t)sl[0] | ((uint64_t)sl[1] << 32);
        const uint64_t len = (uint64_t)sl[2] | ((uint64_t)sl[3] << 32);
        const uint64_t S = recs[e.rec].shard_len;
        const uint64_t p0 = (uint64_t)e.ti * T;
        if (p0 >= S || len == 0u) continue;  // never on a list and words the host built
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        split_walk_tile<M, false>(K, a, b, S, p0, src, len, pats + (size_t)(w & kMPatMask) * 4u, lane);
    }
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of
// shard addresses (shard_rows.h).  The text is gf_split_plan's with the tiles'
// ROWS flag set; it is written out for the reason gf_mixed_plan_rows gives.
template <int M>
__global__ __launch_bounds__(kBlockThreads) void gf_split_plan_rows(const MRec* __restrict__ recs,
                                                                    const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                                    const uint32_t* __restrict__ words,
                                                                    const uint32_t* __restrict__ srcs,
                                                                    const uint32_t* __restrict__ pats, int K) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = words[e.rec];
        if ((w >> kMPatShift) != (uint32_t)M) continue;  // wave-uniform; kSplitSkip reads as 15
        const uint32_t* sl = srcs + (size_t)e.rec * 4u;
        const uint64_t src = (uint64_t)sl[0] | ((uint64_t)sl[1] << 32);
        const uint64_t len = (uint64_t)sl[2] | ((uint64_t)sl[3] << 32);
        const uint64_t S = recs[e.rec].shard_len;
        const uint64_t p0 = (uint64_t)e.ti * T;
        if (p0 >= S || len == 0u) continue;  // never on a list and words the host built
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        split_walk_tile<M, true>(K, a, b, S, p0, src, len, pats + (size_t)(w & kMPatMask) * 4u, lane);
    }
}

static const void* split_plan_kernel(int m, bool rows) {
    if (rows) {
        switch (m) {
            case 0: return reinterpret_cast<const void*>(&gf_split_plan_rows<0>);
            case 1: return reinterpret_cast<const void*>(&gf_split_plan_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_split_plan_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_split_plan_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_split_plan_rows<4>);
        }
        return nullptr;
    }
    switch (m) {
        case 0: return reinterpret_cast<const void*>(&gf_split_plan<0>);
        case 1: return reinterpret_cast<const void*>(&gf_split_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_split_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_split_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_split_plan<4>);
    }
    return nullptr;
}

int launch_split_plan(int k, int m, const MRec* recs, const MTile* tiles, uint32_t n_tiles, const uint32_t* words,
                      const uint32_t* srcs, const uint32_t* pats, int cus, void* stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = split_plan_kernel(m, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &words, &srcs, &pats, &k};
    return (int)launch_plan_walk(fn, fn ? &occ[rows][m] : nullptr, k, n_tiles, cus, args,
                                 static_cast<hipStream_t>(stream));
}

}  // namespace hbec
