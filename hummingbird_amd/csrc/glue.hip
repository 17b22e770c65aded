// glue.hip — the object bytes of a plan's entries from their shards, degraded or
// not (hbec_glue_plan_mixed, hbec_glue_plan_files): ecGlue's loop
// (ecutils.go:134-186) for a batch whose shards are in device memory.
//
// gf_glue_plan<RMAX> walks the plan's static {entry, tile} list grid-stride, as
// gf_mixed_plan does (mixedplan.hip), one wave per tile.  For each tile a wave
// reads, through wave-uniform indices on read-only __restrict__ arguments
// (scalar loads):
//   the list entry        -> the source entry and the tile's shard position,
//   words[entry]          -> this call's pattern record and its count r of
//                            missing data shards (kGlueSkip: not this kernel's),
//   dsts + 4 entry        -> the destination address and length, 64 bits each,
//   recs[entry]           -> the two bases (or the address row) and S,
//   pats + record offset  -> the K survivor and r output shard indices and, per
//                            input, its r tables.
// A tile at or past min(S, len) is left before any shard byte is loaded.  The
// tile is glue_tile.h's: r = 0 gathers, r > 0 codes the missing data shards as
// it gathers the present ones, and nothing is stored outside
// [dst, dst + len).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "glue.h"
#include "glue_tile.h"
#include "kernels.h"
#include "mixedplan.h"
#include "planwalk.h"

namespace hbec {

static_assert(kUnalignedU % 2 == 0, "the four-output tile is coded as two halves");

// RMAX: the largest count of missing data shards among the call's patterns.  One
// launch glues every tile, whatever its entry's count (a wave-uniform branch to
// the tile of that count), for gf_mixed_plan's reason.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_glue_plan(const MRec* __restrict__ recs,
                                                              const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                              const uint32_t* __restrict__ words,
                                                              const uint32_t* __restrict__ dsts,
                                                              const uint32_t* __restrict__ pats, int K) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = words[e.rec];
        const uint32_t r = w >> kMPatShift;  // wave-uniform; kGlueSkip reads as 15
        if (r > (uint32_t)RMAX) continue;
        const uint32_t* dl = dsts + (size_t)e.rec * 4u;
        const uint64_t dst = (uint64_t)dl[0] | ((uint64_t)dl[1] << 32);
        const uint64_t len = (uint64_t)dl[2] | ((uint64_t)dl[3] << 32);
        const uint64_t S = recs[e.rec].shard_len;
        const uint64_t p0 = (uint64_t)e.ti * T;
        if (p0 >= (len < S ? len : S)) continue;  // nothing of this tile is wanted: no load
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint32_t* p = pats + (size_t)(w & kMPatMask) * 4u;
        if (r == 0u) glue_tile<0, false>(K, a, b, S, p0, dst, len, p, lane);
        if constexpr (RMAX >= 1)
            if (r == 1u) glue_tile<1, false>(K, a, b, S, p0, dst, len, p, lane);
        if constexpr (RMAX >= 2)
            if (r == 2u) glue_tile<2, false>(K, a, b, S, p0, dst, len, p, lane);
        if constexpr (RMAX >= 3)
            if (r == 3u) glue_tile<3, false>(K, a, b, S, p0, dst, len, p, lane);
        if constexpr (RMAX >= 4)
            if (r == 4u) {  // two halves: glue_tile.h
                glue_tile<4, false, kUnalignedU / 2>(K, a, b, S, p0, dst, len, p, lane);
                if (p0 + T / 2u < (len < S ? len : S))
                    glue_tile<4, false, kUnalignedU / 2>(K, a, b, S, p0 + T / 2u, dst, len, p, lane);
            }
    }
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of
// shard addresses (shard_rows.h).  The text is gf_glue_plan's with the tiles'
// ROWS flag set; it is written out for the reason gf_mixed_plan_rows gives.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_glue_plan_rows(const MRec* __restrict__ recs,
                                                                   const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                                   const uint32_t* __restrict__ words,
                                                                   const uint32_t* __restrict__ dsts,
                                                                   const uint32_t* __restrict__ pats, int K) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = words[e.rec];
        const uint32_t r = w >> kMPatShift;  // wave-uniform; kGlueSkip reads as 15
        if (r > (uint32_t)RMAX) continue;
        const uint32_t* dl = dsts + (size_t)e.rec * 4u;
        const uint64_t dst = (uint64_t)dl[0] | ((uint64_t)dl[1] << 32);
        const uint64_t len = (uint64_t)dl[2] | ((uint64_t)dl[3] << 32);
        const uint64_t S = recs[e.rec].shard_len;
        const uint64_t p0 = (uint64_t)e.ti * T;
        if (p0 >= (len < S ? len : S)) continue;  // nothing of this tile is wanted: no load
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint32_t* p = pats + (size_t)(w & kMPatMask) * 4u;
        if (r == 0u) glue_tile<0, true>(K, a, b, S, p0, dst, len, p, lane);
        if constexpr (RMAX >= 1)
            if (r == 1u) glue_tile<1, true>(K, a, b, S, p0, dst, len, p, lane);
        if constexpr (RMAX >= 2)
            if (r == 2u) glue_tile<2, true>(K, a, b, S, p0, dst, len, p, lane);
        if constexpr (RMAX >= 3)
            if (r == 3u) glue_tile<3, true>(K, a, b, S, p0, dst, len, p, lane);
        if constexpr (RMAX >= 4)
            if (r == 4u) {  // two halves: glue_tile.h
                glue_tile<4, true, kUnalignedU / 2>(K, a, b, S, p0, dst, len, p, lane);
                if (p0 + T / 2u < (len < S ? len : S))
                    glue_tile<4, true, kUnalignedU / 2>(K, a, b, S, p0 + T / 2u, dst, len, p, lane);
            }
    }
}

static const void* glue_plan_kernel(int r, bool rows) {
    if (rows) {
        switch (r) {
            case 0: return reinterpret_cast<const void*>(&gf_glue_plan_rows<0>);
            case 1: return reinterpret_cast<const void*>(&gf_glue_plan_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_glue_plan_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_glue_plan_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_glue_plan_rows<4>);
        }
        return nullptr;
    }
    switch (r) {
        case 0: return reinterpret_cast<const void*>(&gf_glue_plan<0>);
        case 1: return reinterpret_cast<const void*>(&gf_glue_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_glue_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_glue_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_glue_plan<4>);
    }
    return nullptr;
}

int launch_glue_plan(int k, int rmax, const MRec* recs, const MTile* tiles, uint32_t n_tiles, const uint32_t* words,
                     const uint32_t* dsts, const uint32_t* pats, int cus, void* stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = glue_plan_kernel(rmax, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &words, &dsts, &pats, &k};
    return (int)launch_plan_walk(fn, fn ? &occ[rows][rmax] : nullptr, k, n_tiles, cus, args,
                                 static_cast<hipStream_t>(stream));
}

}  // namespace hbec
