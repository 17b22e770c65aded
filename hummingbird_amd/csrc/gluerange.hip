// gluerange.hip — any byte range of a plan's entries from their shards, degraded
// or not (hbec_glue_plan_range, hbec_glue_plan_files_range): the decode of
// ecObject.CopyRange (ecobj.go:207-267) over ecGlue's layout (ecutils.go:134-186)
// for a batch whose shards are in device memory.
//
// gf_range_plan<RMAX> walks the plan's static {entry, tile} list grid-stride, as
// gf_glue_plan does (glue.hip), one wave per tile.  For each tile a wave reads,
// through wave-uniform indices on read-only __restrict__ arguments (scalar
// loads):
//   the list entry        -> the source entry and the tile's shard position,
//   words[entry]          -> this call's pattern record and its count r of
//                            missing data shards (kGlueSkip: not this kernel's),
//   ranges + 6 entry      -> the destination address, the range's start in D and
//                            its length, 64 bits each,
//   recs[entry]           -> the two bases (or the address row) and S,
//   pats + record offset  -> the K survivor and r output shard indices and, per
//                            input, its r tables.
// A tile with no wanted shard position (gluerange.h gr_tile_live) is left before
// any shard byte is loaded.  A live tile in which no missing data shard has a
// wanted position is gathered (range_tile<0>), whatever its entry's r; the
// others are decoded by the tile of that r.  Nothing is stored outside
// [dst, dst + len).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "glue.h"
#include "gluerange.h"
#include "gluerange_tile.h"
#include "kernels.h"
#include "mixedplan.h"
#include "planwalk.h"

namespace hbec {

static_assert(kUnalignedU % 2 == 0, "the four-output tile is coded as two halves");

// RMAX: the largest count of missing data shards among the call's patterns.  One
// launch glues every tile, whatever its entry's count (a wave-uniform branch to
// the tile of that count), for gf_mixed_plan's reason.
template <int RMAX, bool ROWS>
__device__ __forceinline__ void range_walk(const MRec* __restrict__ recs, const MTile* __restrict__ tiles,
                                           uint32_t n_tiles, const uint32_t* __restrict__ words,
                                           const uint32_t* __restrict__ ranges, const uint32_t* __restrict__ pats,
                                           int K) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile tl = tiles[t];
        const uint32_t w = words[tl.rec];
        const uint32_t r = w >> kMPatShift;  // wave-uniform; kGlueSkip reads as 15
        if (r > (uint32_t)RMAX) continue;
        const uint32_t* dl = ranges + (size_t)tl.rec * 6u;
        const uint64_t s = (uint64_t)dl[2] | ((uint64_t)dl[3] << 32);
        const uint64_t e = s + ((uint64_t)dl[4] | ((uint64_t)dl[5] << 32));
        const uint64_t S = recs[tl.rec].shard_len;
        const uint64_t p0 = (uint64_t)tl.ti * T;
        if (!gr_tile_live(gr_positions(S, s, e), p0, p0 + T)) continue;  // nothing of this tile is wanted: no load
        const uint64_t dst = (uint64_t)dl[0] | ((uint64_t)dl[1] << 32);
        const uint64_t a = recs[tl.rec].a, b = recs[tl.rec].b;
        const uint32_t* p = pats + (size_t)(w & kMPatMask) * 4u;
        if (r == 0u || !gr_tile_coded(S, s, e, p0, p0 + T, p[3], (int)r)) {
            range_tile<0, ROWS>(K, a, b, S, p0, dst, s, e, p, lane);
            continue;
        }
        if constexpr (RMAX >= 1)
            if (r == 1u) range_tile<1, ROWS>(K, a, b, S, p0, dst, s, e, p, lane);
        if constexpr (RMAX >= 2)
            if (r == 2u) range_tile<2, ROWS>(K, a, b, S, p0, dst, s, e, p, lane);
        if constexpr (RMAX >= 3)
            if (r == 3u) range_tile<3, ROWS>(K, a, b, S, p0, dst, s, e, p, lane);
        if constexpr (RMAX >= 4)
            if (r == 4u) {  // two halves (glue_tile.h), each only if a position of it is wanted
                const GrSpan P = gr_positions(S, s, e);
                if (gr_tile_live(P, p0, p0 + T / 2u))
                    range_tile<4, ROWS, kUnalignedU / 2>(K, a, b, S, p0, dst, s, e, p, lane);
                if (gr_tile_live(P, p0 + T / 2u, p0 + T))
                    range_tile<4, ROWS, kUnalignedU / 2>(K, a, b, S, p0 + T / 2u, dst, s, e, p, lane);
            }
    }
}

template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_range_plan(const MRec* __restrict__ recs,
                                                               const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                               const uint32_t* __restrict__ words,
                                                               const uint32_t* __restrict__ ranges,
                                                               const uint32_t* __restrict__ pats, int K) {
    range_walk<RMAX, false>(recs, tiles, n_tiles, words, ranges, pats, K);
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of
// shard addresses (shard_rows.h).
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_range_plan_rows(const MRec* __restrict__ recs,
                                                                    const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                                    const uint32_t* __restrict__ words,
                                                                    const uint32_t* __restrict__ ranges,
                                                                    const uint32_t* __restrict__ pats, int K) {
    range_walk<RMAX, true>(recs, tiles, n_tiles, words, ranges, pats, K);
}

static const void* range_plan_kernel(int r, bool rows) {
    if (rows) {
        switch (r) {
            case 0: return reinterpret_cast<const void*>(&gf_range_plan_rows<0>);
            case 1: return reinterpret_cast<const void*>(&gf_range_plan_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_range_plan_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_range_plan_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_range_plan_rows<4>);
        }
        return nullptr;
    }
    switch (r) {
        case 0: return reinterpret_cast<const void*>(&gf_range_plan<0>);
        case 1: return reinterpret_cast<const void*>(&gf_range_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_range_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_range_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_range_plan<4>);
    }
    return nullptr;
}

int launch_glue_range(int k, int rmax, const MRec* recs, const MTile* tiles, uint32_t n_tiles, const uint32_t* words,
                      const uint32_t* ranges, const uint32_t* pats, int cus, void* stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = range_plan_kernel(rmax, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &words, &ranges, &pats, &k};
    return (int)launch_plan_walk(fn, fn ? &occ[rows][rmax] : nullptr, k, n_tiles, cus, args,
                                 static_cast<hipStream_t>(stream));
}

}  // namespace hbec
