// splitselect.hip — chosen shards of a plan's entries from their object bytes
// (hbec_split_plan_select, hbec_split_plan_files_select): ecSplit's loop
// (ecutils.go:26-72) with a writers mask per entry (line 63), for a batch whose
// objects are in device memory.
//
// gf_split_select_plan<RMAX> walks the plan's static {entry, tile} list
// grid-stride, as gf_split_plan does (splitplan.hip), one wave per tile.  For
// each tile a wave reads, through wave-uniform indices on read-only
// __restrict__ arguments (scalar loads):
//   the list entry        -> the source entry and the tile's shard position,
//   words[entry]          -> the record of the entry's mask and its count R of
//                            selected parity rows (kSsSkip: nothing selected,
//                            no bytes, or not this kernel's: skipped before
//                            any load),
//   srcs + 4 entry        -> the piece's address and length, 64 bits each,
//   recs[entry]           -> the two bases (or the address row) and S,
//   pats + record offset  -> the store and read masks, the selected parity
//                            shards and, per data shard, those rows' tables.
// The tile is splitselect_tile.h's.  RMAX: the largest R among the call's
// masks.  One launch codes every tile whatever its entry's R, through a
// wave-uniform branch to that R's tile, as gf_mixed_plan does and for the
// reason measured there (mixedplan.hip): with a launch per count every launch
// waits for its unluckiest wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "kernels.h"
#include "mixedplan.h"
#include "planwalk.h"
#include "splitselect.h"
#include "splitselect_tile.h"

namespace hbec {

static_assert(kUnalignedU % 2 == 0, "the four-row tile is coded as two halves");
static_assert(kSsShift == kMPatShift && kSsMask == kMPatMask && kSsHdr == kMPatHdr,
              "splitselect.h restates mixedplan.h's word and header");
static_assert(kMaxR == 4 && kOddMaxK <= 12, "a record holds four parity indices and masks of twelve data shards");

// The tile of one list entry, for the two walks below.  R = 4 is coded as two
// halves of kUnalignedU / 2 windows, as split's m = 4 is (splitplan.hip).
template <int R, bool ROWS>
__device__ __forceinline__ void split_select_walk_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0,
                                                       uint64_t src, uint64_t len, const uint32_t* __restrict__ p,
                                                       uint32_t lane) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    if constexpr (R < 4) {
        split_select_tile<R, ROWS>(K, a, b, S, p0, src, len, p, lane);
    } else {
        split_select_tile<R, ROWS, kUnalignedU / 2>(K, a, b, S, p0, src, len, p, lane);
        if (p0 + T / 2u < S)
            split_select_tile<R, ROWS, kUnalignedU / 2>(K, a, b, S, p0 + T / 2u, src, len, p, lane);
    }
}

template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_split_select_plan(const MRec* __restrict__ recs,
                                                                      const MTile* __restrict__ tiles,
                                                                      uint32_t n_tiles,
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
        const uint32_t r = w >> kSsShift;  // wave-uniform; kSsSkip reads as 15
        if (r > (uint32_t)RMAX) continue;
        const uint32_t* sl = srcs + (size_t)e.rec * 4u;
        const uint64_t src = (uint64_t)sl[0] | ((uint64_t)sl[1] << 32);
        const uint64_t len = (uint64_t)sl[2] | ((uint64_t)sl[3] << 32);
        const uint64_t S = recs[e.rec].shard_len;
        const uint64_t p0 = (uint64_t)e.ti * T;
        if (p0 >= S || len == 0u) continue;  // never on a list and words the host built
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint32_t* p = pats + (size_t)(w & kSsMask) * 4u;
        if (r == 0u) split_select_walk_tile<0, false>(K, a, b, S, p0, src, len, p, lane);
        if constexpr (RMAX >= 1)
            if (r == 1u) split_select_walk_tile<1, false>(K, a, b, S, p0, src, len, p, lane);
        if constexpr (RMAX >= 2)
            if (r == 2u) split_select_walk_tile<2, false>(K, a, b, S, p0, src, len, p, lane);
        if constexpr (RMAX >= 3)
            if (r == 3u) split_select_walk_tile<3, false>(K, a, b, S, p0, src, len, p, lane);
        if constexpr (RMAX >= 4)
            if (r == 4u) split_select_walk_tile<4, false>(K, a, b, S, p0, src, len, p, lane);
    }
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of
// shard addresses (shard_rows.h).  The text is gf_split_select_plan's with the
// tiles' ROWS flag set; it is written out for the reason gf_mixed_plan_rows gives.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_split_select_plan_rows(const MRec* __restrict__ recs,
                                                                           const MTile* __restrict__ tiles,
                                                                           uint32_t n_tiles,
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
        const uint32_t r = w >> kSsShift;  // wave-uniform; kSsSkip reads as 15
        if (r > (uint32_t)RMAX) continue;
        const uint32_t* sl = srcs + (size_t)e.rec * 4u;
        const uint64_t src = (uint64_t)sl[0] | ((uint64_t)sl[1] << 32);
        const uint64_t len = (uint64_t)sl[2] | ((uint64_t)sl[3] << 32);
        const uint64_t S = recs[e.rec].shard_len;
        const uint64_t p0 = (uint64_t)e.ti * T;
        if (p0 >= S || len == 0u) continue;  // never on a list and words the host built
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint32_t* p = pats + (size_t)(w & kSsMask) * 4u;
        if (r == 0u) split_select_walk_tile<0, true>(K, a, b, S, p0, src, len, p, lane);
        if constexpr (RMAX >= 1)
            if (r == 1u) split_select_walk_tile<1, true>(K, a, b, S, p0, src, len, p, lane);
        if constexpr (RMAX >= 2)
            if (r == 2u) split_select_walk_tile<2, true>(K, a, b, S, p0, src, len, p, lane);
        if constexpr (RMAX >= 3)
            if (r == 3u) split_select_walk_tile<3, true>(K, a, b, S, p0, src, len, p, lane);
        if constexpr (RMAX >= 4)
            if (r == 4u) split_select_walk_tile<4, true>(K, a, b, S, p0, src, len, p, lane);
    }
}

static const void* split_select_kernel(int rmax, bool rows) {
    if (rows) {
        switch (rmax) {
            case 0: return reinterpret_cast<const void*>(&gf_split_select_plan_rows<0>);
            case 1: return reinterpret_cast<const void*>(&gf_split_select_plan_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_split_select_plan_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_split_select_plan_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_split_select_plan_rows<4>);
        }
        return nullptr;
    }
    switch (rmax) {
        case 0: return reinterpret_cast<const void*>(&gf_split_select_plan<0>);
        case 1: return reinterpret_cast<const void*>(&gf_split_select_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_split_select_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_split_select_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_split_select_plan<4>);
    }
    return nullptr;
}

int launch_split_select_plan(int k, int rmax, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                             const uint32_t* words, const uint32_t* srcs, const uint32_t* pats, int cus, void* stream,
                             bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = split_select_kernel(rmax, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &words, &srcs, &pats, &k};
    return (int)launch_plan_walk(fn, fn ? &occ[rows][rmax] : nullptr, k, n_tiles, cus, args,
                                 static_cast<hipStream_t>(stream));
}

}  // namespace hbec
