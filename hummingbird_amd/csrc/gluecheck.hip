// gluecheck.hip — the object bytes of a plan's entries from ALL their present
// shards: glued as gf_glue_plan glues them (glue.hip), with the surplus shards
// checked and every byte correct.h's rule finds wrong replaced on the way, and
// nothing stored into any shard (hbec_glue_plan_checked,
// hbec_glue_plan_files_checked).  Read-repair on GET: the surplus shards a
// hedged or retried read already fetched decide which survivor byte is wrong.
//
// gf_glue_checked<AMAX> walks the plan's static {entry, tile} list grid-stride,
// one wave per tile, as gf_glue_plan does.  For each tile a wave reads, through
// wave-uniform indices on read-only __restrict__ arguments (scalar loads):
//   the list entry        -> the source entry and the tile's shard position,
//   words[entry]          -> this call's record and its row count A = r + o
//                            (kGlueSkip: not this kernel's),
//   dsts + 4 entry        -> the destination address and length, 64 bits each,
//   recs[entry]           -> the two bases (or the address row) and S,
//   pats + record offset  -> the gc_record of the entry's mask (gluecheck.h).
// A tile at or past min(S, len) is left before any shard byte is loaded.  The
// tile is gluecheck_tile.h's; with no rows at all (exactly the k data shards
// present) it is glue_tile's gather.  Tile 0 of an entry with nothing to check
// says so in the entry's word.  Every write is a per-lane vector store into
// [dst, dst + len) or the tile's one atomicOr; no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "correct.h"
#include "gf_device.h"
#include "glue.h"
#include "glue_tile.h"
#include "gluecheck.h"
#include "gluecheck_tile.h"
#include "kernels.h"
#include "mixedplan.h"
#include "planwalk.h"

namespace hbec {

static_assert(kUnalignedU % 2 == 0, "the four-row tile is coded as two halves");
static_assert(kGcShift == kMPatShift && kGcMask == kMPatMask, "gluecheck.h and mixedplan.h disagree");

// The walk both kernels below share.  AMAX: the largest row count among the
// call's masks.  One launch glues every tile, whatever its entry's counts (a
// wave-uniform branch to the tile of that A; r and o are the record's), for
// gf_mixed_plan's reason.
template <int AMAX, bool ROWS>
__device__ __forceinline__ void glue_checked_walk(const MRec* __restrict__ recs, const MTile* __restrict__ tiles,
                                                  uint32_t n_tiles, const uint32_t* __restrict__ words,
                                                  const uint32_t* __restrict__ dsts,
                                                  const uint32_t* __restrict__ pats, int K, uint32_t* fixed) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = words[e.rec];
        const uint32_t A = w >> kGcShift;  // wave-uniform; kGlueSkip reads as 15
        if (A > (uint32_t)AMAX) continue;
        const uint32_t* dl = dsts + (size_t)e.rec * 4u;
        const uint64_t dst = (uint64_t)dl[0] | ((uint64_t)dl[1] << 32);
        const uint64_t len = (uint64_t)dl[2] | ((uint64_t)dl[3] << 32);
        const uint64_t S = recs[e.rec].shard_len;
        const uint64_t p0 = (uint64_t)e.ti * T;
        const uint64_t Sr = len < S ? len : S;
        if (p0 >= Sr) continue;  // nothing of this tile is wanted or examined: no load
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint32_t* p = pats + (size_t)(w & kGcMask) * 4u;
        uint32_t* out = fixed + e.rec;
        // exactly k present: nothing to check, said once per entry
        if ((p[4] & 0xFFu) == 0u && e.ti == 0u && lane == 0u) atomicOr(out, kCorNothing);
        if (A == 0u) glue_tile<0, ROWS>(K, a, b, S, p0, dst, len, p, lane);
        if constexpr (AMAX >= 1)
            if (A == 1u) gluecheck_tile<1, ROWS>(K, a, b, S, p0, dst, len, p, lane, out);
        if constexpr (AMAX >= 2)
            if (A == 2u) gluecheck_tile<2, ROWS>(K, a, b, S, p0, dst, len, p, lane, out);
        if constexpr (AMAX >= 3)
            if (A == 3u) gluecheck_tile<3, ROWS>(K, a, b, S, p0, dst, len, p, lane, out);
        if constexpr (AMAX >= 4)
            if (A == 4u) {  // two halves: gluecheck_tile.h
                gluecheck_tile<4, ROWS, kUnalignedU / 2>(K, a, b, S, p0, dst, len, p, lane, out);
                if (p0 + T / 2u < Sr)
                    gluecheck_tile<4, ROWS, kUnalignedU / 2>(K, a, b, S, p0 + T / 2u, dst, len, p, lane, out);
            }
    }
}

template <int AMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_glue_checked(const MRec* __restrict__ recs,
                                                                 const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                                 const uint32_t* __restrict__ words,
                                                                 const uint32_t* __restrict__ dsts,
                                                                 const uint32_t* __restrict__ pats, int K,
                                                                 uint32_t* fixed) {
    glue_checked_walk<AMAX, false>(recs, tiles, n_tiles, words, dsts, pats, K, fixed);
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of
// shard addresses (shard_rows.h).
template <int AMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_glue_checked_rows(const MRec* __restrict__ recs,
                                                                      const MTile* __restrict__ tiles,
                                                                      uint32_t n_tiles,
                                                                      const uint32_t* __restrict__ words,
                                                                      const uint32_t* __restrict__ dsts,
                                                                      const uint32_t* __restrict__ pats, int K,
                                                                      uint32_t* fixed) {
    glue_checked_walk<AMAX, true>(recs, tiles, n_tiles, words, dsts, pats, K, fixed);
}

static const void* glue_checked_kernel(int amax, bool rows) {
    if (rows) {
        switch (amax) {
            case 0: return reinterpret_cast<const void*>(&gf_glue_checked_rows<0>);
            case 1: return reinterpret_cast<const void*>(&gf_glue_checked_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_glue_checked_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_glue_checked_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_glue_checked_rows<4>);
        }
        return nullptr;
    }
    switch (amax) {
        case 0: return reinterpret_cast<const void*>(&gf_glue_checked<0>);
        case 1: return reinterpret_cast<const void*>(&gf_glue_checked<1>);
        case 2: return reinterpret_cast<const void*>(&gf_glue_checked<2>);
        case 3: return reinterpret_cast<const void*>(&gf_glue_checked<3>);
        case 4: return reinterpret_cast<const void*>(&gf_glue_checked<4>);
    }
    return nullptr;
}

int launch_glue_checked(int k, int amax, const MRec* recs, const MTile* tiles, uint32_t n_tiles, const uint32_t* words,
                        const uint32_t* dsts, const uint32_t* pats, uint32_t* fixed, int cus, void* stream,
                        bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = glue_checked_kernel(amax, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &words, &dsts, &pats, &k, &fixed};
    return (int)launch_plan_walk(fn, fn ? &occ[rows][amax] : nullptr, k, n_tiles, cus, args,
                                 static_cast<hipStream_t>(stream));
}

}  // namespace hbec
