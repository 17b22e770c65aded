// gluerangecheck.hip — any byte range of a plan's entries from ALL their present
// shards: written as gf_range_plan writes it (gluerange.hip), with the surplus
// shards checked at the shard positions the range touches and every byte
// correct.h's rule finds wrong there replaced on the way, and nothing stored
// into any shard (hbec_glue_plan_range_checked,
// hbec_glue_plan_files_range_checked).  Read-repair on a ranged GET.
//
// gf_range_checked<AMAX> walks the plan's static {entry, tile} list grid-stride,
// one wave per tile, as gf_range_plan does.  For each tile a wave reads, through
// wave-uniform indices on read-only __restrict__ arguments (scalar loads):
//   the list entry        -> the source entry and the tile's shard position,
//   words[entry]          -> this call's record and its rows (gluerangecheck.h;
//                            kGlueSkip: not this kernel's),
//   ranges + 6 entry      -> the destination address, the range's start in D and
//                            its length, 64 bits each,
//   recs[entry]           -> the two bases (or the address row) and S,
//   pats + record offset  -> the gc_record of the entry's mask (gluecheck.h), or
//                            its mp_pattern where exactly k shards are present.
// A tile with no position of P = gr_positions(S, s, e) is left before any shard
// byte is loaded.  An entry with exactly k present has nothing to check: tile 0
// says so in the entry's word, and its live tiles are range_tile's gather and
// decode, chosen as gf_range_plan chooses them.  Every other live tile is
// gluerangecheck_tile.h's for its A = r + o.  Every write is a per-lane vector
// store into [dst, dst + len) or the tile's one atomicOr; no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "correct.h"
#include "gf_device.h"
#include "glue.h"
#include "gluecheck.h"
#include "gluerange.h"
#include "gluerange_tile.h"
#include "gluerangecheck.h"
#include "gluerangecheck_tile.h"
#include "kernels.h"
#include "mixedplan.h"
#include "planwalk.h"

namespace hbec {

static_assert(kUnalignedU % 2 == 0, "the four-row tiles are coded as two halves");
static_assert(kGrcShift == kMPatShift && kGrcMask == kMPatMask && kGrcShift == kGcShift,
              "gluerangecheck.h, gluecheck.h and mixedplan.h disagree");
static_assert((kGrcPlain | (uint32_t)kMaxR) < 15u && (uint32_t)kMaxR < kGrcPlain, "the word's four bits");

// The live tile [p0, p0 + T) of an entry with nothing to check, as range_walk
// (gluerange.hip) glues it: gathered unless one of its R missing data shards has
// a wanted position in it.  p: the entry's mp_pattern.
template <int AMAX, bool ROWS>
__device__ __forceinline__ void range_plain_tile(uint32_t R, int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0,
                                                 uint64_t dst, uint64_t s, uint64_t e, GrSpan P,
                                                 const uint32_t* __restrict__ p, uint32_t lane) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    if (R == 0u || !gr_tile_coded(S, s, e, p0, p0 + T, p[3], (int)R)) {
        range_tile<0, ROWS>(K, a, b, S, p0, dst, s, e, p, lane);
        return;
    }
    if constexpr (AMAX >= 1)
        if (R == 1u) range_tile<1, ROWS>(K, a, b, S, p0, dst, s, e, p, lane);
    if constexpr (AMAX >= 2)
        if (R == 2u) range_tile<2, ROWS>(K, a, b, S, p0, dst, s, e, p, lane);
    if constexpr (AMAX >= 3)
        if (R == 3u) range_tile<3, ROWS>(K, a, b, S, p0, dst, s, e, p, lane);
    if constexpr (AMAX >= 4)
        if (R == 4u) {  // two halves (glue_tile.h), each only if a position of it is wanted
            if (gr_tile_live(P, p0, p0 + T / 2u))
                range_tile<4, ROWS, kUnalignedU / 2>(K, a, b, S, p0, dst, s, e, p, lane);
            if (gr_tile_live(P, p0 + T / 2u, p0 + T))
                range_tile<4, ROWS, kUnalignedU / 2>(K, a, b, S, p0 + T / 2u, dst, s, e, p, lane);
        }
}

// The walk both kernels below share.  AMAX: the largest row count among the
// call's masks (grc_rows).  One launch glues every tile, whatever its entry's
// counts (a wave-uniform branch to the tile of that A; r and o are the
// record's), for gf_mixed_plan's reason.
template <int AMAX, bool ROWS>
__device__ __forceinline__ void range_checked_walk(const MRec* __restrict__ recs, const MTile* __restrict__ tiles,
                                                   uint32_t n_tiles, const uint32_t* __restrict__ words,
                                                   const uint32_t* __restrict__ ranges,
                                                   const uint32_t* __restrict__ pats, int K, uint32_t* fixed) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile tl = tiles[t];
        const uint32_t w = words[tl.rec];
        const uint32_t bits = w >> kGrcShift;  // wave-uniform; kGlueSkip reads as 15
        const bool plain = (bits & kGrcPlain) != 0u;
        const uint32_t A = bits & (kGrcPlain - 1u);
        if (A > (uint32_t)AMAX) continue;
        uint32_t* out = fixed + tl.rec;
        // exactly k present: nothing to check, said once per entry, wherever its range lies
        if (plain && tl.ti == 0u && lane == 0u) atomicOr(out, kCorNothing);
        const uint32_t* dl = ranges + (size_t)tl.rec * 6u;
        const uint64_t s = (uint64_t)dl[2] | ((uint64_t)dl[3] << 32);
        const uint64_t e = s + ((uint64_t)dl[4] | ((uint64_t)dl[5] << 32));
        const uint64_t S = recs[tl.rec].shard_len;
        const uint64_t p0 = (uint64_t)tl.ti * T;
        const GrSpan P = gr_positions(S, s, e);
        if (!gr_tile_live(P, p0, p0 + T)) continue;  // nothing of this tile is wanted or examined: no load
        const uint64_t dst = (uint64_t)dl[0] | ((uint64_t)dl[1] << 32);
        const uint64_t a = recs[tl.rec].a, b = recs[tl.rec].b;
        const uint32_t* p = pats + (size_t)(w & kGrcMask) * 4u;
        if (plain) {
            range_plain_tile<AMAX, ROWS>(A, K, a, b, S, p0, dst, s, e, P, p, lane);
            continue;
        }
        if constexpr (AMAX >= 1)
            if (A == 1u) rangecheck_tile<1, ROWS>(K, a, b, S, p0, dst, s, e, P, p, lane, out);
        if constexpr (AMAX >= 2)
            if (A == 2u) rangecheck_tile<2, ROWS>(K, a, b, S, p0, dst, s, e, P, p, lane, out);
        if constexpr (AMAX >= 3)
            if (A == 3u) rangecheck_tile<3, ROWS>(K, a, b, S, p0, dst, s, e, P, p, lane, out);
        if constexpr (AMAX >= 4)
            if (A == 4u) {  // two halves (gluecheck_tile.h), each only if a position of it is in P
                if (gr_tile_live(P, p0, p0 + T / 2u))
                    rangecheck_tile<4, ROWS, kUnalignedU / 2>(K, a, b, S, p0, dst, s, e, P, p, lane, out);
                if (gr_tile_live(P, p0 + T / 2u, p0 + T))
                    rangecheck_tile<4, ROWS, kUnalignedU / 2>(K, a, b, S, p0 + T / 2u, dst, s, e, P, p, lane, out);
            }
    }
}

template <int AMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_range_checked(const MRec* __restrict__ recs,
                                                                  const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                                  const uint32_t* __restrict__ words,
                                                                  const uint32_t* __restrict__ ranges,
                                                                  const uint32_t* __restrict__ pats, int K,
                                                                  uint32_t* fixed) {
    range_checked_walk<AMAX, false>(recs, tiles, n_tiles, words, ranges, pats, K, fixed);
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of
// shard addresses (shard_rows.h).
template <int AMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_range_checked_rows(const MRec* __restrict__ recs,
                                                                       const MTile* __restrict__ tiles,
                                                                       uint32_t n_tiles,
                                                                       const uint32_t* __restrict__ words,
                                                                       const uint32_t* __restrict__ ranges,
                                                                       const uint32_t* __restrict__ pats, int K,
                                                                       uint32_t* fixed) {
    range_checked_walk<AMAX, true>(recs, tiles, n_tiles, words, ranges, pats, K, fixed);
}

static const void* range_checked_kernel(int amax, bool rows) {
    if (rows) {
        switch (amax) {
            case 0: return reinterpret_cast<const void*>(&gf_range_checked_rows<0>);
            case 1: return reinterpret_cast<const void*>(&gf_range_checked_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_range_checked_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_range_checked_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_range_checked_rows<4>);
        }
        return nullptr;
    }
    switch (amax) {
        case 0: return reinterpret_cast<const void*>(&gf_range_checked<0>);
        case 1: return reinterpret_cast<const void*>(&gf_range_checked<1>);
        case 2: return reinterpret_cast<const void*>(&gf_range_checked<2>);
        case 3: return reinterpret_cast<const void*>(&gf_range_checked<3>);
        case 4: return reinterpret_cast<const void*>(&gf_range_checked<4>);
    }
    return nullptr;
}

int launch_glue_range_checked(int k, int amax, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                              const uint32_t* words, const uint32_t* ranges, const uint32_t* pats, uint32_t* fixed,
                              int cus, void* stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = range_checked_kernel(amax, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &words, &ranges, &pats, &k, &fixed};
    return (int)launch_plan_walk(fn, fn ? &occ[rows][amax] : nullptr, k, n_tiles, cus, args,
                                 static_cast<hipStream_t>(stream));
}

}  // namespace hbec
