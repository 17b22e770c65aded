// repair.hip — rebuild the missing shards of every stripe of a plan and check
// its surplus ones in the same pass (hbec_repair_plan_mixed).  ecReconstruct
// rebuilds from the first k shards it can get (ecutils.go:94-111), so a
// silently corrupt survivor becomes a silently corrupt rebuilt shard unless the
// surplus shards that were fetched anyway are looked at.  hbec_verify_plan_mixed
// then hbec_reconstruct_plan_mixed read the k survivors of every stripe twice;
// here they are read once: (k + r_c + r_o) S bytes per stripe, not
// (2k + r_c + r_o) S.
//
// gf_repair_mixed_plan<RMAX> walks the plan's static {entry, tile} list exactly
// as gf_verify_mixed_plan does (vmixed.hip): the list entry, pat_of[entry], the
// entry's record and its mask's pattern record all come through wave-uniform
// indices on read-only __restrict__ arguments (scalar loads), and a
// wave-uniform branch goes to the tile of the entry's (outputs, checked) counts.
// The tile has one accumulator row per shard that is not a survivor, r_o + r_c
// <= m <= 4 of them: a row whose shard is missing starts at zero and is stored
// as unaligned_tile stores it (unaligned_tile.h), a row whose shard is present
// starts as the stored column, loaded ahead of the first survivor's, and must
// be zero after the k multiplies, as in verify_mixed_tile.  One multiply loop
// serves both kinds.  Tiles are specialised per (r_o, r_c) pair, so nothing
// about a row's kind is decided at run time, and the pairs with r_c = 0 and
// r_o = 0 are the tiles of gf_mixed_plan and gf_verify_mixed_plan.  The tile's
// text is in repair_tile.h: gf_heal_mixed_plan (heal.hip) runs it too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "kernels.h"
#include "planwalk.h"
#include "repair.h"
#include "repair_tile.h"
#include "unaligned_tile.h"

namespace hbec {

// RMAX: the largest count of rows, outputs and checked shards together, among
// the call's entries.  One launch serves every pair of counts, for the reason
// written at gf_mixed_plan.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_repair_mixed_plan(const MRec* __restrict__ recs,
                                                                      const MTile* __restrict__ tiles,
                                                                      uint32_t n_tiles,
                                                                      const uint32_t* __restrict__ pat_of,
                                                                      const uint32_t* __restrict__ pats, int K,
                                                                      uint32_t* flags) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = pat_of[e.rec];
        if (w == 0u) continue;  // no tiles in this call
        const uint32_t ro = (w >> kRpOutShift) & 7u, rc = (w >> kRpChkShift) & 7u;  // wave-uniform
        // exactly k present: nothing to check, said once per entry
        if (rc == 0u && e.ti == 0u && lane == 0u) atomicOr(flags + e.rec, 2u);
        if (ro + rc == 0u || ro + rc > (uint32_t)RMAX) continue;
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t zero = recs[e.rec].pad_;
        const uint32_t* p = pats + (size_t)(w & kRpRecMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        uint32_t* flag = flags + e.rec;
#define HBEC_RP_TILE(O, C)                  \
    if constexpr (RMAX >= (O) + (C))        \
        if (ro == (O) && rc == (C)) repair_tile<O, C>(K, a, b, S, p0, p, lane, flag, zero)
        HBEC_RP_TILE(1, 0);
        HBEC_RP_TILE(0, 1);
        HBEC_RP_TILE(2, 0);
        HBEC_RP_TILE(1, 1);
        HBEC_RP_TILE(0, 2);
        HBEC_RP_TILE(3, 0);
        HBEC_RP_TILE(2, 1);
        HBEC_RP_TILE(1, 2);
        HBEC_RP_TILE(0, 3);
        HBEC_RP_TILE(4, 0);
        HBEC_RP_TILE(3, 1);
        HBEC_RP_TILE(2, 2);
        HBEC_RP_TILE(1, 3);
        HBEC_RP_TILE(0, 4);
#undef HBEC_RP_TILE
    }
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of shard
// addresses (shard_rows.h).  The text is gf_repair_mixed_plan's, word for word, with the
// tiles' ROWS flag set.  It is not shared through a function: wrapping the walk
// moved the register counts of existing instances (gf_heal_mixed_plan<4> from 161
// to 152 VGPRs, md5_plan from 92 to 96), and those are pinned.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_repair_mixed_plan_rows(const MRec* __restrict__ recs,
                                                                           const MTile* __restrict__ tiles,
                                                                           uint32_t n_tiles,
                                                                           const uint32_t* __restrict__ pat_of,
                                                                           const uint32_t* __restrict__ pats, int K,
                                                                           uint32_t* flags) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = pat_of[e.rec];
        if (w == 0u) continue;  // no tiles in this call
        const uint32_t ro = (w >> kRpOutShift) & 7u, rc = (w >> kRpChkShift) & 7u;  // wave-uniform
        // exactly k present: nothing to check, said once per entry
        if (rc == 0u && e.ti == 0u && lane == 0u) atomicOr(flags + e.rec, 2u);
        if (ro + rc == 0u || ro + rc > (uint32_t)RMAX) continue;
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t zero = recs[e.rec].pad_;
        const uint32_t* p = pats + (size_t)(w & kRpRecMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        uint32_t* flag = flags + e.rec;
#define HBEC_RP_TILE(O, C)                  \
    if constexpr (RMAX >= (O) + (C))        \
        if (ro == (O) && rc == (C)) repair_tile<O, C, true>(K, a, b, S, p0, p, lane, flag, zero)
        HBEC_RP_TILE(1, 0);
        HBEC_RP_TILE(0, 1);
        HBEC_RP_TILE(2, 0);
        HBEC_RP_TILE(1, 1);
        HBEC_RP_TILE(0, 2);
        HBEC_RP_TILE(3, 0);
        HBEC_RP_TILE(2, 1);
        HBEC_RP_TILE(1, 2);
        HBEC_RP_TILE(0, 3);
        HBEC_RP_TILE(4, 0);
        HBEC_RP_TILE(3, 1);
        HBEC_RP_TILE(2, 2);
        HBEC_RP_TILE(1, 3);
        HBEC_RP_TILE(0, 4);
#undef HBEC_RP_TILE
    }
}

static const void* repair_mixed_plan_kernel(int r, bool rows) {
    if (rows) {
        switch (r) {
            case 1: return reinterpret_cast<const void*>(&gf_repair_mixed_plan_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_repair_mixed_plan_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_repair_mixed_plan_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_repair_mixed_plan_rows<4>);
        }
        return nullptr;
    }
    switch (r) {
        case 1: return reinterpret_cast<const void*>(&gf_repair_mixed_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_repair_mixed_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_repair_mixed_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_repair_mixed_plan<4>);
    }
    return nullptr;
}

hipError_t launch_repair_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                    const uint32_t* pat_of, const uint32_t* pats, uint32_t* flags, int cus,
                                    hipStream_t stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = repair_mixed_plan_kernel(r, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &pat_of, &pats, &k, &flags};
    return launch_plan_walk(fn, fn ? &occ[rows][r] : nullptr, k, n_tiles, cus, args, stream);
}

}  // namespace hbec
