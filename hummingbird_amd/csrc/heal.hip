// heal.hip — rebuild the shard hbec_locate_plan_mixed named, and the missing
// ones with it, on the same plan (hbec_heal_plan_mixed).  What the caller had to
// do with locate's words (copy them back, decode them, clear a bit of every
// flagged entry's mask, build a second plan, repair it) is one choice per entry:
// of the records of its mask p, the one for p \ {j}.  The word and the mask's
// present bits decide j with a popcount and a ctz, so the choice is made here.
//
// gf_heal_mixed_plan<RMAX> is gf_repair_mixed_plan's walk (repair.hip) with the
// per-entry word looked up on the device: the list entry, index_of[entry],
// where[entry], present_bits[index] and heal_word[index][j] all come through
// wave-uniform indices on read-only __restrict__ arguments (scalar loads).  An
// entry locate did not find inconsistent, and one with no single shard named,
// is left by a wave-uniform continue before any byte of it is loaded.  The tile
// is repair_tile<RO, RC> (repair_tile.h), the same text repair.hip runs; every
// mask p \ {j} has r_o + r_c = m rows, so the instance launched is RMAX = m.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "heal.h"
#include "kernels.h"
#include "planwalk.h"
#include "repair_tile.h"
#include "unaligned_tile.h"

namespace hbec {

template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_heal_mixed_plan(const MRec* __restrict__ recs,
                                                                    const MTile* __restrict__ tiles,
                                                                    uint32_t n_tiles,
                                                                    const uint32_t* __restrict__ index_of,
                                                                    const uint32_t* __restrict__ heal_word,
                                                                    const uint32_t* __restrict__ present_bits,
                                                                    const uint32_t* __restrict__ pats, int K,
                                                                    const uint32_t* __restrict__ where,
                                                                    uint32_t* flags) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t pi = index_of[e.rec];
        if (pi == kHealNone) continue;  // no tiles in this call
        const uint32_t wh = where[e.rec];
        if (!heal_examined(wh)) continue;  // clean, or not checked: nothing of the entry is loaded
        const int j = heal_pick(present_bits[pi], wh);  // wave-uniform
        const uint32_t w = j >= 0 ? heal_word[(size_t)pi * kHealRow + (uint32_t)j] : 0u;
        const uint32_t ro = (w >> kRpOutShift) & 7u, rc = (w >> kRpChkShift) & 7u;
        if (w == 0u || ro + rc != (uint32_t)RMAX) {
            // no single shard named (or one that would leave fewer than k): said once per entry
            if (e.ti == 0u && lane == 0u) atomicOr(flags + e.rec, kHealUnnamed);
            continue;
        }
        // said once per entry, as repair says its bit 1 (nothing left to check: rc == 0)
        if (e.ti == 0u && lane == 0u) atomicOr(flags + e.rec, rc == 0u ? kHealDone | 2u : kHealDone);
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t zero = recs[e.rec].pad_;
        const uint32_t* p = pats + (size_t)(w & kRpRecMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        uint32_t* flag = flags + e.rec;
        // a named shard is an output: every record has ro >= 1 and ro + rc == m
#define HBEC_HEAL_TILE(O, C)                \
    if constexpr (RMAX == (O) + (C))        \
        if (ro == (O) && rc == (C)) repair_tile<O, C>(K, a, b, S, p0, p, lane, flag, zero)
        HBEC_HEAL_TILE(1, 0);
        HBEC_HEAL_TILE(2, 0);
        HBEC_HEAL_TILE(1, 1);
        HBEC_HEAL_TILE(3, 0);
        HBEC_HEAL_TILE(2, 1);
        HBEC_HEAL_TILE(1, 2);
        HBEC_HEAL_TILE(4, 0);
        HBEC_HEAL_TILE(3, 1);
        HBEC_HEAL_TILE(2, 2);
        HBEC_HEAL_TILE(1, 3);
#undef HBEC_HEAL_TILE
    }
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of shard
// addresses (shard_rows.h).  The text is gf_heal_mixed_plan's, word for word, with the
// tiles' ROWS flag set.  It is not shared through a function: wrapping the walk
// moved the register counts of existing instances (gf_heal_mixed_plan<4> from 161
// to 152 VGPRs, md5_plan from 92 to 96), and those are pinned.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_heal_mixed_plan_rows(const MRec* __restrict__ recs,
                                                                         const MTile* __restrict__ tiles,
                                                                         uint32_t n_tiles,
                                                                         const uint32_t* __restrict__ index_of,
                                                                         const uint32_t* __restrict__ heal_word,
                                                                         const uint32_t* __restrict__ present_bits,
                                                                         const uint32_t* __restrict__ pats, int K,
                                                                         const uint32_t* __restrict__ where,
                                                                         uint32_t* flags) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t pi = index_of[e.rec];
        if (pi == kHealNone) continue;  // no tiles in this call
        const uint32_t wh = where[e.rec];
        if (!heal_examined(wh)) continue;  // clean, or not checked: nothing of the entry is loaded
        const int j = heal_pick(present_bits[pi], wh);  // wave-uniform
        const uint32_t w = j >= 0 ? heal_word[(size_t)pi * kHealRow + (uint32_t)j] : 0u;
        const uint32_t ro = (w >> kRpOutShift) & 7u, rc = (w >> kRpChkShift) & 7u;
        if (w == 0u || ro + rc != (uint32_t)RMAX) {
            // no single shard named (or one that would leave fewer than k): said once per entry
            if (e.ti == 0u && lane == 0u) atomicOr(flags + e.rec, kHealUnnamed);
            continue;
        }
        // said once per entry, as repair says its bit 1 (nothing left to check: rc == 0)
        if (e.ti == 0u && lane == 0u) atomicOr(flags + e.rec, rc == 0u ? kHealDone | 2u : kHealDone);
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t zero = recs[e.rec].pad_;
        const uint32_t* p = pats + (size_t)(w & kRpRecMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        uint32_t* flag = flags + e.rec;
        // a named shard is an output: every record has ro >= 1 and ro + rc == m
#define HBEC_HEAL_TILE(O, C)                \
    if constexpr (RMAX == (O) + (C))        \
        if (ro == (O) && rc == (C)) repair_tile<O, C, true>(K, a, b, S, p0, p, lane, flag, zero)
        HBEC_HEAL_TILE(1, 0);
        HBEC_HEAL_TILE(2, 0);
        HBEC_HEAL_TILE(1, 1);
        HBEC_HEAL_TILE(3, 0);
        HBEC_HEAL_TILE(2, 1);
        HBEC_HEAL_TILE(1, 2);
        HBEC_HEAL_TILE(4, 0);
        HBEC_HEAL_TILE(3, 1);
        HBEC_HEAL_TILE(2, 2);
        HBEC_HEAL_TILE(1, 3);
#undef HBEC_HEAL_TILE
    }
}

static const void* heal_mixed_plan_kernel(int r, bool rows) {
    if (rows) {
        switch (r) {
            case 1: return reinterpret_cast<const void*>(&gf_heal_mixed_plan_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_heal_mixed_plan_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_heal_mixed_plan_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_heal_mixed_plan_rows<4>);
        }
        return nullptr;
    }
    switch (r) {
        case 1: return reinterpret_cast<const void*>(&gf_heal_mixed_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_heal_mixed_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_heal_mixed_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_heal_mixed_plan<4>);
    }
    return nullptr;
}

hipError_t launch_heal_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                  const uint32_t* index_of, const uint32_t* heal_word,
                                  const uint32_t* present_bits, const uint32_t* pats, const uint32_t* where,
                                  uint32_t* flags, int cus, hipStream_t stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = heal_mixed_plan_kernel(r, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &index_of, &heal_word, &present_bits, &pats, &k, &where, &flags};
    return launch_plan_walk(fn, fn ? &occ[rows][r] : nullptr, k, n_tiles, cus, args, stream);
}

}  // namespace hbec
