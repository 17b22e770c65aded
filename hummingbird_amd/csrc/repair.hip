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
// r_o = 0 are the tiles of gf_mixed_plan and gf_verify_mixed_plan.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "kernels.h"
#include "repair.h"
#include "unaligned_tile.h"

namespace hbec {

// One tile of a stripe whose mask has RO shards to rebuild and RC to check; the
// record's rows are the outputs' first.  Every capture is a value in SGPRs, as
// in mixed_plan_tile.  `zero` is the entry record's pad word, 0 in every record
// mp_build writes: the output rows start from it and not from a literal, because
// with literal zeros beside loaded rows the compiler allocates 15 to 57 VGPRs
// more than for rows that all start alike (132 against 116 at (1, 1), 209
// against 152 at (1, 3): a wave per SIMD less at both).
template <int RO, int RC>
__device__ __forceinline__ void repair_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0,
                                            const uint32_t* __restrict__ p, uint32_t lane, uint32_t* flag,
                                            uint32_t zero) {
    constexpr int R = RO + RC;
    constexpr int U = kUnalignedU;
    constexpr uint32_t W = kUnalignedWindow;
    const uint64_t s_lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);  // survivors 0..7
    const uint32_t s_hi = p[2], so = p[3];
    const uint32_t k = (uint32_t)K;
    auto shard = [=](uint32_t i) { return i < k ? a + (uint64_t)i * S : b + (uint64_t)(i - k) * S; };
    auto in_base = [=](int j) {
        return shard((j < 8 ? (uint32_t)(s_lo >> (8 * j)) : s_hi >> (8 * (j - 8))) & 0xFFu);
    };
    if constexpr (RC == 0) {
        // nothing to check: gf_mixed_plan's tile as it stands
        unaligned_tile<RO>(
            K, S, p0, false, lane, in_base, [=](int r) { return shard((so >> (8 * r)) & 0xFFu); },
            [=](int r, int j) { return p + kMPatHdr + 5 * (j * RO + r); });
        return;
    }
    uint64_t col[U];
    bool live[U];  // window-uniform
#pragma unroll
    for (int u = 0; u < U; ++u) {
        col[u] = p0 + (uint64_t)u * W + lane * 16u;
        live[u] = p0 + (uint64_t)u * W < S;
    }
    // outputs start at zero (above); checked shards as their stored columns
    // (clamped loads: no branch)
    u32x4 acc[R][U];
#pragma unroll
    for (int r = 0; r < RO; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[r][u] = u32x4{zero, zero, zero, zero};
#pragma unroll
    for (int r = RO; r < R; ++r) {
        const UView ov = uview(shard((so >> (8 * r)) & 0xFFu), S);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u32x4 lo, hi;
            uload(lo, hi, ov, col[u]);
            acc[r][u] = realign16(lo, upper(lo, hi), ov.d);
        }
    }
    u32x4 clo[U], chi[U];
    UView cv = uview(in_base(0), S);
#pragma unroll
    for (int u = 0; u < U; ++u) uload(clo[u], chi[u], cv, col[u]);
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
        u32x4 nlo[U], nhi[U];
        UView nv = cv;
        if (j + 1 < K) {
            nv = uview(in_base(j + 1), S);
#pragma unroll
            for (int u = 0; u < U; ++u) uload(nlo[u], nhi[u], nv, col[u]);
        }
        uint32_t tb[R][5];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < 5; ++q) tb[r][q] = p[kMPatHdr + 5 * (j * R + r) + q];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32x4 x = realign16(clo[u], upper(clo[u], chi[u]), cv.d);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const Sel sx = selectors(x[e]);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    acc[r][u][e] ^= gf_mul_sel(sx, tb[r][0], tb[r][1], tb[r][2], tb[r][3], tb[r][4]);
            }
        }
        if (j + 1 < K) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                clo[u] = nlo[u];
                chi[u] = nhi[u];
            }
            cv = nv;
        }
    }
    // checked rows: columns [c, c + 16) of the window's first 62 lanes; bytes at
    // or past S and windows that start there do not count
    uint32_t diff = 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t nb = col[u] < S ? S - col[u] : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t b0 = 4u * e;
            const uint32_t mask =
                nb >= b0 + 4u ? 0xFFFFFFFFu : (nb <= b0 ? 0u : (0xFFFFFFFFu >> (8u * (uint32_t)(b0 + 4u - nb))));
#pragma unroll
            for (int r = RO; r < R; ++r) diff |= acc[r][u][e] & mask;
        }
    }
    if (lane < kUnalignedStoreLanes && diff != 0u) atomicOr(flag, 1u);
    // output rows: unaligned_tile's stores, on each output's own 16-B grid
#pragma unroll
    for (int r = 0; r < RO; ++r) {
        const uint64_t ob = shard((so >> (8 * r)) & 0xFFu);
        const uint32_t e = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(ob & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!live[u]) continue;  // window-uniform: every lane takes part in the shuffle
            u32x4 nb;
#pragma unroll
            for (int i = 0; i < 4; ++i) nb[i] = __shfl_down(acc[r][u][i], 1u, 64);
            const u32x4 blk = realign16(acc[r][u], nb, e);
            const uint64_t q = col[u] + e;  // block start (shard position); ob + q is 16-B aligned
            if (lane < kUnalignedStoreLanes && q < S) {
                if (q + 16u <= S)
                    st16_addr(ob + q, blk);
                else
                    store_bytes(ob + q, blk, S - q);
            }
            if (lane == 0u && col[u] == 0u && e > 0u) store_bytes(ob, acc[r][u], e < S ? e : S);  // head
        }
    }
}

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

static const void* repair_mixed_plan_kernel(int r) {
    switch (r) {
        case 1: return reinterpret_cast<const void*>(&gf_repair_mixed_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_repair_mixed_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_repair_mixed_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_repair_mixed_plan<4>);
    }
    return nullptr;
}

uint32_t repair_plan_tile_bytes() { return (uint32_t)kUnalignedU * kUnalignedWindow; }

hipError_t launch_repair_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                    const uint32_t* pat_of, const uint32_t* pats, uint32_t* flags, int cus,
                                    hipStream_t stream) {
    const void* fn = repair_mixed_plan_kernel(r);
    if (!fn || k < 1 || k > kOddMaxK || cus < 1) return hipErrorInvalidValue;
    if (n_tiles == 0) return hipSuccess;
    static std::atomic<int> occ[kMaxR + 1] = {};  // blocks per CU, asked once per instance
    int per_cu = occ[r].load(std::memory_order_relaxed);
    if (per_cu == 0) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlockThreads, 0);
        if (e != hipSuccess) return e;
        occ[r].store(std::max(1, per_cu), std::memory_order_relaxed);
    }
    constexpr uint64_t wpb = kBlockThreads / 64;
    const uint64_t grid =
        std::max<uint64_t>(1, std::min<uint64_t>((n_tiles + wpb - 1) / wpb, (uint64_t)cus * std::max(1, per_cu)));
    void* args[] = {&recs, &tiles, &n_tiles, &pat_of, &pats, &k, &flags};
    return hipLaunchKernel(fn, dim3((uint32_t)grid), dim3(kBlockThreads), args, 0, stream);
}

}  // namespace hbec
