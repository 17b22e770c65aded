// repairwide.hip — hbec_repair_plan_wide: the missing shards of every stripe of
// a plan rebuilt and its surplus ones checked in one launch for 1 <= k <= 32
// (16+4, 17+3, 20+4 and their like), which hbec_repair_plan_mixed codes one
// stripe at a time in accumulate passes of twelve inputs.
//
// gf_repair_wide_plan<AMAX, ROWS> walks the plan's static {entry, tile} list
// grid-stride, one wave per tile of kUnalignedU windows, as gf_repair_mixed_plan
// does (repair.hip).  What differs is the tile:
//  * Records (repairwide.h) hold 32 survivors and lie one stride apart; the
//    entry's word names its record by position.
//  * One tile per row total A = r_o + r_c, not per (r_o, r_c) pair.  Which rows
//    are rebuilt is a wave-uniform count looked at before and after the multiply
//    loop only: a row below r_o starts at zero and is stored, a row from r_o on
//    starts as its stored column and must end at zero.  The loop is the same for
//    both, so an instance carries A tile bodies where the pair scheme carries
//    A (A + 3) / 2, and a 32-input loop stays in the instruction cache.
//  * All A rows stay in registers across the k survivors: every survivor byte
//    is read once, every output byte written once, nothing goes through memory.
//  * The pipeline is three deep in scalar terms and kRwDepth deep in vector
//    terms.  While input j is multiplied, the vector loads of inputs j + 1 ..
//    j + kRwDepth are in flight, the address of input j + kRwDepth + 1 is being
//    resolved (its survivor byte, and for ROWS its row entry: two dependent
//    scalar loads) and the 5 A table words of input j + 1 are being fetched, so
//    no iteration waits on a scalar load it issued itself.  The tables come by
//    wave-uniform scalar loads: the four waves of a block work on different
//    entries, so a pattern staged in LDS would be staged per wave and read back
//    through the LDS pipe into VGPRs, where the scalar cache hands a record that
//    neighbouring tiles share to v_perm's SGPR operand directly.
//  * The upper half of a lane's column is lane l + 1's block by a DPP move
//    (gf_device.h lane_next4), not a bpermute through the LDS pipe; a mismatch
//    is one atomic per wave, and the three products of a byte fold into the row
//    with a v_bitop3 and a v_xor.
// Addressing is unaligned_tile.h's: aligned 16-B accesses only, clamped loads,
// bytewise head and tail.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "kernels.h"
#include "repairwide.h"
#include "shard_rows.h"
#include "unaligned_tile.h"

namespace hbec {

// inputs whose vector loads are in flight beside the one being multiplied
#ifndef HBEC_RW_DEPTH
#define HBEC_RW_DEPTH 2
#endif
constexpr int kRwDepth = HBEC_RW_DEPTH;

// One tile of a stripe with A rows, the first `ro` of them rebuilt.  Every
// capture is a value in SGPRs.  `zero` is the entry record's pad word (0 in
// every record): see repair_tile.h for why the rebuilt rows start from it.
template <int A, bool ROWS>
__device__ __forceinline__ void repair_wide_tile(uint32_t K, uint32_t ro, uint64_t a, uint64_t b, uint64_t S,
                                                 uint32_t p0, const uint32_t* __restrict__ p, uint32_t lane,
                                                 uint32_t* flag, uint32_t zero) {
    constexpr int U = kUnalignedU;
    constexpr int D = kRwDepth;
    constexpr uint32_t W = kUnalignedWindow;
    auto shard = [=](uint32_t i) { return shard_at<ROWS>(a, b, S, K, i); };
    // survivor j < K <= 32: a byte of words 0..7
    auto in_base = [=](uint32_t j) { return shard((p[j >> 2] >> (8u * (j & 3u))) & 0xFFu); };
    const uint32_t row_idx = p[kRwRowsWord];
    auto row_base = [=](int r) { return shard((row_idx >> (8 * r)) & 0xFFu); };
    // shard positions are below S + one tile < 2^31 (kPos32MaxShard)
    const uint32_t col0 = p0 + lane * 16u;
    auto col = [=](int u) { return (uint64_t)(col0 + (uint32_t)u * W); };
    auto load = [&](u32x4 (&x)[U], const UView& v) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u32x4 hi;
            uload(x[u], hi, v, col(u));
        }
    };

    u32x4 acc[A][U];
#pragma unroll
    for (int r = 0; r < A; ++r) {
        if ((uint32_t)r < ro) {  // wave-uniform
#pragma unroll
            for (int u = 0; u < U; ++u) acc[r][u] = u32x4{zero, zero, zero, zero};
        } else {
            const UView ov = uview(row_base(r), S);
            u32x4 st[U];
            load(st, ov);
#pragma unroll
            for (int u = 0; u < U; ++u) acc[r][u] = realign16(st[u], lane_next4(st[u]), ov.d);
        }
    }

    // inputs j .. j + D - 1 in buf, the address of input j + D in nb, the tables
    // of input j in tb.  Past the last input the loads repeat it (K < D only).
    u32x4 buf[D][U];
    UView bv[D];
    uint64_t nb = in_base(0);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        bv[d] = uview(nb, S);
        load(buf[d], bv[d]);
        nb = in_base(min((uint32_t)d + 1u, K - 1u));
    }
    uint32_t tb[A][5];
#pragma unroll
    for (int r = 0; r < A; ++r)
#pragma unroll
        for (int q = 0; q < 5; ++q) tb[r][q] = p[kRwHdr + 5 * r + q];

#pragma unroll 1
    for (uint32_t j = 0; j < K; ++j) {
        const bool more = j + (uint32_t)D < K;
        u32x4 nx[U];
        UView nv = bv[D - 1];
        if (more) {
            nv = uview(nb, S);
            load(nx, nv);
        }
        nb = in_base(min(j + (uint32_t)D + 1u, K - 1u));
        const uint32_t jn = min(j + 1u, K - 1u);
        uint32_t tn[A][5];
#pragma unroll
        for (int r = 0; r < A; ++r)
#pragma unroll
            for (int q = 0; q < 5; ++q) tn[r][q] = p[kRwHdr + 5u * (jn * (uint32_t)A + (uint32_t)r) + (uint32_t)q];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32x4 x = realign16(buf[0][u], lane_next4(buf[0][u]), bv[0].d);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const Sel sx = selectors(x[e]);
#pragma unroll
                for (int r = 0; r < A; ++r)
                    acc[r][u][e] = xor3(acc[r][u][e], perm(tb[r][1], tb[r][0], sx.s0), perm(tb[r][3], tb[r][2], sx.s1)) ^
                                   perm(tb[r][4], tb[r][4], sx.s2);
            }
        }
#pragma unroll
        for (int d = 0; d + 1 < D; ++d) {
#pragma unroll
            for (int u = 0; u < U; ++u) buf[d][u] = buf[d + 1][u];
            bv[d] = bv[d + 1];
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) buf[D - 1][u] = nx[u];
            bv[D - 1] = nv;
        }
#pragma unroll
        for (int r = 0; r < A; ++r)
#pragma unroll
            for (int q = 0; q < 5; ++q) tb[r][q] = tn[r][q];
    }

    // checked rows: columns [c, c + 16) of the window's first 62 lanes; bytes at
    // or past S and windows that start there do not count
    uint32_t diff = 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint64_t c = col(u);
        const uint64_t nbytes = c < S ? S - c : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t b0 = 4u * e;
            const uint32_t mask =
                nbytes >= b0 + 4u ? 0xFFFFFFFFu : (nbytes <= b0 ? 0u : (0xFFFFFFFFu >> (8u * (uint32_t)(b0 + 4u - nbytes))));
#pragma unroll
            for (int r = 0; r < A; ++r)
                if ((uint32_t)r >= ro) diff |= acc[r][u][e] & mask;
        }
    }
    const bool bad = __ballot(lane < kUnalignedStoreLanes && diff != 0u) != 0ull;
    if (bad && lane == 0u) atomicOr(flag, 1u);

    // rebuilt rows: unaligned_tile's stores, on each output's own 16-B grid
#pragma unroll
    for (int r = 0; r < A; ++r) {
        if ((uint32_t)r >= ro) continue;  // wave-uniform: every lane takes part in the lane moves
        const uint64_t ob = row_base(r);
        const uint32_t e = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(ob & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if ((uint64_t)p0 + (uint64_t)u * W >= S) continue;  // window-uniform
            const u32x4 blk = realign16(acc[r][u], lane_next4(acc[r][u]), e);
            const uint64_t q = col(u) + e;  // block start (shard position); ob + q is 16-B aligned
            if (lane < kUnalignedStoreLanes && q < S) {
                if (q + 16u <= S)
                    st16_addr(ob + q, blk);
                else
                    store_bytes(ob + q, blk, S - q);
            }
            if (lane == 0u && col0 == 0u && u == 0 && e > 0u) store_bytes(ob, acc[r][u], e < S ? e : S);  // head
        }
    }
}

// AMAX: the largest row total among the call's entries.  One launch serves
// every total up to it, for the reason written at gf_mixed_plan.
template <int AMAX, bool ROWS>
__global__ __launch_bounds__(kBlockThreads) void gf_repair_wide_plan(const MRec* __restrict__ recs,
                                                                     const MTile* __restrict__ tiles,
                                                                     uint32_t n_tiles,
                                                                     const uint32_t* __restrict__ words,
                                                                     const uint32_t* __restrict__ pats,
                                                                     uint32_t stride, uint32_t K, uint32_t* flags) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = words[e.rec];
        if (w == 0u) continue;  // no tiles in this call
        const uint32_t ro = (w >> kRwOutShift) & 7u, rc = (w >> kRwChkShift) & 7u;  // wave-uniform
        // exactly k present: nothing to check, said once per entry
        if (rc == 0u && e.ti == 0u && lane == 0u) atomicOr(flags + e.rec, 2u);
        const uint32_t rows = ro + rc;
        if (rows == 0u || rows > (uint32_t)AMAX) continue;
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t zero = recs[e.rec].pad_;
        const uint32_t* p = pats + (size_t)(w & kRwPatMask) * stride;
        const uint32_t p0 = e.ti * T;
        uint32_t* flag = flags + e.rec;
        if (rows == 1u) repair_wide_tile<1, ROWS>(K, ro, a, b, S, p0, p, lane, flag, zero);
        if constexpr (AMAX >= 2)
            if (rows == 2u) repair_wide_tile<2, ROWS>(K, ro, a, b, S, p0, p, lane, flag, zero);
        if constexpr (AMAX >= 3)
            if (rows == 3u) repair_wide_tile<3, ROWS>(K, ro, a, b, S, p0, p, lane, flag, zero);
        if constexpr (AMAX >= 4)
            if (rows == 4u) repair_wide_tile<4, ROWS>(K, ro, a, b, S, p0, p, lane, flag, zero);
    }
}

template <bool ROWS>
static const void* repair_wide_plan_kernel(int a) {
    switch (a) {
        case 1: return reinterpret_cast<const void*>(&gf_repair_wide_plan<1, ROWS>);
        case 2: return reinterpret_cast<const void*>(&gf_repair_wide_plan<2, ROWS>);
        case 3: return reinterpret_cast<const void*>(&gf_repair_wide_plan<3, ROWS>);
        case 4: return reinterpret_cast<const void*>(&gf_repair_wide_plan<4, ROWS>);
    }
    return nullptr;
}

// launch_plan_walk (planwalk.h) with this kernel's bound on k: one wave per
// tile, as many blocks as fit the device at most.
hipError_t launch_repair_wide_plan(int k, int a, uint32_t stride, const MRec* recs, const MTile* tiles,
                                   uint32_t n_tiles, const uint32_t* words, const uint32_t* pats, uint32_t* flags,
                                   int cus, hipStream_t stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = rows ? repair_wide_plan_kernel<true>(a) : repair_wide_plan_kernel<false>(a);
    if (!fn || k < 1 || k > kRwMaxK || cus < 1 || stride < rw_record_words(k, a)) return hipErrorInvalidValue;
    if (n_tiles == 0) return hipSuccess;
    int per_cu = occ[rows][a].load(std::memory_order_relaxed);
    if (per_cu == 0) {
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlockThreads, 0);
        if (e != hipSuccess) return e;
        per_cu = std::max(1, per_cu);
        occ[rows][a].store(per_cu, std::memory_order_relaxed);
    }
    constexpr uint64_t wpb = kBlockThreads / 64;
    const uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>((n_tiles + wpb - 1) / wpb, (uint64_t)cus * per_cu));
    uint32_t kk = (uint32_t)k;
    void* args[] = {&recs, &tiles, &n_tiles, &words, &pats, &stride, &kk, &flags};
    return hipLaunchKernel(fn, dim3((uint32_t)grid), dim3(kBlockThreads), args, 0, stream);
}

}  // namespace hbec
