// gluewide.hip — hbec_glue_plan_wide: the object bytes of every entry of a plan
// of wide stripes (1 <= k <= 32: 16+4, 17+3, 20+4 and their like) from its
// shards, degraded or not, in one launch: ecGlue's loop (ecutils.go:134-186),
// which hbec_glue_plan_mixed runs above k = 12 as a copy per present data shard
// and an apply per degraded entry.
//
// gf_glue_wide_plan<RMAX, ROWS> walks the plan's static {entry, tile} list
// grid-stride, one wave per tile of kUnalignedU windows, as gf_repair_wide_plan
// does (repairwide.hip); records and words are that call's (gluewide.h).  A tile
// at or past min(S, len) is left before any shard byte is loaded: the list is the
// plan's, so the kernel makes glue_tile_needed's test itself.  Two tiles:
//
//  * r = 0, the healthy GET (and the ranged one that ends before the lost
//    shard): glue_wide_gather, a copy.  A run-time loop over the ceil(len / S)
//    data shards with a byte wanted, no tables, no accumulators, no selectors.
//    The loads of shard j are laid on the DESTINATION's 16-B grid: lane l of
//    window u loads the aligned source block that holds the first byte of
//    destination block dst + j S + e + p0 + u W + 16 l (e: the bytes up to the
//    first aligned destination block), so one realign16 with the wave-uniform
//    shift (src + p0 + e) & 15 turns a lane's block and lane l + 1's into the
//    16 bytes it stores, where a shard-position grid needs two (source residue
//    to shard position, shard position to destination residue).  The first e
//    bytes of a shard (tile 0 only) come from two wave-uniform loads of the
//    shard's first blocks, prefetched with the rest.  With no accumulators
//    there are registers to spare: kGwGatherDepth inputs are in flight (the
//    coded tile has kGwDepth beside the one in hand), kept in a ring of register
//    stages the loop is unrolled over, so no stage is ever moved.
//  * r >= 1: glue_wide_tile<R>.  All r decode rows stay in registers across the
//    k survivors: every survivor byte is read once.  Columns are on the shard
//    position grid (the rows accumulate over inputs of different residues).  A
//    survivor that is a data shard is stored to dst + idx S inside the loop,
//    while its columns are in registers and BEFORE they are multiplied: the
//    realigned block and its DPP neighbour die at the store, so they never live
//    beside the selectors and products, which is what took glue_tile<4> to 256
//    VGPRs.  The r rebuilt shards are stored after the loop.  Table words come by
//    wave-uniform scalar loads one input ahead and the address of input
//    j + kGwDepth + 1 is resolved an iteration early, as in repair_wide_tile.
//
// Every store follows glue_tile.h's junction rule: output shards lie back to
// back, so a 16-B store is made only where the whole block lies inside its own
// shard's [0, V), V = clamp(len - idx S, 0, S); heads and tails go bytewise, each
// output on its own residue.  Loads are clamped inside [shard, shard + min(S,
// len)), aligned 16-B accesses only.  The upper half of a column is lane l + 1's
// block by a DPP move (lane_next4), and the products fold with xor3.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "gluewide.h"
#include "kernels.h"
#include "shard_rows.h"
#include "unaligned_tile.h"

namespace hbec {

// coded tile: inputs whose vector loads are in flight beside the one being multiplied
#ifndef HBEC_GW_DEPTH
#define HBEC_GW_DEPTH 2
#endif
// gather: shards in flight, the one being stored included
#ifndef HBEC_GW_GATHER_DEPTH
#define HBEC_GW_GATHER_DEPTH 4
#endif
constexpr int kGwDepth = HBEC_GW_DEPTH;
constexpr int kGwGatherDepth = HBEC_GW_GATHER_DEPTH;
static_assert(kGwGatherDepth >= kGwDepth + 1, "the gather prefetches at least as deep as the coded tile");

__device__ __forceinline__ uint32_t gw_uniform(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }

// Bytes of data shard i inside the first len bytes of D: clamp(len - i S, 0, S).
__device__ __forceinline__ uint32_t gw_valid(uint64_t len, uint32_t i, uint32_t S) {
    const uint64_t off = (uint64_t)i * S;  // i < 32, S < 2^31
    return len <= off ? 0u : (len - off < (uint64_t)S ? (uint32_t)(len - off) : S);
}

// Columns v (shard positions [col, col + 16) per lane) of one window to the
// shard at ob, of which V bytes are wanted; e = (16 - ob) & 15.  Wave-uniform
// call: every lane takes part in the lane move.
__device__ __forceinline__ void gw_store(uint64_t ob, uint32_t V, uint32_t e, const u32x4& v, uint32_t col,
                                         uint32_t lane) {
    const u32x4 blk = realign16(v, lane_next4(v), e);
    const uint32_t q = col + e;  // block start (shard position); ob + q is 16-B aligned
    if (lane < kUnalignedStoreLanes && q < V) {
        if (q + 16u <= V)
            st16_addr(ob + q, blk);
        else
            store_bytes(ob + q, blk, V - q);  // the tail: the block may hold the next shard's head
    }
    if (lane == 0u && col == 0u && e > 0u) store_bytes(ob, v, e < V ? e : V);  // head
}

// r = 0: data shards 0 .. ceil(len / S) - 1 copied to dst, the tile's part of
// each.  Sr = min(S, len) > p0.  Every argument is wave-uniform.
template <bool ROWS>
__device__ __forceinline__ void glue_wide_gather(uint32_t K, uint64_t a, uint64_t b, uint32_t S, uint32_t Sr,
                                                 uint32_t p0, uint64_t dst, uint64_t len, uint32_t lane) {
    constexpr int U = kUnalignedU;
    constexpr int D = kGwGatherDepth;
    constexpr uint32_t W = kUnalignedWindow;
    const bool first = p0 == 0u;  // the tile that writes the heads
    auto shard = [=](uint32_t i) { return shard_at<ROWS>(a, b, (uint64_t)S, K, i); };
    auto wanted = [=](uint32_t j) { return j < K && (uint64_t)j * S < len; };

    // one ring stage per shard in flight; everything but buf and hd is in SGPRs
    u32x4 buf[D][U], hd[D][2];
    uint64_t ob[D];                  // dst + j S
    uint32_t e[D], sh[D], hs[D];     // (16 - ob) & 15; the blocks' shift; the shard's own residue
    auto fetch = [&](int d, uint32_t j, uint64_t src) {
        ob[d] = dst + (uint64_t)j * S;
        e[d] = gw_uniform((16u - (uint32_t)(ob[d] & 15u)) & 15u);
        const uint64_t s0 = src + p0 + e[d];  // source of the tile's first destination block
        const uint64_t base = s0 & ~(uint64_t)15, last = (src + Sr - 1u) & ~(uint64_t)15;
        sh[d] = gw_uniform((uint32_t)(s0 & 15u));
        hs[d] = gw_uniform((uint32_t)(src & 15u));
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t x = base + (uint32_t)u * W + lane * 16u;
            buf[d][u] = ld16_addr(x < last ? x : last);
        }
        if (first) {  // shard bytes [0, 16): the same two blocks for every lane
            const uint64_t h = src & ~(uint64_t)15;
            hd[d][0] = ld16_addr(h);
            hd[d][1] = ld16_addr(h < last ? h + 16u : last);
        }
    };
    auto store = [&](int d, uint32_t j) {
        const uint32_t V = gw_valid(len, j, S);  // > 0: the shard is wanted
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t q0 = p0 + (uint32_t)u * W + e[d];
            if (q0 >= V) continue;  // window-uniform: every lane takes part in the lane move
            const u32x4 blk = realign16(buf[d][u], lane_next4(buf[d][u]), sh[d]);
            const uint32_t q = q0 + lane * 16u;  // block start (shard position); ob + q is 16-B aligned
            if (lane < kUnalignedStoreLanes && q < V) {
                if (q + 16u <= V)
                    st16_addr(ob[d] + q, blk);
                else
                    store_bytes(ob[d] + q, blk, V - q);
            }
        }
        if (first && e[d] > 0u) {
            const u32x4 x = realign16(hd[d][0], hd[d][1], hs[d]);
            if (lane == 0u) store_bytes(ob[d], x, e[d] < V ? e[d] : V);
        }
    };

    // nsrc: the address of the shard fetched next, resolved one step early (a
    // scalar load on ROWS plans); the row index stays inside the row
    uint64_t nsrc = shard(0u);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        if (wanted((uint32_t)d)) fetch(d, (uint32_t)d, nsrc);
        nsrc = shard(min((uint32_t)d + 1u, K - 1u));
    }
#pragma unroll 1
    for (uint32_t j0 = 0; wanted(j0); j0 += (uint32_t)D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const uint32_t j = j0 + (uint32_t)d;
            if (!wanted(j)) break;  // wave-uniform
            store(d, j);
            if (wanted(j + (uint32_t)D)) fetch(d, j + (uint32_t)D, nsrc);
            nsrc = shard(min(j + (uint32_t)D + 1u, K - 1u));
        }
    }
}

// r = R >= 1: the R missing data shards coded from the K survivors of the record
// p (gluewide.h) and written with the surviving data shards.  Sr = min(S, len) >
// p0.  Every argument is wave-uniform.
template <int R, bool ROWS>
__device__ __forceinline__ void glue_wide_tile(uint32_t K, uint64_t a, uint64_t b, uint32_t S, uint32_t Sr,
                                               uint32_t p0, uint64_t dst, uint64_t len,
                                               const uint32_t* __restrict__ p, uint32_t lane) {
    constexpr int U = kUnalignedU;
    constexpr int D = kGwDepth;
    constexpr uint32_t W = kUnalignedWindow;
    auto shard = [=](uint32_t i) { return shard_at<ROWS>(a, b, (uint64_t)S, K, i); };
    // survivor j < K <= 32: a byte of words 0..7
    auto surv = [=](uint32_t j) { return (p[j >> 2] >> (8u * (j & 3u))) & 0xFFu; };
    const uint32_t row_idx = p[kRwRowsWord];
    const uint32_t col0 = p0 + lane * 16u;  // shard positions are below S + one tile < 2^31
    auto load = [&](u32x4 (&x)[U], const UView& v) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u32x4 hi;
            uload(x[u], hi, v, (uint64_t)(col0 + (uint32_t)u * W));
        }
    };

    u32x4 acc[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[r][u] = u32x4{0u, 0u, 0u, 0u};

    // inputs j .. j + D - 1 in buf (their shard indices in bi), index and address
    // of input j + D in ni / nb, the tables of input j in tb.  Past the last input
    // the loads repeat it (K < D only).
    u32x4 buf[D][U];
    UView bv[D];
    uint32_t bi[D];
    uint32_t ni = surv(0u);
    uint64_t nb = shard(ni);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        bv[d] = uview(nb, (uint64_t)Sr);
        bi[d] = ni;
        load(buf[d], bv[d]);
        ni = surv(min((uint32_t)d + 1u, K - 1u));
        nb = shard(ni);
    }
    uint32_t tb[R][5];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < 5; ++q) tb[r][q] = p[kRwHdr + 5 * r + q];

#pragma unroll 1
    for (uint32_t j = 0; j < K; ++j) {
        const bool more = j + (uint32_t)D < K;
        u32x4 nx[U];
        UView nv = bv[D - 1];
        uint32_t nidx = bi[D - 1];
        if (more) {
            nv = uview(nb, (uint64_t)Sr);
            nidx = ni;
            load(nx, nv);
        }
        ni = surv(min(j + (uint32_t)D + 1u, K - 1u));
        nb = shard(ni);
        const uint32_t jn = min(j + 1u, K - 1u);
        uint32_t tn[R][5];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < 5; ++q) tn[r][q] = p[kRwHdr + 5u * (jn * (uint32_t)R + (uint32_t)r) + (uint32_t)q];
        // a surviving data shard goes to the object as it is (wave-uniform)
        const uint32_t ci = bi[0];
        const uint32_t pv = ci < K ? gw_valid(len, ci, S) : 0u;
        const uint64_t pb = dst + (uint64_t)ci * S;
        const uint32_t pe = gw_uniform((16u - (uint32_t)(pb & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32x4 x = realign16(buf[0][u], lane_next4(buf[0][u]), bv[0].d);
            if (p0 + (uint32_t)u * W < pv) gw_store(pb, pv, pe, x, col0 + (uint32_t)u * W, lane);  // window-uniform
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const Sel sx = selectors(x[q]);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    acc[r][u][q] = xor3(acc[r][u][q], perm(tb[r][1], tb[r][0], sx.s0), perm(tb[r][3], tb[r][2], sx.s1)) ^
                                   perm(tb[r][4], tb[r][4], sx.s2);
            }
        }
#pragma unroll
        for (int d = 0; d + 1 < D; ++d) {
#pragma unroll
            for (int u = 0; u < U; ++u) buf[d][u] = buf[d + 1][u];
            bv[d] = bv[d + 1];
            bi[d] = bi[d + 1];
        }
        if (more) {
#pragma unroll
            for (int u = 0; u < U; ++u) buf[D - 1][u] = nx[u];
            bv[D - 1] = nv;
            bi[D - 1] = nidx;
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < 5; ++q) tb[r][q] = tn[r][q];
    }

    // the rebuilt data shards, each on its own 16-B grid, clipped at its own V
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t i = (row_idx >> (8 * r)) & 0xFFu;
        const uint32_t ov = gw_valid(len, i, S);
        if (ov == 0u) continue;  // wave-uniform
        const uint64_t ob = dst + (uint64_t)i * S;
        const uint32_t e = gw_uniform((16u - (uint32_t)(ob & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p0 + (uint32_t)u * W >= ov) continue;  // window-uniform: every lane takes part in the lane move
            gw_store(ob, ov, e, acc[r][u], col0 + (uint32_t)u * W, lane);
        }
    }
}

// RMAX: the largest count of missing data shards among the call's words.  One
// launch serves every count up to it (a wave-uniform branch to that count's
// tile), for the reason written at gf_mixed_plan.
template <int RMAX, bool ROWS>
__global__ __launch_bounds__(kBlockThreads) void gf_glue_wide_plan(const MRec* __restrict__ recs,
                                                                   const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                                   const uint32_t* __restrict__ words,
                                                                   const uint32_t* __restrict__ dsts,
                                                                   const uint32_t* __restrict__ pats, uint32_t stride,
                                                                   uint32_t K) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = words[e.rec];
        if (w == 0u) continue;  // not this call's: zero length, or nothing asked for
        const uint32_t r = (w >> kRwOutShift) & 7u;  // wave-uniform
        if (r > (uint32_t)RMAX) continue;
        const uint32_t* dl = dsts + (size_t)e.rec * 4u;
        const uint64_t dst = (uint64_t)dl[0] | ((uint64_t)dl[1] << 32);
        const uint64_t len = (uint64_t)dl[2] | ((uint64_t)dl[3] << 32);
        const uint32_t S = recs[e.rec].shard_len;
        const uint32_t Sr = len < (uint64_t)S ? (uint32_t)len : S;  // the shard positions anyone needs
        const uint32_t p0 = e.ti * T;                                // < S < 2^31
        if (p0 >= Sr) continue;  // nothing of this tile is wanted: no load
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint32_t* p = pats + (size_t)(w & kRwPatMask) * stride;
        if (r == 0u) glue_wide_gather<ROWS>(K, a, b, S, Sr, p0, dst, len, lane);
        if constexpr (RMAX >= 1)
            if (r == 1u) glue_wide_tile<1, ROWS>(K, a, b, S, Sr, p0, dst, len, p, lane);
        if constexpr (RMAX >= 2)
            if (r == 2u) glue_wide_tile<2, ROWS>(K, a, b, S, Sr, p0, dst, len, p, lane);
        if constexpr (RMAX >= 3)
            if (r == 3u) glue_wide_tile<3, ROWS>(K, a, b, S, Sr, p0, dst, len, p, lane);
        if constexpr (RMAX >= 4)
            if (r == 4u) glue_wide_tile<4, ROWS>(K, a, b, S, Sr, p0, dst, len, p, lane);
    }
}

template <bool ROWS>
static const void* glue_wide_plan_kernel(int r) {
    switch (r) {
        case 0: return reinterpret_cast<const void*>(&gf_glue_wide_plan<0, ROWS>);
        case 1: return reinterpret_cast<const void*>(&gf_glue_wide_plan<1, ROWS>);
        case 2: return reinterpret_cast<const void*>(&gf_glue_wide_plan<2, ROWS>);
        case 3: return reinterpret_cast<const void*>(&gf_glue_wide_plan<3, ROWS>);
        case 4: return reinterpret_cast<const void*>(&gf_glue_wide_plan<4, ROWS>);
    }
    return nullptr;
}

// launch_plan_walk (planwalk.h) with this kernel's bound on k: one wave per
// tile, as many blocks as fit the device at most.
int launch_glue_wide_plan(int k, int rmax, uint32_t stride, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                          const uint32_t* words, const uint32_t* dsts, const uint32_t* pats, int cus, void* stream,
                          bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = rows ? glue_wide_plan_kernel<true>(rmax) : glue_wide_plan_kernel<false>(rmax);
    if (!fn || k < 1 || k > kRwMaxK || cus < 1 || stride < gw_stride(k, rmax)) return (int)hipErrorInvalidValue;
    if (n_tiles == 0) return (int)hipSuccess;
    int per_cu = occ[rows][rmax].load(std::memory_order_relaxed);
    if (per_cu == 0) {
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlockThreads, 0);
        if (e != hipSuccess) return (int)e;
        per_cu = std::max(1, per_cu);
        occ[rows][rmax].store(per_cu, std::memory_order_relaxed);
    }
    constexpr uint64_t wpb = kBlockThreads / 64;
    const uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>((n_tiles + wpb - 1) / wpb, (uint64_t)cus * per_cu));
    uint32_t kk = (uint32_t)k;
    void* args[] = {&recs, &tiles, &n_tiles, &words, &dsts, &pats, &stride, &kk};
    return (int)hipLaunchKernel(fn, dim3((uint32_t)grid), dim3(kBlockThreads), args, 0,
                                static_cast<hipStream_t>(stream));
}

}  // namespace hbec
