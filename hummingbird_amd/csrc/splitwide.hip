// splitwide.hip — hbec_split_plan_wide: the k + m shards of every entry of a plan
// of wide stripes (1 <= k <= 32 with 1 <= m <= 4: 16+4, 17+3, 20+4 and their
// like) from its object bytes in one launch: ecSplit's loop (ecutils.go:26-72),
// which hbec_split_plan runs above k = 12 as a copy per data shard, a memset per
// padded one and an apply in accumulate passes per entry.
//
// gf_split_wide_plan<M, ROWS> walks the plan's static {entry, tile} list
// grid-stride, one wave per tile of kUnalignedU windows, as gf_glue_wide_plan
// does (gluewide.hip); the record and the words are splitwide.h's.  A call has
// one pattern, the codec's encode rows, so the instance of the plan's own m is
// the only one launched.  The tile is neither split_tile (split_tile.h) nor
// glue_wide_tile:
//
//  * All M parity rows stay in registers across the k virtual inputs (input j is
//    the piece's bytes [j S, (j + 1) S)): every piece byte is read once, every
//    shard byte written once, nothing goes through memory twice.
//  * Three wave-uniform phases instead of a test per input (splitwide.h sw_cut).
//    Inputs [0, whole) are loaded, stored and multiplied with no pad mask in the
//    loop; the one partial input, if there is one, is loaded clamped and masked
//    (split_pad_mask); the inputs past it are ecSplit's pad alone: no load, no
//    table fetch, no multiply, zero stores to the data shard's part of the tile.
//  * The vector loads run D inputs ahead of the one in hand, in a ring of D + 1
//    register stages the loop is unrolled over, so no stage is ever moved.  The
//    input addresses are src + j S, plain arithmetic.  The partial input ends in
//    whichever stage whole % (D + 1) names; it is picked out once per tile by
//    wave-uniform selects, so its text exists once.
//  * The 5 M table words of input j + 1 come by wave-uniform scalar loads while
//    input j is multiplied (repairwide.hip says why not through LDS), and the
//    address of data shard j + 1, a scalar load on ROWS plans, is resolved there
//    too, an iteration before its store.
//  * Store before multiply: a window is realigned to the shard-position grid,
//    masked in the partial phase, stored to data shard j on that shard's own
//    residue and only then multiplied into the rows, so the destination-residue
//    block and its DPP neighbour are dead before selectors and products live.
//    The store block is made from the position-grid column, as split_store makes
//    it; making it from the loaded blocks by the combined shift was not tried.
//
// Every store follows split_tile.h's junction rule: a 16-B store only where the
// whole block lies inside its own shard's [0, S), head and tail bytewise through
// store_bytes, each output on its own residue.  Loads are clamped inside
// [src + j S, src + j S + V_j), aligned 16-B accesses only, so every block loaded
// holds a byte of the piece.  The upper half of a column is lane l + 1's block by
// a DPP move (lane_next4), and the products fold with xor3.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "kernels.h"
#include "shard_rows.h"
#include "split_tile.h"
#include "splitwide.h"
#include "unaligned_tile.h"

namespace hbec {

// inputs whose vector loads are in flight beside the one being multiplied
#ifndef HBEC_SW_DEPTH
#define HBEC_SW_DEPTH 2
#endif
constexpr int kSwDepth = HBEC_SW_DEPTH;  // M = 4 fits three waves per SIMD at two

__device__ __forceinline__ uint32_t sw_uniform(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }

// Columns v (shard positions [col, col + 16) per lane) of one live window to the
// shard of S bytes at ob; e = (16 - ob) & 15.  Wave-uniform call: every lane
// takes part in the lane move.
__device__ __forceinline__ void sw_store(uint64_t ob, uint32_t S, uint32_t e, const u32x4& v, uint32_t col,
                                         uint32_t lane) {
    const u32x4 blk = realign16(v, lane_next4(v), e);
    const uint32_t q = col + e;  // block start (shard position); ob + q is 16-B aligned
    if (lane < kUnalignedStoreLanes && q < S) {
        if (q + 16u <= S)
            st16_addr(ob + q, blk);
        else
            store_bytes(ob + q, blk, S - q);  // the tail: the block may hold the next shard's head
    }
    if (lane == 0u && col == 0u && e > 0u) store_bytes(ob, v, e < S ? e : S);  // head
}

// The same stores of a window that is ecSplit's pad throughout.
__device__ __forceinline__ void sw_store_zero(uint64_t ob, uint32_t S, uint32_t e, uint32_t col, uint32_t lane) {
    const u32x4 z = u32x4{0u, 0u, 0u, 0u};
    const uint32_t q = col + e;
    if (lane < kUnalignedStoreLanes && q < S) {
        if (q + 16u <= S)
            st16_addr(ob + q, z);
        else
            store_bytes(ob + q, z, S - q);
    }
    if (lane == 0u && col == 0u && e > 0u) store_bytes(ob, z, e < S ? e : S);
}

// One input in hand: its U windows `in` (aligned blocks, shift d) realigned,
// padded from position V on where PARTIAL, stored to the data shard at db and
// multiplied into the rows by the tables tb.  Every argument but in, acc and lane
// is wave-uniform.
template <int M, bool PARTIAL>
__device__ __forceinline__ void sw_input(u32x4 (&acc)[M][kUnalignedU], const u32x4 (&in)[kUnalignedU], uint32_t d,
                                         uint64_t db, uint32_t S, uint32_t V, uint32_t p0,
                                         const uint32_t (&tb)[M][5], uint32_t lane) {
    constexpr int U = kUnalignedU;
    constexpr uint32_t W = kUnalignedWindow;
    const uint32_t col0 = p0 + lane * 16u;
    const uint32_t de = sw_uniform((16u - (uint32_t)(db & 15u)) & 15u);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        u32x4 x = realign16(in[u], lane_next4(in[u]), d);
        if constexpr (PARTIAL) x = split_pad_mask(x, col0 + (uint32_t)u * W, V);  // the pad is zero
        if (p0 + (uint32_t)u * W < S) sw_store(db, S, de, x, col0 + (uint32_t)u * W, lane);  // window-uniform
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const Sel sx = selectors(x[q]);
#pragma unroll
            for (int r = 0; r < M; ++r)
                acc[r][u][q] = xor3(acc[r][u][q], perm(tb[r][1], tb[r][0], sx.s0), perm(tb[r][3], tb[r][2], sx.s1)) ^
                               perm(tb[r][4], tb[r][4], sx.s2);
        }
    }
}

// One wave tile: U windows from shard position p0 < S of one entry whose piece
// [src, src + len) passed split_len_ok.  p: the call's record (splitwide.h).
// Every argument but lane is wave-uniform.
template <int M, bool ROWS, int D>
__device__ __forceinline__ void split_wide_tile(uint32_t K, uint64_t a, uint64_t b, uint32_t S, uint32_t p0,
                                                uint64_t src, uint64_t len, const uint32_t* __restrict__ p,
                                                uint32_t lane) {
    constexpr int U = kUnalignedU;
    constexpr int NS = D + 1;  // ring stages: the input in hand and D in flight
    constexpr uint32_t W = kUnalignedWindow;
    auto shard = [=](uint32_t i) { return shard_at<ROWS>(a, b, (uint64_t)S, K, i); };
    const SwCut c = sw_cut(len, S, K);
    const uint32_t col0 = p0 + lane * 16u;  // shard positions are below S + one tile < 2^31

    u32x4 acc[M][U];
#pragma unroll
    for (int r = 0; r < M; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[r][u] = u32x4{0u, 0u, 0u, 0u};

    // stage j % NS holds input j < pad_from: its blocks and their shift
    u32x4 buf[NS][U];
    uint32_t bd[NS];
    auto fetch = [&](int s, uint32_t j) {
        const UView v = uview(src + (uint64_t)j * S, (uint64_t)(j < c.whole ? S : c.partial));
        bd[s] = v.d;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u32x4 hi;
            uload(buf[s][u], hi, v, (uint64_t)(col0 + (uint32_t)u * W));
        }
    };
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        bd[s] = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) buf[s][u] = u32x4{0u, 0u, 0u, 0u};
        if ((uint32_t)s < c.pad_from) fetch(s, (uint32_t)s);
    }
    // the tables and the data shard of the input in hand; those of the next one
    // are asked for while it is multiplied
    uint32_t tb[M][5];
#pragma unroll
    for (int r = 0; r < M; ++r)
#pragma unroll
        for (int z = 0; z < 5; ++z) tb[r][z] = p[kRwHdr + 5 * r + z];
    uint64_t db = shard(0u);

#pragma unroll 1
    for (uint32_t j0 = 0; j0 < c.whole; j0 += (uint32_t)NS) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uint32_t j = j0 + (uint32_t)s;
            if (j >= c.whole) break;  // wave-uniform
            const uint32_t jn = min(j + 1u, K - 1u);
            uint32_t tn[M][5];
#pragma unroll
            for (int r = 0; r < M; ++r)
#pragma unroll
                for (int z = 0; z < 5; ++z) tn[r][z] = p[kRwHdr + 5u * (jn * (uint32_t)M + (uint32_t)r) + (uint32_t)z];
            const uint64_t ndb = shard(jn);
            sw_input<M, false>(acc, buf[s], bd[s], db, S, S, p0, tb, lane);
            if (j + (uint32_t)NS < c.pad_from) fetch(s, j + (uint32_t)NS);
#pragma unroll
            for (int r = 0; r < M; ++r)
#pragma unroll
                for (int z = 0; z < 5; ++z) tb[r][z] = tn[r][z];
            db = ndb;
        }
    }

    // the partial input: tb and db are input `whole`'s already
    if (c.partial > 0u) {
        const uint32_t sd = c.whole % (uint32_t)NS;
        u32x4 in[U];
        uint32_t d = bd[0];
#pragma unroll
        for (int u = 0; u < U; ++u) in[u] = buf[0][u];
#pragma unroll
        for (int s = 1; s < NS; ++s)
            if (sd == (uint32_t)s) {  // wave-uniform
                d = bd[s];
#pragma unroll
                for (int u = 0; u < U; ++u) in[u] = buf[s][u];
            }
        sw_input<M, true>(acc, in, d, db, S, c.partial, p0, tb, lane);
    }

    // ecSplit's pad: whole data shards of zeros, this tile's part of each
    if (c.pad_from < K) {
        uint64_t zb = shard(c.pad_from);
#pragma unroll 1
        for (uint32_t j = c.pad_from; j < K; ++j) {
            const uint64_t nzb = shard(min(j + 1u, K - 1u));
            const uint32_t e = sw_uniform((16u - (uint32_t)(zb & 15u)) & 15u);
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (p0 + (uint32_t)u * W < S) sw_store_zero(zb, S, e, col0 + (uint32_t)u * W, lane);
            zb = nzb;
        }
    }

    // the parity shards, each on its own 16-B grid
#pragma unroll
    for (int r = 0; r < M; ++r) {
        const uint64_t ob = shard(K + (uint32_t)r);
        const uint32_t e = sw_uniform((16u - (uint32_t)(ob & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p0 + (uint32_t)u * W >= S) continue;  // window-uniform: every lane takes part in the lane move
            sw_store(ob, S, e, acc[r][u], col0 + (uint32_t)u * W, lane);
        }
    }
}

template <int M, bool ROWS>
__global__ __launch_bounds__(kBlockThreads) void gf_split_wide_plan(const MRec* __restrict__ recs,
                                                                    const MTile* __restrict__ tiles, uint32_t n_tiles,
                                                                    const uint32_t* __restrict__ words,
                                                                    const uint32_t* __restrict__ srcs,
                                                                    const uint32_t* __restrict__ pats, uint32_t K) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = words[e.rec];
        if (((w >> kRwOutShift) & 7u) != (uint32_t)M) continue;  // wave-uniform; 0: not this call's
        const uint32_t* sl = srcs + (size_t)e.rec * 4u;
        const uint64_t src = (uint64_t)sl[0] | ((uint64_t)sl[1] << 32);
        const uint64_t len = (uint64_t)sl[2] | ((uint64_t)sl[3] << 32);
        const uint32_t S = recs[e.rec].shard_len;
        const uint32_t p0 = e.ti * T;  // < S < 2^31
        if (p0 >= S || len == 0u) continue;  // never on a list and words the host built
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        split_wide_tile<M, ROWS, kSwDepth>(K, a, b, S, p0, src, len, pats, lane);
    }
}

template <bool ROWS>
static const void* split_wide_plan_kernel(int m) {
    switch (m) {
        case 1: return reinterpret_cast<const void*>(&gf_split_wide_plan<1, ROWS>);
        case 2: return reinterpret_cast<const void*>(&gf_split_wide_plan<2, ROWS>);
        case 3: return reinterpret_cast<const void*>(&gf_split_wide_plan<3, ROWS>);
        case 4: return reinterpret_cast<const void*>(&gf_split_wide_plan<4, ROWS>);
    }
    return nullptr;
}

// launch_plan_walk (planwalk.h) with this kernel's bound on k: one wave per
// tile, as many blocks as fit the device at most.
int launch_split_wide_plan(int k, int m, const MRec* recs, const MTile* tiles, uint32_t n_tiles, const uint32_t* words,
                           const uint32_t* srcs, const uint32_t* pats, int cus, void* stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = rows ? split_wide_plan_kernel<true>(m) : split_wide_plan_kernel<false>(m);
    if (!fn || k < 1 || k > kRwMaxK || cus < 1) return (int)hipErrorInvalidValue;
    if (n_tiles == 0) return (int)hipSuccess;
    int per_cu = occ[rows][m].load(std::memory_order_relaxed);
    if (per_cu == 0) {
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlockThreads, 0);
        if (e != hipSuccess) return (int)e;
        per_cu = std::max(1, per_cu);
        occ[rows][m].store(per_cu, std::memory_order_relaxed);
    }
    constexpr uint64_t wpb = kBlockThreads / 64;
    const uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>((n_tiles + wpb - 1) / wpb, (uint64_t)cus * per_cu));
    uint32_t kk = (uint32_t)k;
    void* args[] = {&recs, &tiles, &n_tiles, &words, &srcs, &pats, &kk};
    return (int)hipLaunchKernel(fn, dim3((uint32_t)grid), dim3(kBlockThreads), args, 0,
                                static_cast<hipStream_t>(stream));
}

}  // namespace hbec
