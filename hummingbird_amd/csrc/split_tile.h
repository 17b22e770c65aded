// split_tile.h — the wave tile of gf_split_plan (splitplan.hip): one entry's
// k data shards cut out of its object piece [src, src + len) and its R = m
// parity shards coded from them, every shard written whole (ecSplit,
// ecutils.go:26-72).  It is unaligned_tile's loop (unaligned_tile.h; its views,
// clamped loads and bytewise store are used as they stand) with four
// differences:
//   1. Input j is no stored shard but the virtual one at src + j S, of which
//      V_j = clamp(len - j S, 0, S) bytes exist.  Its loads are clamped inside
//      [src + j S, src + j S + V_j), so every 16-B block loaded holds a byte of
//      the piece; an input with V_j = 0 is not loaded and counts as zero.
//   2. Where V_j < S (wave-uniform) the realigned column's bytes at shard
//      positions >= V_j are zeroed per lane: ecSplit's pad (:51-54).  This is
//      done before the column is stored and before it is multiplied, so what
//      lies behind the piece never reaches a shard.
//   3. Inside the j loop the column is stored to data shard j at that shard's
//      own residue.
//   4. R may be 0 (m = 0): nothing is coded and the tile is a scatter.
// Positions at or past S of a column (the next virtual shard's bytes) are
// computed with and never stored, as in unaligned_tile.
//
// The junction.  The data shards of a databuf lie back to back, so whenever S
// is no multiple of 16 the last 16-B block of one and the first of the next
// are the same block, written by different waves (or by one wave at different
// times).  A 16-B store is therefore made only where the whole block lies
// inside its own shard's [0, S); the head (up to the first aligned block) and
// the tail (the block holding S) go bytewise through store_bytes, exactly as
// unaligned_tile and glue_tile write the head and tail of a shard.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.h"
#include "kernels.h"
#include "mixedplan.h"
#include "shard_rows.h"
#include "unaligned_tile.h"

namespace hbec {

// Columns v (shard positions [col, col + 16) per lane) of one live window to
// the shard of S bytes at ob.  Wave-uniform call: every lane takes part in the
// shuffle.
__device__ __forceinline__ void split_store(uint64_t ob, uint64_t S, uint32_t e, const u32x4& v, uint64_t col,
                                            uint32_t lane) {
    u32x4 nb;
#pragma unroll
    for (int i = 0; i < 4; ++i) nb[i] = __shfl_down(v[i], 1u, 64);
    const u32x4 blk = realign16(v, nb, e);
    const uint64_t q = col + e;  // block start (shard position); ob + q is 16-B aligned
    if (lane < kUnalignedStoreLanes && q < S) {
        if (q + 16u <= S)
            st16_addr(ob + q, blk);
        else
            store_bytes(ob + q, blk, S - q);  // the tail: the block may hold the next shard's head
    }
    if (lane == 0u && col == 0u && e > 0u) store_bytes(ob, v, e < S ? e : S);  // head
}

// The bytes of column x (shard positions [col, col + 16)) below position V; the
// others zero.
__device__ __forceinline__ u32x4 split_pad_mask(const u32x4& x, uint64_t col, uint64_t V) {
    const uint32_t nv = col < V ? (uint32_t)(V - col < 16u ? V - col : 16u) : 0u;
    u32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t b0 = 4u * e;
        const uint32_t mask = nv >= b0 + 4u ? 0xFFFFFFFFu : (nv <= b0 ? 0u : (0xFFFFFFFFu >> (8u * (b0 + 4u - nv))));
        y[e] = x[e] & mask;
    }
    return y;
}

// One wave tile: U windows from shard position p0 < S of one entry.  p: the
// call's pattern record (mixedplan.h mp_pattern: survivors 0..k-1, outputs
// k..k+R-1, then the tables of parity rows k..k+R-1); the tile reads the
// tables alone, since input j is data shard j and output r shard k + r.  Every
// argument is wave-uniform.  U: the windows coded together, kUnalignedU (the
// list's tile) or a part of it (splitplan.hip codes R = 4 in two halves).
template <int R, bool ROWS, int U = kUnalignedU>
__device__ __forceinline__ void split_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0, uint64_t src,
                                           uint64_t len, const uint32_t* __restrict__ p, uint32_t lane) {
    constexpr uint32_t W = kUnalignedWindow;
    constexpr int RA = R > 0 ? R : 1;
    const uint32_t k = (uint32_t)K;
    // bytes of virtual shard i inside the piece: clamp(len - i S, 0, S)
    auto valid = [=](uint32_t i) {
        const uint64_t off = (uint64_t)i * S;  // i < k <= 12, S < 2^31
        return len <= off ? (uint64_t)0 : (len - off < S ? len - off : S);
    };

    uint64_t col[U];
    bool live[U];  // window-uniform
#pragma unroll
    for (int u = 0; u < U; ++u) {
        col[u] = p0 + (uint64_t)u * W + lane * 16u;
        live[u] = p0 + (uint64_t)u * W < S;
    }
    u32x4 acc[RA][U];
#pragma unroll
    for (int r = 0; r < RA; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[r][u] = u32x4{0, 0, 0, 0};
    u32x4 clo[U], chi[U];
    uint64_t cV = valid(0u);  // > 0: the piece is not empty
    UView cv = uview(src, cV);
#pragma unroll
    for (int u = 0; u < U; ++u) uload(clo[u], chi[u], cv, col[u]);  // clamped: no branch
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
        u32x4 nlo[U], nhi[U];
        UView nv = cv;
        uint64_t nV = cV;
        if (j + 1 < K) {
            nV = valid((uint32_t)j + 1u);
            nv = uview(src + (uint64_t)(j + 1) * S, nV);
            if (nV > 0u) {  // wave-uniform
#pragma unroll
                for (int u = 0; u < U; ++u) uload(nlo[u], nhi[u], nv, col[u]);
            } else {  // all pad: nothing of the piece is there to load
#pragma unroll
                for (int u = 0; u < U; ++u) nlo[u] = nhi[u] = u32x4{0, 0, 0, 0};
            }
        }
        uint32_t tb[RA][5];
        if constexpr (R > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int q = 0; q < 5; ++q) tb[r][q] = (p + kMPatHdr + 5 * (j * R + r))[q];
        }
        const uint64_t db = shard_at<ROWS>(a, b, S, k, (uint32_t)j);  // data shard j
        const uint32_t de = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(db & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u32x4 x = realign16(clo[u], upper(clo[u], chi[u]), cv.d);
            if (cV < S) x = split_pad_mask(x, col[u], cV);  // wave-uniform: the pad is zero
            if constexpr (R > 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const Sel sx = selectors(x[e]);
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        acc[r][u][e] ^= gf_mul_sel(sx, tb[r][0], tb[r][1], tb[r][2], tb[r][3], tb[r][4]);
                }
            }
            if (live[u]) split_store(db, S, de, x, col[u], lane);
        }
        if (j + 1 < K) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                clo[u] = nlo[u];
                chi[u] = nhi[u];
            }
            cv = nv;
            cV = nV;
        }
    }
    if constexpr (R > 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t ob = shard_at<ROWS>(a, b, S, k, k + (uint32_t)r);  // parity shard r
            const uint32_t e = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(ob & 15u)) & 15u);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!live[u]) continue;  // window-uniform: every lane takes part in the shuffle
                split_store(ob, S, e, acc[r][u], col[u], lane);
            }
        }
    }
}

}  // namespace hbec
