// glue_tile.h — the wave tile of gf_glue_plan (glue.hip): one entry's data
// shards 0..k-1 written back to back at `dst`, the first `len` bytes of them,
// from the entry's k survivors.  It is unaligned_tile's loop (unaligned_tile.h;
// its views, clamped loads and bytewise store are used as they stand) with three
// differences:
//   1. R, the count of missing data shards, may be 0: nothing is coded and the
//      tile is a gather.
//   2. Output q goes to dst + idx_q S and is clipped at that shard's valid
//      length V = clamp(len - idx_q S, 0, S) instead of at S.
//   3. Inside the j loop a survivor that is a data shard (index < k) has its
//      realigned columns stored to dst + idx S through the same store path,
//      clipped the same way.
// Loads are clamped inside [shard, shard + min(S, len)): no output is longer, so
// shard positions past it are never needed.
//
// The junction.  Output shards lie back to back, so whenever S is no multiple
// of 16 the last 16-B block of one and the first of the next are the same
// block, and they are written by different waves (or by one wave at different
// times).  A 16-B store is therefore made only where the whole block lies
// inside its own shard's [0, V); the head (up to the first aligned block) and
// the tail (the block holding V) go bytewise through store_bytes, exactly as
// unaligned_tile writes the head and tail of a shard.  Each output has its own
// residue (dst + idx S) mod 16.
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
// the shard at ob, of which V bytes are wanted.  Wave-uniform call: every lane
// takes part in the shuffle.
__device__ __forceinline__ void glue_store(uint64_t ob, uint64_t V, uint32_t e, const u32x4& v, uint64_t col,
                                           uint32_t lane) {
    u32x4 nb;
#pragma unroll
    for (int i = 0; i < 4; ++i) nb[i] = __shfl_down(v[i], 1u, 64);
    const u32x4 blk = realign16(v, nb, e);
    const uint64_t q = col + e;  // block start (shard position); ob + q is 16-B aligned
    if (lane < kUnalignedStoreLanes && q < V) {
        if (q + 16u <= V)
            st16_addr(ob + q, blk);
        else
            store_bytes(ob + q, blk, V - q);  // the tail: the block may hold the next shard's head
    }
    if (lane == 0u && col == 0u && e > 0u) store_bytes(ob, v, e < V ? e : V);  // head
}

// One wave tile: U windows from shard position p0 < min(S, len) of one entry.
// p: the entry's pattern record (mixedplan.h mp_pattern: k survivor and R output
// indices, then the tables of the R decode rows).  Every argument is wave-uniform.
// U: the windows coded together, kUnalignedU (the list's tile) or a part of it:
// with R = 4 the stores inside the j loop beside 64 accumulator registers took
// the instance to 256 VGPRs and one wave per SIMD, so the walk codes that tile
// as two halves of two windows (121 VGPRs, four waves).
template <int R, bool ROWS, int U = kUnalignedU>
__device__ __forceinline__ void glue_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0, uint64_t dst,
                                          uint64_t len, const uint32_t* __restrict__ p, uint32_t lane) {
    constexpr uint32_t W = kUnalignedWindow;
    constexpr int RA = R > 0 ? R : 1;
    const uint64_t s_lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);  // survivors 0..7
    const uint32_t s_hi = p[2], so = p[3];
    const uint32_t k = (uint32_t)K;
    const uint64_t Sr = len < S ? len : S;  // the shard positions anyone needs
    auto surv = [=](int j) { return (j < 8 ? (uint32_t)(s_lo >> (8 * j)) : s_hi >> (8 * (j - 8))) & 0xFFu; };
    // bytes of data shard i inside the first len bytes: clamp(len - i S, 0, S)
    auto valid = [=](uint32_t i) {
        const uint64_t off = (uint64_t)i * S;  // i < k <= 12, S < 2^31
        return len <= off ? (uint64_t)0 : (len - off < S ? len - off : S);
    };
    // a gather reads no shard past the last one with a byte wanted (survivors are 0..k-1)
    const int KK = R > 0 ? K : (int)((len + S - 1u) / S < (uint64_t)K ? (len + S - 1u) / S : (uint64_t)K);

    uint64_t col[U];
    bool live[U];  // window-uniform
#pragma unroll
    for (int u = 0; u < U; ++u) {
        col[u] = p0 + (uint64_t)u * W + lane * 16u;
        live[u] = p0 + (uint64_t)u * W < Sr;
    }
    u32x4 acc[RA][U];
#pragma unroll
    for (int r = 0; r < RA; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[r][u] = u32x4{0, 0, 0, 0};
    u32x4 clo[U], chi[U];
    uint32_t ci = surv(0);
    UView cv = uview(shard_at<ROWS>(a, b, S, k, ci), Sr);
#pragma unroll
    for (int u = 0; u < U; ++u) uload(clo[u], chi[u], cv, col[u]);  // clamped: no branch
#pragma unroll 1
    for (int j = 0; j < KK; ++j) {
        u32x4 nlo[U], nhi[U];
        UView nv = cv;
        uint32_t ni = ci;
        if (j + 1 < KK) {
            ni = surv(j + 1);
            nv = uview(shard_at<ROWS>(a, b, S, k, ni), Sr);
#pragma unroll
            for (int u = 0; u < U; ++u) uload(nlo[u], nhi[u], nv, col[u]);
        }
        uint32_t tb[RA][5];
        if constexpr (R > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int q = 0; q < 5; ++q) tb[r][q] = (p + kMPatHdr + 5 * (j * R + r))[q];
        }
        // a surviving data shard goes to the object as it is (wave-uniform)
        const uint64_t pv = ci < k ? valid(ci) : 0u;
        const uint64_t pb = dst + (uint64_t)ci * S;
        const uint32_t pe = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(pb & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32x4 x = realign16(clo[u], upper(clo[u], chi[u]), cv.d);
            if constexpr (R > 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const Sel sx = selectors(x[e]);
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        acc[r][u][e] ^= gf_mul_sel(sx, tb[r][0], tb[r][1], tb[r][2], tb[r][3], tb[r][4]);
                }
            }
            if (pv > 0u && live[u]) glue_store(pb, pv, pe, x, col[u], lane);
        }
        if (j + 1 < KK) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                clo[u] = nlo[u];
                chi[u] = nhi[u];
            }
            cv = nv;
            ci = ni;
        }
    }
    if constexpr (R > 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t i = (so >> (8 * r)) & 0xFFu;  // a missing data shard
            const uint64_t ov = valid(i);
            if (ov == 0u) continue;  // wave-uniform
            const uint64_t ob = dst + (uint64_t)i * S;
            const uint32_t e = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(ob & 15u)) & 15u);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!live[u]) continue;  // window-uniform: every lane takes part in the shuffle
                glue_store(ob, ov, e, acc[r][u], col[u], lane);
            }
        }
    }
}

}  // namespace hbec
