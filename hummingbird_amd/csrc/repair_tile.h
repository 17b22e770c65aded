// repair_tile.h — the tile of gf_repair_mixed_plan (repair.hip) and of
// gf_heal_mixed_plan (heal.hip): rebuild RO shards of a stripe and check RC
// others in one multiply loop over its k survivors.  One text for both kernels;
// which record it runs on is the caller's business.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.h"
#include "kernels.h"
#include "mixedplan.h"
#include "shard_rows.h"
#include "unaligned_tile.h"

namespace hbec {

// One tile of a stripe whose mask has RO shards to rebuild and RC to check; the
// record's rows are the outputs' first.  Every capture is a value in SGPRs, as
// in mixed_plan_tile.  `zero` is the entry record's pad word, 0 in every record
// mp_build writes: the output rows start from it and not from a literal, because
// with literal zeros beside loaded rows the compiler allocates 15 to 57 VGPRs
// more than for rows that all start alike (132 against 116 at (1, 1), 209
// against 152 at (1, 3): a wave per SIMD less at both).  ROWS: the entry names
// every shard (shard_rows.h).
template <int RO, int RC, bool ROWS = false>
__device__ __forceinline__ void repair_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0,
                                            const uint32_t* __restrict__ p, uint32_t lane, uint32_t* flag,
                                            uint32_t zero) {
    constexpr int R = RO + RC;
    constexpr int U = kUnalignedU;
    constexpr uint32_t W = kUnalignedWindow;
    const uint64_t s_lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);  // survivors 0..7
    const uint32_t s_hi = p[2], so = p[3];
    const uint32_t k = (uint32_t)K;
    auto shard = [=](uint32_t i) { return shard_at<ROWS>(a, b, S, k, i); };
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

}  // namespace hbec
