// gluerange_tile.h — the wave tile of gf_range_plan (gluerange.hip): the bytes
// D[s, e) of one entry's D = data shard 0 || ... || data shard k-1 written to
// `dst`, from the entry's k survivors.  It is glue_tile (glue_tile.h; the views,
// clamped loads and realignment are unaligned_tile.h's as they stand) with these
// differences:
//   1. Output shard i has a two-sided window [lo_i, hi_i) (gluerange.h
//      gr_window) and the virtual base dst - s + i S, which may lie below dst
//      (arithmetic modulo 2^64): position p of it lands at base + p.
//   2. R = 0 is the gather of ANY entry's tile in which no missing data shard
//      has a wanted position (the walk decides, gr_tile_coded), not only of a
//      healthy entry: it walks the record's survivor list and skips the
//      survivors that are parity and the data shards whose window misses the
//      tile, loads included.  R > 0 reads all k survivors and stores only the
//      decoded rows and the present data shards whose window meets the tile.
//   3. Loads are clamped inside [shard, shard + S).
//
// The junction, two-sided.  Output shards lie back to back and the range begins
// and ends anywhere, so the first and last 16-B destination block of a shard's
// window may be shared with the next shard's head, the previous one's tail, or
// with bytes outside [dst, dst + len) altogether, and the sharers are different
// waves or one wave at different times.  A 16-B store is made only where the
// whole block lies inside its own shard's [lo, hi); a block cut by lo or by hi
// goes bytewise, only its bytes inside the window (gr_block_bytes).  The head is
// no longer lane 0's at column 0 alone: the block that holds lo is whichever
// lane's, and the bytes [col, col + e) in front of a window's first block, which
// the window before stores when it stores at all, are its first lane's exactly
// when that window holds no wanted position (gr_head_bytes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.h"
#include "gluerange.h"
#include "kernels.h"
#include "mixedplan.h"
#include "shard_rows.h"
#include "unaligned_tile.h"

namespace hbec {

// bytes [b0, b1) of the 16 at addr
__device__ __forceinline__ void range_store_bytes(uint64_t addr, const u32x4& v, uint32_t b0, uint32_t b1) {
    gu8* p = reinterpret_cast<gu8*>(addr);  // global, not flat (unaligned_tile.h store_bytes)
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if ((uint32_t)b >= b0 && (uint32_t)b < b1) p[b] = (uint8_t)(v[b >> 2] >> (8 * (b & 3)));
}

// Columns v (shard positions [col, col + 16) per lane) of one window, whose
// first column is col0, to the shard whose position 0 lands at ob and of which
// the positions w are wanted.  Wave-uniform call: every lane takes part in the
// shuffle.
__device__ __forceinline__ void range_store(uint64_t ob, GrWin w, uint32_t e, const u32x4& v, uint64_t col,
                                            uint64_t col0, uint32_t lane) {
    u32x4 nb;
#pragma unroll
    for (int i = 0; i < 4; ++i) nb[i] = __shfl_down(v[i], 1u, 64);
    const u32x4 blk = realign16(v, nb, e);
    const uint64_t q = col + e;  // block start (shard position); ob + q is 16-B aligned
    uint32_t b0, b1;
    if (lane < kUnalignedStoreLanes && gr_block_bytes(w, q, &b0, &b1)) {
        if (b1 - b0 == 16u)
            st16_addr(ob + q, blk);
        else
            range_store_bytes(ob + q, blk, b0, b1);  // cut by lo or hi: the rest is not this shard's
    }
    if (lane == 0u && gr_head_bytes(w, col0, e, &b0, &b1)) range_store_bytes(ob + col0, v, b0, b1);
}

// One wave tile: U windows from shard position p0 of one entry, a live tile of
// the range [s, e) of its D.  p: the entry's pattern record (mixedplan.h
// mp_pattern).  R: the rows decoded, the record's r in a coded tile, 0 in a
// gather tile whatever the record's r.  Every argument is wave-uniform.
// U: the windows taken together, kUnalignedU or, with R = 4, half of it
// (glue_tile.h gives the reason).
template <int R, bool ROWS, int U = kUnalignedU>
__device__ __forceinline__ void range_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0, uint64_t dst,
                                           uint64_t s, uint64_t e, const uint32_t* __restrict__ p, uint32_t lane) {
    constexpr uint32_t W = kUnalignedWindow;
    constexpr int RA = R > 0 ? R : 1;
    const uint64_t s_lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);  // survivors 0..7
    const uint32_t s_hi = p[2], so = p[3];
    const uint32_t k = (uint32_t)K;
    const uint64_t p1 = p0 + (uint64_t)U * W;
    auto surv = [=](int j) { return (j < 8 ? (uint32_t)(s_lo >> (8 * j)) : s_hi >> (8 * (j - 8))) & 0xFFu; };
    // the next survivor at or after j that this tile reads (K: none): all of
    // them when it decodes, the data shards whose window meets it when it gathers
    auto next = [=](int j) {
        if constexpr (R == 0) {
            while (j < K) {
                const uint32_t i = surv(j);
                if (i < k && gr_shard_in_tile(S, s, e, i, p0, p1)) break;
                ++j;
            }
        }
        return j;
    };

    uint64_t col[U];
#pragma unroll
    for (int u = 0; u < U; ++u) col[u] = p0 + (uint64_t)u * W + lane * 16u;
    u32x4 acc[RA][U];
#pragma unroll
    for (int r = 0; r < RA; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[r][u] = u32x4{0, 0, 0, 0};
    int j = next(0);
    if (j >= K) return;  // wave-uniform
    u32x4 clo[U], chi[U];
    uint32_t ci = surv(j);
    UView cv = uview(shard_at<ROWS>(a, b, S, k, ci), S);
#pragma unroll
    for (int u = 0; u < U; ++u) uload(clo[u], chi[u], cv, col[u]);  // clamped: no branch
#pragma unroll 1
    while (j < K) {
        const int nj = next(j + 1);
        u32x4 nlo[U], nhi[U];
        UView nv = cv;
        uint32_t ni = ci;
        if (nj < K) {
            ni = surv(nj);
            nv = uview(shard_at<ROWS>(a, b, S, k, ni), S);
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
        GrWin pw = gr_window(S, s, e, ci < k ? ci : 0u);
        if (ci >= k) pw.hi = pw.lo;
        const uint64_t pb = gr_base(dst, S, s, ci);
        const uint32_t pe = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(pb & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32x4 x = realign16(clo[u], upper(clo[u], chi[u]), cv.d);
            if constexpr (R > 0) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const Sel sx = selectors(x[c]);
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        acc[r][u][c] ^= gf_mul_sel(sx, tb[r][0], tb[r][1], tb[r][2], tb[r][3], tb[r][4]);
                }
            }
            const uint64_t c0 = p0 + (uint64_t)u * W;
            if (gr_meets(pw, c0, c0 + W)) range_store(pb, pw, pe, x, col[u], c0, lane);  // window-uniform
        }
        if (nj < K) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                clo[u] = nlo[u];
                chi[u] = nhi[u];
            }
            cv = nv;
            ci = ni;
        }
        j = nj;
    }
    if constexpr (R > 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t i = (so >> (8 * r)) & 0xFFu;  // a missing data shard
            const GrWin ow = gr_window(S, s, e, i);
            if (!gr_meets(ow, p0, p1)) continue;  // wave-uniform
            const uint64_t ob = gr_base(dst, S, s, i);
            const uint32_t oe = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(ob & 15u)) & 15u);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint64_t c0 = p0 + (uint64_t)u * W;
                if (!gr_meets(ow, c0, c0 + W)) continue;  // window-uniform: every lane takes part in the shuffle
                range_store(ob, ow, oe, acc[r][u], col[u], c0, lane);
            }
        }
    }
}

}  // namespace hbec
