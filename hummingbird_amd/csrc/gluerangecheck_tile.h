// gluerangecheck_tile.h — the wave tile of gf_range_checked (gluerangecheck.hip):
// the bytes D'[s, e) of one entry written to `dst` from ALL its present shards.
// It is gluecheck_tile (gluecheck_tile.h) with range_tile's stores
// (gluerange_tile.h; range_store and gluerange.h's window rules are used as they
// stand) and another set of examined positions:
//   1. The syndrome is masked per byte to P = gr_positions(S, s, e), one or two
//      intervals anywhere in [0, S), instead of x < min(S, len).  Both ends of
//      both intervals can fall inside a lane's 16 bytes (grc_live_mask).
//   2. Data shard i has the two-sided window gr_window(S, s, e, i) and the
//      virtual base gr_base(dst, S, s, i): a survivor column goes out only in
//      the windows of the tile its shard's window meets, a decoded row likewise,
//      whole 16-B blocks only inside the shard's own window.
//   3. Loads are clamped inside [shard, shard + S): a position outside P is
//      loaded and multiplied like any other and then neither examined nor stored.
//
// A = r + o accumulator rows per column (gluecheck.h): rows 0..r-1 are loaded
// from the r checked shards, rows r..A-1 start as zero, every survivor's column
// is loaded once, one survivor ahead, and multiplied into all A.  One ballot
// over the masked syndrome of lanes 0..62 ends the hot part.  A decoded row
// whose shard has no wanted position in the tile is computed all the same (the
// branch on A is per mask, not per range) and not stored.
//
// The cold part is gc_fix_columns' classification under the mask P.  A survivor
// candidate t with error e XORs D[d][t] e into decoded row d in registers, and,
// where the position lies in t's own window, the byte stored ^ e goes to
// gr_base(dst, S, s, t) + x with the stored byte read again from the shard: one
// byte store, never a read-modify-write of the destination.  A candidate among
// the checked shards, among parity survivors or in a data shard whose window
// does not hold the position changes no written byte of that shard.
//
// The seams, under the new mask.  gluecheck_tile.h's argument stands as written
// because everything it rests on is entry-wide or unchanged.  Lane 62 stays in
// the ballot: lane 61's 16-B block ends with up to 15 bytes of lane 62's column
// (range_store), so its decoded registers must be right and its corrected bytes
// written again.  Lane 62's positions are held again by lane 0 of the next
// window, the second half of an A = 4 tile, or the next tile's wave.  That
// holder masks with the same P (it is the entry's, not the tile's), so it finds
// the same column dirty and writes the same corrected value behind its own
// fence; and where a position of P lies in lane 62's column the holder's window
// and tile are live (gr_tile_live) and its shard's window meets them, so the
// holder does run and does store.  The reverse case, lane 62 correcting a byte
// of a window the hot part of THIS wave never stored for that shard, writes the
// value the holder writes last: a corrected byte is only ever overwritten by a
// corrected byte or by an uncorrected one that its own wave corrects afterwards.
// Narrowing the ballot to kUnalignedStoreLanes, or masking with anything
// narrower than the entry's P, breaks this at window and tile seams.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "correct.h"
#include "gf_device.h"
#include "gluecheck.h"
#include "gluecheck_tile.h"
#include "gluerange.h"
#include "gluerange_tile.h"
#include "gluerangecheck.h"
#include "kernels.h"
#include "shard_rows.h"
#include "unaligned_tile.h"

namespace hbec {

// The cold part of one lane, r >= 2: every byte position of its U columns in P
// whose syndrome (rows 0..r-1 of acc) names a survivor has the decoded rows
// (r..A-1 of acc) and, inside that survivor's window, the range's byte put
// right.  p: the mask's gc_record (wave-uniform), col0: the lane's column in
// window 0, [s, en): the range in D.  Returns the bits of the shards a byte was
// taken as corrected in, and kCorLeft if a position had no candidate.
template <int A, bool ROWS, int U>
__device__ __forceinline__ uint32_t grc_fix_columns(int K, uint32_t r, uint64_t a, uint64_t b, uint64_t S, GrSpan P,
                                                    uint64_t dst, uint64_t s, uint64_t en,
                                                    const uint32_t* __restrict__ p, uint64_t col0,
                                                    u32x4 (&acc)[A][U]) {
    constexpr uint32_t W = kUnalignedWindow;
    const uint32_t rs = p[3];
    const uint32_t* inv = p + gc_inverse_at(K, A);
    uint32_t out = 0u;
#pragma unroll 1
    for (int d = 0; d < 4 * U; ++d) {  // dword d & 3 of the column in window d >> 2 (wave-uniform)
        // a select chain on the uniform d, not an indexed array: the accumulators stay in registers
        uint32_t w[A];
#pragma unroll
        for (int q = 0; q < A; ++q) {
            uint32_t v = 0u;
            if ((uint32_t)q < r) {
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int c = 0; c < 4; ++c) v = d == 4 * u + c ? acc[q][u][c] : v;
            }
            w[q] = v;
        }
        // bytes outside P do not count
        const uint64_t pos = col0 + (uint64_t)(d >> 2) * W + 4u * (uint32_t)(d & 3);
        const uint32_t live = grc_live_mask(P, pos);
        // per byte: is any syndrome row non-zero, are all, is exactly one
        uint32_t any = 0u, all = 0xFFFFFFFFu, twice = 0u, named = 0u;
#pragma unroll
        for (int q = 0; q < A; ++q) {
            if ((uint32_t)q >= r) continue;
            w[q] &= live;
            const uint32_t on = gc_nonzero_bytes(w[q]);
            twice |= any & on;
            any |= on;
            all &= on;
        }
        if (any == 0u) continue;
        const uint32_t once = any & ~twice;
#pragma unroll
        for (int q = 0; q < A; ++q) {
            if ((uint32_t)q >= r) continue;
            const uint32_t here = once & gc_nonzero_bytes(w[q]);  // this checked shard alone: no range byte changes
            if (here != 0u) out |= 1u << ((rs >> (8 * q)) & 0xFFu);
            named |= here;
        }
        if (all != 0u) {
            // the survivor whose column the syndrome is a multiple of, for the 4 positions at once
            const Sel s0 = selectors(w[0]);
            uint32_t fix[A];
#pragma unroll
            for (int q = 0; q < A; ++q) fix[q] = 0u;
#pragma unroll 1
            for (int t = 0; t < K; ++t) {
                const uint32_t* t0 = p + kGcHdr + 5 * (t * A);  // tables of rows[0][t]; row q's 5 q words on
                const uint32_t* ti = inv + 5 * t;               // tables of 1 / rows[0][t]
                uint32_t mis = 0u;
#pragma unroll
                for (int q = 1; q < A; ++q) {
                    if ((uint32_t)q >= r) continue;
                    const uint32_t* tq = t0 + 5 * q;
                    mis |= gf_mul_sel(selectors(w[q]), t0[0], t0[1], t0[2], t0[3], t0[4]) ^
                           gf_mul_sel(s0, tq[0], tq[1], tq[2], tq[3], tq[4]);
                }
                const uint32_t hit = all & ~gc_nonzero_bytes(mis);
                if (hit == 0u) continue;
                const uint32_t err = gf_mul_sel(s0, ti[0], ti[1], ti[2], ti[3], ti[4]) & hit;
                const uint32_t shard = (p[t >> 2] >> (8 * (t & 3))) & 0xFFu;
                out |= 1u << shard;
                named |= hit;
                const Sel se = selectors(err);
#pragma unroll
                for (int q = 0; q < A; ++q) {
                    if ((uint32_t)q < r) continue;
                    const uint32_t* tq = t0 + 5 * q;
                    fix[q] ^= gf_mul_sel(se, tq[0], tq[1], tq[2], tq[3], tq[4]);
                }
                if (shard < (uint32_t)K) {  // a present data shard: its bytes of the range, one byte store each
                    const GrWin tw = gr_window(S, s, en, shard);
                    const uint64_t to = gr_base(dst, S, s, shard);
                    const uint64_t from = shard_at<ROWS>(a, b, S, (uint32_t)K, shard);
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const uint64_t at = pos + (uint32_t)x;
                        if (((hit >> (8 * x)) & 0xFFu) == 0u || at < tw.lo || at >= tw.hi) continue;
                        const uint8_t stored = *reinterpret_cast<gu8_c*>(from + at);
                        *reinterpret_cast<gu8*>(to + at) = (uint8_t)(stored ^ (uint8_t)(err >> (8 * x)));
                    }
                }
            }
            // the decoded rows, in registers, before they are stored
#pragma unroll
            for (int q = 0; q < A; ++q) {
                if ((uint32_t)q < r) continue;
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[q][u][c] ^= d == 4 * u + c ? fix[q] : 0u;
            }
        }
        if ((any & ~named) != 0u) out |= kCorLeft;
    }
    return out;
}

// One wave tile: U windows from shard position p0 of one entry whose mask has
// r >= 1 checked shards and A = r + o rows, a live tile of the range [s, en) of
// its D.  P: gr_positions(S, s, en).  p: the mask's gc_record.  Every argument
// is wave-uniform.  U: kUnalignedU, or half of it at A = 4 (gluecheck_tile.h).
template <int A, bool ROWS, int U = kUnalignedU>
__device__ __forceinline__ void rangecheck_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0, uint64_t dst,
                                                uint64_t s, uint64_t en, GrSpan P, const uint32_t* __restrict__ p,
                                                uint32_t lane, uint32_t* fixed) {
    static_assert(A >= 1, "no rows: range_tile<0> gathers");
    constexpr uint32_t W = kUnalignedWindow;
    const uint64_t s_lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);  // survivors 0..7
    const uint32_t s_hi = p[2], rs = p[3];
    const uint32_t r = p[4] & 0xFFu;  // checked shards; A - r missing data shards
    const uint32_t k = (uint32_t)K;
    auto surv = [=](int j) { return (j < 8 ? (uint32_t)(s_lo >> (8 * j)) : s_hi >> (8 * (j - 8))) & 0xFFu; };

    uint64_t col[U];
#pragma unroll
    for (int u = 0; u < U; ++u) col[u] = p0 + (uint64_t)u * W + lane * 16u;
    // rows 0..r-1: the stored columns of the checked shards (clamped loads: no branch); the rest zero
    u32x4 acc[A][U];
#pragma unroll
    for (int q = 0; q < A; ++q) {
#pragma unroll
        for (int u = 0; u < U; ++u) acc[q][u] = u32x4{0, 0, 0, 0};
        if ((uint32_t)q < r) {  // wave-uniform: every lane takes part in the shuffle
            const UView ov = uview(shard_at<ROWS>(a, b, S, k, (rs >> (8 * q)) & 0xFFu), S);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                u32x4 lo, hi;
                uload(lo, hi, ov, col[u]);
                acc[q][u] = realign16(lo, upper(lo, hi), ov.d);
            }
        }
    }
    u32x4 clo[U], chi[U];
    uint32_t ci = surv(0);
    UView cv = uview(shard_at<ROWS>(a, b, S, k, ci), S);
#pragma unroll
    for (int u = 0; u < U; ++u) uload(clo[u], chi[u], cv, col[u]);
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
        u32x4 nlo[U], nhi[U];
        UView nv = cv;
        uint32_t ni = ci;
        if (j + 1 < K) {
            ni = surv(j + 1);
            nv = uview(shard_at<ROWS>(a, b, S, k, ni), S);
#pragma unroll
            for (int u = 0; u < U; ++u) uload(nlo[u], nhi[u], nv, col[u]);
        }
        uint32_t tb[A][5];
#pragma unroll
        for (int q = 0; q < A; ++q)
#pragma unroll
            for (int x = 0; x < 5; ++x) tb[q][x] = (p + kGcHdr + 5 * (j * A + q))[x];
        // a surviving data shard goes to the range as it is, inside its window (wave-uniform)
        GrWin pw = gr_window(S, s, en, ci < k ? ci : 0u);
        if (ci >= k) pw.hi = pw.lo;
        const uint64_t pb = gr_base(dst, S, s, ci);
        const uint32_t pe = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(pb & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32x4 x = realign16(clo[u], upper(clo[u], chi[u]), cv.d);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const Sel sx = selectors(x[c]);
#pragma unroll
                for (int q = 0; q < A; ++q)
                    acc[q][u][c] ^= gf_mul_sel(sx, tb[q][0], tb[q][1], tb[q][2], tb[q][3], tb[q][4]);
            }
            const uint64_t c0 = p0 + (uint64_t)u * W;
            if (gr_meets(pw, c0, c0 + W)) range_store(pb, pw, pe, x, col[u], c0, lane);  // window-uniform
        }
        if (j + 1 < K) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                clo[u] = nlo[u];
                chi[u] = nhi[u];
            }
            cv = nv;
            ci = ni;
        }
    }
    // the syndrome of columns [c, c + 16) inside P; lane 63's column is partial
    uint32_t diff = 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint32_t mask = grc_live_mask(P, col[u] + 4u * (uint32_t)c);
#pragma unroll
            for (int q = 0; q < A; ++q)
                if ((uint32_t)q < r) diff |= acc[q][u][c] & mask;
        }
    }
    const bool bad = lane < 63u && diff != 0u;
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull) {  // wave-uniform: a clean tile skips all of this
        uint32_t done = kCorLeft;  // one checked shard: inconsistent, and nothing can be decided
        if (r >= 2u) {
            __threadfence();  // the hot part's stores first
            done = bad ? grc_fix_columns<A, ROWS, U>(K, r, a, b, S, P, dst, s, en, p, col[0], acc) : 0u;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) done |= (uint32_t)__shfl_xor((int)done, o, 64);
        }
        if (lane == 0u) atomicOr(fixed, kCorBad | (done & (kCorLeft | kCorShardMask)));
    }
    const uint64_t p1 = p0 + (uint64_t)U * W;
#pragma unroll
    for (int q = 0; q < A; ++q) {
        if ((uint32_t)q < r) continue;               // wave-uniform
        const uint32_t i = (rs >> (8 * q)) & 0xFFu;  // a missing data shard
        const GrWin ow = gr_window(S, s, en, i);
        if (!gr_meets(ow, p0, p1)) continue;  // no wanted position of it in this tile
        const uint64_t ob = gr_base(dst, S, s, i);
        const uint32_t oe = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(ob & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t c0 = p0 + (uint64_t)u * W;
            if (!gr_meets(ow, c0, c0 + W)) continue;  // window-uniform: every lane takes part in the shuffle
            range_store(ob, ow, oe, acc[q][u], col[u], c0, lane);
        }
    }
}

}  // namespace hbec
