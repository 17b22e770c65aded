// gluecheck_tile.h — the wave tile of gf_glue_checked (gluecheck.hip): glue_tile's
// gather and decode (glue_tile.h; its store rules are used as they stand) and
// correct_mixed_tile's check (correct.hip) in one pass over the entry's present
// shards, with nothing stored into any shard.
//
// A = r + o accumulator rows per column (gluecheck.h): rows 0..r-1 are loaded
// from the r checked shards, rows r..A-1 start as zero, and every survivor's
// column, loaded once and one survivor ahead, is multiplied into all A through
// the [t][A] table block of the record.  A survivor that is a data shard with a
// byte wanted goes to its place in the destination as it is loaded.  After the
// last survivor rows 0..r-1 are the syndrome and rows r..A-1 the missing data
// shards.  One ballot over the syndrome, masked at min(S, len), ends the hot
// part: a clean tile stores its o decoded rows and leaves.
//
// A dirty tile (cold) classifies its columns per dword as correct_columns does
// (correct.hip).  A candidate among the checked shards changes no object byte.
// A survivor candidate t with error e changes two things.  Decoded row d gets
// D[d][t] e XORed into its registers before it is stored; the (d, t) table is
// in the survivor's block.  If t is a data shard with the byte wanted, the byte
// stored ^ e is stored over the byte the hot part wrote, with the stored byte
// read again from the shard: one byte store, never a read-modify-write of the
// destination.
//
// Who does the cold part.  Lanes 0..62 of every window: lane 62's column is not
// this window's to store, but lane 61's 16-B block ends with up to 15 bytes of
// it (glue_store), so its decoded registers must be right and the bytes of it
// that the hot part wrote must be written again.  Its positions are also held
// by lane 0 of the next window, or of the next tile's wave, which then writes
// the same values: harmless, where an XOR into memory applied twice would not
// be.  Lane 63's column is partial (unaligned_tile.h) and is never looked at.
// The hot part's stores are fenced from the cold part's, so that a corrected
// byte always lands after the uncorrected one of the same wave.
//
// Why the last write of a two-holder byte is always a corrected one: every
// wave that writes such a byte uncorrected (tile n's lane 61 block, tile n + 1's
// lane 0, the second half of an A = 4 tile over what the first half put right)
// writes it corrected afterwards, behind its fence.  That holds only while both
// holders find the same column dirty: lane 62 must stay in `bad` (the ballot is
// over lanes 0..62, NOT kUnalignedStoreLanes), and both waves must mask the
// syndrome at the same Sr.  Narrowing either leaves stale bytes at window and
// tile seams that no test catches deterministically.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "correct.h"
#include "gf_device.h"
#include "glue_tile.h"
#include "gluecheck.h"
#include "kernels.h"
#include "shard_rows.h"
#include "unaligned_tile.h"

namespace hbec {

typedef __attribute__((address_space(1))) const uint8_t gu8_c;

// 0xFF in every byte of x that is not zero
__device__ __forceinline__ uint32_t gc_nonzero_bytes(uint32_t x) {
    uint32_t m = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) m |= ((x >> (8 * b)) & 0xFFu) != 0u ? 0xFFu << (8 * b) : 0u;
    return m;
}

// The cold part of one lane, r >= 2: every byte position of its U columns below
// Sr = min(S, len) whose syndrome (rows 0..r-1 of acc) names a survivor has the
// decoded rows (r..A-1 of acc) and the object byte put right.  p: the mask's
// gc_record (wave-uniform), col0: the lane's column in window 0.  Returns the
// bits of the shards a byte was taken as corrected in, and kCorLeft if a
// position had no candidate.
template <int A, bool ROWS, int U>
__device__ __forceinline__ uint32_t gc_fix_columns(int K, uint32_t r, uint64_t a, uint64_t b, uint64_t S, uint64_t Sr,
                                                   uint64_t dst, uint64_t len, const uint32_t* __restrict__ p,
                                                   uint64_t col0, u32x4 (&acc)[A][U]) {
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
                    for (int e = 0; e < 4; ++e) v = d == 4 * u + e ? acc[q][u][e] : v;
            }
            w[q] = v;
        }
        // bytes at or past Sr do not count
        const uint64_t pos = col0 + (uint64_t)(d >> 2) * W + 4u * (uint32_t)(d & 3);
        const uint64_t nb = pos < Sr ? Sr - pos : 0u;
        const uint32_t live = nb >= 4u ? 0xFFFFFFFFu : (nb == 0u ? 0u : (0xFFFFFFFFu >> (8u * (uint32_t)(4u - nb))));
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
            const uint32_t here = once & gc_nonzero_bytes(w[q]);  // this checked shard alone: no object byte changes
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
                const uint32_t e = gf_mul_sel(s0, ti[0], ti[1], ti[2], ti[3], ti[4]) & hit;
                const uint32_t shard = (p[t >> 2] >> (8 * (t & 3))) & 0xFFu;
                out |= 1u << shard;
                named |= hit;
                const Sel se = selectors(e);
#pragma unroll
                for (int q = 0; q < A; ++q) {
                    if ((uint32_t)q < r) continue;
                    const uint32_t* tq = t0 + 5 * q;
                    fix[q] ^= gf_mul_sel(se, tq[0], tq[1], tq[2], tq[3], tq[4]);
                }
                if (shard < (uint32_t)K) {  // a present data shard: its object bytes, one byte store each
                    const uint64_t off = (uint64_t)shard * S;
                    const uint64_t V = len <= off ? (uint64_t)0 : (len - off < S ? len - off : S);
                    const uint64_t from = shard_at<ROWS>(a, b, S, (uint32_t)K, shard);
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        if (((hit >> (8 * x)) & 0xFFu) == 0u || pos + (uint32_t)x >= V) continue;
                        const uint8_t stored = *reinterpret_cast<gu8_c*>(from + pos + (uint32_t)x);
                        *reinterpret_cast<gu8*>(dst + off + pos + (uint32_t)x) = (uint8_t)(stored ^ (uint8_t)(e >> (8 * x)));
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
                    for (int e = 0; e < 4; ++e) acc[q][u][e] ^= d == 4 * u + e ? fix[q] : 0u;
            }
        }
        if ((any & ~named) != 0u) out |= kCorLeft;
    }
    return out;
}

// One wave tile: U windows from shard position p0 < min(S, len) of one entry
// whose mask has A >= 1 rows.  p: the mask's gc_record.  Every argument is
// wave-uniform.  U: kUnalignedU, or half of it where the instance would not
// keep its accumulators in registers otherwise (glue_tile.h gives the figures
// for its own four-row tile).
template <int A, bool ROWS, int U = kUnalignedU>
__device__ __forceinline__ void gluecheck_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0, uint64_t dst,
                                               uint64_t len, const uint32_t* __restrict__ p, uint32_t lane,
                                               uint32_t* fixed) {
    static_assert(A >= 1, "no rows: glue_tile<0> gathers");
    constexpr uint32_t W = kUnalignedWindow;
    const uint64_t s_lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);  // survivors 0..7
    const uint32_t s_hi = p[2], rs = p[3];
    const uint32_t r = p[4] & 0xFFu;  // checked shards; A - r missing data shards
    const uint32_t k = (uint32_t)K;
    const uint64_t Sr = len < S ? len : S;  // the shard positions examined and needed
    auto surv = [=](int j) { return (j < 8 ? (uint32_t)(s_lo >> (8 * j)) : s_hi >> (8 * (j - 8))) & 0xFFu; };
    // bytes of data shard i inside the first len bytes: clamp(len - i S, 0, S)
    auto valid = [=](uint32_t i) {
        const uint64_t off = (uint64_t)i * S;  // i < k <= 12, S < 2^31
        return len <= off ? (uint64_t)0 : (len - off < S ? len - off : S);
    };

    uint64_t col[U];
    bool live[U];  // window-uniform
#pragma unroll
    for (int u = 0; u < U; ++u) {
        col[u] = p0 + (uint64_t)u * W + lane * 16u;
        live[u] = p0 + (uint64_t)u * W < Sr;
    }
    // rows 0..r-1: the stored columns of the checked shards (clamped loads: no branch); the rest zero
    u32x4 acc[A][U];
#pragma unroll
    for (int q = 0; q < A; ++q) {
#pragma unroll
        for (int u = 0; u < U; ++u) acc[q][u] = u32x4{0, 0, 0, 0};
        if ((uint32_t)q < r) {  // wave-uniform: every lane takes part in the shuffle
            const UView ov = uview(shard_at<ROWS>(a, b, S, k, (rs >> (8 * q)) & 0xFFu), Sr);
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
    UView cv = uview(shard_at<ROWS>(a, b, S, k, ci), Sr);
#pragma unroll
    for (int u = 0; u < U; ++u) uload(clo[u], chi[u], cv, col[u]);
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
        u32x4 nlo[U], nhi[U];
        UView nv = cv;
        uint32_t ni = ci;
        if (j + 1 < K) {
            ni = surv(j + 1);
            nv = uview(shard_at<ROWS>(a, b, S, k, ni), Sr);
#pragma unroll
            for (int u = 0; u < U; ++u) uload(nlo[u], nhi[u], nv, col[u]);
        }
        uint32_t tb[A][5];
#pragma unroll
        for (int q = 0; q < A; ++q)
#pragma unroll
            for (int x = 0; x < 5; ++x) tb[q][x] = (p + kGcHdr + 5 * (j * A + q))[x];
        // a surviving data shard goes to the object as it is (wave-uniform)
        const uint64_t pv = ci < k ? valid(ci) : 0u;
        const uint64_t pb = dst + (uint64_t)ci * S;
        const uint32_t pe = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(pb & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const u32x4 x = realign16(clo[u], upper(clo[u], chi[u]), cv.d);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const Sel sx = selectors(x[e]);
#pragma unroll
                for (int q = 0; q < A; ++q)
                    acc[q][u][e] ^= gf_mul_sel(sx, tb[q][0], tb[q][1], tb[q][2], tb[q][3], tb[q][4]);
            }
            if (pv > 0u && live[u]) glue_store(pb, pv, pe, x, col[u], lane);
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
    if (r > 0u) {
        // the syndrome of columns [c, c + 16) below Sr; lane 63's column is partial
        uint32_t diff = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t nb = col[u] < Sr ? Sr - col[u] : 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint64_t b0 = 4u * e;
                const uint32_t mask =
                    nb >= b0 + 4u ? 0xFFFFFFFFu : (nb <= b0 ? 0u : (0xFFFFFFFFu >> (8u * (uint32_t)(b0 + 4u - nb))));
#pragma unroll
                for (int q = 0; q < A; ++q)
                    if ((uint32_t)q < r) diff |= acc[q][u][e] & mask;
            }
        }
        const bool bad = lane < 63u && diff != 0u;
        if (__builtin_amdgcn_ballot_w64(bad) != 0ull) {  // wave-uniform: a clean tile skips all of this
            uint32_t done = kCorLeft;  // one checked shard: inconsistent, and nothing can be decided
            if (r >= 2u) {
                __threadfence();  // the hot part's stores first
                done = bad ? gc_fix_columns<A, ROWS, U>(K, r, a, b, S, Sr, dst, len, p, col[0], acc) : 0u;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) done |= (uint32_t)__shfl_xor((int)done, o, 64);
            }
            if (lane == 0u) atomicOr(fixed, kCorBad | (done & (kCorLeft | kCorShardMask)));
        }
    }
#pragma unroll
    for (int q = 0; q < A; ++q) {
        if ((uint32_t)q < r) continue;                 // wave-uniform
        const uint32_t i = (rs >> (8 * q)) & 0xFFu;  // a missing data shard
        const uint64_t ov = valid(i);
        if (ov == 0u) continue;
        const uint64_t ob = dst + (uint64_t)i * S;
        const uint32_t e = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(ob & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!live[u]) continue;  // window-uniform: every lane takes part in the shuffle
            glue_store(ob, ov, e, acc[q][u], col[u], lane);
        }
    }
}

}  // namespace hbec
