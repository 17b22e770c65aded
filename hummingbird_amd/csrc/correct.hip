// correct.hip — correct the corrupt bytes of a plan column by column
// (hbec_correct_plan_mixed).  Locate (locate.hip) ends with the syndrome of
// every byte position in its accumulators, finds the position's candidate shard
// and keeps only who is ruled out, so that one shard of the entry can be named
// and rewritten whole (heal.hip).  Two disks that each lost a sector at
// different offsets of a stripe leave no single shard to name; yet every byte
// column has one bad byte at most, and the syndrome says which shard it is in
// and by how much it is off (correct.h: the rule).  This kernel writes that one
// byte back.
//
// gf_correct_mixed_plan<RMAX> walks the plan's static {entry, tile} list as
// gf_locate_mixed_plan does: list entry, pat_of[entry], the caller's flag, the
// entry's record and its mask's pattern record come through wave-uniform
// indices on read-only __restrict__ arguments (scalar loads), and an entry the
// filter leaves out is skipped before anything of it is loaded.
//
// Hot part: the tile computes the r syndrome rows as locate_mixed_tile does
// (checked shards loaded as accumulators, the k survivors multiplied in, loads
// one survivor ahead) and one ballot ends a clean tile.
//
// Cold part: a lane below kUnalignedStoreLanes with a non-zero masked syndrome
// owns its 16 columns of each of the U windows (lanes 62 and 63 hold columns
// the next window's lanes 0 and 1 own: a position corrected twice would be a
// position un-corrected).  It walks its 4 U dwords with a wave-uniform index,
// four positions at a time.  Per dword it builds an error dword and a shard
// byte per position: where one syndrome row is non-zero, that row's byte and
// its checked shard; where all are, it loops over the survivors t uniformly,
// computes locate's `mis` and, with one more multiply through the record's
// table of 1 / rows[0][t], s[0] / rows[0][t], and takes both bytewise where
// `mis` is zero.  Then each position with a shard loads the stored byte at the
// shard's own address, XORs and stores that one byte: never more, since the
// other bytes of an aligned group may belong to another lane or wave that is
// correcting them at the same moment.  The corrected shards' bits and
// kCorLeft are ORed across the wave with shuffles and lane 0 issues the tile's
// one atomicOr.  No LDS, no per-lane table gather, and every write is a
// per-lane vector byte store or that atomic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "correct.h"
#include "gf_device.h"
#include "kernels.h"
#include "planwalk.h"
#include "shard_rows.h"
#include "unaligned_tile.h"

namespace hbec {

// 0xFF in every byte of x that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) {
    uint32_t m = 0u;
#pragma unroll
    for (int b = 0; b < 4; ++b) m |= ((x >> (8 * b)) & 0xFFu) != 0u ? 0xFFu << (8 * b) : 0u;
    return m;
}

// The cold path of one lane: every byte position of its U columns whose
// syndrome has a candidate gets that shard's byte corrected.  p: the mask's
// cor_pattern record (wave-uniform), col0: the lane's column in window 0.
// Returns the corrected shards' bits, and kCorLeft if a position was left.
template <int R, bool ROWS>
__device__ __forceinline__ uint32_t correct_columns(int K, uint64_t a, uint64_t b, uint64_t S,
                                                    const uint32_t* __restrict__ p, uint64_t col0,
                                                    const u32x4 (&acc)[R][kUnalignedU]) {
    static_assert(R >= 2, "one checked shard decides nothing");
    constexpr int U = kUnalignedU;
    constexpr uint32_t W = kUnalignedWindow;
    const uint32_t so = p[3];
    const uint32_t* inv = p + cor_inverse_at(K, R);
    uint32_t out = 0u;
#pragma unroll 1
    for (int d = 0; d < 4 * U; ++d) {  // dword d & 3 of the column in window d >> 2 (wave-uniform)
        // a select chain on the uniform d, not an indexed array: the accumulators stay in registers
        uint32_t w[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            uint32_t v = 0u;
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) v = d == 4 * u + e ? acc[q][u][e] : v;
            w[q] = v;
        }
        // bytes at or past S do not count
        const uint64_t pos = col0 + (uint64_t)(d >> 2) * W + 4u * (uint32_t)(d & 3);
        const uint64_t nb = pos < S ? S - pos : 0u;
        const uint32_t live = nb >= 4u ? 0xFFFFFFFFu : (nb == 0u ? 0u : (0xFFFFFFFFu >> (8u * (uint32_t)(4u - nb))));
        // per byte: is any row non-zero, are all, is exactly one (then which)
        uint32_t any = 0u, all = 0xFFFFFFFFu, twice = 0u, err = 0u, who = 0xFFFFFFFFu;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            w[q] &= live;
            const uint32_t on = nonzero_bytes(w[q]);
            twice |= any & on;
            any |= on;
            all &= on;
        }
        if (any == 0u) continue;
        const uint32_t once = any & ~twice;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const uint32_t here = once & nonzero_bytes(w[q]);  // this checked shard alone
            err |= w[q] & here;
            who = (who & ~here) | ((((so >> (8 * q)) & 0xFFu) * 0x01010101u) & here);
        }
        if (all != 0u) {
            // the survivor whose column the syndrome is a multiple of, for the 4 positions at once
            const Sel s0 = selectors(w[0]);
#pragma unroll 1
            for (int t = 0; t < K; ++t) {
                const uint32_t* t0 = p + kMPatHdr + 5 * (t * R);  // tables of rows[0][t]; rows[q][t] 5 q words on
                const uint32_t* ti = inv + 5 * t;                 // tables of 1 / rows[0][t]
                uint32_t mis = 0u;
#pragma unroll
                for (int q = 1; q < R; ++q) {
                    const uint32_t* tq = t0 + 5 * q;
                    mis |= gf_mul_sel(selectors(w[q]), t0[0], t0[1], t0[2], t0[3], t0[4]) ^
                           gf_mul_sel(s0, tq[0], tq[1], tq[2], tq[3], tq[4]);
                }
                const uint32_t e = gf_mul_sel(s0, ti[0], ti[1], ti[2], ti[3], ti[4]);
                const uint32_t hit = all & ~nonzero_bytes(mis);
                const uint32_t shard = (p[t >> 2] >> (8 * (t & 3))) & 0xFFu;
                err = (err & ~hit) | (e & hit);
                who = (who & ~hit) | ((shard * 0x01010101u) & hit);
            }
        }
        // one byte each: the neighbours may be another lane's or another wave's
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const uint32_t i = (who >> (8 * x)) & 0xFFu;
            if (i != 0xFFu) {
                gu8* at = reinterpret_cast<gu8*>(shard_at<ROWS>(a, b, S, (uint32_t)K, i) + pos + (uint32_t)x);
                *at = (uint8_t)(*at ^ (uint8_t)(err >> (8 * x)));
                out |= 1u << i;
            } else if ((any >> (8 * x)) & 1u) {
                out |= kCorLeft;
            }
        }
    }
    return out;
}

// One tile of a stripe whose mask has R checked shards: locate_mixed_tile's
// loads and multiplies (locate.hip) up to `diff`, the ballot, then the cold
// path.  The text up to the ballot is a copy of locate's, whose instances are
// pinned and stay where they are: a change to either goes into both.
// ROWS: the entry names every shard (shard_rows.h).
template <int R, bool ROWS>
__device__ __forceinline__ void correct_mixed_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0,
                                                   const uint32_t* __restrict__ p, uint32_t lane, uint32_t* fixed) {
    constexpr int U = kUnalignedU;
    constexpr uint32_t W = kUnalignedWindow;
    const uint64_t s_lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);  // survivors 0..7
    const uint32_t s_hi = p[2], so = p[3];
    const uint32_t k = (uint32_t)K;
    auto shard = [=](uint32_t i) { return shard_at<ROWS>(a, b, S, k, i); };
    auto in_base = [=](int j) {
        return shard((j < 8 ? (uint32_t)(s_lo >> (8 * j)) : s_hi >> (8 * (j - 8))) & 0xFFu);
    };
    uint64_t col[U];
#pragma unroll
    for (int u = 0; u < U; ++u) col[u] = p0 + (uint64_t)u * W + lane * 16u;
    // the stored columns of the checked shards (clamped loads: no branch)
    u32x4 acc[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r) {
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
    // columns [c, c + 16) of the window's first 62 lanes; bytes at or past S and
    // windows that start there do not count
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
            for (int r = 0; r < R; ++r) diff |= acc[r][u][e] & mask;
        }
    }
    // each position has one owner: lanes 62 and 63 hold the next window's first columns
    const bool bad = lane < kUnalignedStoreLanes && diff != 0u;
    if (__builtin_amdgcn_ballot_w64(bad) == 0ull) return;  // wave-uniform: a clean tile ends here
    uint32_t done = kCorLeft;  // one checked shard: inconsistent, and nothing can be decided
    if constexpr (R >= 2) {
        done = bad ? correct_columns<R, ROWS>(K, a, b, S, p, col[0], acc) : 0u;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) done |= (uint32_t)__shfl_xor((int)done, o, 64);
    }
    if (lane == 0u) atomicOr(fixed, kCorBad | (done & (kCorLeft | kCorShardMask)));
}

// The walk both kernels below share.  RMAX: the largest count of checked shards
// among the call's masks; one launch serves every count, for the reason written
// at gf_mixed_plan.
template <int RMAX, bool ROWS>
__device__ __forceinline__ void correct_walk(const MRec* __restrict__ recs, const MTile* __restrict__ tiles,
                                             uint32_t n_tiles, const uint32_t* __restrict__ pat_of,
                                             const uint32_t* __restrict__ pats, int K,
                                             const uint32_t* __restrict__ flags, uint32_t* fixed) {
    constexpr uint32_t T = (uint32_t)kUnalignedU * kUnalignedWindow;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave =
        __builtin_amdgcn_readfirstlane(xcd_block() * (kBlockThreads / 64) + (threadIdx.x >> 6));
    const uint32_t nwaves = gridDim.x * (kBlockThreads / 64);
    for (uint32_t t = wave; t < n_tiles; t += nwaves) {
        const MTile e = tiles[t];
        const uint32_t w = pat_of[e.rec];
        const uint32_t r = w >> kMPatShift;  // wave-uniform
        if (r == 0u) {
            // exactly k present: nothing to check, said once per entry; nothing loaded
            if (w == kVmNothing && e.ti == 0u && lane == 0u) atomicOr(fixed + e.rec, kCorNothing);
            continue;
        }
        // the filter: an entry the caller's Verify did not flag loads nothing more
        if (flags != nullptr && (flags[e.rec] & 1u) == 0u) continue;
        if (r > (uint32_t)RMAX) continue;
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t* p = pats + (size_t)(w & kMPatMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        uint32_t* out = fixed + e.rec;
        if (r == 1u) correct_mixed_tile<1, ROWS>(K, a, b, S, p0, p, lane, out);
        if constexpr (RMAX >= 2)
            if (r == 2u) correct_mixed_tile<2, ROWS>(K, a, b, S, p0, p, lane, out);
        if constexpr (RMAX >= 3)
            if (r == 3u) correct_mixed_tile<3, ROWS>(K, a, b, S, p0, p, lane, out);
        if constexpr (RMAX >= 4)
            if (r == 4u) correct_mixed_tile<4, ROWS>(K, a, b, S, p0, p, lane, out);
    }
}

template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_correct_mixed_plan(const MRec* __restrict__ recs,
                                                                       const MTile* __restrict__ tiles,
                                                                       uint32_t n_tiles,
                                                                       const uint32_t* __restrict__ pat_of,
                                                                       const uint32_t* __restrict__ pats, int K,
                                                                       const uint32_t* __restrict__ flags,
                                                                       uint32_t* fixed) {
    correct_walk<RMAX, false>(recs, tiles, n_tiles, pat_of, pats, K, flags, fixed);
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of
// shard addresses (shard_rows.h).
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_correct_mixed_plan_rows(const MRec* __restrict__ recs,
                                                                            const MTile* __restrict__ tiles,
                                                                            uint32_t n_tiles,
                                                                            const uint32_t* __restrict__ pat_of,
                                                                            const uint32_t* __restrict__ pats, int K,
                                                                            const uint32_t* __restrict__ flags,
                                                                            uint32_t* fixed) {
    correct_walk<RMAX, true>(recs, tiles, n_tiles, pat_of, pats, K, flags, fixed);
}

static const void* correct_mixed_plan_kernel(int r, bool rows) {
    if (rows) {
        switch (r) {
            case 1: return reinterpret_cast<const void*>(&gf_correct_mixed_plan_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_correct_mixed_plan_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_correct_mixed_plan_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_correct_mixed_plan_rows<4>);
        }
        return nullptr;
    }
    switch (r) {
        case 1: return reinterpret_cast<const void*>(&gf_correct_mixed_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_correct_mixed_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_correct_mixed_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_correct_mixed_plan<4>);
    }
    return nullptr;
}

hipError_t launch_correct_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                     const uint32_t* pat_of, const uint32_t* pats, const uint32_t* flags,
                                     uint32_t* fixed, int cus, hipStream_t stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = correct_mixed_plan_kernel(r, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &pat_of, &pats, &k, &flags, &fixed};
    return launch_plan_walk(fn, fn ? &occ[rows][r] : nullptr, k, n_tiles, cus, args, stream);
}

}  // namespace hbec
