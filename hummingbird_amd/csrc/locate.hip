// locate.hip — which shard of an inconsistent stripe is the corrupt one
// (hbec_locate_plan_mixed).  The degraded Verify (vmixed.hip) leaves, in the
// accumulators of verify_mixed_tile, the syndrome of every byte position:
// s[q] = stored[checked q] ^ sum_t rows[q][t] survivor_t.  Verify keeps one bit
// of it.  With two or more checked shards the vector names the single shard
// that can explain it (locate.h: the rule), so a stripe Verify has flagged need
// not be read k + m more times with one more shard masked each time.
//
// gf_locate_mixed_plan<RMAX> walks the plan's static {entry, tile} list exactly
// as gf_verify_mixed_plan does: list entry, pat_of[entry], the caller's flag of
// the entry, its record and its mask's pattern record all come through
// wave-uniform indices on read-only __restrict__ arguments (scalar loads).  An
// entry the filter leaves out is skipped by a wave-uniform branch before
// anything of it is loaded.  The tile is verify_mixed_tile's, instruction for
// instruction, up to the OR of the masked accumulators; a wave whose 62 lanes
// all have diff == 0 ends there (one ballot), so a clean tile costs what it
// costs in Verify.  Only a wave with a bad byte goes on: its lanes with
// diff != 0 classify their byte positions one dword (4 positions) at a time,
// the ruled-out shards are ORed across the wave with shuffles, and lane 0
// issues the tile's one atomicOr.  No LDS, no tables beyond the pattern record:
// the proportionality test s[q] rows[0][t] == s[0] rows[q][t] multiplies with
// the v_perm tables the record already holds for rows[q][t].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "kernels.h"
#include "locate.h"
#include "planwalk.h"
#include "shard_rows.h"
#include "unaligned_tile.h"

namespace hbec {

// The cold path of one lane: every byte position of its U columns whose
// syndrome is non-zero rules out all present shards but its candidate.  p: the
// mask's pattern record (wave-uniform), col0: the lane's column in window 0.
template <int R>
__device__ __forceinline__ uint32_t locate_classify(int K, uint64_t S, const uint32_t* __restrict__ p,
                                                    uint64_t col0, const u32x4 (&acc)[R][kUnalignedU]) {
    static_assert(R >= 2, "one checked shard rules nothing out");
    constexpr int U = kUnalignedU;
    constexpr uint32_t W = kUnalignedWindow;
    auto surv_bit = [=](int t) { return 1u << ((p[t >> 2] >> (8 * (t & 3))) & 0xFFu); };
    const uint32_t so = p[3];
    uint32_t unit[R], present = 0u;
#pragma unroll
    for (int q = 0; q < R; ++q) {
        unit[q] = 1u << ((so >> (8 * q)) & 0xFFu);
        present |= unit[q];
    }
#pragma unroll 1
    for (int t = 0; t < K; ++t) present |= surv_bit(t);
    uint32_t ruled = 0u;
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
        uint32_t any = 0u;
#pragma unroll
        for (int q = 0; q < R; ++q) {
            w[q] &= live;
            any |= w[q];
        }
        if (any == 0u) continue;
        // survivors whose column the syndrome is a multiple of, for the 4 positions at once
        uint32_t prop[4] = {0u, 0u, 0u, 0u};
        const Sel s0 = selectors(w[0]);
#pragma unroll 1
        for (int t = 0; t < K; ++t) {
            const uint32_t* t0 = p + kMPatHdr + 5 * (t * R);  // tables of rows[0][t]; rows[q][t] 5 q words on
            uint32_t mis = 0u;
#pragma unroll
            for (int q = 1; q < R; ++q) {
                const uint32_t* tq = t0 + 5 * q;
                mis |= gf_mul_sel(selectors(w[q]), t0[0], t0[1], t0[2], t0[3], t0[4]) ^
                       gf_mul_sel(s0, tq[0], tq[1], tq[2], tq[3], tq[4]);
            }
            const uint32_t bit = surv_bit(t);
#pragma unroll
            for (int b = 0; b < 4; ++b) prop[b] |= ((mis >> (8 * b)) & 0xFFu) == 0u ? bit : 0u;
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            uint32_t nz = 0u, units = 0u;
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const bool on = ((w[q] >> (8 * b)) & 0xFFu) != 0u;
                nz += on ? 1u : 0u;
                units |= on ? unit[q] : 0u;
            }
            // one component: that checked shard; all: the proportional survivor; else nobody
            const uint32_t cand = nz == 1u ? units : (nz == (uint32_t)R ? prop[b] : 0u);
            ruled |= nz != 0u ? present & ~cand : 0u;
        }
    }
    return ruled;
}

// One tile of a stripe whose mask has R checked shards: verify_mixed_tile
// (vmixed.hip) up to `diff`, then the ballot.  ROWS: the entry names every shard
// (shard_rows.h).
template <int R, bool ROWS = false>
__device__ __forceinline__ void locate_mixed_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0,
                                                  const uint32_t* __restrict__ p, uint32_t lane, uint32_t* where) {
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
    const bool bad = lane < kUnalignedStoreLanes && diff != 0u;
    if (__builtin_amdgcn_ballot_w64(bad) == 0ull) return;  // wave-uniform: a clean tile ends here
    uint32_t ruled = 0u;
    if constexpr (R >= 2) {
        if (bad) ruled = locate_classify<R>(K, S, p, col[0], acc);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) ruled |= (uint32_t)__shfl_xor((int)ruled, o, 64);
    }
    if (lane == 0u) atomicOr(where, kLocBad | (ruled & kLocRuledMask));
}

// RMAX: the largest count of checked shards among the call's masks.  One launch
// serves every count, for the reason written at gf_mixed_plan.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_locate_mixed_plan(const MRec* __restrict__ recs,
                                                                      const MTile* __restrict__ tiles,
                                                                      uint32_t n_tiles,
                                                                      const uint32_t* __restrict__ pat_of,
                                                                      const uint32_t* __restrict__ pats, int K,
                                                                      const uint32_t* __restrict__ flags,
                                                                      uint32_t* where) {
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
            if (w == kVmNothing && e.ti == 0u && lane == 0u) atomicOr(where + e.rec, kLocNothing);
            continue;
        }
        // the filter: an entry the caller's Verify did not flag loads nothing more
        if (flags != nullptr && (flags[e.rec] & 1u) == 0u) continue;
        if (r > (uint32_t)RMAX) continue;
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t* p = pats + (size_t)(w & kMPatMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        uint32_t* out = where + e.rec;
        if (r == 1u) locate_mixed_tile<1>(K, a, b, S, p0, p, lane, out);
        if constexpr (RMAX >= 2)
            if (r == 2u) locate_mixed_tile<2>(K, a, b, S, p0, p, lane, out);
        if constexpr (RMAX >= 3)
            if (r == 3u) locate_mixed_tile<3>(K, a, b, S, p0, p, lane, out);
        if constexpr (RMAX >= 4)
            if (r == 4u) locate_mixed_tile<4>(K, a, b, S, p0, p, lane, out);
    }
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of shard
// addresses (shard_rows.h).  The text is gf_locate_mixed_plan's, word for word, with the
// tiles' ROWS flag set.  It is not shared through a function: wrapping the walk
// moved the register counts of existing instances (gf_heal_mixed_plan<4> from 161
// to 152 VGPRs, md5_plan from 92 to 96), and those are pinned.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_locate_mixed_plan_rows(const MRec* __restrict__ recs,
                                                                           const MTile* __restrict__ tiles,
                                                                           uint32_t n_tiles,
                                                                           const uint32_t* __restrict__ pat_of,
                                                                           const uint32_t* __restrict__ pats, int K,
                                                                           const uint32_t* __restrict__ flags,
                                                                           uint32_t* where) {
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
            if (w == kVmNothing && e.ti == 0u && lane == 0u) atomicOr(where + e.rec, kLocNothing);
            continue;
        }
        // the filter: an entry the caller's Verify did not flag loads nothing more
        if (flags != nullptr && (flags[e.rec] & 1u) == 0u) continue;
        if (r > (uint32_t)RMAX) continue;
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t* p = pats + (size_t)(w & kMPatMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        uint32_t* out = where + e.rec;
        if (r == 1u) locate_mixed_tile<1, true>(K, a, b, S, p0, p, lane, out);
        if constexpr (RMAX >= 2)
            if (r == 2u) locate_mixed_tile<2, true>(K, a, b, S, p0, p, lane, out);
        if constexpr (RMAX >= 3)
            if (r == 3u) locate_mixed_tile<3, true>(K, a, b, S, p0, p, lane, out);
        if constexpr (RMAX >= 4)
            if (r == 4u) locate_mixed_tile<4, true>(K, a, b, S, p0, p, lane, out);
    }
}

static const void* locate_mixed_plan_kernel(int r, bool rows) {
    if (rows) {
        switch (r) {
            case 1: return reinterpret_cast<const void*>(&gf_locate_mixed_plan_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_locate_mixed_plan_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_locate_mixed_plan_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_locate_mixed_plan_rows<4>);
        }
        return nullptr;
    }
    switch (r) {
        case 1: return reinterpret_cast<const void*>(&gf_locate_mixed_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_locate_mixed_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_locate_mixed_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_locate_mixed_plan<4>);
    }
    return nullptr;
}

hipError_t launch_locate_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                    const uint32_t* pat_of, const uint32_t* pats, const uint32_t* flags,
                                    uint32_t* where, int cus, hipStream_t stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = locate_mixed_plan_kernel(r, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &pat_of, &pats, &k, &flags, &where};
    return launch_plan_walk(fn, fn ? &occ[rows][r] : nullptr, k, n_tiles, cus, args, stream);
}

}  // namespace hbec
