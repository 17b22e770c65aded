// vmixed.hip — Verify over a plan with a present mask per stripe
// (hbec_verify_plan_mixed): are the shards that survive a failed disk safe to
// rebuild from?  Shard i of a partition's objects lives on
// ring.GetNodes(partition)[i] (ecobj.go:348-357), so the stripes a repair sweep
// reads have lost different shards; the surplus survivors ecReconstruct fetches
// anyway (ecutils.go:94-111) over-determine each codeword.
//
// gf_verify_mixed_plan<RMAX> walks the plan's static {entry, tile} list exactly
// as gf_mixed_plan does (mixedplan.hip): the list entry, pat_of[entry], the
// entry's record and its mask's pattern record all come through wave-uniform
// indices on read-only __restrict__ arguments (scalar loads), and a
// wave-uniform branch goes to the tile of the entry's count of checked shards.
// The tile is gf_apply_unaligned's frame (unaligned_tile.h: any base, any S,
// 16-B-aligned loads clamped inside their shard), but it stores nothing: the
// accumulator of checked shard c STARTS as the stored column of c, loaded ahead
// of the first survivor's column, so after the k multiplies it holds
// stored[c] ^ sum_t row_c[t] survivor_t and the stripe is consistent at a byte
// when that byte is zero.  One exposed load latency per tile, where comparing
// after the multiply (unaligned_tile's VERIFY mode) has two.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "gf_device.h"
#include "kernels.h"
#include "planwalk.h"
#include "shard_rows.h"
#include "unaligned_tile.h"
#include "vmixed.h"

// tuning builds: 1 = the tile is unaligned_tile's VERIFY mode as it stands (the
// stored columns loaded after the multiply), for an A/B against the shipped tile
#ifndef HBEC_VM_FLOOR
#define HBEC_VM_FLOOR 0
#endif

namespace hbec {

// One tile of a stripe whose mask has R checked shards.  Every capture is a
// value in SGPRs, as in mixed_plan_tile.  ROWS: the entry names every shard
// (shard_rows.h).
template <int R, bool ROWS = false>
__device__ __forceinline__ void verify_mixed_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0,
                                                  const uint32_t* __restrict__ p, uint32_t lane, uint32_t* flag) {
    constexpr int U = kUnalignedU;
    constexpr uint32_t W = kUnalignedWindow;
    const uint64_t s_lo = (uint64_t)p[0] | ((uint64_t)p[1] << 32);  // survivors 0..7
    const uint32_t s_hi = p[2], so = p[3];
    const uint32_t k = (uint32_t)K;
    auto shard = [=](uint32_t i) { return shard_at<ROWS>(a, b, S, k, i); };
    auto in_base = [=](int j) {
        return shard((j < 8 ? (uint32_t)(s_lo >> (8 * j)) : s_hi >> (8 * (j - 8))) & 0xFFu);
    };
#if HBEC_VM_FLOOR
    unaligned_tile<R, true>(
        K, S, p0, false, lane, in_base, [=](int r) { return shard((so >> (8 * r)) & 0xFFu); },
        [=](int r, int j) { return p + kMPatHdr + 5 * (j * R + r); }, flag);
    return;
#endif
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
    if (lane < kUnalignedStoreLanes && diff != 0u) atomicOr(flag, 1u);
}

// RMAX: the largest count of checked shards among the call's masks.  One launch
// serves every count, for the reason written at gf_mixed_plan.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_verify_mixed_plan(const MRec* __restrict__ recs,
                                                                      const MTile* __restrict__ tiles,
                                                                      uint32_t n_tiles,
                                                                      const uint32_t* __restrict__ pat_of,
                                                                      const uint32_t* __restrict__ pats, int K,
                                                                      uint32_t* flags) {
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
            if (w == kVmNothing && e.ti == 0u && lane == 0u) atomicOr(flags + e.rec, 2u);
            continue;
        }
        if (r > (uint32_t)RMAX) continue;
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t* p = pats + (size_t)(w & kMPatMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        uint32_t* flag = flags + e.rec;
        if (r == 1u) verify_mixed_tile<1>(K, a, b, S, p0, p, lane, flag);
        if constexpr (RMAX >= 2)
            if (r == 2u) verify_mixed_tile<2>(K, a, b, S, p0, p, lane, flag);
        if constexpr (RMAX >= 3)
            if (r == 3u) verify_mixed_tile<3>(K, a, b, S, p0, p, lane, flag);
        if constexpr (RMAX >= 4)
            if (r == 4u) verify_mixed_tile<4>(K, a, b, S, p0, p, lane, flag);
    }
}

// The same walk over a shards plan's records: recs[e].a is the entry's row of shard
// addresses (shard_rows.h).  The text is gf_verify_mixed_plan's, word for word, with the
// tiles' ROWS flag set.  It is not shared through a function: wrapping the walk
// moved the register counts of existing instances (gf_heal_mixed_plan<4> from 161
// to 152 VGPRs, md5_plan from 92 to 96), and those are pinned.
template <int RMAX>
__global__ __launch_bounds__(kBlockThreads) void gf_verify_mixed_plan_rows(const MRec* __restrict__ recs,
                                                                           const MTile* __restrict__ tiles,
                                                                           uint32_t n_tiles,
                                                                           const uint32_t* __restrict__ pat_of,
                                                                           const uint32_t* __restrict__ pats, int K,
                                                                           uint32_t* flags) {
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
            if (w == kVmNothing && e.ti == 0u && lane == 0u) atomicOr(flags + e.rec, 2u);
            continue;
        }
        if (r > (uint32_t)RMAX) continue;
        const uint64_t a = recs[e.rec].a, b = recs[e.rec].b;
        const uint64_t S = recs[e.rec].shard_len;
        const uint32_t* p = pats + (size_t)(w & kMPatMask) * 4u;
        const uint64_t p0 = (uint64_t)e.ti * T;
        uint32_t* flag = flags + e.rec;
        if (r == 1u) verify_mixed_tile<1, true>(K, a, b, S, p0, p, lane, flag);
        if constexpr (RMAX >= 2)
            if (r == 2u) verify_mixed_tile<2, true>(K, a, b, S, p0, p, lane, flag);
        if constexpr (RMAX >= 3)
            if (r == 3u) verify_mixed_tile<3, true>(K, a, b, S, p0, p, lane, flag);
        if constexpr (RMAX >= 4)
            if (r == 4u) verify_mixed_tile<4, true>(K, a, b, S, p0, p, lane, flag);
    }
}

static const void* verify_mixed_plan_kernel(int r, bool rows) {
    if (rows) {
        switch (r) {
            case 1: return reinterpret_cast<const void*>(&gf_verify_mixed_plan_rows<1>);
            case 2: return reinterpret_cast<const void*>(&gf_verify_mixed_plan_rows<2>);
            case 3: return reinterpret_cast<const void*>(&gf_verify_mixed_plan_rows<3>);
            case 4: return reinterpret_cast<const void*>(&gf_verify_mixed_plan_rows<4>);
        }
        return nullptr;
    }
    switch (r) {
        case 1: return reinterpret_cast<const void*>(&gf_verify_mixed_plan<1>);
        case 2: return reinterpret_cast<const void*>(&gf_verify_mixed_plan<2>);
        case 3: return reinterpret_cast<const void*>(&gf_verify_mixed_plan<3>);
        case 4: return reinterpret_cast<const void*>(&gf_verify_mixed_plan<4>);
    }
    return nullptr;
}

hipError_t launch_verify_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                    const uint32_t* pat_of, const uint32_t* pats, uint32_t* flags, int cus,
                                    hipStream_t stream, bool rows) {
    static std::atomic<int> occ[2][kMaxR + 1] = {};  // blocks per CU, asked once per instance
    const void* fn = verify_mixed_plan_kernel(r, rows);
    void* args[] = {&recs, &tiles, &n_tiles, &pat_of, &pats, &k, &flags};
    return launch_plan_walk(fn, fn ? &occ[rows][r] : nullptr, k, n_tiles, cus, args, stream);
}

// ---- the other route: a rebuilt shard against the stored one ----

__global__ __launch_bounds__(kBlockThreads) void gf_vm_compare(const uint8_t* __restrict__ x,
                                                               const uint8_t* __restrict__ y, uint64_t n,
                                                               uint32_t* flag) {
    const uint64_t step = (uint64_t)gridDim.x * kBlockThreads;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x; i < n; i += step) bad |= x[i] != y[i];
    if (bad) atomicOr(flag, 1u);
}

__global__ void gf_vm_or(uint32_t* flag, uint32_t bits) { atomicOr(flag, bits); }

hipError_t launch_vm_compare(const void* x, const void* y, uint64_t n, uint32_t* flag, int cus, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (cus < 1) return hipErrorInvalidValue;
    const uint64_t grid = std::min<uint64_t>((n + kBlockThreads - 1) / kBlockThreads, (uint64_t)cus * 8);
    gf_vm_compare<<<dim3((uint32_t)grid), dim3(kBlockThreads), 0, stream>>>(
        static_cast<const uint8_t*>(x), static_cast<const uint8_t*>(y), n, flag);
    return hipGetLastError();
}

hipError_t launch_vm_or(uint32_t* flag, uint32_t bits, hipStream_t stream) {
    gf_vm_or<<<dim3(1), dim3(1), 0, stream>>>(flag, bits);
    return hipGetLastError();
}

}  // namespace hbec
