// unaligned_tile.h — the any-alignment wave tile of gf_apply_unaligned (kernels.hip,
// where the scheme is described), for gf_mixed_plan (mixedplan.hip).  The same
// text as kernels.hip's own copy, which stays where it is: the committed PMC
// summary is keyed to kernels.hip's bytes (bench.py KERNEL_SOURCES), so moving
// the tile out of it would make bench.py drop its traffic figures until the
// counters are collected again.  A change to either copy goes into both;
// kernels.hip does not include this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.h"
#include "kernels.h"

namespace hbec {

// stored bytes per 64-lane window: 62 blocks, the column's upper block from
// lane l+1 (lane 63's column is partial); one load per input column, +3-9 %
// over two (profiles/r02_tune_unaligned_shfl.jsonl)
constexpr uint32_t kUnalignedWindow = 992;
constexpr uint32_t kUnalignedStoreLanes = 62;
constexpr int kUnalignedU = HBEC_UNALIGNED_U;  // windows per wave tile (loads in flight)

// A view of one object's shard: aligned base, misalignment, last aligned block.
struct UView {
    uint64_t abase;  // base & ~15
    uint64_t last;   // (base + S - 1) & ~15
    uint32_t d;      // base & 15 (wave-uniform)
};

__device__ __forceinline__ UView uview(uint64_t b, uint64_t s) {
    UView v;
    v.abase = b & ~(uint64_t)15;
    v.last = (b + s - 1u) & ~(uint64_t)15;
    v.d = __builtin_amdgcn_readfirstlane((uint32_t)(b & 15u));
    return v;
}

__device__ __forceinline__ void uload(u32x4& lo, u32x4& hi, const UView& v, uint64_t col) {
    const uint64_t x = v.abase + col;
    lo = ld16_addr(x < v.last ? x : v.last);
    hi = lo;  // replaced by lane l+1's block at use (upper)
}

// the column's upper block: lane l+1's lower block
__device__ __forceinline__ u32x4 upper(const u32x4& lo, const u32x4& hi) {
    (void)hi;
    u32x4 h;
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = __shfl_down(lo[i], 1u, 64);
    return h;
}

typedef __attribute__((address_space(1))) uint8_t gu8;

__device__ __forceinline__ void store_bytes(uint64_t addr, const u32x4& v, uint64_t n) {
    gu8* p = reinterpret_cast<gu8*>(addr);  // global, not flat: flat stores also count in lgkmcnt
#pragma unroll
    for (int b = 0; b < 16; ++b)
        if ((uint64_t)b < n) p[b] = (uint8_t)(v[b >> 2] >> (8 * (b & 3)));
}

// One wave tile: U windows from shard position p0 of one object / stripe.
// in_base(j) / out_base(r) give the byte address of that object's input j /
// output r shard (wave-uniform); tab(r, j) its coefficient tables.
// VERIFY: compare the coded columns with the stored outputs instead of
// storing them, and OR 1 into *flag on any mismatching byte (Encoder.Verify).
template <int R, bool VERIFY = false, class InBase, class OutBase, class Tab>
__device__ __forceinline__ void unaligned_tile(int K, uint64_t S, uint64_t p0, bool accumulate, uint32_t lane,
                                               InBase in_base, OutBase out_base, Tab tab,
                                               uint32_t* flag = nullptr) {
    constexpr int U = kUnalignedU;
    constexpr uint32_t W = kUnalignedWindow;
    uint64_t col[U];
    bool live[U];  // window-uniform
#pragma unroll
    for (int u = 0; u < U; ++u) {
        col[u] = p0 + (uint64_t)u * W + lane * 16u;
        live[u] = p0 + (uint64_t)u * W < S;
    }
    u32x4 acc[R][U];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const UView ov = uview(out_base(r), S);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            acc[r][u] = u32x4{0, 0, 0, 0};
            if (accumulate) {  // kernel-uniform; clamped loads need no per-window branch
                u32x4 lo, hi;
                uload(lo, hi, ov, col[u]);
                acc[r][u] = realign16(lo, upper(lo, hi), ov.d);
            }
        }
    }
    u32x4 clo[U], chi[U];
    UView cv = uview(in_base(0), S);
#pragma unroll
    for (int u = 0; u < U; ++u) uload(clo[u], chi[u], cv, col[u]);  // clamped: no branch
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
            for (int q = 0; q < 5; ++q) tb[r][q] = tab(r, j)[q];
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
    if constexpr (VERIFY) {
        bool bad = false;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const UView ov = uview(out_base(r), S);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!live[u]) continue;  // window-uniform (the upper block is a shuffle)
                u32x4 lo, hi;
                uload(lo, hi, ov, col[u]);
                const u32x4 st = realign16(lo, upper(lo, hi), ov.d);
                // columns [c, c + 16) of this window's lanes; bytes at or past S do not count
                const uint64_t nv = col[u] < S ? S - col[u] : 0u;
                if (lane < kUnalignedStoreLanes) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint64_t b0 = 4u * e;
                        const uint32_t mask = nv >= b0 + 4u ? 0xFFFFFFFFu
                                              : (nv <= b0 ? 0u : (0xFFFFFFFFu >> (8u * (uint32_t)(b0 + 4u - nv))));
                        bad |= ((acc[r][u][e] ^ st[e]) & mask) != 0u;
                    }
                }
            }
        }
        if (bad) atomicOr(flag, 1u);
        return;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint64_t ob = out_base(r);
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
