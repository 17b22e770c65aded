// vplan.hip — Encoder.Verify over a plan (hbec_verify_plan, hbec_verify_host):
// stripes / objects of mixed shard lengths at any alignment checked in a
// number of launches that does not depend on how many there are.  Read-only:
// each parity column is recomputed in registers from the k data columns and
// compared with the stored one; the only write is atomicOr(flag of the
// stripe, 1) from one lane of a wave that saw a difference.
//
//  * gf_verify_tiles<K, R>: the plan's aligned tile records (TileRec, 16-B
//    aligned base and S; K <= 8).  gf_apply_stripes' walk (the next tile's
//    loads and the record after that in flight while this tile is checked)
//    with gf_verify_pipe's compare; lanes at offsets >= valid take no part.
//  * gf_verify_recs<R>: any base and S, runtime K <= 12, over {record, tile}
//    pairs.  gf_wide's element stream (wide.hip): dword-aligned 16-B loads
//    clamped to their shard, shifted into the shard's byte frame (one DPP lane
//    shift + 4 v_alignbyte), a ring of kVpD loads running ahead across tile
//    boundaries, coefficient tables in LDS.
//  * gf_verify_recs_tail<R>: the last < 32 bytes of every parity shard of
//    every record, byte per thread, one launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "gf_device.h"
#include "kernels.h"
#include "vplan.h"

namespace hbec {

// ---- aligned tiles ----

template <int K, int R, int U>
__device__ __forceinline__ void load_vtile(u32x4 (&x)[U][K + R], const VTileArgs& a, const TileRec& t, uint32_t lane) {
    const uint64_t par = a.split ? t.out_addr : t.in_addr + (uint64_t)K * t.in_stride;
    const uint64_t pst = a.split ? t.out_stride : t.in_stride;
    const uint64_t last = (uint64_t)t.valid - 16u;  // valid >= 16, multiple of 16
#pragma unroll
    for (int u = 0; u < U; ++u) {
        uint64_t off = (uint64_t)lane * 16u + (uint64_t)u * 1024u;
        off = off < last ? off : last;
#pragma unroll
        for (int j = 0; j < K; ++j) x[u][j] = ld16_addr(t.in_addr + (uint64_t)j * t.in_stride + off);
#pragma unroll
        for (int r = 0; r < R; ++r) x[u][K + r] = ld16_addr(par + (uint64_t)r * pst + off);
    }
}

template <int K, int R, int U>
__device__ __forceinline__ void check_vtile(const u32x4 (&x)[U][K + R], const VTileArgs& a, const Tables<K, R>& tb,
                                            const TileRec& t, uint32_t lane, uint32_t* flags) {
    uint32_t bad = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t off = lane * 16u + (uint32_t)u * 1024u;
        u32x4 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = u32x4{0, 0, 0, 0};
        u32x4 in[K];
#pragma unroll
        for (int j = 0; j < K; ++j) in[j] = x[u][j];
        gf_dot<K, R>(acc, in, a.tab, tb);
        if (off < t.valid) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const u32x4 d = acc[r] ^ x[u][K + r];
                bad |= d.x | d.y | d.z | d.w;
            }
        }
    }
    if (__any(bad != 0)) {
        if (lane == 0u) atomicOr(flags + t.pad_, 1u);
    }
}

template <int K, int R>
__global__ __launch_bounds__(kBlockThreads, 1) void gf_verify_tiles(VTileArgs a, const TileRec* __restrict__ tiles,
                                                                    uint32_t* flags) {
    constexpr int U = stripes_u(K);  // the plan's tile size
    constexpr uint32_t WPB = kBlockThreads / 64;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * WPB + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * WPB;
    const uint32_t n = a.n_tiles;
    if (wave >= n) return;
    const Tables<K, R> tb = load_tables<K, R>(a.tab);
    TileRec cur = tiles[wave];
    u32x4 x[U][K + R];
    load_vtile<K, R, U>(x, a, cur, lane);
    uint32_t tn = wave + nw;
    TileRec nxt = tiles[tn < n ? tn : n - 1u];
    for (; tn < n; tn += nw) {
        u32x4 y[U][K + R];
        load_vtile<K, R, U>(y, a, nxt, lane);  // data one tile ahead
        // record two tiles ahead, after the data loads (scalar loads return
        // out of order: waiting for `nxt` here would be an lgkmcnt(0))
        const uint32_t t2 = tn + nw;
        const TileRec after = tiles[t2 < n ? t2 : n - 1u];
        check_vtile<K, R, U>(x, a, tb, cur, lane, flags);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < K + R; ++j) x[u][j] = y[u][j];
        cur = nxt;
        nxt = after;
    }
    check_vtile<K, R, U>(x, a, tb, cur, lane, flags);
}

// ---- any alignment ----

__device__ __forceinline__ u32x4 vp_shift(const u32x4& v, uint32_t sh) {
    const uint32_t n0 = lane_next(v[0]);
    return u32x4{__builtin_amdgcn_alignbyte(v[1], v[0], sh), __builtin_amdgcn_alignbyte(v[2], v[1], sh),
                 __builtin_amdgcn_alignbyte(v[3], v[2], sh), __builtin_amdgcn_alignbyte(n0, v[3], sh)};
}

// Stream pointer: element j (inputs 0..K-1, then stored parity K..K+R-1) of
// list entry t, with that entry's stripe.
struct VpPtr {
    uint32_t t, ti, j, flag;
    uint64_t a, b;
    int32_t S;
};

__device__ __forceinline__ void vp_set(VpPtr& p, uint32_t t, const VRec* __restrict__ recs,
                                       const VTile* __restrict__ tiles) {
    const VTile e = tiles[t];
    const VRec r = recs[e.rec];
    p.t = t;
    p.ti = e.ti;
    p.j = 0;
    p.flag = r.flag;
    p.a = r.a;
    p.b = r.b;
    p.S = (int32_t)r.shard_len;
}

template <int R>
__global__ __launch_bounds__(kPipeBlockThreads) void gf_verify_recs(const VRec* __restrict__ recs,
                                                                    const VTile* __restrict__ tiles, uint32_t n,
                                                                    uint32_t K, const uint32_t* __restrict__ tab,
                                                                    uint32_t* flags) {
    constexpr uint32_t ts = vp_tab_stride(R);
    __shared__ __attribute__((aligned(16))) uint32_t lds_tab[kOddMaxK * ts];
    for (uint32_t i = threadIdx.x; i < K * ts; i += blockDim.x) lds_tab[i] = tab[i];
    __syncthreads();

    constexpr uint32_t WPB = kPipeBlockThreads / 64;
    const uint32_t L = K + R;  // elements per tile
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nw = gridDim.x * WPB;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * WPB + (threadIdx.x >> 6));
    if (w >= n) return;
    const uint32_t total = ((n - 1u - w) / nw + 1u) * L;  // this wave's elements

    // producer: loads run kVpD elements ahead of the consumer, across tile
    // boundaries; past the wave's last element it reloads that element
    VpPtr pp, cp;
    vp_set(pp, w, recs, tiles);
    cp = pp;
    uint32_t issued = 0;
    auto issue = [&](u32x4 (&buf)[kVpU], uint32_t& sh) {
        const uint64_t S = (uint64_t)(uint32_t)pp.S;
        const uint64_t base = pp.j < K ? pp.a + (uint64_t)pp.j * S : pp.b + (uint64_t)(pp.j - K) * S;
        const int32_t l4 = (int32_t)((uint32_t)base & 3u);
        const int32_t t = l4 + (int32_t)(pp.ti * kVpTile);
        sh = (uint32_t)t & 3u;
        // no load leaves [base & ~3, (base + S + 3) & ~3): S >= 32 here
        const int32_t lim = ((l4 + pp.S + 3) & ~3) - 16;
#pragma unroll
        for (int u = 0; u < kVpU; ++u) {
            int32_t v = t - (int32_t)sh + 16 * (int32_t)lane + u * (int32_t)kVpWin;
            v = v < 0 ? 0 : (v > lim ? lim : v);
            buf[u] = ld16_addr((base & ~(uint64_t)3) + (uint64_t)(uint32_t)v);
        }
        if (++issued < total) {
            if (++pp.j == L) vp_set(pp, pp.t + nw, recs, tiles);
        }
    };
    u32x4 ring[kVpD][kVpU];
    uint32_t rsh[kVpD];
#pragma unroll
    for (int i = 0; i < kVpD; ++i) issue(ring[i], rsh[i]);

    u32x4 acc[kVpU][R];
#pragma unroll
    for (int u = 0; u < kVpU; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[u][r] = u32x4{0, 0, 0, 0};
    bool bad = false;
    for (uint32_t p0 = 0; p0 < total; p0 += kVpD) {
#pragma unroll
        for (int i = 0; i < kVpD; ++i) {
            u32x4 xs[kVpU];
#pragma unroll
            for (int u = 0; u < kVpU; ++u) xs[u] = vp_shift(ring[i][u], rsh[i]);
            // the reload reuses ring[i]'s registers only after xs is computed
            __builtin_amdgcn_sched_barrier(0);
            issue(ring[i], rsh[i]);  // unconditional: no data load under a branch
            if (p0 + (uint32_t)i < total) {  // wave-uniform
                const uint32_t j = cp.j;
                if (j < K) {
                    const u32x4* tp = reinterpret_cast<const u32x4*>(lds_tab + j * ts);
                    uint32_t tw[ts];
#pragma unroll
                    for (int q = 0; q < (int)(ts / 4); ++q) {
                        const u32x4 v = tp[q];
                        tw[4 * q] = v[0];
                        tw[4 * q + 1] = v[1];
                        tw[4 * q + 2] = v[2];
                        tw[4 * q + 3] = v[3];
                    }
#pragma unroll
                    for (int u = 0; u < kVpU; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const Sel sx = selectors(xs[u][e]);
#pragma unroll
                            for (int r = 0; r < R; ++r)
                                acc[u][r][e] ^= gf_mul_sel(sx, tw[5 * r], tw[5 * r + 1], tw[5 * r + 2], tw[5 * r + 3],
                                                           tw[5 * r + 4]);
                        }
                } else {
                    // stored parity r0 = j - K against the recomputed column
                    const uint32_t r0 = j - K;
                    const int32_t main_end = (int32_t)vp_main_bytes((uint32_t)cp.S);
#pragma unroll
                    for (int u = 0; u < kVpU; ++u) {
                        const int32_t cpos = (int32_t)(cp.ti * kVpTile + u * kVpWin) + 16 * (int32_t)lane;
                        const bool mine = lane < kVpStore && cpos + 16 <= main_end;
                        u32x4 want = acc[u][0];
#pragma unroll
                        for (int r = 1; r < R; ++r)
                            if (r0 == (uint32_t)r) want = acc[u][r];
                        const u32x4 df = want ^ xs[u];
                        bad |= mine && (df[0] | df[1] | df[2] | df[3]) != 0u;
                    }
                    if (r0 == R - 1u) {
                        if (__any(bad) && lane == 0u) atomicOr(flags + cp.flag, 1u);
                        bad = false;
#pragma unroll
                        for (int u = 0; u < kVpU; ++u)
#pragma unroll
                            for (int r = 0; r < R; ++r) acc[u][r] = u32x4{0, 0, 0, 0};
                    }
                }
                if (++cp.j == L && cp.t + nw < n) vp_set(cp, cp.t + nw, recs, tiles);
            }
        }
    }
}

// Bytes [vp_main_bytes(S), S) of every parity shard of every record: thread
// (record, row, slot) recomputes one byte and compares it with the stored one.
template <int R>
__global__ __launch_bounds__(kBlockThreads) void gf_verify_recs_tail(const VRec* __restrict__ recs, uint32_t n_recs,
                                                                     uint32_t K, const uint32_t* __restrict__ tab,
                                                                     uint32_t* flags) {
    constexpr uint32_t ts = vp_tab_stride(R);
    constexpr uint32_t per = (uint32_t)R * kVpTailSlots;
    const uint64_t total = (uint64_t)n_recs * per;
    typedef __attribute__((address_space(1))) const uint8_t gu8_c;
    for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t e = v / per;
        const uint32_t rem = (uint32_t)(v - e * per);
        const uint32_t r = rem / kVpTailSlots, slot = rem - r * kVpTailSlots;
        const VRec rec = recs[e];
        const uint32_t q0 = vp_main_bytes(rec.shard_len);
        if (slot >= rec.shard_len - q0) continue;
        const uint64_t S = rec.shard_len, q = (uint64_t)q0 + slot;
        uint32_t x = 0;
        for (uint32_t j = 0; j < K; ++j) {
            const uint32_t b = *reinterpret_cast<gu8_c*>(rec.a + (uint64_t)j * S + q);
            const uint32_t* t = tab + j * ts + 5 * r;
            x ^= gf_mul_sel(selectors(b), t[0], t[1], t[2], t[3], t[4]);
        }
        const uint32_t s = *reinterpret_cast<gu8_c*>(rec.b + (uint64_t)r * S + q);
        if (((x ^ s) & 0xFFu) != 0u) atomicOr(flags + rec.flag, 1u);
    }
}

template <int R>
static hipError_t launch_recs_r(const VRec* recs, uint32_t n_recs, const VTile* tiles, uint32_t n_tiles, uint32_t K,
                                const uint32_t* tab, uint32_t* flags, int cus, hipStream_t stream, int max_blocks) {
    void* args[] = {&recs, &tiles, &n_tiles, &K, &tab, &flags};
    hipError_t e = hipSuccess;
    if (n_tiles > 0) {
        // several waves per SIMD keep kVpD loads per lane in flight (as the gf_wide Verify grid)
        uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>((n_tiles + 3) / 4, (uint64_t)cus * 8));
        if (max_blocks > 0) grid = std::min<uint64_t>(grid, (uint64_t)max_blocks);
        e = hipLaunchKernel((const void*)&gf_verify_recs<R>, dim3((uint32_t)grid), dim3(kPipeBlockThreads), args, 0,
                            stream);
    }
    if (e != hipSuccess) return e;
    const uint64_t total = (uint64_t)n_recs * R * kVpTailSlots;
    const uint64_t tg = std::max<uint64_t>(1, std::min<uint64_t>((total + kBlockThreads - 1) / kBlockThreads, 4096));
    void* targs[] = {&recs, &n_recs, &K, &tab, &flags};
    return hipLaunchKernel((const void*)&gf_verify_recs_tail<R>, dim3((uint32_t)tg), dim3(kBlockThreads), targs, 0,
                           stream);
}

hipError_t launch_verify_recs(int k, int r, const VRec* recs, uint32_t n_recs, const VTile* tiles, uint32_t n_tiles,
                              const uint32_t* tab, uint32_t* flags, int cus, hipStream_t stream, int max_blocks) {
    if (!vp_fast_shape(k, r) || cus < 1) return hipErrorInvalidValue;
    if (n_recs == 0) return hipSuccess;
    switch (r) {
        case 1: return launch_recs_r<1>(recs, n_recs, tiles, n_tiles, (uint32_t)k, tab, flags, cus, stream, max_blocks);
        case 2: return launch_recs_r<2>(recs, n_recs, tiles, n_tiles, (uint32_t)k, tab, flags, cus, stream, max_blocks);
        case 3: return launch_recs_r<3>(recs, n_recs, tiles, n_tiles, (uint32_t)k, tab, flags, cus, stream, max_blocks);
        case 4: return launch_recs_r<4>(recs, n_recs, tiles, n_tiles, (uint32_t)k, tab, flags, cus, stream, max_blocks);
    }
    return hipErrorInvalidValue;
}

template <int K>
static const void* vtiles_for_r(int r) {
    switch (r) {
        case 1: return reinterpret_cast<const void*>(&gf_verify_tiles<K, 1>);
        case 2: return reinterpret_cast<const void*>(&gf_verify_tiles<K, 2>);
        case 3: return reinterpret_cast<const void*>(&gf_verify_tiles<K, 3>);
        case 4: return reinterpret_cast<const void*>(&gf_verify_tiles<K, 4>);
    }
    return nullptr;
}

static const void* vtiles_kernel(int k, int r) {
    switch (k) {
        case 1: return vtiles_for_r<1>(r);
        case 2: return vtiles_for_r<2>(r);
        case 3: return vtiles_for_r<3>(r);
        case 4: return vtiles_for_r<4>(r);
        case 5: return vtiles_for_r<5>(r);
        case 6: return vtiles_for_r<6>(r);
        case 7: return vtiles_for_r<7>(r);
        case 8: return vtiles_for_r<8>(r);
    }
    return nullptr;
}

hipError_t launch_verify_tiles(int k, int r, const VTileArgs& a, const TileRec* tiles, uint32_t* flags, int cus,
                               hipStream_t stream) {
    const void* fn = vp_tiles_shape(k, r) ? vtiles_kernel(k, r) : nullptr;
    if (!fn || cus < 1) return hipErrorInvalidValue;
    if (a.n_tiles == 0) return hipSuccess;
    // one 4-wave block per CU, as the strided Verify (kPipeBlocksPerCu)
    const uint64_t bpc = (uint64_t)std::max(1, kPipeBlocksPerCu);
    const uint64_t grid = std::max<uint64_t>(1, std::min<uint64_t>((a.n_tiles + 3) / 4, (uint64_t)cus * bpc));
    void* args[] = {const_cast<VTileArgs*>(&a), &tiles, &flags};
    return hipLaunchKernel(fn, dim3((uint32_t)grid), dim3(kBlockThreads), args, 0, stream);
}

}  // namespace hbec
