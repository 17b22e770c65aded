// mixed.hip — one-launch GF(2^8) reconstruct over a batch whose objects have
// lost DIFFERENT shards (hbec_reconstruct_batch_mixed): a repair sweep over
// the objects hit by a failed device, where shard i of a partition's objects
// lives on ring.GetNodes(partition)[i] (objectserver/ecobj.go:348-357), so the
// dead disk held shard 0 of one object and a parity shard of the next.
//
// The strided and stripe kernels carry one coefficient table and one set of
// shard roles in their launch arguments.  Here both come from memory: the
// host writes one record per erasure pattern (mixed.h MixedRec: the k
// survivor and r output bases and strides of object 0, and the v_perm tables
// of the r decode rows) and a list of {object, record} entries sorted by
// record.  Tile t of a launch is TILE = stripes_u(K) KiB of shard column
// (t % tiles_per_obj) of entry t / tiles_per_obj.  Waves walk the tiles with
// the pipeline of gf_apply_stripes: the NEXT tile's data loads are in flight,
// and the bases of the tile after that resolved, while the current tile
// computes and stores.  The tables live in VGPRs (8+3 needs 120 words) and
// are refreshed only when the wave's record changes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.h"
#include "kernels.h"
#include "mixed.h"

namespace hbec {

// every word in VGPRs whatever K*R: the SGPRs hold three tiles' shard addresses
template <int K, int R>
using MixedTables = Tables<K, R, 1>;

// The record index is wave-uniform and `recs` a read-only __restrict__
// argument, so these are scalar loads.
template <int K, int R>
__device__ __forceinline__ MixedTables<K, R> load_mixed_tables(const MixedRec* __restrict__ recs, uint32_t rec) {
    MixedTables<K, R> t;
    const MixedRec& m = recs[rec];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            t.lo0[r][j] = to_vgpr(m.tab[r][j][0]);
            t.lo2[r][j] = to_vgpr(m.tab[r][j][2]);
            t.hi[r][j][0] = to_vgpr(m.tab[r][j][1]);
            t.hi[r][j][1] = to_vgpr(m.tab[r][j][3]);
            t.hi[r][j][2] = to_vgpr(m.tab[r][j][4]);
        }
    return t;
}

// One tile, resolved: the shard addresses of its first byte, all wave-uniform.
template <int K, int R>
struct MixedTile {
    uint64_t src[K];
    uint64_t dst[R];
    uint32_t rec;
    uint32_t valid;  // bytes of the tile inside the shard (>= 16, multiple of 16)
    uint32_t live;   // bytes this wave stores: valid, or 0 for a past-the-end stand-in
};

template <int K, int R, int U>
__device__ __forceinline__ MixedTile<K, R> mixed_tile(const MixedArgs& a, const MixedRec* __restrict__ recs,
                                                      const MixedEnt* __restrict__ list, uint32_t t) {
    MixedTile<K, R> o;
    const bool in = t < a.n_tiles;
    const uint32_t tc = in ? t : a.n_tiles - 1u;  // stand-in: the launch's last tile, nothing stored
    const uint32_t e = tc / a.tiles_per_obj;
    const uint32_t p0 = (tc - e * a.tiles_per_obj) * ((uint32_t)U * 1024u);  // < shard_len <= kPos32MaxShard
    const MixedEnt ent = list[e];
    const MixedRec& m = recs[ent.rec];
#pragma unroll
    for (int j = 0; j < K; ++j) o.src[j] = m.in_base[j] + (uint64_t)ent.obj * m.in_stride[j] + p0;
#pragma unroll
    for (int r = 0; r < R; ++r) o.dst[r] = m.out_base[r] + (uint64_t)ent.obj * m.out_stride[r] + p0;
    const uint32_t left = a.shard_len - p0;
    o.rec = ent.rec;
    o.valid = left < (uint32_t)U * 1024u ? left : (uint32_t)U * 1024u;
    o.live = in ? o.valid : 0u;
    return o;
}

template <int K, int U>
__device__ __forceinline__ void load_mixed_tile(u32x4 (&x)[U][K], const uint64_t (&src)[K], uint32_t valid,
                                                uint32_t lane) {
    const uint32_t last = valid - 16u;  // lanes past the shard's end re-read its last 16 B
#pragma unroll
    for (int u = 0; u < U; ++u) {
        uint32_t off = lane * 16u + (uint32_t)u * 1024u;
        off = off < last ? off : last;
#pragma unroll
        for (int j = 0; j < K; ++j) x[u][j] = ld16_addr(src[j] + off);
    }
}

template <int K, int R, int U, bool FULL>
__device__ __forceinline__ void store_mixed_tile_(const u32x4 (&x)[U][K], const MixedTables<K, R>& tb,
                                                  const uint64_t (&dst)[R], uint32_t live, uint32_t lane,
                                                  const TabArray& none) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t off = lane * 16u + (uint32_t)u * 1024u;
        u32x4 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = u32x4{0, 0, 0, 0};
        gf_dot<K, R, 1>(acc, x[u], none, tb);  // all five words from tb: `none` is never read
        if (FULL || off < live) {
#pragma unroll
            for (int r = 0; r < R; ++r) st16_addr(dst[r] + off, acc[r]);
        }
    }
}

template <int K, int R, int U>
__device__ __forceinline__ void store_mixed_tile(const u32x4 (&x)[U][K], const MixedTables<K, R>& tb,
                                                 const uint64_t (&dst)[R], uint32_t live, uint32_t lane,
                                                 const TabArray& none) {
    if (live >= (uint32_t)U * 1024u)  // wave-uniform: whole tile live
        store_mixed_tile_<K, R, U, true>(x, tb, dst, live, lane, none);
    else
        store_mixed_tile_<K, R, U, false>(x, tb, dst, live, lane, none);
}

// Wave w of the launch takes tiles w * wave_step + i * iter_step, i < iters:
// (1, waves) is the grid-stride walk of gf_apply_stripes, (iters, 1) a
// contiguous run of the sorted list per wave, so a wave meets few records.
// Either way the trip count is block-uniform (one block barrier per tile, as
// gf_apply_stripes): waves past the end load a stand-in tile and store nothing.
template <int K, int R>
__global__ __launch_bounds__(kBlockThreads, 1) void gf_apply_mixed(MixedArgs a, const MixedRec* __restrict__ recs,
                                                                   const MixedEnt* __restrict__ list) {
    constexpr int U = stripes_u(K);
    constexpr uint32_t WPB = kBlockThreads / 64;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave0 = __builtin_amdgcn_readfirstlane(xcd_block() * WPB);
    const uint32_t dw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave0 * a.wave_step >= a.n_tiles) return;  // whole blocks only: the loop below has block barriers
    // never read (gf_dot's table argument when every word is in VGPRs)
    const TabArray& none = *reinterpret_cast<const TabArray*>(recs);
    uint32_t t = (wave0 + dw) * a.wave_step;
    MixedTile<K, R> cur = mixed_tile<K, R, U>(a, recs, list, t);
    MixedTables<K, R> tb = load_mixed_tables<K, R>(recs, cur.rec);
    u32x4 x[U][K];
    load_mixed_tile<K, U>(x, cur.src, cur.valid, lane);
    MixedTile<K, R> nxt = mixed_tile<K, R, U>(a, recs, list, t + a.iter_step);
    for (uint32_t i = 1; i < a.iters; ++i) {  // block-uniform trip count
        t += a.iter_step;
        u32x4 y[U][K];
        load_mixed_tile<K, U>(y, nxt.src, nxt.valid, lane);  // data one tile ahead
        // the entry, record and addresses two tiles ahead, after the data
        // loads are issued: their scalar-load latency overlaps the wait for x
        const MixedTile<K, R> after = mixed_tile<K, R, U>(a, recs, list, t + a.iter_step);
        __builtin_amdgcn_s_barrier();
        store_mixed_tile<K, R, U>(x, tb, cur.dst, cur.live, lane, none);
        if (nxt.rec != cur.rec) tb = load_mixed_tables<K, R>(recs, nxt.rec);  // wave-uniform
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < K; ++j) x[u][j] = y[u][j];
        cur = nxt;
        nxt = after;
    }
    store_mixed_tile<K, R, U>(x, tb, cur.dst, cur.live, lane, none);
}

template <int K>
static const void* mixed_for_r(int r) {
    switch (r) {
        case 1: return reinterpret_cast<const void*>(&gf_apply_mixed<K, 1>);
        case 2: return reinterpret_cast<const void*>(&gf_apply_mixed<K, 2>);
        case 3: return reinterpret_cast<const void*>(&gf_apply_mixed<K, 3>);
        case 4: return reinterpret_cast<const void*>(&gf_apply_mixed<K, 4>);
    }
    return nullptr;
}

static const void* mixed_kernel(int k, int r) {
    switch (k) {
        case 1: return mixed_for_r<1>(r);
        case 2: return mixed_for_r<2>(r);
        case 3: return mixed_for_r<3>(r);
        case 4: return mixed_for_r<4>(r);
        case 5: return mixed_for_r<5>(r);
        case 6: return mixed_for_r<6>(r);
        case 7: return mixed_for_r<7>(r);
        case 8: return mixed_for_r<8>(r);
    }
    return nullptr;
}

int mixed_tile_bytes(int k) { return stripes_u(k) * 1024; }

hipError_t launch_mixed(int k, int r, const MixedArgs& a, const MixedRec* recs, const MixedEnt* list, int grid,
                        hipStream_t stream) {
    const void* fn = mixed_kernel(k, r);
    if (!fn) return hipErrorInvalidValue;
    void* args[] = {const_cast<MixedArgs*>(&a), &recs, &list};
    return hipLaunchKernel(fn, dim3(grid), dim3(kBlockThreads), args, 0, stream);
}

}  // namespace hbec
