// mixed.h — launch interface of gf_apply_mixed (mixed.hip): reconstruct with
// an erasure pattern per object in one launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace hbec {

// One record per pattern: input j of object o starts at in_base[j] +
// o*in_stride[j] (the pattern's k survivors in index order), output r at
// out_base[r] + o*out_stride[r] (its missing shards), tab[r][j] the v_perm
// tables of decode row r (gf256.h perm_table).  A launch codes n_tiles tiles
// of mixed_tile_bytes(k) bytes: tile t is shard column t % tiles_per_obj of
// list entry t / tiles_per_obj; every record a launch's entries name has that
// launch's r outputs.
constexpr int kMixedMaxK = 8;
struct MixedRec {
    uint64_t in_base[kMixedMaxK];
    uint64_t in_stride[kMixedMaxK];
    uint64_t out_base[kMaxR];
    uint64_t out_stride[kMaxR];
    uint32_t tab[kMaxR][kMixedMaxK][5];
};
struct MixedEnt {
    uint32_t obj;
    uint32_t rec;
};
struct MixedArgs {
    uint32_t n_tiles;        // entries * tiles_per_obj (< 2^31)
    uint32_t tiles_per_obj;  // ceil(shard_len / mixed_tile_bytes(k))
    uint32_t shard_len;      // multiple of 16, <= kPos32MaxShard
    // wave w takes tiles w*wave_step + i*iter_step, i < iters; every tile
    // below n_tiles is taken once: (1, waves, ceil(n_tiles / waves)) or
    // (iters, 1, iters) with waves = grid * kBlockThreads / 64
    uint32_t wave_step;
    uint32_t iter_step;
    uint32_t iters;
};
int mixed_tile_bytes(int k);
hipError_t launch_mixed(int k, int r, const MixedArgs& a, const MixedRec* recs, const MixedEnt* list, int grid,
                        hipStream_t stream);

}  // namespace hbec
