// vplan.h — Verify over a plan (vplan.hip): the records of the read-only
// kernels and the host-side routing of a plan's stripes to them.
#pragma once
#include <stdint.h>

#include <vector>

#include "kernels.h"

namespace hbec {

// gf_verify_recs walks wave tiles of kVpU windows of 62 compared 16-B columns
// (gf_wide's frame, wide.hip): kVpTile shard bytes per tile.
constexpr uint32_t kVpStore = 62;
constexpr uint32_t kVpWin = kVpStore * 16;
constexpr int kVpU = HBEC_WIDE_U;
constexpr uint32_t kVpTile = kVpU * kVpWin;
constexpr int kVpD = HBEC_WIDE_D;
constexpr uint32_t kVpTailSlots = 32;  // S - vp_main_bytes(S) < 32

// coefficient tables: per input j the R tables of 5 words, padded to 4 words
__host__ __device__ constexpr uint32_t vp_tab_stride(int r) { return (uint32_t)((r * 5 + 3) & ~3); }
// columns 16 i + 16 <= S - 16 are compared by gf_verify_recs, the rest of each
// parity shard (< 32 bytes; all of a shard of S < 32) by gf_verify_recs_tail
__host__ __device__ constexpr uint32_t vp_main_bytes(uint32_t s) { return s >= 32u ? ((s - 16u) / 16u) * 16u : 0u; }

// One stripe (b = a + k S) or object (a = data, b = parity) at any alignment.
struct VRec {
    uint64_t a;
    uint64_t b;
    uint32_t shard_len;  // <= kPos32MaxShard
    uint32_t flag;       // the stripe's position in the caller's array
};
struct VTile {
    uint32_t rec;  // index into the VRec array
    uint32_t ti;   // tile of that stripe: shard positions from ti * kVpTile
};
// A stripe of the other route (one verify call each): any k, m, shard length.
struct VOther {
    uint64_t a, b, shard_len, idx;
};

struct VerifyRecs {
    std::vector<VRec> recs;
    std::vector<VTile> tiles;
    std::vector<VOther> other;
};

// the shapes the plan Verify kernels take (others: one verify call per stripe)
inline bool vp_fast_shape(int k, int m) { return k >= 1 && k <= kOddMaxK && m >= 1 && m <= kMaxR; }
// tile records (TileRec, pad_ = flag index) are verified by gf_verify_tiles for k <= kStripeMaxK
inline bool vp_tiles_shape(int k, int m) { return vp_fast_shape(k, m) && k <= kStripeMaxK; }

// Route one non-empty stripe / object that has no tile records of its own
// (or whose shape gf_verify_tiles does not take).  false: too many tiles.
inline bool vp_add(VerifyRecs& v, int k, int m, uint64_t a, uint64_t b, uint64_t shard_len, uint64_t idx) {
    if (!vp_fast_shape(k, m) || !pos32_shard(shard_len)) {
        v.other.push_back({a, b, shard_len, idx});
        return true;
    }
    const uint32_t s = (uint32_t)shard_len, rec = (uint32_t)v.recs.size();
    const uint32_t nt = (vp_main_bytes(s) + kVpTile - 1) / kVpTile;
    if (v.recs.size() >= (1ull << 31) - 1 || v.tiles.size() + nt >= (1ull << 31)) return false;
    v.recs.push_back({a, b, s, (uint32_t)idx});
    for (uint32_t t = 0; t < nt; ++t) v.tiles.push_back({rec, t});
    return true;
}

// tab: device, k * vp_tab_stride(r) words, coefficient (r, j) at j * stride + 5 r.
// The tile kernel over the records, then the byte tail of every record.
// max_blocks > 0 caps the tile kernel's grid (records read over PCIe).
hipError_t launch_verify_recs(int k, int r, const VRec* recs, uint32_t n_recs, const VTile* tiles, uint32_t n_tiles,
                              const uint32_t* tab, uint32_t* flags, int cus, hipStream_t stream, int max_blocks = 0);
// Aligned tiles (TileRec::pad_ = flag index): data shard j of a tile at in_addr +
// j * in_stride, parity r at in_addr + (k + r) * in_stride, or (split, object
// plans) at out_addr + r * out_stride.
struct VTileArgs {
    uint32_t n_tiles;
    uint32_t split;
    uint32_t tab[kMaxR][kMaxK][5];  // parity row r, data shard j (gf256.h perm_table)
};
hipError_t launch_verify_tiles(int k, int r, const VTileArgs& a, const TileRec* tiles, uint32_t* flags, int cus,
                               hipStream_t stream);

}  // namespace hbec
