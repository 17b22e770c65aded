// mixedplan.h — reconstruct over a plan with an erasure pattern per stripe
// (hbec_reconstruct_plan_mixed): the records of gf_mixed_plan (mixedplan.hip)
// and the host-side routing of a plan's source entries to it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "gf256.h"
#include "kernels.h"
#include "vplan.h"

namespace hbec {

// One source entry of a plan, by its position in the caller's array: shard i
// is at (i < k ? a + i S : b + (i - k) S).  Stripes: b = a + k S; objects:
// a = data, b = parity.  Zero-length entries have S = 0.
struct MSrc {
    uint64_t a, b, shard_len;
};

// Device record of one source entry (every entry has one, so the per-call
// pattern array is indexed by the caller's positions).
struct MRec {
    uint64_t a;
    uint64_t b;
    uint32_t shard_len;  // <= kPos32MaxShard; 0: zero-length or other route (no tiles)
    uint32_t pad_;
};
// Static list in source order: tile `ti` of entry `rec` (shard positions from
// ti * mixed_plan_tile_bytes()).
struct MTile {
    uint32_t rec;
    uint32_t ti;
};

// One erasure pattern of a call, as words: the k survivor and r output shard
// indices, a byte each (input j in word j / 4, bits 8 (j % 4); outputs in word
// 3), then the v_perm tables of decode row q x survivor j (gf256.h perm_table)
// at word kMPatHdr + 5 (j r + q): the kernel reads the r rows of one input
// together.  Records are padded to 16 B and only as long as their k r needs
// (4+2 double loss: 176 B; 12+4 quadruple: 976 B), since they travel with
// every call.
constexpr uint32_t kMPatHdr = 4;
inline uint32_t mp_pattern_words(int k, int r) { return (kMPatHdr + 5u * (uint32_t)(k * r) + 3u) & ~3u; }
// Per-call word of a source entry: (r << kMPatShift) | record offset in 16-B
// units, r its output count; 0 = nothing to rebuild.  65536 records of 976 B
// are 2^22 units.
constexpr uint32_t kMPatShift = 28;
constexpr uint32_t kMPatMask = (1u << kMPatShift) - 1u;

struct MixedPlanRecs {
    std::vector<MRec> recs;    // one per source entry
    std::vector<MTile> tiles;  // kernel-route entries only
    std::vector<uint32_t> other;  // source positions coded one call each
};

// shard bytes per tile of the list, for every kernel that walks it (Verify,
// repair, locate and heal too)
uint32_t mixed_plan_tile_bytes();

// the shapes gf_mixed_plan takes: those of the plan Verify kernels
inline bool mp_fast_shape(int k, int m) { return vp_fast_shape(k, m); }

// Route every source entry.  false: too many tiles (>= 2^31).
inline bool mp_build(MixedPlanRecs& o, int k, int m, const std::vector<MSrc>& src, uint32_t tile_bytes) {
    o.recs.assign(src.size(), MRec{0, 0, 0, 0});
    for (size_t i = 0; i < src.size(); ++i) {
        const MSrc& s = src[i];
        if (s.shard_len == 0) continue;
        if (!mp_fast_shape(k, m) || !pos32_shard(s.shard_len)) {
            o.other.push_back((uint32_t)i);
            continue;
        }
        o.recs[i] = MRec{s.a, s.b, (uint32_t)s.shard_len, 0};
        const uint64_t nt = (s.shard_len + tile_bytes - 1) / tile_bytes;
        if (o.tiles.size() + nt >= (1ull << 31)) return false;
        for (uint64_t t = 0; t < nt; ++t) o.tiles.push_back(MTile{(uint32_t)i, (uint32_t)t});
    }
    return true;
}

// Append one pattern record built from its decode rows (n_out x k
// coefficients; k <= kOddMaxK, n_out <= kMaxR); returns its offset in 16-B units.
inline uint32_t mp_pattern(std::vector<uint32_t>& buf, int k, const int* surv, const int* outs, int n_out,
                           const uint8_t* rows) {
    const size_t at = buf.size();
    buf.resize(at + mp_pattern_words(k, n_out), 0u);
    uint32_t* p = buf.data() + at;
    for (int j = 0; j < k; ++j) p[j / 4] |= (uint32_t)surv[j] << (8 * (j % 4));
    for (int q = 0; q < n_out; ++q) {
        p[3] |= (uint32_t)outs[q] << (8 * q);
        for (int j = 0; j < k; ++j) perm_table(rows[(size_t)q * k + j], p + kMPatHdr + 5 * (j * n_out + q));
    }
    return (uint32_t)(at / 4);
}

// Tiles [0, n_tiles) of `tiles`: codes every tile whose entry's pattern has 1..r
// outputs (r: the largest count in the call).  K <= kOddMaxK inputs, 1 <= r <= kMaxR.
// rows: the records are a shards plan's (a = the entry's address row, shardplan.h).
hipError_t launch_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                             const uint32_t* pat_of, const uint32_t* pats, int cus, hipStream_t stream,
                             bool rows = false);

}  // namespace hbec
