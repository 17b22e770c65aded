// plan_internal.h — what plan.cpp (building a plan, the calls with one pattern
// for all) and plan_calls.cpp (the calls with a pattern or selection per source
// entry) share: the plan itself and a few helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/hbec.h"
#include "hashplan.h"
#include "heal.h"
#include "internal.h"
#include "kernels.h"
#include "mixedplan.h"
#include "vplan.h"

struct hbec_plan {
    int k = 0, m = 0;
    int tile_bytes = 0;
    hbec::TileRec* d_tiles = nullptr;
    uint64_t n_tiles = 0;
    std::vector<hbec_stripe> tiled;     // stripes covered by d_tiles
    std::vector<hbec_stripe> fallback;  // stripes coded one by one
    // object plans (hbec_plan_objects): data shards and parity shards in
    // separate regions; tiles carry base A = data, base B = parity
    bool objects = false;
    std::vector<hbec_object> obj_tiled, obj_fallback;
    uint64_t shard_bytes = 0;           // sum of shard_len over all stripes
    // stripes / objects the tiled kernel cannot take: unaligned-kernel records
    hbec::URec* d_urecs = nullptr;
    uint64_t n_urecs = 0;
    // gf_odd: one edge record per such stripe / object (its guard-band bytes)
    hbec::URec* d_erecs = nullptr;
    uint64_t n_erecs = 0;
    // shards of 2^31 bytes or more (gf_odd positions are 32-bit), or all of
    // them with HBEC_ODD=0: round-2 gf_apply_unaligned_plan records
    hbec::URec* d_brecs = nullptr;
    uint64_t n_brecs = 0;
    // gf_odd_rec: one record per stripe / object with a main-kernel part,
    // and the tile lists the record kernels walk (one per tile span)
    hbec::URec* d_orecs = nullptr;
    uint32_t* d_lists[hbec::kOddSpans] = {};
    hbec::OddStripeRecs orecs;
    std::unique_ptr<hbec::OddRecCache> rec_cache;  // plan.cpp: built and freed there only
    // Verify (hbec_verify_plan).  Every tile record carries its stripe's
    // position in the caller's array (TileRec::pad_); the stripes without tile
    // records, or of a shape gf_verify_tiles does not take, have a VRec and
    // their {record, tile} list; `vother` are the stripes verified one by one.
    uint64_t n_src = 0;  // entries of the caller's array (zero-length ones included)
    hbec::VRec* d_vrecs = nullptr;
    hbec::VTile* d_vtiles = nullptr;
    uint32_t* d_vtab = nullptr;  // [k][vp_tab_stride(m)] parity coefficient tables
    uint64_t n_vrecs = 0, n_vtiles = 0;
    std::vector<hbec::VOther> vother;
    // Reconstruct and Verify with a pattern per stripe (hbec_reconstruct_plan_mixed,
    // hbec_verify_plan_mixed): where
    // every source entry lives, by its position in the caller's array; the
    // device records and the static {entry, tile} list are built by the first
    // such call (mp_mu), so a plan that never makes one pays for neither.
    std::vector<hbec::MSrc> src;
    mutable std::mutex mp_mu;
    mutable bool mp_built = false;
    mutable hbec::MRec* d_mrecs = nullptr;
    mutable hbec::MTile* d_mtiles = nullptr;
    mutable uint64_t n_mtiles = 0;
    mutable std::vector<uint32_t> mp_other;  // source positions rebuilt one call each
    // a call's pattern records and per-entry words (device), reused call after
    // call (plan_calls.cpp staged_launches: the discipline of mp_mu and mp_ev)
    mutable uint32_t* d_mstage = nullptr;
    mutable size_t mstage_words = 0;
    mutable hipEvent_t mp_ev = nullptr;  // after the last call's launches, on mp_stream
    mutable hipStream_t mp_stream = nullptr;
    // hbec_split_plan on a plan of m = 0, a scatter: no _mixed call has work
    // there, so mp_build lists no tile of it and the first split builds records
    // and a list of its own (mp_mu), routed by k and S alone.  With m > 0 the
    // call walks d_mrecs / d_mtiles.
    mutable bool sp_built = false;
    mutable hbec::MRec* d_sprecs = nullptr;
    mutable hbec::MTile* d_sptiles = nullptr;
    mutable uint64_t n_sptiles = 0;
    mutable std::vector<uint32_t> sp_other;
    // hbec_heal_plan_mixed: the records and tables of the last call's masks, on
    // the host (heal_mu) and on the device (d_heal, under mp_mu and ordered by
    // mp_ev like d_mstage).  They depend on (k, m) and the masks alone, and a
    // sweep heals under the masks it has, call after call: the next call with
    // the same masks inverts no matrix per mask with one shard left out and
    // stages one index per source entry, nothing else.
    mutable std::mutex heal_mu;
    mutable std::vector<uint32_t> heal_bits;
    mutable std::shared_ptr<const hbec::HealStage> heal_cache;
    mutable uint32_t* d_heal = nullptr;
    mutable size_t heal_dev_words = 0;
    mutable std::shared_ptr<const hbec::HealStage> heal_on_device;  // what d_heal holds
    // hbec_hash_plan_mixed: a record per source entry with its length in 64 bits
    // and the non-empty entries longest first, built by the first such call (mp_mu)
    mutable bool hash_built = false;
    mutable hbec::HRec* d_hrecs = nullptr;
    mutable std::vector<uint32_t> hash_order;
    // shards plans (hbec_plan_shards, hbec_plan_files): shard j of source entry i
    // is at rows[i (k + m) + j]; d_rows is the same table on the device and
    // src[i].a the device address of row i (b = 0).
    // No tile, unaligned or Verify records: every call runs over src.
    bool shards = false;
    std::vector<uint64_t> rows;
    uint64_t* d_rows = nullptr;
};

namespace hbec {

// (static: helpers of the two files, not symbols of the library)
template <class T>
static int upload(const std::vector<T>& recs, T** dst, const char* what) {
    if (recs.empty()) return HBEC_OK;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), recs.size() * sizeof(T));
    if (e != hipSuccess) return hip_fail(e, what);
    e = hipMemcpy(*dst, recs.data(), recs.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(*dst);
        *dst = nullptr;
        return hip_fail(e, what);
    }
    return HBEC_OK;
}

// Where shard `sh` of source entry i of a plan is (the host's copy of the rule
// the kernels hold: two bases, or the entry's row of a shards plan).
static inline uint64_t shard_addr(const hbec_plan* p, uint32_t i, int sh) {
    if (p->shards) return p->rows[(size_t)i * (size_t)(p->k + p->m) + (size_t)sh];
    const MSrc& s = p->src[i];
    return sh < p->k ? s.a + (uint64_t)sh * s.shard_len : s.b + (uint64_t)(sh - p->k) * s.shard_len;
}

// CU count of the current device
static inline int current_cus(int* cus) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    return device_cus(dev, cus);
}

// One verify call for source entry i of a plan, all of its shards present
// (plan.cpp: what verify_other_run does, counted with it, for any kind of plan).
int verify_plan_entry(hbec_codec* codec, const hbec_plan* plan, uint32_t i, uint32_t* d_flags, hipStream_t stream);

}  // namespace hbec
