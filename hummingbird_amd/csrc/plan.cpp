// plan.cpp — stripe plans: a batch of stripes of mixed shard lengths coded in
// one launch (stripes.hip).  A stripe is ecSplit's databuf layout
// (objectserver/ecutils.go:31-35,55-58): k+m shards of shard_len bytes back
// to back, data first.  Stripes the tiled kernel cannot take (unaligned:
// S % 16 != 0 for 15 object sizes in 16; every object of an object plan with
// k > 8) are coded by one more launch per pass of gf_apply_unaligned_plan over
// their own records; stripe plans with k > 8 run the tiled kernel in
// accumulate passes.  Verify of a plan (hbec_verify_plan) is read-only and
// runs over the same tile records plus per-stripe records of its own
// (vplan.h, vplan.hip).  Reconstruct with an erasure pattern per stripe
// (hbec_reconstruct_plan_mixed) runs over per-source-entry records and a tile
// list of its own, built on first use (mixedplan.h, mixedplan.hip); Verify with
// a present mask per stripe (hbec_verify_plan_mixed) reads the same records and
// list (vmixed.h, vmixed.hip), and so does the call that rebuilds and checks in
// one pass (hbec_repair_plan_mixed; repair.h, repair.hip) and the call that
// rebuilds the shard locate named (hbec_heal_plan_mixed; heal.h, heal.hip).
// The ShardHash audit of a plan (hbec_hash_plan_mixed; hashplan.h, hashplan.hip)
// has records of its own with 64-bit lengths, built on first use likewise, and
// stages its chain list where those calls stage their words.  The hash of
// multi-stripe shard files (hbec_hash_plan_files; hashfiles.h, hashfiles.hip)
// reads the same records and stages its chains and object table there too.
// A plan whose entries name every shard (hbec_plan_shards, hbec_plan_files;
// shardplan.h) has those records and lists only, with a row of shard addresses
// where the others have two bases: every call with a pattern per entry takes it
// as it takes the others, and the calls with one pattern for all run the same
// kernels with that pattern for every entry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/hbec.h"
#include "gf256.h"
#include "hashfiles.h"
#include "hashplan.h"
#include "heal.h"
#include "internal.h"
#include "kernels.h"
#include "locate.h"
#include "mixedplan.h"
#include "repair.h"
#include "shardplan.h"
#include "vmixed.h"
#include "vplan.h"

using hbec::fail;
using hbec::hip_fail;

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
    std::unique_ptr<hbec::OddRecCache> rec_cache;
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
    // a call's pattern records and per-entry words (device), reused call after call
    mutable uint32_t* d_mstage = nullptr;
    mutable size_t mstage_words = 0;
    mutable hipEvent_t mp_ev = nullptr;  // after the last call's launches, on mp_stream
    mutable hipStream_t mp_stream = nullptr;
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

// The gf_odd_rec records of a plan pass depend only on the plan's stripes and
// on which shards the pass reads and writes, not on its coefficients: a
// plan keeps those it built (the encode pass, recurring erasure patterns)
// instead of rebuilding them on every call (gf_odd_planrec: 13-15 us of a
// 16384-stripe 8+3 plan's 250 us, r6_trace_mid).  Built on the first
// caller's stream; a caller on another stream waits for that build's event.
struct hbec::OddRecCache {
    static constexpr size_t kMaxEntries = 16;
    struct Entry {
        std::vector<uint32_t> key;
        uint32_t* d = nullptr;
        hipEvent_t ev = nullptr;
        hipStream_t stream = nullptr;
    };
    std::mutex mu;
    std::vector<Entry> entries;
    ~OddRecCache() {
        for (auto& x : entries) {
            if (x.ev) (void)hipEventDestroy(x.ev);
            if (x.d) (void)hipFree(x.d);
        }
    }
};

namespace {

bool aligned_stripe(const hbec_stripe& s) {
    return (reinterpret_cast<uintptr_t>(s.base) & 15u) == 0 && (s.shard_len % 16) == 0 &&
           s.shard_len < (1ull << 32);
}

bool aligned_object(const hbec_object& o) {
    return ((reinterpret_cast<uintptr_t>(o.data) | reinterpret_cast<uintptr_t>(o.parity)) & 15u) == 0 &&
           (o.shard_len % 16) == 0 && o.shard_len < (1ull << 32);
}

std::mutex g_occ_mu;

void add_urecs(std::vector<hbec::URec>& recs, std::vector<hbec::URec>& erecs, std::vector<hbec::URec>& brecs,
               std::vector<hbec::URec>& orecs, const void* a, const void* b, uint64_t s, int k) {
    const uint64_t ua = reinterpret_cast<uint64_t>(a), ub = reinterpret_cast<uint64_t>(b);
    if (!hbec::odd_enabled() || !hbec::pos32_shard(s)) {
        const uint64_t tile = (uint64_t)hbec::unaligned_tile_bytes();
        for (uint64_t p0 = 0; p0 < s; p0 += tile) brecs.push_back({ua, ub, s, p0});
        return;
    }
    const uint64_t tile = hbec::urec_tile_for(std::min(k, hbec::kOddMaxK), false), span = hbec::urec_span(s);
    for (uint64_t p0 = 0; p0 < span; p0 += tile) recs.push_back({ua, ub, s, p0});
    erecs.push_back({ua, ub, s, 0});
    if (span > 0) orecs.push_back({ua, ub, s, 0});
}

// Tile lists of the per-stripe records: for each record-kernel tile span,
// tile t of stripe e for t < odd_frame_tiles(S_e, span), stripe by stripe,
// as {e, t, S_e | flags << 30, 0} (kernels.h kOddListWords): flag 1 the
// stripe's first tile, 2 its last (apply passes code the guard band there,
// HBEC_ODD_EDGE_FUSE; bits 0-29 hold S when S < 2^30, else the stripe's edges
// go to gf_odd_edges_plan).  A one-tile stripe has two entries, {e, 0, S | 1 <<
// 30} and {e, 0, S | 2 << 30 | 1 << 29}: bit 29 = guard-band bytes only.
int build_tile_lists(hbec_plan* p, const std::vector<hbec::URec>& orecs) {
    p->orecs = hbec::OddStripeRecs{};
    if (orecs.empty()) return HBEC_OK;
    uint32_t spans[hbec::kOddSpans];
    hbec::odd_plan_spans(spans);
    uint64_t s_max = 0;
    for (const auto& r : orecs) s_max = std::max<uint64_t>(s_max, r.shard_len);
    for (int i = 0; i < hbec::kOddSpans; ++i) {
        std::vector<uint32_t> l;
        for (size_t e = 0; e < orecs.size(); ++e) {
            const uint64_t S = orecs[e].shard_len;
            const uint64_t nt = hbec::odd_frame_tiles(S, spans[i]);
            const bool small = S < (1ull << 30);
            auto put = [&](uint64_t t, uint32_t fl, uint32_t only) {
                l.push_back((uint32_t)e);
                l.push_back((uint32_t)t);
                l.push_back(small && fl ? (uint32_t)S | (fl << 30) | only : 0u);
                l.push_back(0u);
            };
            for (uint64_t t = 0; t < nt; ++t) put(t, t == 0 ? 1u : (t + 1 == nt ? 2u : 0u), 0u);
            if (nt == 1 && small) put(0, 2u, 1u << 29);
        }
        if (l.size() / hbec::kOddListWords >= (1ull << 31))
            return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^31 record tiles)");
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_lists[i]), l.size() * 4);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc plan tile list");
        e = hipMemcpy(p->d_lists[i], l.data(), l.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpy plan tile list");
        p->orecs.lists[i] = hbec::OddTileList{spans[i], p->d_lists[i], l.size() / hbec::kOddListWords};
    }
    p->rec_cache = std::make_unique<hbec::OddRecCache>();
    p->orecs.cache = p->rec_cache.get();
    p->orecs.recs = p->d_orecs;
    p->orecs.n = orecs.size();
    p->orecs.s_max = s_max;
    return HBEC_OK;
}

template <class T>
int upload(const std::vector<T>& recs, T** dst, const char* what) {
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
uint64_t shard_addr(const hbec_plan* p, uint32_t i, int sh) {
    if (p->shards) return p->rows[(size_t)i * (size_t)(p->k + p->m) + (size_t)sh];
    const hbec::MSrc& s = p->src[i];
    return sh < p->k ? s.a + (uint64_t)sh * s.shard_len : s.b + (uint64_t)(sh - p->k) * s.shard_len;
}

// One pass of a plan over per-stripe records: the records of every stripe in
// one launch (stream-ordered scratch), then one gf_odd_rec launch over the
// tile list of the span the pass's kernel uses.
int odd_stripe_rec_pass(int K, int R, int mode, const hbec::UPlanArgs& a, const hbec::OddStripeRecs& o, int cus,
                        int max_blocks, hipStream_t stream, bool one_pass, bool* fused) {
    const uint64_t rw = hbec::odd_rec_words(K, R, mode);
    const int xs = hbec::odd_bp_schedule(K, R, mode, a.tab, true);
    const uint32_t span = hbec::odd_rec_tile_span(K, mode, xs);
    const hbec::OddTileList* tl = nullptr;
    for (const auto& l : o.lists)
        if (l.span == span) tl = &l;
    if (!tl || !tl->d) return fail(HBEC_ERR_INVALID_ARG, "plan has no tile list for this pass");
    uint32_t* recs = nullptr;
    bool cached = false;
    hipError_t e = hipSuccess;
    if (o.cache) {
        std::vector<uint32_t> key{(uint32_t)K, (uint32_t)R, (uint32_t)mode, a.in_sel, a.out_sel};
        key.insert(key.end(), a.in_idx, a.in_idx + K);
        key.insert(key.end(), a.out_idx, a.out_idx + R);
        std::lock_guard<std::mutex> lk(o.cache->mu);
        for (const auto& x : o.cache->entries) {
            if (x.key != key) continue;
            if (x.stream != stream) {
                e = hipStreamWaitEvent(stream, x.ev, 0);
                if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent (plan records)");
            }
            recs = x.d;
            cached = true;
        }
        if (!cached && o.cache->entries.size() < hbec::OddRecCache::kMaxEntries) {
            hbec::OddRecCache::Entry x;
            x.key = std::move(key);
            x.stream = stream;
            if (hipMalloc(reinterpret_cast<void**>(&x.d), o.n * rw * 4) == hipSuccess) {
                e = hbec::launch_odd_planrec(K, R, mode, a, o.recs, (uint32_t)o.n, x.d, stream);
                if (e == hipSuccess) e = hipEventCreateWithFlags(&x.ev, hipEventDisableTiming);
                if (e == hipSuccess) e = hipEventRecord(x.ev, stream);
                if (e != hipSuccess) {
                    if (x.ev) (void)hipEventDestroy(x.ev);
                    (void)hipFree(x.d);
                    return hip_fail(e, "launch gf_odd_planrec (plan records)");
                }
                recs = x.d;
                cached = true;
                o.cache->entries.push_back(std::move(x));
            } else {
                (void)hipGetLastError();  // HBM full: per-call scratch records below
            }
        }
    }
    if (!cached) {
        int rc = hbec::scratch_alloc(o.n * rw * 4, stream, reinterpret_cast<void**>(&recs));
        if (rc) return rc;
        e = hbec::launch_odd_planrec(K, R, mode, a, o.recs, (uint32_t)o.n, recs, stream);
        if (e != hipSuccess) {
            hbec::scratch_free(recs, stream);
            return hip_fail(e, "launch gf_odd_planrec");
        }
    }
    hbec::PassArgs c;
    std::memset(&c, 0, sizeof(c));
    std::memcpy(c.tab, a.tab, sizeof(c.tab));
    c.n_obj = o.n;
    c.shard_len = o.s_max;
    c.tiles_per_obj = 1;
    c.n_tiles = (uint32_t)tl->n;
    c.list = tl->d;
    // the record kernel codes the guard band of the stripes it covers (the
    // tile list's edge flags) when this pass's inputs are all of them
    *fused = one_pass && o.s_max < (1ull << 30) && hbec::odd_edge_fuse(K, R, mode, true, xs, true, o.s_max);
    c.fuse = *fused ? 1u : 0u;
    const uint64_t wpb = hbec::odd_waves_per_block(xs);
    const uint64_t want = (c.n_tiles + wpb - 1) / wpb;
    uint64_t cap = (uint64_t)cus * (uint64_t)hbec::odd_blocks_per_cu(mode, K, R, false, true, xs);
    if (max_blocks > 0) cap = std::min<uint64_t>(cap, (uint64_t)max_blocks);
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(want, cap));
    e = hbec::launch_odd(K, R, mode, c, nullptr, recs, grid, stream, xs);
    if (!cached) hbec::scratch_free(recs, stream);
    if (e != hipSuccess) return hip_fail(e, "launch gf_odd_rec (plan)");
    return HBEC_OK;
}

// The plan's Verify records and the codec's parity tables, to the device.
int upload_verify(hbec_plan* p, hbec_codec* codec, hbec::VerifyRecs& vr) {
    p->vother = std::move(vr.other);
    if (vr.recs.empty()) return HBEC_OK;
    std::vector<uint32_t> tab;
    hbec::verify_tab(codec, tab);
    int rc = upload(vr.recs, &p->d_vrecs, "plan verify records");
    if (!rc) rc = upload(vr.tiles, &p->d_vtiles, "plan verify tile list");
    if (!rc) rc = upload(tab, &p->d_vtab, "plan verify tables");
    if (rc) return rc;
    p->n_vrecs = vr.recs.size();
    p->n_vtiles = vr.tiles.size();
    return HBEC_OK;
}

std::atomic<uint64_t> g_vplan_launches{0}, g_vplan_per_stripe{0};

// CU count of the current device
int current_cus(int* cus) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    return hbec::device_cus(dev, cus);
}

// One pass of an unaligned plan: inputs [c0, c0 + K) and outputs [r0, r0 + R)
// of the index lists with their coefficient tables; sel_k > 0: object records
// (indices >= sel_k are parity, base b).
hbec::UPlanArgs uplan_pass(const hbec::URec* recs, uint64_t n_recs, const std::vector<int>& in_idx,
                           const std::vector<int>& out_idx, const std::vector<uint8_t>& rows, int sel_k, int r0, int R,
                           int c0, int K) {
    hbec::UPlanArgs a;
    std::memset(&a, 0, sizeof(a));
    a.recs = recs;
    a.n_recs = (uint32_t)n_recs;
    a.accumulate = c0 > 0 ? 1u : 0u;
    for (int j = 0; j < K; ++j) {
        int i = in_idx[c0 + j];
        if (sel_k > 0 && i >= sel_k) {
            a.in_sel |= 1u << j;
            i -= sel_k;
        }
        a.in_idx[j] = (uint32_t)i;
    }
    for (int r = 0; r < R; ++r) {
        int i = out_idx[r0 + r];
        if (sel_k > 0 && i >= sel_k) {
            a.out_sel |= 1u << r;
            i -= sel_k;
        }
        a.out_idx[r] = (uint32_t)i;
        for (int j = 0; j < K; ++j)
            hbec::perm_table(rows[(size_t)(r0 + r) * in_idx.size() + c0 + j], a.tab[r][j]);
    }
    return a;
}

}  // namespace

// ---- Verify over records (hbec_verify_plan, hbec_verify_host) ----

void hbec::verify_tab(hbec_codec* codec, std::vector<uint32_t>& tab) {
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
    std::vector<uint8_t> mat((size_t)(k + m) * k);
    hbec_matrix(codec, mat.data());
    const uint32_t ts = hbec::vp_tab_stride(m);
    tab.assign((size_t)k * ts, 0u);
    for (int j = 0; j < k; ++j)
        for (int r = 0; r < m; ++r) hbec::perm_table(mat[(size_t)(k + r) * k + j], tab.data() + (size_t)j * ts + 5 * r);
}

int hbec::verify_recs_run(hbec_codec* codec, const VRec* d_recs, uint64_t n_recs, const VTile* d_tiles,
                          uint64_t n_tiles, const uint32_t* d_tab, uint32_t* d_flags, hipStream_t stream,
                          int max_blocks) {
    if (n_recs == 0) return HBEC_OK;
    int cus = 0;
    int rc = current_cus(&cus);
    if (rc) return rc;
    hipError_t e = hbec::launch_verify_recs(hbec_data_shards(codec), hbec_parity_shards(codec), d_recs, (uint32_t)n_recs,
                                            d_tiles, (uint32_t)n_tiles, d_tab, d_flags, cus, stream, max_blocks);
    if (e != hipSuccess) return hip_fail(e, "launch gf_verify_recs");
    g_vplan_launches.fetch_add(n_tiles > 0 ? 2 : 1, std::memory_order_relaxed);  // tiles + byte tail
    return HBEC_OK;
}

int hbec::verify_other_run(hbec_codec* codec, const VOther& o, uint32_t* d_flags, hipStream_t stream) {
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
    std::vector<hbec_view> v((size_t)k + m);
    for (int j = 0; j < k; ++j) v[j] = {reinterpret_cast<void*>(o.a + (uint64_t)j * o.shard_len), 0};
    for (int r = 0; r < m; ++r) v[(size_t)k + r] = {reinterpret_cast<void*>(o.b + (uint64_t)r * o.shard_len), 0};
    g_vplan_per_stripe.fetch_add(1, std::memory_order_relaxed);
    return hbec_verify_batch(codec, v.data(), 1, o.shard_len, d_flags + o.idx, stream);
}

// out rows (^)= rows x in over unaligned-kernel records, in passes of <= 4
// outputs x <= kMaxK inputs (later input passes accumulate).  sel_k > 0:
// object records (shard indices >= sel_k are parity, base b).
int hbec::launch_unaligned_passes(const URec* recs, uint64_t n_recs, const std::vector<int>& in_idx,
                                  const std::vector<int>& out_idx, const std::vector<uint8_t>& rows, int sel_k,
                                  hipStream_t stream, int max_blocks, const URec* erecs, uint64_t n_erecs,
                                  bool mirror, bool round2, const OddStripeRecs* orecs) {
    const int K_all = (int)in_idx.size(), R_all = (int)out_idx.size();
    if ((n_recs == 0 && n_erecs == 0) || R_all == 0) return HBEC_OK;
    if (mirror && (!hbec::odd_enabled() || sel_k > 0 || round2))
        return fail(HBEC_ERR_INVALID_ARG, "mirrored unaligned plans need gf_odd and stripe records");
    int cus = 0, per_cu = 0;
    int rc = current_cus(&cus);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (hbec::odd_enabled() && !round2) {
        // per-stripe records over the plan's tile lists (unmirrored plans)
        const bool use_orecs = orecs && orecs->n > 0 && !mirror;
        // gf_odd_plan: launches of <= 4 outputs x <= kOddMaxK inputs, later input
        // launches accumulating; one 4-wave block per CU
        for (int r0 = 0; r0 < R_all; r0 += hbec::kMaxR) {
            const int R = std::min(hbec::kMaxR, R_all - r0);
            for (int c0 = 0; c0 < K_all; c0 += hbec::kOddMaxK) {
                const int K = std::min(hbec::kOddMaxK, K_all - c0);
                hbec::UPlanArgs a = uplan_pass(recs, n_recs, in_idx, out_idx, rows, sel_k, r0, R, c0, K);
                // mirror: each pass's inputs once (first output group), the
                // outputs when one input pass makes them final
                if (mirror) a.mirror = (r0 == 0 ? 1u : 0u) | (K_all <= hbec::kOddMaxK ? 2u : 0u);
                // records built as carried tiles (K_all <= 4, not mirrored) take the carry kernel
                a.carry = (!mirror && K <= 4 &&
                           hbec::urec_tile_for(std::min(K_all, hbec::kOddMaxK), false) != hbec::urec_tile_for(K, true))
                              ? 1u : 0u;
                const uint64_t want = (n_recs + 3) / 4;  // 4 waves per block
                uint64_t cap = (uint64_t)cus * (uint64_t)hbec::odd_blocks_per_cu(c0 > 0 ? 1 : 0, K, R, mirror);
                if (max_blocks > 0) cap = std::min<uint64_t>(cap, (uint64_t)max_blocks);
                const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(want, cap));
                const int mode = c0 > 0 ? 1 : 0;
                bool fused = false;
                if (use_orecs) {
                    rc = odd_stripe_rec_pass(K, R, mode, a, *orecs, cus, max_blocks, stream, K == K_all, &fused);
                    if (rc) return rc;
                } else if (n_recs > 0) {
                    e = hbec::launch_odd_plan(K, R, mode, a, grid, stream);
                    if (e != hipSuccess) return hip_fail(e, "launch gf_odd_plan");
                }
                // guard-band bytes of every stripe, this pass's inputs (fused:
                // only the stripes of S <= odd_min_main(), which have no main
                // tiles; the edge records list them first)
                const uint64_t ne = fused ? orecs->n_short_edges : n_erecs;
                e = hbec::launch_odd_edges_plan(K, R, c0 > 0 ? 1 : 0, a, erecs, (uint32_t)ne, stream,
                                                !fused && orecs && orecs->edges_long);
                if (e != hipSuccess) return hip_fail(e, "launch gf_odd_edges_plan");
            }
        }
        if (mirror && n_erecs > 0) {
            // the bytes the main kernel did not mirror, read back from the
            // (final) stripes: guard bands of every shard, and whole outputs
            // when k > kOddMaxK made them final only after the last pass
            std::vector<int> all(in_idx);
            all.insert(all.end(), out_idx.begin(), out_idx.end());
            for (int pass = 0; pass < 2; ++pass) {
                const bool full = pass == 1;
                if (full && K_all <= hbec::kOddMaxK) break;
                const std::vector<int>& idx = full ? out_idx : all;
                for (size_t t0 = 0; t0 < idx.size(); t0 += hbec::kMirrorMaxIdx) {
                    hbec::MirrorCopyArgs m;
                    std::memset(&m, 0, sizeof(m));
                    m.n_idx = (uint32_t)std::min<size_t>(hbec::kMirrorMaxIdx, idx.size() - t0);
                    for (uint32_t t = 0; t < m.n_idx; ++t) m.idx[t] = (uint32_t)idx[t0 + t];
                    m.full = full ? 1u : 0u;
                    e = hbec::launch_odd_mirror_copy(erecs, (uint32_t)n_erecs, m, stream);
                    if (e != hipSuccess) return hip_fail(e, "launch gf_odd_mirror_copy");
                }
            }
        }
        return HBEC_OK;
    }
    for (int r0 = 0; r0 < R_all; r0 += hbec::kMaxR) {
        const int R = std::min(hbec::kMaxR, R_all - r0);
        e = hbec::unaligned_occupancy(R, &per_cu);
        if (e != hipSuccess) return hip_fail(e, "unaligned occupancy");
        if (const long long v = hbec::tune_knob("HBEC_UNALIGNED_BPC", 0); v > 0) per_cu = std::min(per_cu, (int)v);
        for (int c0 = 0; c0 < K_all; c0 += hbec::kMaxK) {
            const int K = std::min(hbec::kMaxK, K_all - c0);
            const hbec::UPlanArgs a = uplan_pass(recs, n_recs, in_idx, out_idx, rows, sel_k, r0, R, c0, K);
            const uint64_t want = (n_recs + 3) / 4;  // 4 waves per block
            uint64_t cap = (uint64_t)cus * std::max(1, per_cu);
            if (max_blocks > 0) cap = std::min<uint64_t>(cap, (uint64_t)max_blocks);
            const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>(want, cap));
            e = hbec::launch_unaligned_plan(K, R, a, grid, stream);
            if (e != hipSuccess) return hip_fail(e, "launch gf_apply_unaligned_plan");
        }
    }
    return HBEC_OK;
}

// test hook (hbec_set_stripes_grid_cap): blocks per gf_apply_stripes launch, so
// a plan of a few hundred tiles walks the pipelined loop; 0 = no cap
static std::atomic<int> g_stripes_grid_cap{0};

int hbec::stripes_grid(int k, int r, uint64_t n_tiles, int* grid, int blocks_per_cu, int max_blocks) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    static int occ[64][9][4] = {};
    if (dev < 0 || dev >= 64) return fail(HBEC_ERR_DEVICE, "device index out of range");
    int cus = 0;
    int rc = hbec::device_cus(dev, &cus);
    if (rc) return rc;
    std::lock_guard<std::mutex> g(g_occ_mu);
    if (occ[dev][k][r] == 0) {
        int b = 0;
        e = hbec::stripes_occupancy(k, r, &b);
        if (e != hipSuccess) return hip_fail(e, "stripes occupancy");
        b = std::max(1, b);
        if (hbec::kPipeBlocksPerCu > 0) b = std::min(b, hbec::kPipeBlocksPerCu);  // same HBM sweet spot
        if (const long long v = hbec::tune_knob("HBEC_STRIPE_BLOCKS_PER_CU", 0); v > 0) b = std::max(1, std::min(b, (int)v));
        occ[dev][k][r] = b;
    }
    const uint64_t want = (n_tiles + 3) / 4;  // 4 waves per block
    int bpc = occ[dev][k][r];
    if (blocks_per_cu > 0) {  // caller's choice (zero-copy over PCIe), within what fits
        int fit = 1;
        if (hbec::stripes_occupancy(k, r, &fit) != hipSuccess) fit = 1;
        bpc = std::max(1, std::min(fit, blocks_per_cu));
    }
    uint64_t cap = (uint64_t)cus * (uint64_t)bpc;
    if (max_blocks > 0) cap = std::min<uint64_t>(cap, (uint64_t)max_blocks);
    if (const int hook = g_stripes_grid_cap.load(std::memory_order_relaxed); hook > 0)
        cap = std::min<uint64_t>(cap, (uint64_t)hook);
    *grid = (int)std::max<uint64_t>(1, std::min(want, cap));
    return HBEC_OK;
}

// out[r] (^)= XOR_j rows[r][j] * in[j] over every tile record: launches of
// <= 3 outputs x <= kStripeMaxK inputs; a shape with more inputs (k > 8)
// runs in passes, the later ones accumulating into the outputs.  sel_k > 0
// marks an object plan (split bases: shard indices >= sel_k are parity).
int hbec::launch_stripe_passes(const TileRec* tiles, uint64_t n_tiles, const std::vector<int>& in_idx,
                               const std::vector<int>& out_idx, const std::vector<uint8_t>& rows, int sel_k,
                               hipStream_t stream, int blocks_per_cu, bool mirror, int max_blocks) {
    const int K_all = (int)in_idx.size(), R_all = (int)out_idx.size();
    if (n_tiles == 0 || R_all == 0) return HBEC_OK;
    if (sel_k > 0 && K_all > kStripeMaxK) return fail(HBEC_ERR_INVALID_ARG, "object plans take <= 8 inputs per pass");
    if (sel_k > 0 && mirror) return fail(HBEC_ERR_INVALID_ARG, "object plans are not mirrored");
    for (int r0 = 0; r0 < R_all; r0 += 3) {
        const int R = std::min(3, R_all - r0);
        for (int c0 = 0; c0 < K_all; c0 += kStripeMaxK) {
            const int K = std::min(kStripeMaxK, K_all - c0);
            StripeArgs a;
            std::memset(&a, 0, sizeof(a));
            a.tiles = tiles;
            a.n_tiles = (uint32_t)n_tiles;
            a.split = sel_k > 0 ? 1u : 0u;
            a.accumulate = c0 > 0 ? 1u : 0u;
            a.mirror = mirror ? 1u : 0u;
            for (int j = 0; j < K; ++j) {
                a.in_idx[j] = (uint32_t)in_idx[c0 + j];
                if (sel_k > 0 && in_idx[c0 + j] >= sel_k) {  // parity shard: base B
                    a.in_sel |= 1u << j;
                    a.in_idx[j] -= (uint32_t)sel_k;
                }
            }
            for (int r = 0; r < R; ++r) {
                a.out_idx[r] = (uint32_t)out_idx[r0 + r];
                if (sel_k > 0) {
                    if (out_idx[r0 + r] < sel_k) a.out_sel |= 1u << r;  // data shard: base A
                    else a.out_idx[r] -= (uint32_t)sel_k;
                }
                for (int j = 0; j < K; ++j) perm_table(rows[(size_t)(r0 + r) * K_all + c0 + j], a.tab[r][j]);
            }
            int grid = 0;
            int rc = stripes_grid(K, R, n_tiles, &grid, blocks_per_cu, max_blocks);
            if (rc) return rc;
            hipError_t e = launch_stripes(K, R, a, grid, stream);
            if (e != hipSuccess) return hip_fail(e, "launch gf_apply_stripes");
        }
    }
    return HBEC_OK;
}

namespace {

// out rows (given as shard indices + coefficient rows over in_idx) for every stripe
int run_plan(const hbec_plan* p, const std::vector<int>& in_idx, const std::vector<int>& out_idx,
             const std::vector<uint8_t>& rows, hipStream_t stream) {
    const int K = (int)in_idx.size();
    const int R_all = (int)out_idx.size();
    if (R_all == 0 || p->shard_bytes == 0) return HBEC_OK;
    // stripe plans take any k (inputs beyond 8 accumulate in later passes);
    // object plans keep the tiled kernel to k <= 8
    const bool tiled_ok = p->objects ? K <= hbec::kStripeMaxK : true;
    if (tiled_ok && p->n_tiles > 0) {
        int rc = hbec::launch_stripe_passes(p->d_tiles, p->n_tiles, in_idx, out_idx, rows, p->objects ? p->k : 0,
                                            stream);
        if (rc) return rc;
    }
    // with k > 8 every object is in the unaligned records (hbec_plan_objects)
    const int sel_k = p->objects ? p->k : 0;
    int rc = hbec::launch_unaligned_passes(p->d_urecs, p->n_urecs, in_idx, out_idx, rows, sel_k, stream, 0,
                                           p->d_erecs, p->n_erecs, false, false, &p->orecs);
    if (rc || p->n_brecs == 0) return rc;
    return hbec::launch_unaligned_passes(p->d_brecs, p->n_brecs, in_idx, out_idx, rows, sel_k, stream, 0, nullptr, 0,
                                         false, true);
}

// ---- reconstruct with a pattern per stripe (hbec_reconstruct_plan_mixed) ----

std::atomic<uint64_t> g_mplan_launches{0}, g_mplan_per_stripe{0};
// test hook (hbec_set_mixed_plan_chunk_tiles): tiles per gf_mixed_plan launch
std::atomic<uint64_t> g_mplan_chunk_override{0};
// per-call staging of at most this many bytes goes through kernel arguments
// (kPutWordsMax words a launch: 18 launches), more through a copy
constexpr size_t kMPlanPutBytes = 64 * 1024;

// The device side of a plan's mixed reconstruct, built once.
int mixed_plan_device(const hbec_plan* p) {
    std::lock_guard<std::mutex> lk(p->mp_mu);
    if (p->mp_built) return HBEC_OK;
    hbec::MixedPlanRecs mr;
    if (!hbec::mp_build(mr, p->k, p->m, p->src, hbec::mixed_plan_tile_bytes()))
        return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^31 tiles)");
    if (!mr.tiles.empty()) {
        int rc = upload(mr.recs, &p->d_mrecs, "plan mixed records");
        if (!rc) rc = upload(mr.tiles, &p->d_mtiles, "plan mixed tile list");
        if (rc) {
            if (p->d_mrecs) (void)hipFree(p->d_mrecs);
            p->d_mrecs = nullptr;
            return rc;
        }
    }
    p->n_mtiles = mr.tiles.size();
    p->mp_other = std::move(mr.other);
    p->mp_built = true;
    return HBEC_OK;
}

// One distinct pattern of a call, resolved.
struct PlanPattern {
    std::vector<int> surv, outs;
    std::vector<uint8_t> rows;  // outs.size() x k
    uint64_t uses = 0;          // source entries with this pattern
    uint32_t rec = 0;           // its pattern record (kernel route)
};

// The argument checks of a call with a pattern per source entry
// (hbec_reconstruct_plan_mixed, hbec_verify_plan_mixed), all made before anything
// is queued; counts the non-empty entries of every pattern.
int check_plan_patterns(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                        const uint32_t* pattern_of, std::vector<PlanPattern>& pats) {
    if (!codec || !plan || !patterns || !pattern_of) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
    if (n_patterns > 65536) return fail(HBEC_ERR_INVALID_ARG, "more than 65536 patterns");
    const uint64_t n_src = plan->n_src;
    if (n_src && !n_patterns) return fail(HBEC_ERR_INVALID_ARG, "stripes but no patterns");
    pats.assign(n_patterns, PlanPattern());
    for (uint32_t p = 0; p < n_patterns; ++p) {
        int n_present = 0;
        for (int i = 0; i < n; ++i) n_present += patterns[(size_t)p * n + i] ? 1 : 0;
        if (n_present < k)
            return fail(HBEC_ERR_TOO_FEW_SHARDS, "too few shards given (pattern " + std::to_string(p) + ")");
    }
    for (uint64_t i = 0; i < n_src; ++i) {  // zero-length entries too
        if (pattern_of[i] >= n_patterns)
            return fail(HBEC_ERR_INVALID_ARG, "pattern index out of range (stripe " + std::to_string(i) + ")");
        if (plan->src[i].shard_len) ++pats[pattern_of[i]].uses;
    }
    return HBEC_OK;
}

// After a call's launches: the next call on another stream waits for them.
int stage_end(const hbec_plan* plan, hipStream_t stream) {
    plan->mp_stream = stream;
    const hipError_t e = hipEventRecord(plan->mp_ev, stream);
    return e == hipSuccess ? HBEC_OK : hip_fail(e, "hipEventRecord (plan mixed staging)");
}

// A call's staging words (pattern records, then one word per source entry) go
// to a buffer the plan owns, not to stream-ordered scratch: with a scratch
// allocation and a copy from pageable memory per call, a call returned only
// when the one before it had run (4096 stripes 4+2: 0.70 of a call's 0.74 ms
// on the host, against 0.016 ms for hbec_reconstruct_plan), so back-to-back
// calls never overlapped.  Up to kMPlanPutBytes the words travel in kernel
// arguments (launch_put_words).  Calls on one plan, reconstruct and verify
// alike, take turns under mp_mu from stage_begin to stage_end; a call on
// another stream than the last waits for that call's event, so the words of one
// call are never overwritten while its launches may still read them.
int stage_begin(const hbec_plan* plan, const std::vector<uint32_t>& stage, hipStream_t stream) {
    hipError_t e = hipSuccess;
    if (stage.size() > plan->mstage_words) {
        if (plan->d_mstage) (void)hipFree(plan->d_mstage);  // waits for the work that reads it
        plan->d_mstage = nullptr;
        plan->mstage_words = 0;
        const size_t cap = std::max<size_t>(2 * stage.size(), 4096);
        e = hipMalloc(reinterpret_cast<void**>(&plan->d_mstage), cap * 4);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc plan mixed staging");
        plan->mstage_words = cap;
    }
    if (!plan->mp_ev) {
        e = hipEventCreateWithFlags(&plan->mp_ev, hipEventDisableTiming);
        if (e != hipSuccess) return hip_fail(e, "hipEventCreate (plan mixed staging)");
    } else if (plan->mp_stream != stream) {
        e = hipStreamWaitEvent(stream, plan->mp_ev, 0);
        if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent (plan mixed staging)");
    }
    e = stage.size() * 4 <= kMPlanPutBytes
            ? hbec::launch_put_words(plan->d_mstage, stage.data(), stage.size() * 4, stream)
            : hipMemcpyAsync(plan->d_mstage, stage.data(), stage.size() * 4, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) return HBEC_OK;
    (void)stage_end(plan, stream);
    return hip_fail(e, "plan mixed staging");
}

// The other route of the calls with a pattern per source entry (any k, m, S),
// one source entry at a time; hbec_reconstruct_plan_mixed, hbec_verify_plan_mixed
// and hbec_repair_plan_mixed share both.
// Rebuild: one single-pattern apply of pp's decode rows (pp.outs not empty).
int reconstruct_other_entry(const hbec_plan* plan, uint32_t i, const PlanPattern& pp, hipStream_t stream) {
    const int k = plan->k;
    const hbec::MSrc& s = plan->src[i];
    auto at = [&](int sh) { return hbec_view{reinterpret_cast<void*>(shard_addr(plan, i, sh)), 0}; };
    std::vector<hbec_view> vin((size_t)k), vout(pp.outs.size());
    for (int j = 0; j < k; ++j) vin[j] = at(pp.surv[j]);
    for (size_t q = 0; q < pp.outs.size(); ++q) vout[q] = at(pp.outs[q]);
    return hbec::apply_views((int)pp.outs.size(), k, pp.rows.data(), vin.data(), vout.data(), 1, s.shard_len, stream);
}

// Check (pp.outs: the checked shards): exactly k present, bit 1; all present,
// the per-stripe Verify; degraded, the checked shards rebuilt from the survivors
// into scratch and compared with the stored ones.
int verify_other_entry(hbec_codec* codec, const hbec_plan* plan, uint32_t i, const PlanPattern& pp,
                       uint32_t* d_flags, int cus, hipStream_t stream) {
    const int k = plan->k, m = plan->m;
    const hbec::MSrc& s = plan->src[i];
    if (pp.outs.empty()) {
        const hipError_t e = hbec::launch_vm_or(d_flags + i, 2u, stream);
        return e == hipSuccess ? HBEC_OK : hip_fail(e, "launch gf_vm_or");
    }
    if ((int)pp.outs.size() == m) {
        if (!plan->shards) return hbec::verify_other_run(codec, hbec::VOther{s.a, s.b, s.shard_len, i}, d_flags, stream);
        // what verify_other_run does, with the entry's own shard addresses
        std::vector<hbec_view> v((size_t)k + m);
        for (int sh = 0; sh < k + m; ++sh) v[sh] = {reinterpret_cast<void*>(shard_addr(plan, i, sh)), 0};
        g_vplan_per_stripe.fetch_add(1, std::memory_order_relaxed);
        return hbec_verify_batch(codec, v.data(), 1, s.shard_len, d_flags + i, stream);
    }
    auto at = [&](int sh) { return shard_addr(plan, i, sh); };
    void* scratch = nullptr;
    int rc = hbec::scratch_alloc(pp.outs.size() * (size_t)s.shard_len, stream, &scratch);
    if (rc) return rc;
    uint8_t* rebuilt = static_cast<uint8_t*>(scratch);
    std::vector<hbec_view> vin((size_t)k), vout(pp.outs.size());
    for (int j = 0; j < k; ++j) vin[j] = hbec_view{reinterpret_cast<void*>(at(pp.surv[j])), 0};
    for (size_t q = 0; q < pp.outs.size(); ++q) vout[q] = hbec_view{rebuilt + q * (size_t)s.shard_len, 0};
    rc = hbec::apply_views((int)pp.outs.size(), k, pp.rows.data(), vin.data(), vout.data(), 1, s.shard_len, stream);
    hipError_t e = hipSuccess;
    for (size_t q = 0; q < pp.outs.size() && !rc && e == hipSuccess; ++q)
        e = hbec::launch_vm_compare(rebuilt + q * (size_t)s.shard_len, reinterpret_cast<const void*>(at(pp.outs[q])),
                                    s.shard_len, d_flags + i, cus, stream);
    hbec::scratch_free(scratch, stream);
    if (rc) return rc;
    return e == hipSuccess ? HBEC_OK : hip_fail(e, "launch gf_vm_compare");
}

int reconstruct_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                           const uint32_t* pattern_of, bool data_only, hipStream_t stream) {
    std::vector<PlanPattern> pats;
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    const uint64_t n_src = plan->n_src;
    std::vector<uint8_t> mask((size_t)n);
    bool work = false;
    for (uint32_t p = 0; p < n_patterns; ++p) {
        PlanPattern& pp = pats[p];
        if (!pp.uses) continue;
        int n_present = 0, data_present = 0;
        for (int i = 0; i < n; ++i) {
            mask[i] = patterns[(size_t)p * n + i] ? 1 : 0;
            n_present += mask[i];
            if (i < k) data_present += mask[i];
        }
        if (n_present == n || (data_only && data_present == k)) continue;  // nothing to rebuild
        pp.surv.resize(k);
        pp.outs.resize(n);
        pp.rows.resize((size_t)n * k);
        int n_out = 0;
        int rc = hbec_decode_rows(codec, mask.data(), data_only ? 1 : 0, pp.surv.data(), pp.outs.data(), &n_out,
                                  pp.rows.data());
        if (rc) return rc;
        pp.outs.resize(n_out);
        pp.rows.resize((size_t)n_out * k);
        work = work || n_out > 0;
    }
    if (!work) return HBEC_OK;
    rc = mixed_plan_device(plan);
    if (rc) return rc;

    if (plan->n_mtiles > 0) {
        // per call: the records of the patterns in use and one word per source
        // entry, in one buffer, to stream-ordered scratch
        std::vector<uint32_t> stage;
        for (PlanPattern& pp : pats) {
            if (!pp.uses || pp.outs.empty()) continue;
            pp.rec = hbec::mp_pattern(stage, k, pp.surv.data(), pp.outs.data(), (int)pp.outs.size(), pp.rows.data());
        }
        const size_t rec_words = stage.size();
        stage.resize(rec_words + (size_t)n_src);
        uint32_t* words = stage.data() + rec_words;
        bool has_r[hbec::kMaxR + 1] = {};
        for (uint64_t i = 0; i < n_src; ++i) {
            const PlanPattern& pp = pats[pattern_of[i]];
            const uint64_t S = plan->src[i].shard_len;
            const bool kernel = S > 0 && hbec::pos32_shard(S) && !pp.outs.empty();  // mp_build's route
            words[i] = kernel ? ((uint32_t)pp.outs.size() << hbec::kMPatShift) | pp.rec : 0u;
            if (kernel) has_r[pp.outs.size()] = true;
        }
        int cus = 0;
        rc = current_cus(&cus);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(plan->mp_mu);
        rc = stage_begin(plan, stage, stream);
        if (rc) return rc;
        const uint32_t* d_pats = plan->d_mstage;
        const uint32_t* d_words = d_pats + rec_words;
        hipError_t e = hipSuccess;
        const uint64_t hook = g_mplan_chunk_override.load(std::memory_order_relaxed);
        const uint64_t chunk = std::min<uint64_t>((1ull << 31) - 1, hook ? hook : ~0ull);
        // one launch per chunk of the list, of the instance for the largest
        // output count in use: it codes every tile with something to rebuild
        int rmax = 0;
        for (int r = 1; r <= hbec::kMaxR; ++r)
            if (has_r[r]) rmax = r;
        for (uint64_t t0 = 0; rmax > 0 && t0 < plan->n_mtiles && e == hipSuccess; t0 += chunk) {
            const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, plan->n_mtiles - t0);
            g_mplan_launches.fetch_add(1, std::memory_order_relaxed);
            e = hbec::launch_mixed_plan(k, rmax, plan->d_mrecs, plan->d_mtiles + t0, nt, d_words, d_pats, cus, stream,
                                        plan->shards);
        }
        rc = stage_end(plan, stream);
        if (e != hipSuccess) return hip_fail(e, "launch gf_mixed_plan");
        if (rc) return rc;
    }
    // the other route: one single-pattern apply per stripe (any k, m, S)
    for (uint32_t i : plan->mp_other) {
        const PlanPattern& pp = pats[pattern_of[i]];
        if (pp.outs.empty()) continue;
        g_mplan_per_stripe.fetch_add(1, std::memory_order_relaxed);
        rc = reconstruct_other_entry(plan, i, pp, stream);
        if (rc) return rc;
    }
    return HBEC_OK;
}

// ---- Verify with a present mask per stripe (hbec_verify_plan_mixed) ----

std::atomic<uint64_t> g_vmplan_launches{0}, g_vmplan_per_stripe{0};
// test hook (hbec_set_verify_mixed_plan_chunk_tiles): tiles per gf_verify_mixed_plan launch
std::atomic<uint64_t> g_vmplan_chunk_override{0};

int verify_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                      const uint32_t* pattern_of, uint32_t* d_flags, hipStream_t stream) {
    std::vector<PlanPattern> pats;  // outs: the checked shards
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    if (!d_flags && plan->n_src) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    const uint64_t n_src = plan->n_src;
    std::vector<uint8_t> mask((size_t)n);
    bool used = false;
    for (uint32_t p = 0; p < n_patterns; ++p) {
        PlanPattern& pp = pats[p];
        if (!pp.uses) continue;
        used = true;
        for (int i = 0; i < n; ++i) mask[i] = patterns[(size_t)p * n + i] ? 1 : 0;
        pp.surv.resize(k);
        pp.outs.resize(std::max(1, m));
        pp.rows.resize((size_t)std::max(1, m) * k);
        int n_checked = 0;
        rc = hbec_check_rows(codec, mask.data(), pp.surv.data(), pp.outs.data(), &n_checked, pp.rows.data());
        if (rc) return rc;
        pp.outs.resize(n_checked);
        pp.rows.resize((size_t)n_checked * k);
    }
    if (!used) return HBEC_OK;  // zero-length entries only
    rc = mixed_plan_device(plan);
    if (rc) return rc;
    int cus = 0;
    rc = current_cus(&cus);
    if (rc) return rc;

    if (plan->n_mtiles > 0) {
        // per call, as reconstruct_plan_mixed: the records of the masks with
        // something to check and one word per source entry, in one buffer
        std::vector<uint32_t> stage;
        for (PlanPattern& pp : pats) {
            if (!pp.uses || pp.outs.empty()) continue;
            pp.rec = hbec::vm_pattern(stage, k, pp.surv.data(), pp.outs.data(), (int)pp.outs.size(), pp.rows.data());
        }
        const size_t rec_words = stage.size();
        stage.resize(rec_words + (size_t)n_src);
        uint32_t* words = stage.data() + rec_words;
        int rmax = 1;  // exactly-k entries alone: any instance sets their bit
        for (uint64_t i = 0; i < n_src; ++i) {
            const PlanPattern& pp = pats[pattern_of[i]];
            const bool kernel = hbec::vm_route(k, m, plan->src[i].shard_len) == hbec::kVmKernel;
            words[i] = kernel ? hbec::vm_word((int)pp.outs.size(), pp.rec) : 0u;
            if (kernel) rmax = std::max(rmax, (int)pp.outs.size());
        }
        std::lock_guard<std::mutex> lk(plan->mp_mu);
        rc = stage_begin(plan, stage, stream);
        if (rc) return rc;
        const uint32_t* d_pats = plan->d_mstage;
        const uint32_t* d_words = d_pats + rec_words;
        hipError_t e = hipSuccess;
        const uint64_t hook = g_vmplan_chunk_override.load(std::memory_order_relaxed);
        const uint64_t chunk = std::min<uint64_t>((1ull << 31) - 1, hook ? hook : ~0ull);
        // one launch per chunk of the list, of the instance for the largest count
        // of checked shards in use
        for (uint64_t t0 = 0; t0 < plan->n_mtiles && e == hipSuccess; t0 += chunk) {
            const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, plan->n_mtiles - t0);
            g_vmplan_launches.fetch_add(1, std::memory_order_relaxed);
            e = hbec::launch_verify_mixed_plan(k, rmax, plan->d_mrecs, plan->d_mtiles + t0, nt, d_words, d_pats,
                                               d_flags, cus, stream, plan->shards);
        }
        rc = stage_end(plan, stream);
        if (e != hipSuccess) return hip_fail(e, "launch gf_verify_mixed_plan");
        if (rc) return rc;
    }
    // the other route, one stripe at a time (any k, m, S)
    for (uint32_t i : plan->mp_other) {
        g_vmplan_per_stripe.fetch_add(1, std::memory_order_relaxed);
        rc = verify_other_entry(codec, plan, i, pats[pattern_of[i]], d_flags, cus, stream);
        if (rc) return rc;
    }
    return HBEC_OK;
}

// ---- rebuild the missing shards and check the surplus ones (hbec_repair_plan_mixed) ----

std::atomic<uint64_t> g_rplan_launches{0}, g_rplan_per_stripe{0};
// test hook (hbec_set_repair_plan_chunk_tiles): tiles per gf_repair_mixed_plan launch
std::atomic<uint64_t> g_rplan_chunk_override{0};

int repair_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                      const uint32_t* pattern_of, bool data_only, uint32_t* d_flags, hipStream_t stream) {
    std::vector<PlanPattern> outp;  // outs: the shards to rebuild (reconstruct_plan_mixed's)
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, outp);
    if (rc) return rc;
    if (!d_flags && plan->n_src) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    const uint64_t n_src = plan->n_src;
    std::vector<PlanPattern> chkp(n_patterns);  // outs: the checked shards (verify_plan_mixed's)
    std::vector<uint8_t> mask((size_t)n);
    bool used = false;
    for (uint32_t p = 0; p < n_patterns; ++p) {
        PlanPattern &po = outp[p], &pc = chkp[p];
        if (!po.uses) continue;
        used = true;
        int n_present = 0, data_present = 0;
        for (int i = 0; i < n; ++i) {
            mask[i] = patterns[(size_t)p * n + i] ? 1 : 0;
            n_present += mask[i];
            if (i < k) data_present += mask[i];
        }
        pc.surv.resize(k);
        pc.outs.resize(std::max(1, m));
        pc.rows.resize((size_t)std::max(1, m) * k);
        int n_checked = 0;
        rc = hbec_check_rows(codec, mask.data(), pc.surv.data(), pc.outs.data(), &n_checked, pc.rows.data());
        if (rc) return rc;
        pc.outs.resize(n_checked);
        pc.rows.resize((size_t)n_checked * k);
        if (n_present == n || (data_only && data_present == k)) continue;  // nothing to rebuild
        po.surv.resize(k);
        po.outs.resize(n);
        po.rows.resize((size_t)n * k);
        int n_out = 0;
        rc = hbec_decode_rows(codec, mask.data(), data_only ? 1 : 0, po.surv.data(), po.outs.data(), &n_out,
                              po.rows.data());
        if (rc) return rc;
        po.outs.resize(n_out);
        po.rows.resize((size_t)n_out * k);
    }
    if (!used) return HBEC_OK;  // zero-length entries only
    rc = mixed_plan_device(plan);
    if (rc) return rc;
    int cus = 0;
    rc = current_cus(&cus);
    if (rc) return rc;

    if (plan->n_mtiles > 0) {
        // per call, as verify_plan_mixed: the records of the masks with a shard
        // to rebuild or to check and one word per source entry, in one buffer
        std::vector<uint32_t> stage;
        for (uint32_t p = 0; p < n_patterns; ++p) {
            PlanPattern &po = outp[p], &pc = chkp[p];
            if (!po.uses || po.outs.size() + pc.outs.size() == 0) continue;
            po.rec = hbec::rp_pattern(stage, k, pc.surv.data(), po.outs.data(), (int)po.outs.size(), po.rows.data(),
                                      pc.outs.data(), (int)pc.outs.size(), pc.rows.data());
        }
        const size_t rec_words = stage.size();
        stage.resize(rec_words + (size_t)n_src);
        uint32_t* words = stage.data() + rec_words;
        int rmax = 1;  // exactly-k entries with nothing to rebuild alone: any instance sets their bit
        for (uint64_t i = 0; i < n_src; ++i) {
            const PlanPattern &po = outp[pattern_of[i]], &pc = chkp[pattern_of[i]];
            const bool kernel = hbec::rp_route(k, m, plan->src[i].shard_len) == hbec::kVmKernel;
            words[i] = kernel ? hbec::rp_word((int)po.outs.size(), (int)pc.outs.size(), po.rec) : 0u;
            if (kernel) rmax = std::max(rmax, (int)(po.outs.size() + pc.outs.size()));
        }
        std::lock_guard<std::mutex> lk(plan->mp_mu);
        rc = stage_begin(plan, stage, stream);
        if (rc) return rc;
        const uint32_t* d_pats = plan->d_mstage;
        const uint32_t* d_words = d_pats + rec_words;
        hipError_t e = hipSuccess;
        const uint64_t hook = g_rplan_chunk_override.load(std::memory_order_relaxed);
        const uint64_t chunk = std::min<uint64_t>((1ull << 31) - 1, hook ? hook : ~0ull);
        // one launch per chunk of the list, of the instance for the largest count
        // of rows (outputs and checked shards together) in use
        for (uint64_t t0 = 0; t0 < plan->n_mtiles && e == hipSuccess; t0 += chunk) {
            const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, plan->n_mtiles - t0);
            g_rplan_launches.fetch_add(1, std::memory_order_relaxed);
            e = hbec::launch_repair_mixed_plan(k, rmax, plan->d_mrecs, plan->d_mtiles + t0, nt, d_words, d_pats,
                                               d_flags, cus, stream, plan->shards);
        }
        rc = stage_end(plan, stream);
        if (e != hipSuccess) return hip_fail(e, "launch gf_repair_mixed_plan");
        if (rc) return rc;
    }
    // the other route, one stripe at a time (any k, m, S): what verify_plan_mixed
    // does with the entry, then what reconstruct_plan_mixed does with it
    for (uint32_t i : plan->mp_other) {
        g_rplan_per_stripe.fetch_add(1, std::memory_order_relaxed);
        rc = verify_other_entry(codec, plan, i, chkp[pattern_of[i]], d_flags, cus, stream);
        if (rc) return rc;
        const PlanPattern& po = outp[pattern_of[i]];
        if (po.outs.empty()) continue;
        rc = reconstruct_other_entry(plan, i, po, stream);
        if (rc) return rc;
    }
    return HBEC_OK;
}

// ---- the corrupt shard of every inconsistent stripe (hbec_locate_plan_mixed) ----

std::atomic<uint64_t> g_locplan_launches{0}, g_locplan_skipped{0};
// test hook (hbec_set_locate_plan_chunk_tiles): tiles per gf_locate_mixed_plan launch
std::atomic<uint64_t> g_locplan_chunk_override{0};

int locate_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                      const uint32_t* pattern_of, const uint32_t* d_flags, uint32_t* d_where, hipStream_t stream) {
    std::vector<PlanPattern> pats;  // outs: the checked shards
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    if (!d_where && plan->n_src) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    if (d_where && d_where == d_flags) return fail(HBEC_ERR_INVALID_ARG, "d_where aliases d_flags");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    const uint64_t n_src = plan->n_src;
    std::vector<uint8_t> mask((size_t)n);
    bool used = false;
    for (uint32_t p = 0; p < n_patterns; ++p) {
        PlanPattern& pp = pats[p];
        if (!pp.uses) continue;
        used = true;
        for (int i = 0; i < n; ++i) mask[i] = patterns[(size_t)p * n + i] ? 1 : 0;
        pp.surv.resize(k);
        pp.outs.resize(std::max(1, m));
        pp.rows.resize((size_t)std::max(1, m) * k);
        int n_checked = 0;
        rc = hbec_check_rows(codec, mask.data(), pp.surv.data(), pp.outs.data(), &n_checked, pp.rows.data());
        if (rc) return rc;
        pp.outs.resize(n_checked);
        pp.rows.resize((size_t)n_checked * k);
    }
    if (!used) return HBEC_OK;  // zero-length entries only
    rc = mixed_plan_device(plan);
    if (rc) return rc;

    if (plan->n_mtiles > 0) {
        // per call, as verify_plan_mixed: the records of the masks with something
        // to check and one word per source entry, in one buffer
        std::vector<uint32_t> stage;
        for (PlanPattern& pp : pats) {
            if (!pp.uses || pp.outs.empty()) continue;
            pp.rec = hbec::loc_pattern(stage, k, pp.surv.data(), pp.outs.data(), (int)pp.outs.size(), pp.rows.data());
        }
        const size_t rec_words = stage.size();
        stage.resize(rec_words + (size_t)n_src);
        uint32_t* words = stage.data() + rec_words;
        int rmax = 1;  // exactly-k entries alone: any instance sets their bit
        for (uint64_t i = 0; i < n_src; ++i) {
            const PlanPattern& pp = pats[pattern_of[i]];
            const bool kernel = hbec::loc_route(k, m, plan->src[i].shard_len) == hbec::kVmKernel;
            words[i] = kernel ? hbec::vm_word((int)pp.outs.size(), pp.rec) : 0u;
            if (kernel) rmax = std::max(rmax, (int)pp.outs.size());
        }
        int cus = 0;
        rc = current_cus(&cus);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(plan->mp_mu);
        rc = stage_begin(plan, stage, stream);
        if (rc) return rc;
        const uint32_t* d_pats = plan->d_mstage;
        const uint32_t* d_words = d_pats + rec_words;
        hipError_t e = hipSuccess;
        const uint64_t hook = g_locplan_chunk_override.load(std::memory_order_relaxed);
        const uint64_t chunk = std::min<uint64_t>((1ull << 31) - 1, hook ? hook : ~0ull);
        for (uint64_t t0 = 0; t0 < plan->n_mtiles && e == hipSuccess; t0 += chunk) {
            const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, plan->n_mtiles - t0);
            g_locplan_launches.fetch_add(1, std::memory_order_relaxed);
            e = hbec::launch_locate_mixed_plan(k, rmax, plan->d_mrecs, plan->d_mtiles + t0, nt, d_words, d_pats,
                                               d_flags, d_where, cus, stream, plan->shards);
        }
        rc = stage_end(plan, stream);
        if (e != hipSuccess) return hip_fail(e, "launch gf_locate_mixed_plan");
        if (rc) return rc;
    }
    // the other route is not examined: said in the entry's word, and counted
    for (uint32_t i : plan->mp_other) {
        g_locplan_skipped.fetch_add(1, std::memory_order_relaxed);
        const hipError_t e = hbec::launch_vm_or(d_where + i, hbec::kLocSkipped, stream);
        if (e != hipSuccess) return hip_fail(e, "launch gf_vm_or");
    }
    return HBEC_OK;
}

// ---- rebuild the shard locate named (hbec_heal_plan_mixed) ----

std::atomic<uint64_t> g_healplan_launches{0}, g_healplan_skipped{0};
// test hook (hbec_set_heal_plan_chunk_tiles): tiles per gf_heal_mixed_plan launch
std::atomic<uint64_t> g_healplan_chunk_override{0};

int heal_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                    const uint32_t* pattern_of, const uint32_t* d_where, uint32_t* d_flags, hipStream_t stream) {
    std::vector<PlanPattern> pats;
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    if ((!d_where || !d_flags) && plan->n_src) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    if (d_where && d_where == d_flags) return fail(HBEC_ERR_INVALID_ARG, "d_where aliases d_flags");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    const uint64_t n_src = plan->n_src;
    // the masks kernel-route entries use, in order of first use: their rows of the tables
    std::vector<uint32_t> row_of(n_patterns, hbec::kHealNone), bits;
    for (uint64_t i = 0; i < n_src; ++i) {
        if (hbec::heal_route(k, m, plan->src[i].shard_len) != hbec::kVmKernel) continue;
        uint32_t& row = row_of[pattern_of[i]];
        if (row != hbec::kHealNone) continue;
        row = (uint32_t)bits.size();
        bits.push_back(hbec::heal_mask_bits(n, patterns + (size_t)pattern_of[i] * n));
    }
    std::shared_ptr<const hbec::HealStage> hs;
    if (!bits.empty()) {
        {
            std::lock_guard<std::mutex> lk(plan->heal_mu);
            if (plan->heal_cache && plan->heal_bits == bits) hs = plan->heal_cache;
        }
        if (!hs) {
            auto built = std::make_shared<hbec::HealStage>();
            int err = HBEC_OK;
            const bool ok = hbec::heal_build(
                *built, k, m, bits,
                [&](const uint8_t* mask, int* surv, int* outs, int* n_out, uint8_t* orows, int* chk, int* n_chk,
                    uint8_t* crows) {
                    err = hbec_decode_rows(codec, mask, 0, surv, outs, n_out, orows);
                    if (!err) err = hbec_check_rows(codec, mask, surv, chk, n_chk, crows);
                    return err == HBEC_OK;
                });
            if (built->overflow)
                return fail(HBEC_ERR_INVALID_ARG,
                            "pattern records of the masks with one shard left out exceed 64 MiB");
            if (!ok) return err ? err : fail(HBEC_ERR_INVALID_ARG, "heal records");
            built->rec_of.clear();  // only the build needs it
            hs = built;
            std::lock_guard<std::mutex> lk(plan->heal_mu);
            plan->heal_bits = bits;
            plan->heal_cache = hs;
        }
    }
    rc = mixed_plan_device(plan);
    if (rc) return rc;

    if (plan->n_mtiles > 0 && !bits.empty()) {
        const hbec::HealStage& h = *hs;
        std::vector<uint32_t> index((size_t)n_src);
        for (uint64_t i = 0; i < n_src; ++i)
            index[i] = hbec::heal_route(k, m, plan->src[i].shard_len) == hbec::kVmKernel ? row_of[pattern_of[i]]
                                                                                         : hbec::kHealNone;
        int cus = 0;
        rc = current_cus(&cus);
        if (rc) return rc;
        std::lock_guard<std::mutex> lk(plan->mp_mu);
        rc = stage_begin(plan, index, stream);
        if (rc) return rc;
        hipError_t e = hipSuccess;
        if (plan->heal_on_device != hs) {
            // other masks than the last call's: their records and tables replace those.  This
            // stream has waited for the last call's launches (stage_begin), so nothing reads them.
            plan->heal_on_device.reset();
            if (h.stage.size() > plan->heal_dev_words) {
                if (plan->d_heal) (void)hipFree(plan->d_heal);
                plan->d_heal = nullptr;
                plan->heal_dev_words = 0;
                const size_t cap = std::max<size_t>(2 * h.stage.size(), 4096);
                e = hipMalloc(reinterpret_cast<void**>(&plan->d_heal), cap * 4);
                if (e == hipSuccess) plan->heal_dev_words = cap;
            }
            if (e == hipSuccess)
                e = h.stage.size() * 4 <= kMPlanPutBytes
                        ? hbec::launch_put_words(plan->d_heal, h.stage.data(), h.stage.size() * 4, stream)
                        : hipMemcpyAsync(plan->d_heal, h.stage.data(), h.stage.size() * 4, hipMemcpyHostToDevice,
                                         stream);
            if (e != hipSuccess) {
                (void)stage_end(plan, stream);
                return hip_fail(e, "plan heal records");
            }
            plan->heal_on_device = hs;
        }
        const uint32_t* d_pats = plan->d_heal;
        const uint32_t* d_index = plan->d_mstage;
        const uint64_t hook = g_healplan_chunk_override.load(std::memory_order_relaxed);
        const uint64_t chunk = std::min<uint64_t>((1ull << 31) - 1, hook ? hook : ~0ull);
        // one launch per chunk of the list; every mask with one shard left out has m rows
        for (uint64_t t0 = 0; t0 < plan->n_mtiles && e == hipSuccess; t0 += chunk) {
            const uint32_t nt = (uint32_t)std::min<uint64_t>(chunk, plan->n_mtiles - t0);
            g_healplan_launches.fetch_add(1, std::memory_order_relaxed);
            e = hbec::launch_heal_mixed_plan(k, std::max(1, m), plan->d_mrecs, plan->d_mtiles + t0, nt, d_index,
                                             d_pats + h.words_at, d_pats + h.present_at, d_pats, d_where, d_flags,
                                             cus, stream, plan->shards);
        }
        rc = stage_end(plan, stream);
        if (e != hipSuccess) return hip_fail(e, "launch gf_heal_mixed_plan");
        if (rc) return rc;
    }
    // the other route is never healed (locate gave it kLocSkipped): counted
    g_healplan_skipped.fetch_add(plan->mp_other.size(), std::memory_order_relaxed);
    return HBEC_OK;
}

// ---- the ShardHash of a plan's shards against the stored ones (hbec_hash_plan_mixed) ----

std::atomic<uint64_t> g_hashplan_launches{0}, g_hashplan_chains{0};

// The device side of a plan's hash call, built once: a record per source entry
// and the order its chains are listed in.
int hash_plan_device(const hbec_plan* p) {
    std::lock_guard<std::mutex> lk(p->mp_mu);
    if (p->hash_built) return HBEC_OK;
    std::vector<hbec::HRec> recs(p->src.size());
    for (size_t i = 0; i < p->src.size(); ++i) {
        const hbec::MSrc& s = p->src[i];
        recs[i] = hbec::HRec{s.a, s.b, s.shard_len, (uint32_t)hbec::loc_route(p->k, p->m, s.shard_len), 0u};
    }
    int rc = upload(recs, &p->d_hrecs, "plan hash records");
    if (rc) return rc;
    hbec::hash_order(p->src, p->hash_order);
    p->hash_built = true;
    return HBEC_OK;
}

int hash_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* select, uint32_t n_select,
                    const uint32_t* select_of, const uint32_t* d_filter, uint32_t filter_bits,
                    const uint8_t* d_expected, uint8_t* d_digests, uint32_t* d_bad, uint32_t* d_where,
                    hipStream_t stream) {
    if (!codec || !plan) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
    if (n_select > 65536) return fail(HBEC_ERR_INVALID_ARG, "more than 65536 selection rows");
    // what the given pointers say about each other holds for any plan
    if (d_where && !d_bad) return fail(HBEC_ERR_INVALID_ARG, "d_where needs d_bad");
    if (d_expected && !d_bad) return fail(HBEC_ERR_INVALID_ARG, "d_expected needs d_bad");
    if (d_expected && n > 32) return fail(HBEC_ERR_INVALID_ARG, "d_expected needs k + m <= 32 (one bit per shard)");
    if ((d_bad && (d_bad == d_where || d_bad == d_filter)) || (d_where && d_where == d_filter))
        return fail(HBEC_ERR_INVALID_ARG, "d_bad, d_where and d_filter must be distinct");
    if ((reinterpret_cast<uintptr_t>(d_digests) | reinterpret_cast<uintptr_t>(d_expected)) & 3u)
        return fail(HBEC_ERR_INVALID_ARG, "digest buffer not 4-byte aligned");
    const uint64_t n_src = plan->n_src;
    if (n_src == 0) return HBEC_OK;
    if (!select || !select_of) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    if (!n_select) return fail(HBEC_ERR_INVALID_ARG, "stripes but no selection rows");
    if (!d_digests && !d_expected) return fail(HBEC_ERR_INVALID_ARG, "neither d_digests nor d_expected given");
    bool any = false;
    for (uint64_t i = 0; i < n_src; ++i) {  // zero-length entries too
        if (select_of[i] >= n_select)
            return fail(HBEC_ERR_INVALID_ARG, "selection index out of range (stripe " + std::to_string(i) + ")");
        any = any || plan->src[i].shard_len;
    }
    if (!any) return HBEC_OK;  // zero-length entries only
    int rc = hash_plan_device(plan);
    if (rc) return rc;
    // per call: the chain list, then (for d_where) every entry's selected-shard bits
    std::vector<hbec::HChain> chains;
    hbec::hash_chains(plan->hash_order, n, select, n_select, select_of, chains);
    if (chains.empty()) return HBEC_OK;
    if (chains.size() / 64 >= (1ull << 31)) return fail(HBEC_ERR_INVALID_ARG, "call too large (>= 2^37 chains)");
    const size_t chain_words = chains.size() * (sizeof(hbec::HChain) / 4);
    std::vector<uint32_t> stage(chain_words + (d_where ? (size_t)n_src : 0));
    std::memcpy(stage.data(), chains.data(), chain_words * 4);
    if (d_where) {
        std::vector<uint32_t> bits(n_select);
        for (uint32_t p = 0; p < n_select; ++p) bits[p] = hbec::hash_select_bits(n, select + (size_t)p * n);
        for (uint64_t i = 0; i < n_src; ++i) stage[chain_words + i] = bits[select_of[i]];
    }
    std::lock_guard<std::mutex> lk(plan->mp_mu);
    rc = stage_begin(plan, stage, stream);
    if (rc) return rc;
    const hbec::HChain* d_chains = reinterpret_cast<const hbec::HChain*>(plan->d_mstage);
    g_hashplan_launches.fetch_add(1, std::memory_order_relaxed);
    g_hashplan_chains.fetch_add(chains.size(), std::memory_order_relaxed);
    hipError_t e = hbec::launch_md5_plan(plan->d_hrecs, d_chains, chains.size(), k, n, d_filter, filter_bits,
                                         d_expected, d_digests, d_expected ? d_bad : nullptr, stream, plan->shards);
    if (e == hipSuccess && d_where) {
        g_hashplan_launches.fetch_add(1, std::memory_order_relaxed);
        e = hbec::launch_hash_where(plan->d_hrecs, (uint32_t)n_src, plan->d_mstage + chain_words, d_filter,
                                    filter_bits, d_bad, d_where, stream);
    }
    rc = stage_end(plan, stream);
    if (e != hipSuccess) return hip_fail(e, "launch md5_plan");
    return rc;
}

// ---- the ShardHash of multi-stripe shard files on a plan (hbec_hash_plan_files) ----

std::atomic<uint64_t> g_hashfiles_launches{0}, g_hashfiles_chains{0}, g_hashfiles_segments{0};

int hash_plan_files(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                    const uint8_t* select, uint32_t n_select, const uint32_t* select_of, const uint32_t* d_filter,
                    uint32_t filter_bits, const uint8_t* d_expected, uint8_t* d_digests, uint32_t* d_bad,
                    uint32_t* d_where, hipStream_t stream) {
    if (!codec || !plan) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
    if (n_select > 65536) return fail(HBEC_ERR_INVALID_ARG, "more than 65536 selection rows");
    // what the given pointers say about each other holds for any plan, as in hash_plan_mixed
    if (d_where && !d_bad) return fail(HBEC_ERR_INVALID_ARG, "d_where needs d_bad");
    if (d_expected && !d_bad) return fail(HBEC_ERR_INVALID_ARG, "d_expected needs d_bad");
    if (d_expected && n > 32) return fail(HBEC_ERR_INVALID_ARG, "d_expected needs k + m <= 32 (one bit per shard)");
    if ((d_bad && (d_bad == d_where || d_bad == d_filter)) || (d_where && d_where == d_filter))
        return fail(HBEC_ERR_INVALID_ARG, "d_bad, d_where and d_filter must be distinct");
    if ((reinterpret_cast<uintptr_t>(d_digests) | reinterpret_cast<uintptr_t>(d_expected)) & 3u)
        return fail(HBEC_ERR_INVALID_ARG, "digest buffer not 4-byte aligned");
    const uint64_t n_src = plan->n_src;
    if (n_src == 0) return HBEC_OK;
    if (const char* why = hbec::files_check_objects(object_start, n_objects, n_src))
        return fail(HBEC_ERR_INVALID_ARG, why);
    if (!select || !select_of) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    if (!d_digests && !d_expected) return fail(HBEC_ERR_INVALID_ARG, "neither d_digests nor d_expected given");
    for (uint32_t g = 0; g < n_objects; ++g)  // empty objects too
        if (select_of[g] >= n_select)
            return fail(HBEC_ERR_INVALID_ARG, "selection index out of range (object " + std::to_string(g) + ")");
    // per call: the chain list and the object table, then (for d_where) every entry's object
    // and every object's selected-shard bits
    std::vector<hbec::FChain> chains;
    const uint64_t segments = hbec::files_chains(plan->src, object_start, n_objects, n, select, n_select, select_of,
                                                 chains);
    if (chains.empty()) return HBEC_OK;  // zero-length entries only, or nothing selected
    if (chains.size() / 64 >= (1ull << 31)) return fail(HBEC_ERR_INVALID_ARG, "call too large (>= 2^37 chains)");
    int rc = hash_plan_device(plan);
    if (rc) return rc;
    const size_t chain_words = chains.size() * (sizeof(hbec::FChain) / 4);
    const size_t objects_at = chain_words, of_at = objects_at + n_objects + 1, sel_at = of_at + (size_t)n_src;
    std::vector<uint32_t> stage(d_where ? sel_at + n_objects : of_at);
    std::memcpy(stage.data(), chains.data(), chain_words * 4);
    std::memcpy(stage.data() + objects_at, object_start, ((size_t)n_objects + 1) * 4);
    if (d_where) {
        std::vector<uint32_t> object_of;
        hbec::files_entry_objects(object_start, n_objects, object_of);
        std::memcpy(stage.data() + of_at, object_of.data(), (size_t)n_src * 4);
        for (uint32_t g = 0; g < n_objects; ++g)
            stage[sel_at + g] = hbec::hash_select_bits(n, select + (size_t)select_of[g] * n);
    }
    std::lock_guard<std::mutex> lk(plan->mp_mu);
    rc = stage_begin(plan, stage, stream);
    if (rc) return rc;
    const uint32_t* d_stage = plan->d_mstage;
    g_hashfiles_launches.fetch_add(1, std::memory_order_relaxed);
    g_hashfiles_chains.fetch_add(chains.size(), std::memory_order_relaxed);
    g_hashfiles_segments.fetch_add(segments, std::memory_order_relaxed);
    hipError_t e = hbec::launch_md5_files(plan->d_hrecs, d_stage + objects_at,
                                          reinterpret_cast<const hbec::FChain*>(d_stage), chains.size(), k, n,
                                          d_filter, filter_bits, d_expected, d_digests,
                                          d_expected ? d_bad : nullptr, stream, plan->shards);
    if (e == hipSuccess && d_where) {
        g_hashfiles_launches.fetch_add(1, std::memory_order_relaxed);
        e = hbec::launch_hash_files_where(plan->d_hrecs, (uint32_t)n_src, d_stage + of_at, d_stage + sel_at, d_filter,
                                          filter_bits, d_bad, d_where, stream);
    }
    rc = stage_end(plan, stream);
    if (e != hipSuccess) return hip_fail(e, "launch md5_files");
    return rc;
}

// The calls with one pattern for all (hbec_encode_plan, hbec_reconstruct_plan,
// hbec_verify_plan) on a shards plan: the call with a pattern per entry, every
// entry given pattern 0.
template <class F>
int uniform_mixed(const hbec_plan* plan, F&& call) {
    const std::vector<uint32_t> of((size_t)plan->n_src, 0u);
    return call(of.data());
}

// A shards plan from its table: shard j of entry e at rows[e n + j], lens[e]
// bytes each.  Every argument error is found before the first HIP call.
int build_shards_plan(hbec_codec* codec, std::vector<uint64_t>&& rows, const std::vector<uint64_t>& lens,
                      hbec_plan** out) {
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    const uint64_t n_src = lens.size();
    if (n_src >= (1ull << 32)) return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^32 entries)");
    std::unique_ptr<hbec_plan> p(new (std::nothrow) hbec_plan());
    if (!p) return fail(HBEC_ERR_NOMEM, "plan allocation");
    p->k = k;
    p->m = m;
    p->shards = true;
    p->n_src = n_src;
    p->src.assign((size_t)n_src, hbec::MSrc{0, 0, 0});
    std::vector<uint64_t> tmp;
    for (uint64_t e = 0; e < n_src; ++e) {
        if (lens[e] == 0) continue;
        if (const char* why = hbec::shards_check_row(rows.data() + (size_t)e * n, n, lens[e], tmp))
            return fail(HBEC_ERR_INVALID_ARG, std::string(why) + " (entry " + std::to_string(e) + ")");
        p->src[e].shard_len = lens[e];
        p->shard_bytes += lens[e];
    }
    p->rows = std::move(rows);
    if (p->shard_bytes > 0) {
        int rc = upload(p->rows, &p->d_rows, "plan shard address rows");
        if (rc) return rc;
        for (uint64_t e = 0; e < n_src; ++e)
            if (lens[e]) p->src[e].a = reinterpret_cast<uint64_t>(p->d_rows + (size_t)e * n);
    }
    *out = p.release();
    return HBEC_OK;
}

}  // namespace

extern "C" {

int hbec_plan_shards(hbec_codec* codec, void* const* shards, const uint64_t* shard_lens, uint64_t n_entries,
                     hbec_plan** out) {
    return hbec::guarded("hbec_plan_shards", [&]() -> int {
        if (!codec || !out || !shards || !shard_lens) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *out = nullptr;
        if (n_entries >= (1ull << 32)) return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^32 entries)");
        const size_t n = (size_t)(hbec_data_shards(codec) + hbec_parity_shards(codec));
        std::vector<uint64_t> rows((size_t)n_entries * n), lens(shard_lens, shard_lens + n_entries);
        for (size_t i = 0; i < rows.size(); ++i) rows[i] = reinterpret_cast<uint64_t>(shards[i]);
        return build_shards_plan(codec, std::move(rows), lens, out);
    });
}

int hbec_plan_files(hbec_codec* codec, const hbec_file_object* objects, uint32_t n_objects, uint64_t chunk_size,
                    uint32_t* object_start, hbec_plan** out) {
    return hbec::guarded("hbec_plan_files", [&]() -> int {
        if (!codec || !out || !object_start || (n_objects && !objects))
            return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *out = nullptr;
        if (chunk_size == 0 || chunk_size > (uint64_t)INT64_MAX)
            return fail(HBEC_ERR_INVALID_ARG, "chunk_size must be 1 .. 2^63 - 1");
        const int k = hbec_data_shards(codec), n = k + hbec_parity_shards(codec);
        uint64_t total = 0;
        for (uint32_t g = 0; g < n_objects; ++g) {
            const hbec_file_object& o = objects[g];
            if (o.content_length > (uint64_t)INT64_MAX)
                return fail(HBEC_ERR_INVALID_ARG, "content_length above 2^63 - 1 (object " + std::to_string(g) + ")");
            const uint64_t c = hbec::ec_stripe_count((int64_t)o.content_length, k, (int64_t)chunk_size);
            if (c && !o.files) return fail(HBEC_ERR_INVALID_ARG, "null files (object " + std::to_string(g) + ")");
            for (int j = 0; c && j < n; ++j)
                if (!o.files[j])
                    return fail(HBEC_ERR_INVALID_ARG, "null file pointer in an object with content_length > 0 "
                                                      "(object " + std::to_string(g) + ")");
            total += c;
            if (total > 0xFFFFFFFFull) return fail(HBEC_ERR_INVALID_ARG, "more than 2^32 - 1 entries");
        }
        std::vector<uint64_t> rows, lens;
        rows.reserve((size_t)total * n);
        lens.reserve((size_t)total);
        object_start[0] = 0;
        for (uint32_t g = 0; g < n_objects; ++g) {
            const hbec_file_object& o = objects[g];
            const uint64_t c = hbec::ec_stripe_count((int64_t)o.content_length, k, (int64_t)chunk_size);
            for (uint64_t t = 0; t < c; ++t) {
                lens.push_back(hbec::ec_stripe_shard_length((int64_t)o.content_length, k, (int64_t)chunk_size, t));
                for (int j = 0; j < n; ++j) rows.push_back(reinterpret_cast<uint64_t>(o.files[j]) + t * chunk_size);
            }
            object_start[g + 1] = (uint32_t)lens.size();
        }
        return build_shards_plan(codec, std::move(rows), lens, out);
    });
}

int hbec_plan_stripes(hbec_codec* codec, const hbec_stripe* stripes, uint64_t n, hbec_plan** out) {
    return hbec::guarded("hbec_plan_stripes", [&]() -> int {
        if (!codec || !out || (n && !stripes)) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *out = nullptr;
        const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
        std::unique_ptr<hbec_plan> p(new (std::nothrow) hbec_plan());
        if (!p) return fail(HBEC_ERR_NOMEM, "plan allocation");
        p->k = k;
        p->m = m;
        p->tile_bytes = hbec::stripes_tile_bytes(std::min(k, hbec::kStripeMaxK));
        if (n >= (1ull << 32)) return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^32 stripes)");
        p->n_src = n;
        p->src.assign((size_t)n, hbec::MSrc{0, 0, 0});
        std::vector<hbec::TileRec> recs;
        std::vector<hbec::URec> urecs, erecs, brecs, orecs;
        hbec::VerifyRecs vr;
        for (uint64_t i = 0; i < n; ++i) {
            const hbec_stripe& s = stripes[i];
            if (s.shard_len == 0) continue;
            if (!s.base) return fail(HBEC_ERR_INVALID_ARG, "stripe with null base");
            p->src[i] = {reinterpret_cast<uint64_t>(s.base),
                         reinterpret_cast<uint64_t>(s.base) + (uint64_t)k * s.shard_len, s.shard_len};
            p->shard_bytes += s.shard_len;
            const uint64_t sa = reinterpret_cast<uint64_t>(s.base);
            // (aligned stripes the record kernels code faster join them, hbec.cpp rec_route)
            const bool tiled = aligned_stripe(s) &&
                               !hbec::plan_rec_route(codec, s.shard_len, (sa & 127u) == 0 && s.shard_len % 128 == 0);
            if (m > 0 && !(tiled && hbec::vp_tiles_shape(k, m)) &&
                !hbec::vp_add(vr, k, m, sa, sa + (uint64_t)k * s.shard_len, s.shard_len, i))
                return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^31 tiles)");
            if (!tiled) {
                p->fallback.push_back(s);
                add_urecs(urecs, erecs, brecs, orecs, s.base, nullptr, s.shard_len, k);
                continue;
            }
            p->tiled.push_back(s);
            for (uint64_t off = 0; off < s.shard_len; off += (uint64_t)p->tile_bytes) {
                hbec::TileRec r;
                r.in_addr = r.out_addr = reinterpret_cast<uint64_t>(s.base) + off;
                r.in_stride = r.out_stride = (uint32_t)s.shard_len;
                r.valid = (uint32_t)std::min<uint64_t>((uint64_t)p->tile_bytes, s.shard_len - off);
                r.pad_ = (uint32_t)i;  // Verify: the flag of this tile's stripe
                recs.push_back(r);
            }
        }
        // both record counts are checked before anything is allocated on the device
        if (recs.size() >= (1ull << 31) || urecs.size() >= (1ull << 31) || erecs.size() >= (1ull << 31) ||
            brecs.size() >= (1ull << 31))
            return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^31 tiles)");
        p->n_tiles = recs.size();
        if (!recs.empty()) {
            hipError_t e = hipMalloc(&p->d_tiles, recs.size() * sizeof(hbec::TileRec));
            if (e != hipSuccess) return hip_fail(e, "hipMalloc plan tiles");
            e = hipMemcpy(p->d_tiles, recs.data(), recs.size() * sizeof(hbec::TileRec), hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(p->d_tiles);
                p->d_tiles = nullptr;
                return hip_fail(e, "hipMemcpy plan tiles");
            }
        }
        // edge records of the stripes with no main tiles (S <= odd_min_main()) first
        const auto short_end = std::stable_partition(erecs.begin(), erecs.end(), [](const hbec::URec& e) {
            return e.shard_len <= hbec::odd_min_main();
        });
        const uint64_t n_short = (uint64_t)(short_end - erecs.begin());
        int urc = upload(urecs, &p->d_urecs, "plan unaligned records");
        if (!urc) urc = upload(erecs, &p->d_erecs, "plan edge records");
        if (!urc) urc = upload(brecs, &p->d_brecs, "plan large-shard records");
        if (!urc) urc = upload(orecs, &p->d_orecs, "plan stripe records");
        if (!urc) urc = build_tile_lists(p.get(), orecs);
        if (!urc) urc = upload_verify(p.get(), codec, vr);
        if (urc) {
            hbec_plan_free(p.release());
            return urc;
        }
        p->n_urecs = urecs.size();
        p->n_erecs = erecs.size();
        p->orecs.edges_long = n_short == 0;
        p->orecs.n_short_edges = n_short;
        p->n_brecs = brecs.size();
        *out = p.release();
        return HBEC_OK;
    });
}

int hbec_plan_objects(hbec_codec* codec, const hbec_object* objects, uint64_t n, hbec_plan** out) {
    return hbec::guarded("hbec_plan_objects", [&]() -> int {
        if (!codec || !out || (n && !objects)) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *out = nullptr;
        const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
        std::unique_ptr<hbec_plan> p(new (std::nothrow) hbec_plan());
        if (!p) return fail(HBEC_ERR_NOMEM, "plan allocation");
        p->k = k;
        p->m = m;
        p->objects = true;
        p->tile_bytes = hbec::stripes_tile_bytes(std::min(k, hbec::kStripeMaxK));
        if (n >= (1ull << 32)) return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^32 objects)");
        p->n_src = n;
        p->src.assign((size_t)n, hbec::MSrc{0, 0, 0});
        std::vector<hbec::TileRec> recs;
        std::vector<hbec::URec> urecs, erecs, brecs, orecs;
        hbec::VerifyRecs vr;
        for (uint64_t i = 0; i < n; ++i) {
            const hbec_object& o = objects[i];
            if (o.shard_len == 0) continue;
            if (!o.data || (m > 0 && !o.parity)) return fail(HBEC_ERR_INVALID_ARG, "object with null data or parity");
            p->src[i] = {reinterpret_cast<uint64_t>(o.data), reinterpret_cast<uint64_t>(o.parity), o.shard_len};
            p->shard_bytes += o.shard_len;
            const bool line = ((reinterpret_cast<uintptr_t>(o.data) | reinterpret_cast<uintptr_t>(o.parity)) & 127u) == 0 &&
                              o.shard_len % 128 == 0;
            const bool to_recs =
                !aligned_object(o) || (k <= hbec::kStripeMaxK && hbec::plan_rec_route(codec, o.shard_len, line));
            // tile records exist for aligned objects of k <= 8 that stay off the record route
            if (m > 0 && !(!to_recs && hbec::vp_tiles_shape(k, m)) &&
                !hbec::vp_add(vr, k, m, reinterpret_cast<uint64_t>(o.data), reinterpret_cast<uint64_t>(o.parity),
                              o.shard_len, i))
                return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^31 tiles)");
            if (to_recs) {
                p->obj_fallback.push_back(o);
                add_urecs(urecs, erecs, brecs, orecs, o.data, o.parity, o.shard_len, k);
                continue;
            }
            if (k > hbec::kStripeMaxK) {
                // the object-plan tiled kernel takes <= 8 inputs: every object goes to
                // the unaligned kernel's records (one launch per pass, not one per object)
                add_urecs(urecs, erecs, brecs, orecs, o.data, o.parity, o.shard_len, k);
                continue;
            }
            p->obj_tiled.push_back(o);
            for (uint64_t off = 0; off < o.shard_len; off += (uint64_t)p->tile_bytes) {
                hbec::TileRec r;
                r.in_addr = reinterpret_cast<uint64_t>(o.data) + off;
                r.out_addr = reinterpret_cast<uint64_t>(o.parity) + off;
                r.in_stride = r.out_stride = (uint32_t)o.shard_len;
                r.valid = (uint32_t)std::min<uint64_t>((uint64_t)p->tile_bytes, o.shard_len - off);
                r.pad_ = (uint32_t)i;  // Verify: the flag of this tile's stripe
                recs.push_back(r);
            }
        }
        // both record counts are checked before anything is allocated on the device
        if (recs.size() >= (1ull << 31) || urecs.size() >= (1ull << 31) || erecs.size() >= (1ull << 31) ||
            brecs.size() >= (1ull << 31))
            return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^31 tiles)");
        p->n_tiles = recs.size();
        if (!recs.empty()) {
            hipError_t e = hipMalloc(&p->d_tiles, recs.size() * sizeof(hbec::TileRec));
            if (e != hipSuccess) return hip_fail(e, "hipMalloc plan tiles");
            e = hipMemcpy(p->d_tiles, recs.data(), recs.size() * sizeof(hbec::TileRec), hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(p->d_tiles);
                p->d_tiles = nullptr;
                return hip_fail(e, "hipMemcpy plan tiles");
            }
        }
        // edge records of the stripes with no main tiles (S <= odd_min_main()) first
        const auto short_end = std::stable_partition(erecs.begin(), erecs.end(), [](const hbec::URec& e) {
            return e.shard_len <= hbec::odd_min_main();
        });
        const uint64_t n_short = (uint64_t)(short_end - erecs.begin());
        int urc = upload(urecs, &p->d_urecs, "plan unaligned records");
        if (!urc) urc = upload(erecs, &p->d_erecs, "plan edge records");
        if (!urc) urc = upload(brecs, &p->d_brecs, "plan large-shard records");
        if (!urc) urc = upload(orecs, &p->d_orecs, "plan stripe records");
        if (!urc) urc = build_tile_lists(p.get(), orecs);
        if (!urc) urc = upload_verify(p.get(), codec, vr);
        if (urc) {
            hbec_plan_free(p.release());
            return urc;
        }
        p->n_urecs = urecs.size();
        p->n_erecs = erecs.size();
        p->orecs.edges_long = n_short == 0;
        p->orecs.n_short_edges = n_short;
        p->n_brecs = brecs.size();
        *out = p.release();
        return HBEC_OK;
    });
}

void hbec_plan_free(hbec_plan* plan) {
    if (!plan) return;
    if (plan->d_tiles) (void)hipFree(plan->d_tiles);
    if (plan->d_urecs) (void)hipFree(plan->d_urecs);
    if (plan->d_erecs) (void)hipFree(plan->d_erecs);
    if (plan->d_brecs) (void)hipFree(plan->d_brecs);
    if (plan->d_orecs) (void)hipFree(plan->d_orecs);
    if (plan->d_vrecs) (void)hipFree(plan->d_vrecs);
    if (plan->d_vtiles) (void)hipFree(plan->d_vtiles);
    if (plan->d_vtab) (void)hipFree(plan->d_vtab);
    if (plan->d_mrecs) (void)hipFree(plan->d_mrecs);
    if (plan->d_mtiles) (void)hipFree(plan->d_mtiles);
    if (plan->d_mstage) (void)hipFree(plan->d_mstage);
    if (plan->d_heal) (void)hipFree(plan->d_heal);
    if (plan->d_hrecs) (void)hipFree(plan->d_hrecs);
    if (plan->d_rows) (void)hipFree(plan->d_rows);
    if (plan->mp_ev) (void)hipEventDestroy(plan->mp_ev);
    for (uint32_t* l : plan->d_lists)
        if (l) (void)hipFree(l);
    delete plan;
}

int hbec_plan_info(const hbec_plan* plan, uint64_t* n_tiles, int* tile_bytes, uint64_t* n_fallback,
                   uint64_t* shard_bytes) {
    return hbec::guarded("hbec_plan_info", [&]() -> int {
        if (!plan) return fail(HBEC_ERR_INVALID_ARG, "null plan");
        if (n_tiles) *n_tiles = plan->n_tiles;
        if (tile_bytes) *tile_bytes = plan->tile_bytes;
        if (n_fallback) *n_fallback = plan->objects ? plan->obj_fallback.size() : plan->fallback.size();
        if (shard_bytes) *shard_bytes = plan->shard_bytes;
        return HBEC_OK;
    });
}

int hbec_encode_plan(hbec_codec* codec, const hbec_plan* plan, void* hip_stream) {
    return hbec::guarded("hbec_encode_plan", [&]() -> int {
        if (!codec || !plan) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
        if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
        if (m == 0) return HBEC_OK;
        if (plan->shards) {
            // data present, parity missing: that mask's decode rows are the parity rows
            std::vector<uint8_t> mask((size_t)k + m, 0);
            std::fill(mask.begin(), mask.begin() + k, (uint8_t)1);
            return uniform_mixed(plan, [&](const uint32_t* of) {
                return reconstruct_plan_mixed(codec, plan, mask.data(), 1, of, false,
                                              static_cast<hipStream_t>(hip_stream));
            });
        }
        std::vector<uint8_t> mat((size_t)(k + m) * k);
        hbec_matrix(codec, mat.data());
        std::vector<uint8_t> rows(mat.begin() + (size_t)k * k, mat.end());
        std::vector<int> in_idx(k), out_idx(m);
        for (int j = 0; j < k; ++j) in_idx[j] = j;
        for (int r = 0; r < m; ++r) out_idx[r] = k + r;
        return run_plan(plan, in_idx, out_idx, rows, static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_reconstruct_plan(hbec_codec* codec, const hbec_plan* plan, const uint8_t* present, int data_only,
                          void* hip_stream) {
    return hbec::guarded("hbec_reconstruct_plan", [&]() -> int {
        if (!codec || !plan || !present) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
        if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
        int n_present = 0, data_present = 0;
        for (int i = 0; i < n; ++i) {
            n_present += present[i] ? 1 : 0;
            if (i < k) data_present += present[i] ? 1 : 0;
        }
        if (n_present == n || (data_only && data_present == k)) return HBEC_OK;
        if (n_present < k) return fail(HBEC_ERR_TOO_FEW_SHARDS, "too few shards given");
        if (plan->shards)
            return uniform_mixed(plan, [&](const uint32_t* of) {
                return reconstruct_plan_mixed(codec, plan, present, 1, of, data_only != 0,
                                              static_cast<hipStream_t>(hip_stream));
            });
        std::vector<int> surv(k), outs(n);
        std::vector<uint8_t> rows((size_t)n * k);
        int n_out = 0;
        int rc = hbec_decode_rows(codec, present, data_only, surv.data(), outs.data(), &n_out, rows.data());
        if (rc) return rc;
        outs.resize(n_out);
        rows.resize((size_t)n_out * k);
        return run_plan(plan, surv, outs, rows, static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_reconstruct_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                                const uint32_t* pattern_of, int data_only, void* hip_stream) {
    return hbec::guarded("hbec_reconstruct_plan_mixed", [&]() -> int {
        return reconstruct_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, data_only != 0,
                                      static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_mixed_plan_stats(uint64_t* kernel_launches, uint64_t* per_stripe_calls) {
    return hbec::guarded("hbec_mixed_plan_stats", [&]() -> int {
        if (!kernel_launches || !per_stripe_calls) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *kernel_launches = g_mplan_launches.load(std::memory_order_relaxed);
        *per_stripe_calls = g_mplan_per_stripe.load(std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_stripes_kernel_stats(uint64_t* plain, uint64_t* split, uint64_t* accumulate, uint64_t* mirror,
                              uint64_t* mirror_accumulate) {
    return hbec::guarded("hbec_stripes_kernel_stats", [&]() -> int {
        uint64_t* const out[hbec::kSkCount] = {plain, split, accumulate, mirror, mirror_accumulate};
        for (int i = 0; i < hbec::kSkCount; ++i)
            if (out[i]) *out[i] = hbec::stripes_launches(i);
        return HBEC_OK;
    });
}

int hbec_set_stripes_grid_cap(int blocks) {
    return hbec::guarded("hbec_set_stripes_grid_cap", [&]() -> int {
        if (blocks < 0) return fail(HBEC_ERR_INVALID_ARG, "stripes grid cap: negative");
        g_stripes_grid_cap.store(blocks, std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_mixed_plan_tile_bytes(void) { return (int)hbec::mixed_plan_tile_bytes(); }

int hbec_set_mixed_plan_chunk_tiles(uint64_t tiles) {
    return hbec::guarded("hbec_set_mixed_plan_chunk_tiles", [&]() -> int {
        g_mplan_chunk_override.store(tiles, std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_verify_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                           const uint32_t* pattern_of, uint32_t* d_flags, void* hip_stream) {
    return hbec::guarded("hbec_verify_plan_mixed", [&]() -> int {
        return verify_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, d_flags,
                                 static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_verify_mixed_plan_stats(uint64_t* kernel_launches, uint64_t* per_stripe_calls) {
    return hbec::guarded("hbec_verify_mixed_plan_stats", [&]() -> int {
        if (!kernel_launches || !per_stripe_calls) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *kernel_launches = g_vmplan_launches.load(std::memory_order_relaxed);
        *per_stripe_calls = g_vmplan_per_stripe.load(std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_verify_mixed_plan_tile_bytes(void) { return (int)hbec::verify_mixed_plan_tile_bytes(); }

int hbec_set_verify_mixed_plan_chunk_tiles(uint64_t tiles) {
    return hbec::guarded("hbec_set_verify_mixed_plan_chunk_tiles", [&]() -> int {
        g_vmplan_chunk_override.store(tiles, std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_repair_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                           const uint32_t* pattern_of, int data_only, uint32_t* d_flags, void* hip_stream) {
    return hbec::guarded("hbec_repair_plan_mixed", [&]() -> int {
        return repair_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, data_only != 0, d_flags,
                                 static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_repair_plan_stats(uint64_t* kernel_launches, uint64_t* per_stripe_calls) {
    return hbec::guarded("hbec_repair_plan_stats", [&]() -> int {
        if (!kernel_launches || !per_stripe_calls) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *kernel_launches = g_rplan_launches.load(std::memory_order_relaxed);
        *per_stripe_calls = g_rplan_per_stripe.load(std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_repair_plan_tile_bytes(void) { return (int)hbec::repair_plan_tile_bytes(); }

int hbec_set_repair_plan_chunk_tiles(uint64_t tiles) {
    return hbec::guarded("hbec_set_repair_plan_chunk_tiles", [&]() -> int {
        g_rplan_chunk_override.store(tiles, std::memory_order_relaxed);
        return HBEC_OK;
    });
}

static_assert(HBEC_LOC_BAD == hbec::kLocBad && HBEC_LOC_SKIPPED == hbec::kLocSkipped &&
                  HBEC_LOC_NOTHING == hbec::kLocNothing && HBEC_LOC_CLEAN == hbec::kLocClean &&
                  HBEC_LOC_AMBIGUOUS == hbec::kLocAmbiguous && HBEC_LOC_MULTIPLE == hbec::kLocMultiple &&
                  HBEC_LOC_UNCHECKED == hbec::kLocUnchecked,
              "include/hbec.h and locate.h disagree");

int hbec_locate_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                           const uint32_t* pattern_of, const uint32_t* d_flags, uint32_t* d_where, void* hip_stream) {
    return hbec::guarded("hbec_locate_plan_mixed", [&]() -> int {
        return locate_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, d_flags, d_where,
                                 static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_locate_decode(int k, int m, const uint8_t* present, uint32_t where) {
    if (!present || k < 1 || m < 0 || k + m > 256) return HBEC_ERR_INVALID_ARG;
    return hbec::loc_decode(k, m, present, where);
}

int hbec_locate_plan_stats(uint64_t* kernel_launches, uint64_t* skipped_entries) {
    return hbec::guarded("hbec_locate_plan_stats", [&]() -> int {
        if (!kernel_launches || !skipped_entries) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *kernel_launches = g_locplan_launches.load(std::memory_order_relaxed);
        *skipped_entries = g_locplan_skipped.load(std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_locate_plan_tile_bytes(void) { return (int)hbec::locate_plan_tile_bytes(); }

int hbec_set_locate_plan_chunk_tiles(uint64_t tiles) {
    return hbec::guarded("hbec_set_locate_plan_chunk_tiles", [&]() -> int {
        g_locplan_chunk_override.store(tiles, std::memory_order_relaxed);
        return HBEC_OK;
    });
}

static_assert(HBEC_HEAL_DONE == hbec::kHealDone && HBEC_HEAL_UNNAMED == hbec::kHealUnnamed,
              "include/hbec.h and heal.h disagree");

int hbec_heal_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                         const uint32_t* pattern_of, const uint32_t* d_where, uint32_t* d_flags, void* hip_stream) {
    return hbec::guarded("hbec_heal_plan_mixed", [&]() -> int {
        return heal_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, d_where, d_flags,
                               static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_heal_plan_stats(uint64_t* kernel_launches, uint64_t* skipped_entries) {
    return hbec::guarded("hbec_heal_plan_stats", [&]() -> int {
        if (!kernel_launches || !skipped_entries) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *kernel_launches = g_healplan_launches.load(std::memory_order_relaxed);
        *skipped_entries = g_healplan_skipped.load(std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_heal_plan_tile_bytes(void) { return (int)hbec::heal_plan_tile_bytes(); }

int hbec_set_heal_plan_chunk_tiles(uint64_t tiles) {
    return hbec::guarded("hbec_set_heal_plan_chunk_tiles", [&]() -> int {
        g_healplan_chunk_override.store(tiles, std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_hash_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* select, uint32_t n_select,
                         const uint32_t* select_of, const uint32_t* d_filter, uint32_t filter_bits,
                         const uint8_t* d_expected, uint8_t* d_digests, uint32_t* d_bad, uint32_t* d_where,
                         void* hip_stream) {
    return hbec::guarded("hbec_hash_plan_mixed", [&]() -> int {
        return hash_plan_mixed(codec, plan, select, n_select, select_of, d_filter, filter_bits, d_expected, d_digests,
                               d_bad, d_where, static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_hash_plan_stats(uint64_t* kernel_launches, uint64_t* chains) {
    return hbec::guarded("hbec_hash_plan_stats", [&]() -> int {
        if (!kernel_launches || !chains) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *kernel_launches = g_hashplan_launches.load(std::memory_order_relaxed);
        *chains = g_hashplan_chains.load(std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_hash_plan_files(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                         const uint8_t* select, uint32_t n_select, const uint32_t* select_of,
                         const uint32_t* d_filter, uint32_t filter_bits, const uint8_t* d_expected,
                         uint8_t* d_digests, uint32_t* d_bad, uint32_t* d_where, void* hip_stream) {
    return hbec::guarded("hbec_hash_plan_files", [&]() -> int {
        return hash_plan_files(codec, plan, object_start, n_objects, select, n_select, select_of, d_filter,
                               filter_bits, d_expected, d_digests, d_bad, d_where,
                               static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_hash_files_stats(uint64_t* kernel_launches, uint64_t* chains, uint64_t* segments) {
    return hbec::guarded("hbec_hash_files_stats", [&]() -> int {
        if (!kernel_launches || !chains || !segments) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *kernel_launches = g_hashfiles_launches.load(std::memory_order_relaxed);
        *chains = g_hashfiles_chains.load(std::memory_order_relaxed);
        *segments = g_hashfiles_segments.load(std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_verify_plan(hbec_codec* codec, const hbec_plan* plan, uint32_t* d_flags, void* hip_stream) {
    return hbec::guarded("hbec_verify_plan", [&]() -> int {
        if (!codec || !plan || (!d_flags && plan->n_src)) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
        if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
        if (m == 0 || plan->shard_bytes == 0) return HBEC_OK;
        hipStream_t stream = static_cast<hipStream_t>(hip_stream);
        if (plan->shards) {
            // every shard present: the m parity shards are the checked ones, bit 0 only
            const std::vector<uint8_t> mask((size_t)k + m, 1);
            return uniform_mixed(plan, [&](const uint32_t* of) {
                return verify_plan_mixed(codec, plan, mask.data(), 1, of, d_flags, stream);
            });
        }
        if (plan->n_tiles > 0 && hbec::vp_tiles_shape(k, m)) {
            // the aligned stripes' tile records (the other shapes have a VRec each)
            std::vector<uint8_t> mat((size_t)(k + m) * k);
            hbec_matrix(codec, mat.data());
            hbec::VTileArgs a;
            std::memset(&a, 0, sizeof(a));
            a.n_tiles = (uint32_t)plan->n_tiles;
            a.split = plan->objects ? 1u : 0u;
            for (int r = 0; r < m; ++r)
                for (int j = 0; j < k; ++j) hbec::perm_table(mat[(size_t)(k + r) * k + j], a.tab[r][j]);
            int cus = 0;
            int rc = current_cus(&cus);
            if (rc) return rc;
            hipError_t e = hbec::launch_verify_tiles(k, m, a, plan->d_tiles, d_flags, cus, stream);
            if (e != hipSuccess) return hip_fail(e, "launch gf_verify_tiles");
            g_vplan_launches.fetch_add(1, std::memory_order_relaxed);
        }
        int rc = hbec::verify_recs_run(codec, plan->d_vrecs, plan->n_vrecs, plan->d_vtiles, plan->n_vtiles,
                                       plan->d_vtab, d_flags, stream);
        for (size_t i = 0; i < plan->vother.size() && !rc; ++i)
            rc = hbec::verify_other_run(codec, plan->vother[i], d_flags, stream);
        return rc;
    });
}

int hbec_verify_plan_stats(uint64_t* plan_launches, uint64_t* per_stripe_calls) {
    return hbec::guarded("hbec_verify_plan_stats", [&]() -> int {
        if (!plan_launches || !per_stripe_calls) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *plan_launches = g_vplan_launches.load(std::memory_order_relaxed);
        *per_stripe_calls = g_vplan_per_stripe.load(std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int hbec_verify_plan_tile_bytes(int k) {
    (void)k;  // gf_verify_recs takes k at run time: one tile size
    return (int)hbec::kVpTile;
}

}  // extern "C"
