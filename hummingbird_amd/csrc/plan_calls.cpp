// plan_calls.cpp — the calls on a plan with a pattern or a selection per source
// entry.  Reconstruct with an erasure pattern per stripe
// (hbec_reconstruct_plan_mixed) runs over per-source-entry records and a tile
// list of its own, built on first use (mixedplan.h, mixedplan.hip); Verify with
// a present mask per stripe (hbec_verify_plan_mixed) reads the same records and
// list (vmixed.h, vmixed.hip), and so do the call that names the corrupt shard
// (hbec_locate_plan_mixed; locate.h, locate.hip), the call that rebuilds and
// checks in one pass (hbec_repair_plan_mixed; repair.h, repair.hip) and the call
// that rebuilds the shard locate named (hbec_heal_plan_mixed; heal.h, heal.hip).
// The ShardHash audit of a plan (hbec_hash_plan_mixed; hashplan.h, hashplan.hip)
// has records of its own with 64-bit lengths, built on first use likewise, and
// stages its chain list where those calls stage their words.  The hash of
// multi-stripe shard files (hbec_hash_plan_files; hashfiles.h, hashfiles.hip)
// reads the same records and stages its chains and object table there too.
// The object bytes of every entry from its shards (hbec_glue_plan_mixed and its
// object-level form hbec_glue_plan_files; glue.h, glue.hip) walk Reconstruct's
// records and list and stage a destination per entry beside the words.  The
// inverse, every entry's shards from its object bytes (hbec_split_plan and
// hbec_split_plan_files; splitplan.h, splitplan.hip), walks them too and stages
// a source per entry.  Any byte range of every entry (hbec_glue_plan_range and
// hbec_glue_plan_files_range; gluerange.h, gluerange.hip) is the glue call with a
// start beside each length.  The ETag of every object (hbec_etag_plan_mixed and
// hbec_etag_plan_files; etag.h, etag.hip) decodes what is missing through that
// call into scratch and hashes the object bytes where they lie, on the hash
// calls' records.
// All of them stage and launch through staged_launches; plan.cpp builds the plans.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/hbec.h"
#include "etag.h"
#include "gf256.h"
#include "glue.h"
#include "gluerange.h"
#include "hashfiles.h"
#include "hashplan.h"
#include "heal.h"
#include "internal.h"
#include "kernels.h"
#include "locate.h"
#include "mixedplan.h"
#include "plan_internal.h"
#include "repair.h"
#include "shardplan.h"
#include "splitplan.h"
#include "vmixed.h"

using hbec::current_cus;
using hbec::fail;
using hbec::hip_fail;
using hbec::shard_addr;
using hbec::upload;

namespace {

// ---- counters and test hooks, a slot per call ----

enum Call { kReconstruct = 0, kVerify, kRepair, kLocate, kHeal, kHash, kHashFiles, kGlue, kSplit, kGlueRange, kEtag, kCalls };
struct CallSlot {
    std::atomic<uint64_t> launches{0};     // kernel launches
    std::atomic<uint64_t> second{0};       // per-stripe calls; skipped entries (locate, heal); chains (hash calls)
    std::atomic<uint64_t> chunk_tiles{0};  // test hook (hbec_set_*_chunk_tiles): tiles per launch of the walk kernel
};
CallSlot g_calls[kCalls];
std::atomic<uint64_t> g_hashfiles_segments{0};
std::atomic<uint64_t> g_etag_segments{0}, g_etag_decoded{0};  // hbec_etag_plan_stats' third and fourth

void count(std::atomic<uint64_t>& c, uint64_t n = 1) { c.fetch_add(n, std::memory_order_relaxed); }

int call_stats(const char* entry, Call c, uint64_t* launches, uint64_t* second) {
    return hbec::guarded(entry, [&]() -> int {
        if (!launches || !second) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        *launches = g_calls[c].launches.load(std::memory_order_relaxed);
        *second = g_calls[c].second.load(std::memory_order_relaxed);
        return HBEC_OK;
    });
}

int set_chunk_tiles(const char* entry, Call c, uint64_t tiles) {
    return hbec::guarded(entry, [&]() -> int {
        g_calls[c].chunk_tiles.store(tiles, std::memory_order_relaxed);
        return HBEC_OK;
    });
}

// ---- staging and launching, one skeleton for every call ----

// per-call staging of at most this many bytes goes through kernel arguments
// (kPutWordsMax words a launch: 18 launches), more through a copy
constexpr size_t kMPlanPutBytes = 64 * 1024;

// What a call queued under the lock: the first error of its launches and the
// words the error is reported with ("launch gf_...").
struct Queued {
    hipError_t e;
    const char* what;
};

// Words to a device buffer the plan owns (d_mstage, d_heal), grown to twice
// their size when they do not fit.  The caller holds mp_mu and `stream` has
// waited for whatever read the buffer last.
Queued put_words(uint32_t** d, size_t* cap_words, const std::vector<uint32_t>& w, hipStream_t stream,
                 const char* what_alloc, const char* what_put) {
    if (w.size() > *cap_words) {
        if (*d) (void)hipFree(*d);  // waits for the work that reads it
        *d = nullptr;
        *cap_words = 0;
        const size_t cap = std::max<size_t>(2 * w.size(), 4096);
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(d), cap * 4);
        if (e != hipSuccess) return Queued{e, what_alloc};
        *cap_words = cap;
    }
    return Queued{w.size() * 4 <= kMPlanPutBytes
                      ? hbec::launch_put_words(*d, w.data(), w.size() * 4, stream)
                      : hipMemcpyAsync(*d, w.data(), w.size() * 4, hipMemcpyHostToDevice, stream),
                  what_put};
}

// The staging discipline of every call on a plan with per-entry words.  A
// call's staging words go to a buffer the plan owns (d_mstage), not to
// stream-ordered scratch: with a scratch allocation and a copy from pageable
// memory per call, a call returned only when the one before it had run (4096
// stripes 4+2: 0.70 of a call's 0.74 ms on the host, against 0.016 ms for
// hbec_reconstruct_plan), so back-to-back calls never overlapped.  Up to
// kMPlanPutBytes the words travel in kernel arguments (launch_put_words).
// Calls on one plan, whichever of the seven, take turns under mp_mu from the
// upload of their words to the event recorded after their launches (mp_ev, on
// mp_stream); a call on another stream than the last waits for that event
// before it uploads, so the words of one call are never overwritten while its
// launches may still read them.  `queue(d_stage)` makes the call's launches
// inside that region.  Whatever else it keeps on the device for them (heal's
// d_heal) it uploads there too, with put_words: under the same lock, after the
// same wait, ordered by the same event.  A launch error wins over an error of
// the event record.
template <class Queue>
int staged_launches(const hbec_plan* plan, const std::vector<uint32_t>& stage, hipStream_t stream, Queue&& queue) {
    std::lock_guard<std::mutex> lk(plan->mp_mu);
    // after a call's launches: the next call on another stream waits for them
    auto end = [&]() -> int {
        plan->mp_stream = stream;
        const hipError_t e = hipEventRecord(plan->mp_ev, stream);
        return e == hipSuccess ? HBEC_OK : hip_fail(e, "hipEventRecord (plan mixed staging)");
    };
    if (!plan->mp_ev) {
        const hipError_t e = hipEventCreateWithFlags(&plan->mp_ev, hipEventDisableTiming);
        if (e != hipSuccess) return hip_fail(e, "hipEventCreate (plan mixed staging)");
    } else if (plan->mp_stream != stream) {
        const hipError_t e = hipStreamWaitEvent(stream, plan->mp_ev, 0);
        if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent (plan mixed staging)");
    }
    const Queued put = put_words(&plan->d_mstage, &plan->mstage_words, stage, stream, "hipMalloc plan mixed staging",
                                 "plan mixed staging");
    if (put.e != hipSuccess) {
        if (plan->d_mstage) (void)end();
        return hip_fail(put.e, put.what);
    }
    const Queued q = queue(static_cast<const uint32_t*>(plan->d_mstage));
    const int rc = end();
    if (q.e != hipSuccess) return hip_fail(q.e, q.what);
    return rc;
}

// The launches of a kernel that walks the plan's {entry, tile} list: one per
// chunk of n_tiles tiles (all of them in one, unless the call's test hook says
// otherwise), counted, until one fails.  launch(t0, nt) -> hipError_t.
template <class Launch>
Queued walk_chunks(Call c, uint64_t n_tiles, const char* what, Launch&& launch) {
    const uint64_t hook = g_calls[c].chunk_tiles.load(std::memory_order_relaxed);
    const uint64_t chunk = std::min<uint64_t>((1ull << 31) - 1, hook ? hook : ~0ull);
    hipError_t e = hipSuccess;
    for (uint64_t t0 = 0; t0 < n_tiles && e == hipSuccess; t0 += chunk) {
        count(g_calls[c].launches);
        e = launch(t0, (uint32_t)std::min<uint64_t>(chunk, n_tiles - t0));
    }
    return Queued{e, what};
}

// ---- the patterns of a call ----

// The device side of the calls that walk a plan's {entry, tile} list, built
// once: records and list into the plan's fields given, the entries of the other
// route into *other.  route_m: the parity count the entries are routed by.
int walk_list_device(const hbec_plan* p, int route_m, bool* built, hbec::MRec** d_recs, hbec::MTile** d_tiles,
                     uint64_t* n_tiles, std::vector<uint32_t>* other) {
    std::lock_guard<std::mutex> lk(p->mp_mu);
    if (*built) return HBEC_OK;
    hbec::MixedPlanRecs mr;
    if (!hbec::mp_build(mr, p->k, route_m, p->src, hbec::mixed_plan_tile_bytes()))
        return fail(HBEC_ERR_INVALID_ARG, "plan too large (>= 2^31 tiles)");
    if (!mr.tiles.empty()) {
        int rc = upload(mr.recs, d_recs, "plan mixed records");
        if (!rc) rc = upload(mr.tiles, d_tiles, "plan mixed tile list");
        if (rc) {
            if (*d_recs) (void)hipFree(*d_recs);
            *d_recs = nullptr;
            return rc;
        }
    }
    *n_tiles = mr.tiles.size();
    *other = std::move(mr.other);
    *built = true;
    return HBEC_OK;
}

// The device side of a plan's calls with a pattern per entry.
int mixed_plan_device(const hbec_plan* p) {
    return walk_list_device(p, p->m, &p->mp_built, &p->d_mrecs, &p->d_mtiles, &p->n_mtiles, &p->mp_other);
}

// Shards computed from a pattern's k survivors: idx.size() x k coefficients.
struct ShardSet {
    std::vector<int> surv, idx;
    std::vector<uint8_t> rows;
};
// One distinct pattern of a call, resolved.
struct PlanPattern {
    ShardSet out;       // the shards to rebuild (hbec_decode_rows)
    ShardSet chk;       // the present shards checked against the survivors (hbec_check_rows)
    uint64_t uses = 0;  // source entries with this pattern
    uint32_t rec = 0;   // its pattern record (kernel route)
};

// The argument checks every call with a pattern per source entry makes first,
// all before anything is queued; counts the non-empty entries of every pattern.
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

// For every pattern in use (check_plan_patterns counted them): its checked set
// (want_chk) and, unless nothing of it needs rebuilding, its rebuild set
// (want_out; data_only: missing parity stays missing).  *used: some pattern is
// in use.  Reconstruct asks for the second, Verify and locate for the first,
// repair for both.
int resolve_patterns(hbec_codec* codec, const uint8_t* patterns, bool want_out, bool data_only, bool want_chk,
                     std::vector<PlanPattern>& pats, bool* used) {
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    std::vector<uint8_t> mask((size_t)n);
    *used = false;
    // surv / idx / rows at the size the call may fill, then cut to what it filled
    auto fill = [k](ShardSet& s, int max_idx, auto&& rows_of) -> int {
        s.surv.resize(k);
        s.idx.resize(max_idx);
        s.rows.resize((size_t)max_idx * k);
        int n_idx = 0;
        const int rc = rows_of(s.surv.data(), s.idx.data(), &n_idx, s.rows.data());
        if (rc) return rc;
        s.idx.resize(n_idx);
        s.rows.resize((size_t)n_idx * k);
        return HBEC_OK;
    };
    for (size_t p = 0; p < pats.size(); ++p) {
        PlanPattern& pp = pats[p];
        if (!pp.uses) continue;
        *used = true;
        int n_present = 0, data_present = 0;
        for (int i = 0; i < n; ++i) {
            mask[i] = patterns[p * n + i] ? 1 : 0;
            n_present += mask[i];
            if (i < k) data_present += mask[i];
        }
        if (want_chk) {
            const int rc = fill(pp.chk, std::max(1, m), [&](int* surv, int* idx, int* n_idx, uint8_t* rows) {
                return hbec_check_rows(codec, mask.data(), surv, idx, n_idx, rows);
            });
            if (rc) return rc;
        }
        if (!want_out || n_present == n || (data_only && data_present == k)) continue;  // nothing to rebuild
        const int rc = fill(pp.out, n, [&](int* surv, int* idx, int* n_idx, uint8_t* rows) {
            return hbec_decode_rows(codec, mask.data(), data_only ? 1 : 0, surv, idx, n_idx, rows);
        });
        if (rc) return rc;
    }
    return HBEC_OK;
}

// A call's staging words: the records of its patterns in use (`record(pp)`
// appends one, or none), then one word per source entry (`word(i, pp)`).
// Returns where the words start.
template <class Record, class Word>
size_t stage_patterns(const hbec_plan* plan, std::vector<PlanPattern>& pats, const uint32_t* pattern_of,
                      std::vector<uint32_t>& stage, Record&& record, Word&& word) {
    for (PlanPattern& pp : pats)
        if (pp.uses) record(pp);
    const size_t rec_words = stage.size();
    stage.resize(rec_words + (size_t)plan->n_src);
    for (uint64_t i = 0; i < plan->n_src; ++i) stage[rec_words + i] = word(i, pats[pattern_of[i]]);
    return rec_words;
}

// The other route of the calls with a pattern per source entry (any k, m, S),
// one source entry at a time; hbec_reconstruct_plan_mixed, hbec_verify_plan_mixed
// and hbec_repair_plan_mixed share both.
// Rebuild: one single-pattern apply of the decode rows (out.idx not empty).
int reconstruct_other_entry(const hbec_plan* plan, uint32_t i, const ShardSet& out, hipStream_t stream) {
    const int k = plan->k;
    const hbec::MSrc& s = plan->src[i];
    auto at = [&](int sh) { return hbec_view{reinterpret_cast<void*>(shard_addr(plan, i, sh)), 0}; };
    std::vector<hbec_view> vin((size_t)k), vout(out.idx.size());
    for (int j = 0; j < k; ++j) vin[j] = at(out.surv[j]);
    for (size_t q = 0; q < out.idx.size(); ++q) vout[q] = at(out.idx[q]);
    return hbec::apply_views((int)out.idx.size(), k, out.rows.data(), vin.data(), vout.data(), 1, s.shard_len, stream);
}

// Check (chk.idx: the checked shards): exactly k present, bit 1; all present,
// the per-stripe Verify; degraded, the checked shards rebuilt from the survivors
// into scratch and compared with the stored ones.
int verify_other_entry(hbec_codec* codec, const hbec_plan* plan, uint32_t i, const ShardSet& chk, uint32_t* d_flags,
                       int cus, hipStream_t stream) {
    const int k = plan->k, m = plan->m;
    const hbec::MSrc& s = plan->src[i];
    if (chk.idx.empty()) {
        const hipError_t e = hbec::launch_vm_or(d_flags + i, 2u, stream);
        return e == hipSuccess ? HBEC_OK : hip_fail(e, "launch gf_vm_or");
    }
    if ((int)chk.idx.size() == m) return hbec::verify_plan_entry(codec, plan, i, d_flags, stream);
    auto at = [&](int sh) { return shard_addr(plan, i, sh); };
    void* scratch = nullptr;
    int rc = hbec::scratch_alloc(chk.idx.size() * (size_t)s.shard_len, stream, &scratch);
    if (rc) return rc;
    uint8_t* rebuilt = static_cast<uint8_t*>(scratch);
    std::vector<hbec_view> vin((size_t)k), vout(chk.idx.size());
    for (int j = 0; j < k; ++j) vin[j] = hbec_view{reinterpret_cast<void*>(at(chk.surv[j])), 0};
    for (size_t q = 0; q < chk.idx.size(); ++q) vout[q] = hbec_view{rebuilt + q * (size_t)s.shard_len, 0};
    rc = hbec::apply_views((int)chk.idx.size(), k, chk.rows.data(), vin.data(), vout.data(), 1, s.shard_len, stream);
    hipError_t e = hipSuccess;
    for (size_t q = 0; q < chk.idx.size() && !rc && e == hipSuccess; ++q)
        e = hbec::launch_vm_compare(rebuilt + q * (size_t)s.shard_len, reinterpret_cast<const void*>(at(chk.idx[q])),
                                    s.shard_len, d_flags + i, cus, stream);
    hbec::scratch_free(scratch, stream);
    if (rc) return rc;
    return e == hipSuccess ? HBEC_OK : hip_fail(e, "launch gf_vm_compare");
}

// ---- reconstruct with a pattern per stripe (hbec_reconstruct_plan_mixed) ----

int reconstruct_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                           const uint32_t* pattern_of, bool data_only, hipStream_t stream) {
    std::vector<PlanPattern> pats;
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    const int k = plan->k;
    bool used = false, work = false;
    rc = resolve_patterns(codec, patterns, true, data_only, false, pats, &used);
    if (rc) return rc;
    for (const PlanPattern& pp : pats) work = work || !pp.out.idx.empty();
    if (!work) return HBEC_OK;
    rc = mixed_plan_device(plan);
    if (rc) return rc;

    if (plan->n_mtiles > 0) {
        // one launch per chunk of the list, of the instance for the largest
        // output count in use: it codes every tile with something to rebuild
        int rmax = 0;
        std::vector<uint32_t> stage;
        const size_t rec_words = stage_patterns(
            plan, pats, pattern_of, stage,
            [&](PlanPattern& pp) {
                const ShardSet& o = pp.out;
                if (!o.idx.empty())
                    pp.rec = hbec::mp_pattern(stage, k, o.surv.data(), o.idx.data(), (int)o.idx.size(), o.rows.data());
            },
            [&](uint64_t i, const PlanPattern& pp) {
                const uint64_t S = plan->src[i].shard_len;
                const int r = (int)pp.out.idx.size();
                if (S == 0 || !hbec::pos32_shard(S) || r == 0) return 0u;  // mp_build's route
                rmax = std::max(rmax, r);
                return ((uint32_t)r << hbec::kMPatShift) | pp.rec;
            });
        int cus = 0;
        rc = current_cus(&cus);
        if (rc) return rc;
        rc = staged_launches(plan, stage, stream, [&](const uint32_t* d_pats) {
            return walk_chunks(kReconstruct, rmax > 0 ? plan->n_mtiles : 0, "launch gf_mixed_plan",
                               [&](uint64_t t0, uint32_t nt) {
                                   return hbec::launch_mixed_plan(k, rmax, plan->d_mrecs, plan->d_mtiles + t0, nt,
                                                                  d_pats + rec_words, d_pats, cus, stream,
                                                                  plan->shards);
                               });
        });
        if (rc) return rc;
    }
    // the other route: one single-pattern apply per stripe (any k, m, S)
    for (uint32_t i : plan->mp_other) {
        const ShardSet& out = pats[pattern_of[i]].out;
        if (out.idx.empty()) continue;
        count(g_calls[kReconstruct].second);
        rc = reconstruct_other_entry(plan, i, out, stream);
        if (rc) return rc;
    }
    return HBEC_OK;
}

// ---- Verify with a present mask per stripe (hbec_verify_plan_mixed) ----

// The staging words of the calls that check (Verify, locate): the records of
// the masks with something to check and one word per source entry.  *rmax: the
// largest count of checked shards among the kernel route's entries, 1 at least
// (exactly-k entries alone: any instance sets their bit).
size_t stage_checked(const hbec_plan* plan, std::vector<PlanPattern>& pats, const uint32_t* pattern_of,
                     std::vector<uint32_t>& stage, int* rmax) {
    const int k = plan->k, m = plan->m;
    *rmax = 1;
    return stage_patterns(
        plan, pats, pattern_of, stage,
        [&](PlanPattern& pp) {
            const ShardSet& c = pp.chk;
            if (!c.idx.empty())
                pp.rec = hbec::vm_pattern(stage, k, c.surv.data(), c.idx.data(), (int)c.idx.size(), c.rows.data());
        },
        [&](uint64_t i, const PlanPattern& pp) {
            if (hbec::vm_route(k, m, plan->src[i].shard_len) != hbec::kVmKernel) return 0u;
            *rmax = std::max(*rmax, (int)pp.chk.idx.size());
            return hbec::vm_word((int)pp.chk.idx.size(), pp.rec);
        });
}

int verify_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                      const uint32_t* pattern_of, uint32_t* d_flags, hipStream_t stream) {
    std::vector<PlanPattern> pats;
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    if (!d_flags && plan->n_src) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    bool used = false;
    rc = resolve_patterns(codec, patterns, false, false, true, pats, &used);
    if (rc) return rc;
    if (!used) return HBEC_OK;  // zero-length entries only
    rc = mixed_plan_device(plan);
    if (rc) return rc;
    int cus = 0;
    rc = current_cus(&cus);
    if (rc) return rc;

    if (plan->n_mtiles > 0) {
        // one launch per chunk of the list, of the instance for the largest count
        // of checked shards in use
        int rmax = 1;
        std::vector<uint32_t> stage;
        const size_t rec_words = stage_checked(plan, pats, pattern_of, stage, &rmax);
        rc = staged_launches(plan, stage, stream, [&](const uint32_t* d_pats) {
            return walk_chunks(kVerify, plan->n_mtiles, "launch gf_verify_mixed_plan", [&](uint64_t t0, uint32_t nt) {
                return hbec::launch_verify_mixed_plan(plan->k, rmax, plan->d_mrecs, plan->d_mtiles + t0, nt,
                                                      d_pats + rec_words, d_pats, d_flags, cus, stream, plan->shards);
            });
        });
        if (rc) return rc;
    }
    // the other route, one stripe at a time (any k, m, S)
    for (uint32_t i : plan->mp_other) {
        count(g_calls[kVerify].second);
        rc = verify_other_entry(codec, plan, i, pats[pattern_of[i]].chk, d_flags, cus, stream);
        if (rc) return rc;
    }
    return HBEC_OK;
}

// ---- rebuild the missing shards and check the surplus ones (hbec_repair_plan_mixed) ----

int repair_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                      const uint32_t* pattern_of, bool data_only, uint32_t* d_flags, hipStream_t stream) {
    std::vector<PlanPattern> pats;
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    if (!d_flags && plan->n_src) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = plan->k, m = plan->m;
    bool used = false;
    rc = resolve_patterns(codec, patterns, true, data_only, true, pats, &used);
    if (rc) return rc;
    if (!used) return HBEC_OK;  // zero-length entries only
    rc = mixed_plan_device(plan);
    if (rc) return rc;
    int cus = 0;
    rc = current_cus(&cus);
    if (rc) return rc;

    if (plan->n_mtiles > 0) {
        // the records of the masks with a shard to rebuild or to check and one
        // word per source entry; one launch per chunk of the list, of the
        // instance for the largest count of rows (outputs and checked shards
        // together) in use
        int rmax = 1;  // exactly-k entries with nothing to rebuild alone: any instance sets their bit
        std::vector<uint32_t> stage;
        const size_t rec_words = stage_patterns(
            plan, pats, pattern_of, stage,
            [&](PlanPattern& pp) {
                const ShardSet &o = pp.out, &c = pp.chk;
                if (o.idx.size() + c.idx.size() > 0)
                    pp.rec = hbec::rp_pattern(stage, k, c.surv.data(), o.idx.data(), (int)o.idx.size(), o.rows.data(),
                                              c.idx.data(), (int)c.idx.size(), c.rows.data());
            },
            [&](uint64_t i, const PlanPattern& pp) {
                if (hbec::rp_route(k, m, plan->src[i].shard_len) != hbec::kVmKernel) return 0u;
                rmax = std::max(rmax, (int)(pp.out.idx.size() + pp.chk.idx.size()));
                return hbec::rp_word((int)pp.out.idx.size(), (int)pp.chk.idx.size(), pp.rec);
            });
        rc = staged_launches(plan, stage, stream, [&](const uint32_t* d_pats) {
            return walk_chunks(kRepair, plan->n_mtiles, "launch gf_repair_mixed_plan", [&](uint64_t t0, uint32_t nt) {
                return hbec::launch_repair_mixed_plan(k, rmax, plan->d_mrecs, plan->d_mtiles + t0, nt,
                                                      d_pats + rec_words, d_pats, d_flags, cus, stream, plan->shards);
            });
        });
        if (rc) return rc;
    }
    // the other route, one stripe at a time (any k, m, S): what verify_plan_mixed
    // does with the entry, then what reconstruct_plan_mixed does with it
    for (uint32_t i : plan->mp_other) {
        const PlanPattern& pp = pats[pattern_of[i]];
        count(g_calls[kRepair].second);
        rc = verify_other_entry(codec, plan, i, pp.chk, d_flags, cus, stream);
        if (rc) return rc;
        if (pp.out.idx.empty()) continue;
        rc = reconstruct_other_entry(plan, i, pp.out, stream);
        if (rc) return rc;
    }
    return HBEC_OK;
}

// ---- the corrupt shard of every inconsistent stripe (hbec_locate_plan_mixed) ----

static_assert(HBEC_LOC_BAD == hbec::kLocBad && HBEC_LOC_SKIPPED == hbec::kLocSkipped &&
                  HBEC_LOC_NOTHING == hbec::kLocNothing && HBEC_LOC_CLEAN == hbec::kLocClean &&
                  HBEC_LOC_AMBIGUOUS == hbec::kLocAmbiguous && HBEC_LOC_MULTIPLE == hbec::kLocMultiple &&
                  HBEC_LOC_UNCHECKED == hbec::kLocUnchecked,
              "include/hbec.h and locate.h disagree");

int locate_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                      const uint32_t* pattern_of, const uint32_t* d_flags, uint32_t* d_where, hipStream_t stream) {
    std::vector<PlanPattern> pats;
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    if (!d_where && plan->n_src) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    if (d_where && d_where == d_flags) return fail(HBEC_ERR_INVALID_ARG, "d_where aliases d_flags");
    bool used = false;
    rc = resolve_patterns(codec, patterns, false, false, true, pats, &used);
    if (rc) return rc;
    if (!used) return HBEC_OK;  // zero-length entries only
    rc = mixed_plan_device(plan);
    if (rc) return rc;

    if (plan->n_mtiles > 0) {
        // Verify's records and words (loc_route is vm_route, loc_pattern vm_pattern)
        int rmax = 1;
        std::vector<uint32_t> stage;
        const size_t rec_words = stage_checked(plan, pats, pattern_of, stage, &rmax);
        int cus = 0;
        rc = current_cus(&cus);
        if (rc) return rc;
        rc = staged_launches(plan, stage, stream, [&](const uint32_t* d_pats) {
            return walk_chunks(kLocate, plan->n_mtiles, "launch gf_locate_mixed_plan", [&](uint64_t t0, uint32_t nt) {
                return hbec::launch_locate_mixed_plan(plan->k, rmax, plan->d_mrecs, plan->d_mtiles + t0, nt,
                                                      d_pats + rec_words, d_pats, d_flags, d_where, cus, stream,
                                                      plan->shards);
            });
        });
        if (rc) return rc;
    }
    // the other route is not examined: said in the entry's word, and counted
    for (uint32_t i : plan->mp_other) {
        count(g_calls[kLocate].second);
        const hipError_t e = hbec::launch_vm_or(d_where + i, hbec::kLocSkipped, stream);
        if (e != hipSuccess) return hip_fail(e, "launch gf_vm_or");
    }
    return HBEC_OK;
}

// ---- rebuild the shard locate named (hbec_heal_plan_mixed) ----

static_assert(HBEC_HEAL_DONE == hbec::kHealDone && HBEC_HEAL_UNNAMED == hbec::kHealUnnamed,
              "include/hbec.h and heal.h disagree");

// Heal shares the argument checks, the skeleton and the chunk walk.  Its
// patterns are not resolved by resolve_patterns: every mask stands for the
// masks with one more shard left out, built by heal_build and kept on the plan.
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
        rc = staged_launches(plan, index, stream, [&](const uint32_t* d_index) {
            if (plan->heal_on_device != hs) {
                // other masks than the last call's: their records and tables replace those
                plan->heal_on_device.reset();
                const Queued put = put_words(&plan->d_heal, &plan->heal_dev_words, h.stage, stream,
                                             "plan heal records", "plan heal records");
                if (put.e != hipSuccess) return put;
                plan->heal_on_device = hs;
            }
            const uint32_t* d_pats = plan->d_heal;
            // one launch per chunk of the list; every mask with one shard left out has m rows
            return walk_chunks(kHeal, plan->n_mtiles, "launch gf_heal_mixed_plan", [&](uint64_t t0, uint32_t nt) {
                return hbec::launch_heal_mixed_plan(k, std::max(1, m), plan->d_mrecs, plan->d_mtiles + t0, nt, d_index,
                                                    d_pats + h.words_at, d_pats + h.present_at, d_pats, d_where,
                                                    d_flags, cus, stream, plan->shards);
            });
        });
        if (rc) return rc;
    }
    // the other route is never healed (locate gave it kLocSkipped): counted
    count(g_calls[kHeal].second, plan->mp_other.size());
    return HBEC_OK;
}

// ---- the ShardHash of a plan's shards against the stored ones (hbec_hash_plan_mixed) ----

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

// The argument checks both hash calls open with: what the given pointers say
// about each other holds for any plan, an empty one too.
int check_hash_args(hbec_codec* codec, const hbec_plan* plan, uint32_t n_select, const uint32_t* d_filter,
                    const uint8_t* d_expected, const uint8_t* d_digests, const uint32_t* d_bad,
                    const uint32_t* d_where) {
    if (!codec || !plan) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
    if (n_select > 65536) return fail(HBEC_ERR_INVALID_ARG, "more than 65536 selection rows");
    if (d_where && !d_bad) return fail(HBEC_ERR_INVALID_ARG, "d_where needs d_bad");
    if (d_expected && !d_bad) return fail(HBEC_ERR_INVALID_ARG, "d_expected needs d_bad");
    if (d_expected && n > 32) return fail(HBEC_ERR_INVALID_ARG, "d_expected needs k + m <= 32 (one bit per shard)");
    if ((d_bad && (d_bad == d_where || d_bad == d_filter)) || (d_where && d_where == d_filter))
        return fail(HBEC_ERR_INVALID_ARG, "d_bad, d_where and d_filter must be distinct");
    if ((reinterpret_cast<uintptr_t>(d_digests) | reinterpret_cast<uintptr_t>(d_expected)) & 3u)
        return fail(HBEC_ERR_INVALID_ARG, "digest buffer not 4-byte aligned");
    return HBEC_OK;
}

// The hash calls make one launch, and one more for d_where, where the pattern
// calls walk chunks: they share the skeleton and count for themselves.
int hash_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* select, uint32_t n_select,
                    const uint32_t* select_of, const uint32_t* d_filter, uint32_t filter_bits,
                    const uint8_t* d_expected, uint8_t* d_digests, uint32_t* d_bad, uint32_t* d_where,
                    hipStream_t stream) {
    int rc = check_hash_args(codec, plan, n_select, d_filter, d_expected, d_digests, d_bad, d_where);
    if (rc) return rc;
    const int k = plan->k, n = k + plan->m;
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
    rc = hash_plan_device(plan);
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
    return staged_launches(plan, stage, stream, [&](const uint32_t* d_stage) {
        count(g_calls[kHash].launches);
        count(g_calls[kHash].second, chains.size());
        hipError_t e = hbec::launch_md5_plan(plan->d_hrecs, reinterpret_cast<const hbec::HChain*>(d_stage),
                                             chains.size(), k, n, d_filter, filter_bits, d_expected, d_digests,
                                             d_expected ? d_bad : nullptr, stream, plan->shards);
        if (e == hipSuccess && d_where) {
            count(g_calls[kHash].launches);
            e = hbec::launch_hash_where(plan->d_hrecs, (uint32_t)n_src, d_stage + chain_words, d_filter, filter_bits,
                                        d_bad, d_where, stream);
        }
        return Queued{e, "launch md5_plan"};
    });
}

// ---- the ShardHash of multi-stripe shard files on a plan (hbec_hash_plan_files) ----

int hash_plan_files(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                    const uint8_t* select, uint32_t n_select, const uint32_t* select_of, const uint32_t* d_filter,
                    uint32_t filter_bits, const uint8_t* d_expected, uint8_t* d_digests, uint32_t* d_bad,
                    uint32_t* d_where, hipStream_t stream) {
    int rc = check_hash_args(codec, plan, n_select, d_filter, d_expected, d_digests, d_bad, d_where);
    if (rc) return rc;
    const int k = plan->k, n = k + plan->m;
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
    rc = hash_plan_device(plan);
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
    return staged_launches(plan, stage, stream, [&](const uint32_t* d_stage) {
        count(g_calls[kHashFiles].launches);
        count(g_calls[kHashFiles].second, chains.size());
        count(g_hashfiles_segments, segments);
        hipError_t e = hbec::launch_md5_files(plan->d_hrecs, d_stage + objects_at,
                                              reinterpret_cast<const hbec::FChain*>(d_stage), chains.size(), k, n,
                                              d_filter, filter_bits, d_expected, d_digests,
                                              d_expected ? d_bad : nullptr, stream, plan->shards);
        if (e == hipSuccess && d_where) {
            count(g_calls[kHashFiles].launches);
            e = hbec::launch_hash_files_where(plan->d_hrecs, (uint32_t)n_src, d_stage + of_at, d_stage + sel_at,
                                              d_filter, filter_bits, d_bad, d_where, stream);
        }
        return Queued{e, "launch md5_files"};
    });
}

// ---- the object bytes of every entry from its shards (hbec_glue_plan_mixed) ----

// The other route (any k, m, S), one source entry: every present data shard with
// a byte wanted is one device-to-device copy, clipped; the missing ones with a
// byte wanted are rebuilt by one single-pattern apply, straight into the
// destination where the shard is written whole, through scratch and a clipped
// copy where it is cut (at most one shard of an entry is).  Every copy and every
// apply counts as a per-stripe call.
int glue_other_entry(const hbec_plan* plan, uint32_t i, const uint8_t* mask, const ShardSet& out, uint64_t dst,
                     uint64_t len, hipStream_t stream) {
    const int k = plan->k;
    const uint64_t S = plan->src[i].shard_len;
    auto copy = [&](uint64_t to, const void* from, uint64_t bytes) -> int {
        count(g_calls[kGlue].second);
        const hipError_t e = hipMemcpyAsync(reinterpret_cast<void*>(to), from, bytes, hipMemcpyDeviceToDevice, stream);
        return e == hipSuccess ? HBEC_OK : hip_fail(e, "hipMemcpyAsync (glue)");
    };
    for (int j = 0; j < k; ++j) {
        const uint64_t V = hbec::glue_valid(len, (uint64_t)j, S);
        if (!V || !mask[j]) continue;
        const int rc = copy(dst + (uint64_t)j * S, reinterpret_cast<const void*>(shard_addr(plan, i, j)), V);
        if (rc) return rc;
    }
    std::vector<size_t> sel;  // the rebuilt shards with a byte wanted, as positions in out.idx
    size_t cut = out.idx.size();
    for (size_t q = 0; q < out.idx.size(); ++q) {
        const uint64_t V = hbec::glue_valid(len, (uint64_t)out.idx[q], S);
        if (!V) continue;
        if (V < S) cut = q;
        sel.push_back(q);
    }
    if (sel.empty()) return HBEC_OK;
    void* scratch = nullptr;
    if (cut < out.idx.size()) {
        const int rc = hbec::scratch_alloc((size_t)S, stream, &scratch);
        if (rc) return rc;
    }
    std::vector<hbec_view> vin((size_t)k), vout(sel.size());
    std::vector<uint8_t> rows(sel.size() * (size_t)k);
    for (int j = 0; j < k; ++j) vin[j] = hbec_view{reinterpret_cast<void*>(shard_addr(plan, i, out.surv[j])), 0};
    for (size_t s = 0; s < sel.size(); ++s) {
        const size_t q = sel[s];
        vout[s] = hbec_view{q == cut ? scratch : reinterpret_cast<void*>(dst + (uint64_t)out.idx[q] * S), 0};
        std::memcpy(rows.data() + s * (size_t)k, out.rows.data() + q * (size_t)k, (size_t)k);
    }
    count(g_calls[kGlue].second);
    int rc = hbec::apply_views((int)sel.size(), k, rows.data(), vin.data(), vout.data(), 1, S, stream);
    if (!rc && scratch)
        rc = copy(dst + (uint64_t)out.idx[cut] * S, scratch, hbec::glue_valid(len, (uint64_t)out.idx[cut], S));
    if (scratch) hbec::scratch_free(scratch, stream);
    return rc;
}

int glue_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                    const uint32_t* pattern_of, void* const* dsts, const uint64_t* dst_lens, hipStream_t stream) {
    std::vector<PlanPattern> pats;
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    if (!dsts || !dst_lens) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = plan->k, n = k + plan->m;
    const uint64_t n_src = plan->n_src;
    bool any = false;
    for (uint64_t i = 0; i < n_src; ++i) {  // zero-length entries too
        const uint64_t S = plan->src[i].shard_len, len = dst_lens[i];
        const uint64_t dst = reinterpret_cast<uintptr_t>(dsts[i]);
        if ((unsigned __int128)len > (unsigned __int128)S * (uint64_t)k)
            return fail(HBEC_ERR_INVALID_ARG, "dst_lens exceeds k * shard_len (entry " + std::to_string(i) + ")");
        if (!len) continue;
        if (!dst) return fail(HBEC_ERR_INVALID_ARG, "null destination with dst_lens > 0 (entry " + std::to_string(i) + ")");
        for (int sh = 0; sh < n; ++sh)
            if (hbec::glue_overlaps(dst, len, shard_addr(plan, (uint32_t)i, sh), S))
                return fail(HBEC_ERR_INVALID_ARG, "destination overlaps shard " + std::to_string(sh) +
                                                      " of its own entry (entry " + std::to_string(i) + ")");
        any = true;
    }
    if (!any) return HBEC_OK;  // nothing asked for
    bool used = false;
    rc = resolve_patterns(codec, patterns, true, true, false, pats, &used);
    if (rc) return rc;
    rc = mixed_plan_device(plan);
    if (rc) return rc;

    if (plan->n_mtiles > 0) {
        // Every pattern in use has a record, the masks with no data shard missing
        // too (r = 0, the header alone: survivors 0..k-1): the tile gathers through
        // its survivor list.  Then one word per source entry and its destination;
        // one launch per chunk of the list, of the instance for the largest count
        // of missing data shards in use.
        int rmax = -1;
        std::vector<int> data((size_t)k);
        for (int j = 0; j < k; ++j) data[j] = j;
        std::vector<uint32_t> stage;
        const size_t rec_words = stage_patterns(
            plan, pats, pattern_of, stage,
            [&](PlanPattern& pp) {
                const ShardSet& o = pp.out;
                pp.rec = o.idx.empty()
                             ? hbec::mp_pattern(stage, k, data.data(), nullptr, 0, nullptr)
                             : hbec::mp_pattern(stage, k, o.surv.data(), o.idx.data(), (int)o.idx.size(), o.rows.data());
            },
            [&](uint64_t i, const PlanPattern& pp) {
                const uint64_t S = plan->src[i].shard_len;
                if (S == 0 || !hbec::pos32_shard(S) || dst_lens[i] == 0) return hbec::kGlueSkip;  // mp_build's route
                const int r = (int)pp.out.idx.size();
                rmax = std::max(rmax, r);
                return ((uint32_t)r << hbec::kMPatShift) | pp.rec;
            });
        const size_t dst_at = stage.size();
        stage.resize(dst_at + 4 * (size_t)n_src);
        for (uint64_t i = 0; i < n_src; ++i) {
            const uint64_t dst = reinterpret_cast<uintptr_t>(dsts[i]), len = dst_lens[i];
            uint32_t* d = stage.data() + dst_at + 4 * i;
            d[0] = (uint32_t)dst, d[1] = (uint32_t)(dst >> 32), d[2] = (uint32_t)len, d[3] = (uint32_t)(len >> 32);
        }
        if (rmax >= 0) {
            int cus = 0;
            rc = current_cus(&cus);
            if (rc) return rc;
            rc = staged_launches(plan, stage, stream, [&](const uint32_t* d_pats) {
                return walk_chunks(kGlue, plan->n_mtiles, "launch gf_glue_plan", [&](uint64_t t0, uint32_t nt) {
                    return (hipError_t)hbec::launch_glue_plan(k, rmax, plan->d_mrecs, plan->d_mtiles + t0, nt,
                                                              d_pats + rec_words, d_pats + dst_at, d_pats, cus, stream,
                                                              plan->shards);
                });
            });
            if (rc) return rc;
        }
    }
    // the other route, one entry at a time (any k, m, S)
    for (uint32_t i : plan->mp_other) {
        if (!dst_lens[i]) continue;
        rc = glue_other_entry(plan, i, patterns + (size_t)pattern_of[i] * n, pats[pattern_of[i]].out,
                              reinterpret_cast<uintptr_t>(dsts[i]), dst_lens[i], stream);
        if (rc) return rc;
    }
    return HBEC_OK;
}

// ---- whole objects of a files plan from their shard files (hbec_glue_plan_files) ----

// What hbec_glue_plan_files checks of the object table, the chunk size and the
// content lengths of a plan with entries, and the cut of every object into its
// entries: each(g, i, off, len) for entry i of object g, which holds the
// object's bytes [off, off + len).  hbec_etag_plan_files takes the same checks.
template <class Each>
int files_cut_entries(const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                      const uint64_t* content_lengths, uint64_t chunk_size, Each&& each) {
    const int k = plan->k;
    if (const char* why = hbec::files_check_objects(object_start, n_objects, plan->n_src))
        return fail(HBEC_ERR_INVALID_ARG, why);
    if (chunk_size == 0 || chunk_size > (uint64_t)INT64_MAX) return fail(HBEC_ERR_INVALID_ARG, "chunk_size out of range");
    for (uint32_t g = 0; g < n_objects; ++g) {
        const uint64_t L = content_lengths[g], cnt = object_start[g + 1] - object_start[g];
        if (L > (uint64_t)INT64_MAX || hbec::ec_stripe_count((int64_t)L, k, (int64_t)chunk_size) != cnt)
            return fail(HBEC_ERR_INVALID_ARG, "content length does not give the entry count (object " +
                                                  std::to_string(g) + ")");
        for (uint64_t t = 0; t < cnt; ++t) {
            const uint64_t i = object_start[g] + t;
            if (plan->src[i].shard_len != hbec::ec_stripe_shard_length((int64_t)L, k, (int64_t)chunk_size, t))
                return fail(HBEC_ERR_INVALID_ARG, "shard length mismatch (object " + std::to_string(g) +
                                                      ", stripe " + std::to_string(t) + ")");
            uint64_t off = 0, len = 0;
            hbec::glue_files_cut(L, (uint64_t)k, chunk_size, t, &off, &len);
            each(g, i, off, len);
        }
    }
    return HBEC_OK;
}

int glue_plan_files(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                    const uint64_t* content_lengths, uint64_t chunk_size, const uint8_t* patterns,
                    uint32_t n_patterns, const uint32_t* pattern_of, void* const* object_dsts, hipStream_t stream) {
    if (!codec || !plan || !content_lengths || !object_dsts) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
    if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
    const uint64_t n_src = plan->n_src;
    std::vector<void*> dsts((size_t)std::max<uint64_t>(1, n_src), nullptr);
    std::vector<uint64_t> lens((size_t)std::max<uint64_t>(1, n_src), 0u);
    if (n_src) {
        const int rc = files_cut_entries(plan, object_start, n_objects, content_lengths, chunk_size,
                                         [&](uint32_t g, uint64_t i, uint64_t off, uint64_t len) {
                                             lens[i] = len;
                                             dsts[i] = object_dsts[g] ? static_cast<uint8_t*>(object_dsts[g]) + off
                                                                      : nullptr;
                                         });
        if (rc) return rc;
    }
    return glue_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, dsts.data(), lens.data(), stream);
}

// ---- any byte range of every entry from its shards (hbec_glue_plan_range) ----

// The other route (any k, m, S), one source entry: every present data shard with
// a byte wanted is one device-to-device copy of its window.  The missing ones
// with a byte wanted are rebuilt by one single-pattern apply over the shard
// positions [A, B) their windows span (GF apply is bytewise): straight into the
// destination where a shard's window is all of [A, B), through scratch and a
// clipped copy where it is not.  Every copy and every apply counts as a
// per-stripe call.
int glue_range_other_entry(const hbec_plan* plan, uint32_t i, const uint8_t* mask, const ShardSet& out, uint64_t dst,
                           uint64_t s, uint64_t len, hipStream_t stream) {
    const int k = plan->k;
    const uint64_t S = plan->src[i].shard_len, e = s + len;
    auto copy = [&](uint64_t to, uint64_t from, uint64_t bytes) -> int {
        count(g_calls[kGlueRange].second);
        const hipError_t err = hipMemcpyAsync(reinterpret_cast<void*>(to), reinterpret_cast<const void*>(from), bytes,
                                              hipMemcpyDeviceToDevice, stream);
        return err == hipSuccess ? HBEC_OK : hip_fail(err, "hipMemcpyAsync (glue range)");
    };
    for (int j = 0; j < k; ++j) {
        const hbec::GrWin w = hbec::gr_window(S, s, e, (uint64_t)j);
        if (hbec::gr_empty(w) || !mask[j]) continue;
        const int rc = copy(hbec::gr_base(dst, S, s, (uint64_t)j) + w.lo, shard_addr(plan, i, j) + w.lo, w.hi - w.lo);
        if (rc) return rc;
    }
    std::vector<size_t> sel;  // the rebuilt shards with a byte wanted, as positions in out.idx
    uint64_t A = S, B = 0;
    for (size_t q = 0; q < out.idx.size(); ++q) {
        const hbec::GrWin w = hbec::gr_window(S, s, e, (uint64_t)out.idx[q]);
        if (hbec::gr_empty(w)) continue;
        A = std::min(A, w.lo), B = std::max(B, w.hi);
        sel.push_back(q);
    }
    if (sel.empty()) return HBEC_OK;
    auto whole = [&](size_t q) {
        const hbec::GrWin w = hbec::gr_window(S, s, e, (uint64_t)out.idx[q]);
        return w.lo == A && w.hi == B;
    };
    size_t n_cut = 0;
    for (size_t q : sel) n_cut += whole(q) ? 0 : 1;
    void* scratch = nullptr;
    if (n_cut) {
        const int rc = hbec::scratch_alloc((size_t)(n_cut * (B - A)), stream, &scratch);
        if (rc) return rc;
    }
    std::vector<hbec_view> vin((size_t)k), vout(sel.size());
    std::vector<uint8_t> rows(sel.size() * (size_t)k);
    for (int j = 0; j < k; ++j) vin[j] = hbec_view{reinterpret_cast<void*>(shard_addr(plan, i, out.surv[j]) + A), 0};
    size_t cut = 0;
    for (size_t t = 0; t < sel.size(); ++t) {
        const size_t q = sel[t];
        const uint64_t at = whole(q) ? hbec::gr_base(dst, S, s, (uint64_t)out.idx[q]) + A
                                     : reinterpret_cast<uintptr_t>(scratch) + (cut++) * (B - A);
        vout[t] = hbec_view{reinterpret_cast<void*>(at), 0};
        std::memcpy(rows.data() + t * (size_t)k, out.rows.data() + q * (size_t)k, (size_t)k);
    }
    count(g_calls[kGlueRange].second);
    int rc = hbec::apply_views((int)sel.size(), k, rows.data(), vin.data(), vout.data(), 1, B - A, stream);
    for (size_t t = 0; t < sel.size() && !rc; ++t) {
        if (whole(sel[t])) continue;
        const hbec::GrWin w = hbec::gr_window(S, s, e, (uint64_t)out.idx[sel[t]]);
        rc = copy(hbec::gr_base(dst, S, s, (uint64_t)out.idx[sel[t]]) + w.lo,
                  reinterpret_cast<uintptr_t>(vout[t].base) + (w.lo - A), w.hi - w.lo);
    }
    if (scratch) hbec::scratch_free(scratch, stream);
    return rc;
}

int glue_plan_range(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                    const uint32_t* pattern_of, void* const* dsts, const uint64_t* starts, const uint64_t* lens,
                    hipStream_t stream) {
    std::vector<PlanPattern> pats;
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    if (!dsts || !starts || !lens) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = plan->k, n = k + plan->m;
    const uint64_t n_src = plan->n_src;
    bool any = false;
    for (uint64_t i = 0; i < n_src; ++i) {  // zero-length entries too
        const uint64_t S = plan->src[i].shard_len, len = lens[i];
        if (!len) continue;  // whatever starts[i] and dsts[i] are
        const uint64_t dst = reinterpret_cast<uintptr_t>(dsts[i]);
        if (!hbec::gr_range_ok(starts[i], len, (uint64_t)k, S))
            return fail(HBEC_ERR_INVALID_ARG, "starts + lens exceeds k * shard_len (entry " + std::to_string(i) + ")");
        if (!dst) return fail(HBEC_ERR_INVALID_ARG, "null destination with lens > 0 (entry " + std::to_string(i) + ")");
        for (int sh = 0; sh < n; ++sh)
            if (hbec::glue_overlaps(dst, len, shard_addr(plan, (uint32_t)i, sh), S))
                return fail(HBEC_ERR_INVALID_ARG, "destination overlaps shard " + std::to_string(sh) +
                                                      " of its own entry (entry " + std::to_string(i) + ")");
        any = true;
    }
    if (!any) return HBEC_OK;  // nothing asked for
    bool used = false;
    rc = resolve_patterns(codec, patterns, true, true, false, pats, &used);
    if (rc) return rc;
    rc = mixed_plan_device(plan);
    if (rc) return rc;

    if (plan->n_mtiles > 0) {
        // glue_plan_mixed's staging, with {address, start, length} per source entry
        int rmax = -1;
        std::vector<int> data((size_t)k);
        for (int j = 0; j < k; ++j) data[j] = j;
        std::vector<uint32_t> stage;
        const size_t rec_words = stage_patterns(
            plan, pats, pattern_of, stage,
            [&](PlanPattern& pp) {
                const ShardSet& o = pp.out;
                pp.rec = o.idx.empty()
                             ? hbec::mp_pattern(stage, k, data.data(), nullptr, 0, nullptr)
                             : hbec::mp_pattern(stage, k, o.surv.data(), o.idx.data(), (int)o.idx.size(), o.rows.data());
            },
            [&](uint64_t i, const PlanPattern& pp) {
                const uint64_t S = plan->src[i].shard_len;
                if (S == 0 || !hbec::pos32_shard(S) || lens[i] == 0) return hbec::kGlueSkip;  // mp_build's route
                const int r = (int)pp.out.idx.size();
                rmax = std::max(rmax, r);
                return ((uint32_t)r << hbec::kMPatShift) | pp.rec;
            });
        const size_t range_at = stage.size();
        stage.resize(range_at + 6 * (size_t)n_src);
        for (uint64_t i = 0; i < n_src; ++i) {
            const uint64_t v[3] = {reinterpret_cast<uintptr_t>(dsts[i]), starts[i], lens[i]};
            uint32_t* d = stage.data() + range_at + 6 * i;
            for (int q = 0; q < 3; ++q) d[2 * q] = (uint32_t)v[q], d[2 * q + 1] = (uint32_t)(v[q] >> 32);
        }
        if (rmax >= 0) {
            int cus = 0;
            rc = current_cus(&cus);
            if (rc) return rc;
            rc = staged_launches(plan, stage, stream, [&](const uint32_t* d_pats) {
                return walk_chunks(kGlueRange, plan->n_mtiles, "launch gf_range_plan", [&](uint64_t t0, uint32_t nt) {
                    return (hipError_t)hbec::launch_glue_range(k, rmax, plan->d_mrecs, plan->d_mtiles + t0, nt,
                                                               d_pats + rec_words, d_pats + range_at, d_pats, cus,
                                                               stream, plan->shards);
                });
            });
            if (rc) return rc;
        }
    }
    // the other route, one entry at a time (any k, m, S)
    for (uint32_t i : plan->mp_other) {
        if (!lens[i]) continue;
        rc = glue_range_other_entry(plan, i, patterns + (size_t)pattern_of[i] * n, pats[pattern_of[i]].out,
                                    reinterpret_cast<uintptr_t>(dsts[i]), starts[i], lens[i], stream);
        if (rc) return rc;
    }
    return HBEC_OK;
}

// ---- a byte range of whole objects of a files plan (hbec_glue_plan_files_range) ----

int glue_plan_files_range(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                          const uint64_t* content_lengths, uint64_t chunk_size, const uint8_t* patterns,
                          uint32_t n_patterns, const uint32_t* pattern_of, void* const* object_dsts,
                          const uint64_t* range_starts, const uint64_t* range_ends, hipStream_t stream) {
    if (!codec || !plan || !content_lengths || !object_dsts || !range_starts || !range_ends)
        return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
    if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
    const uint64_t n_src = plan->n_src;
    std::vector<void*> dsts((size_t)std::max<uint64_t>(1, n_src), nullptr);
    std::vector<uint64_t> starts((size_t)std::max<uint64_t>(1, n_src), 0u), lens(starts);
    if (n_src) {
        if (const char* why = hbec::files_check_objects(object_start, n_objects, n_src))
            return fail(HBEC_ERR_INVALID_ARG, why);
        if (chunk_size == 0 || chunk_size > (uint64_t)INT64_MAX) return fail(HBEC_ERR_INVALID_ARG, "chunk_size out of range");
        for (uint32_t g = 0; g < n_objects; ++g) {
            const uint64_t L = content_lengths[g], cnt = object_start[g + 1] - object_start[g];
            if (L > (uint64_t)INT64_MAX || hbec::ec_stripe_count((int64_t)L, k, (int64_t)chunk_size) != cnt)
                return fail(HBEC_ERR_INVALID_ARG, "content length does not give the entry count (object " +
                                                      std::to_string(g) + ")");
            for (uint64_t t = 0; t < cnt; ++t)
                if (plan->src[object_start[g] + t].shard_len !=
                    hbec::ec_stripe_shard_length((int64_t)L, k, (int64_t)chunk_size, t))
                    return fail(HBEC_ERR_INVALID_ARG, "shard length mismatch (object " + std::to_string(g) +
                                                          ", stripe " + std::to_string(t) + ")");
            if (range_starts[g] > range_ends[g] || range_ends[g] > L)
                return fail(HBEC_ERR_INVALID_ARG, "range is not inside the object (object " + std::to_string(g) + ")");
            for (uint64_t t = 0; t < cnt; ++t) {
                const uint64_t i = object_start[g] + t;
                uint64_t off = 0, len = 0, dst_off = 0;
                hbec::glue_files_cut(L, (uint64_t)k, chunk_size, t, &off, &len);
                hbec::gr_files_cut(off, len, range_starts[g], range_ends[g], &starts[i], &lens[i], &dst_off);
                dsts[i] = object_dsts[g] ? static_cast<uint8_t*>(object_dsts[g]) + dst_off : nullptr;
            }
        }
    }
    return glue_plan_range(codec, plan, patterns, n_patterns, pattern_of, dsts.data(), starts.data(), lens.data(),
                           stream);
}

// ---- the ETag of every object from its shards (hbec_etag_plan_mixed, hbec_etag_plan_files) ----

// Both ETag calls after the checks of their own.  lens: the bytes of D hashed,
// per source entry; object_start: the chains' entries (nullptr: every entry is
// an object of its own).  The call decodes first, then hashes: the span of
// every entry with a missing data shard below its length (etag.h) goes through
// hbec_glue_plan_range into one scratch allocation, on the same stream, and the
// chain kernel reads it there.  The span is decoded whether or not the entry
// passes the device-side filter: the host cannot know.
int etag_plan(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
              const uint32_t* pattern_of, const uint64_t* lens, const uint32_t* object_start, uint32_t n_objects,
              const uint32_t* d_filter, uint32_t filter_bits, const uint8_t* d_expected, uint8_t* d_digests,
              uint32_t* d_bad, hipStream_t stream) {
    std::vector<PlanPattern> pats;
    int rc = check_plan_patterns(codec, plan, patterns, n_patterns, pattern_of, pats);
    if (rc) return rc;
    if (!lens) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    if (d_expected && !d_bad) return fail(HBEC_ERR_INVALID_ARG, "d_expected needs d_bad");
    if (d_bad && d_bad == d_filter) return fail(HBEC_ERR_INVALID_ARG, "d_bad and d_filter must be distinct");
    if ((reinterpret_cast<uintptr_t>(d_digests) | reinterpret_cast<uintptr_t>(d_expected)) & 3u)
        return fail(HBEC_ERR_INVALID_ARG, "digest buffer not 4-byte aligned");
    const int k = plan->k, n = k + plan->m;
    const uint64_t n_src = plan->n_src;
    std::vector<hbec::ERec> erecs((size_t)n_src);
    bool any = false;
    for (uint64_t i = 0; i < n_src; ++i) {  // zero-length entries too
        const uint64_t S = plan->src[i].shard_len;
        if ((unsigned __int128)lens[i] > (unsigned __int128)S * (uint64_t)k)
            return fail(HBEC_ERR_INVALID_ARG, "lens exceeds k * shard_len (entry " + std::to_string(i) + ")");
        erecs[i] = hbec::ERec{lens[i], 0u, 0u, 0u};
        any = any || lens[i];
    }
    if (!any) return HBEC_OK;  // no chain
    if (!d_digests && !d_expected) return fail(HBEC_ERR_INVALID_ARG, "neither d_digests nor d_expected given");
    std::vector<hbec::EChain> chains;
    hbec::etag_chains(erecs, object_start, object_start ? n_objects : (uint32_t)n_src, chains);
    if (chains.size() / 64 >= (1ull << 31)) return fail(HBEC_ERR_INVALID_ARG, "call too large (>= 2^37 chains)");
    rc = hash_plan_device(plan);
    if (rc) return rc;

    // the spans to decode, back to back in one scratch allocation
    std::vector<void*> dsts((size_t)n_src, nullptr);
    std::vector<uint64_t> starts((size_t)n_src, 0u), span((size_t)n_src, 0u);
    uint64_t scratch_bytes = 0, decoded = 0;
    for (uint64_t i = 0; i < n_src; ++i) {
        hbec::ERec& r = erecs[i];
        const uint64_t S = plan->src[i].shard_len;
        if (!r.len || !hbec::etag_span((uint32_t)k, S, r.len, patterns + (size_t)pattern_of[i] * n, &r.j0, &r.j1))
            continue;
        starts[i] = hbec::etag_span_lo(S, r.j0);
        span[i] = hbec::etag_span_hi(S, r.len, r.j1) - starts[i];
        r.red = 1u;  // its place in scratch, below
        scratch_bytes += span[i];
        ++decoded;
    }
    void* scratch = nullptr;
    if (decoded) {
        // whole dwords: the chain kernel loads the dword a byte lies in
        rc = hbec::scratch_alloc((size_t)((scratch_bytes + 3u) & ~(uint64_t)3u), stream, &scratch);
        if (rc) return rc;
        uint64_t at = reinterpret_cast<uintptr_t>(scratch);
        for (uint64_t i = 0; i < n_src; ++i) {
            if (!erecs[i].red) continue;
            dsts[i] = reinterpret_cast<void*>(at);
            erecs[i].red = at - starts[i];
            at += span[i];
        }
        rc = glue_plan_range(codec, plan, patterns, n_patterns, pattern_of, dsts.data(), starts.data(), span.data(),
                             stream);
        if (rc) {
            hbec::scratch_free(scratch, stream);
            return rc;
        }
    }
    uint64_t segments = 0;
    for (uint64_t i = 0; i < n_src; ++i)
        segments += hbec::etag_entry_segments(plan->shards, (uint32_t)k, plan->src[i].shard_len, erecs[i]);

    static_assert(sizeof(hbec::EChain) == 24 && sizeof(hbec::ERec) == 24, "staged as words, 8-byte aligned");
    const size_t chain_words = chains.size() * (sizeof(hbec::EChain) / 4);
    std::vector<uint32_t> stage(chain_words + erecs.size() * (sizeof(hbec::ERec) / 4));
    std::memcpy(stage.data(), chains.data(), chain_words * 4);
    std::memcpy(stage.data() + chain_words, erecs.data(), erecs.size() * sizeof(hbec::ERec));
    rc = staged_launches(plan, stage, stream, [&](const uint32_t* d_stage) {
        count(g_calls[kEtag].launches);
        count(g_calls[kEtag].second, chains.size());
        count(g_etag_segments, segments);
        count(g_etag_decoded, decoded);
        const hipError_t e = (hipError_t)hbec::launch_etag_chains(
            plan->d_hrecs, reinterpret_cast<const hbec::ERec*>(d_stage + chain_words),
            reinterpret_cast<const hbec::EChain*>(d_stage), chains.size(), k, d_filter, filter_bits, d_expected,
            d_digests, d_expected ? d_bad : nullptr, stream, plan->shards);
        return Queued{e, "launch md5_etag"};
    });
    hbec::scratch_free(scratch, stream);
    return rc;
}

int etag_plan_files(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                    const uint64_t* content_lengths, uint64_t chunk_size, const uint8_t* patterns,
                    uint32_t n_patterns, const uint32_t* pattern_of, const uint32_t* d_filter, uint32_t filter_bits,
                    const uint8_t* d_expected, uint8_t* d_digests, uint32_t* d_bad, hipStream_t stream) {
    if (!codec || !plan || !content_lengths) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
    if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
    std::vector<uint64_t> lens((size_t)std::max<uint64_t>(1, plan->n_src), 0u);
    if (plan->n_src) {
        const int rc = files_cut_entries(plan, object_start, n_objects, content_lengths, chunk_size,
                                         [&](uint32_t, uint64_t i, uint64_t, uint64_t len) { lens[i] = len; });
        if (rc) return rc;
    }
    return etag_plan(codec, plan, patterns, n_patterns, pattern_of, lens.data(), plan->n_src ? object_start : nullptr,
                     n_objects, d_filter, filter_bits, d_expected, d_digests, d_bad, stream);
}

// ---- the k + m shards of every entry from its object bytes (hbec_split_plan) ----

// The other route (any k, m, S), one source entry: every data shard with a byte
// of the piece is one device-to-device copy, clipped; ecSplit's pad is one
// memset per data shard it reaches; the parity is one apply of the encode rows
// over the data shards just written.  Every copy, memset and apply counts as a
// per-stripe call.
int split_other_entry(const hbec_plan* plan, uint32_t i, const std::vector<uint8_t>& rows, uint64_t src, uint64_t len,
                      hipStream_t stream) {
    const int k = plan->k, m = plan->m;
    const uint64_t S = plan->src[i].shard_len;
    for (int j = 0; j < k; ++j) {
        const uint64_t V = hbec::split_valid(len, (uint64_t)j, S);
        uint8_t* shard = reinterpret_cast<uint8_t*>(shard_addr(plan, i, j));
        hipError_t e = hipSuccess;
        if (V) {
            count(g_calls[kSplit].second);
            e = hipMemcpyAsync(shard, reinterpret_cast<const void*>(src + (uint64_t)j * S), V,
                               hipMemcpyDeviceToDevice, stream);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync (split)");
        }
        if (V < S) {
            count(g_calls[kSplit].second);
            e = hipMemsetAsync(shard + V, 0, S - V, stream);
            if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync (split)");
        }
    }
    if (m == 0) return HBEC_OK;
    std::vector<hbec_view> vin((size_t)k), vout((size_t)m);
    for (int j = 0; j < k; ++j) vin[j] = hbec_view{reinterpret_cast<void*>(shard_addr(plan, i, j)), 0};
    for (int r = 0; r < m; ++r) vout[r] = hbec_view{reinterpret_cast<void*>(shard_addr(plan, i, k + r)), 0};
    count(g_calls[kSplit].second);
    return hbec::apply_views(m, k, rows.data(), vin.data(), vout.data(), 1, S, stream);
}

int split_plan(hbec_codec* codec, const hbec_plan* plan, const void* const* srcs, const uint64_t* src_lens,
               hipStream_t stream) {
    if (!codec || !plan || !srcs || !src_lens) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
    if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
    const uint64_t n_src = plan->n_src;
    bool any = false;
    for (uint64_t i = 0; i < n_src; ++i) {  // zero-length entries too
        const uint64_t S = plan->src[i].shard_len, len = src_lens[i];
        const uint64_t src = reinterpret_cast<uintptr_t>(srcs[i]);
        if (!len) continue;
        if (!hbec::split_len_ok(len, (uint64_t)k, S))
            return fail(HBEC_ERR_INVALID_ARG,
                        "src_lens does not give the entry's shard length (entry " + std::to_string(i) + ")");
        if (!src) return fail(HBEC_ERR_INVALID_ARG, "null source with src_lens > 0 (entry " + std::to_string(i) + ")");
        for (int sh = 0; sh < n; ++sh)
            if (hbec::glue_overlaps(src, len, shard_addr(plan, (uint32_t)i, sh), S))
                return fail(HBEC_ERR_INVALID_ARG, "source overlaps shard " + std::to_string(sh) +
                                                      " of its own entry (entry " + std::to_string(i) + ")");
        any = true;
    }
    if (!any) return HBEC_OK;  // nothing given
    // a plan of m = 0 has a list of the call's own (plan_internal.h)
    const bool own = m == 0;
    int rc = own ? walk_list_device(plan, 1, &plan->sp_built, &plan->d_sprecs, &plan->d_sptiles, &plan->n_sptiles,
                                    &plan->sp_other)
                 : mixed_plan_device(plan);
    if (rc) return rc;
    const hbec::MRec* d_recs = own ? plan->d_sprecs : plan->d_mrecs;
    const hbec::MTile* d_tiles = own ? plan->d_sptiles : plan->d_mtiles;
    const uint64_t n_tiles = own ? plan->n_sptiles : plan->n_mtiles;
    const std::vector<uint32_t>& other = own ? plan->sp_other : plan->mp_other;
    // the encode rows: rows k..k+m-1 of the coding matrix
    std::vector<uint8_t> mat((size_t)n * k);
    hbec_matrix(codec, mat.data());
    const std::vector<uint8_t> rows(mat.begin() + (size_t)k * k, mat.end());

    if (n_tiles > 0) {
        // One pattern record for the call (data shards in, parity shards out, the
        // encode rows; for m = 0 the header alone), one word per source entry and
        // its piece; one launch per chunk of the list, of the instance for m.
        std::vector<int> data((size_t)k), par((size_t)std::max(1, m));
        for (int j = 0; j < k; ++j) data[j] = j;
        for (int r = 0; r < m; ++r) par[r] = k + r;
        std::vector<uint32_t> stage;
        const uint32_t rec = hbec::mp_pattern(stage, k, data.data(), m ? par.data() : nullptr, m, m ? rows.data() : nullptr);
        const size_t rec_words = stage.size();
        stage.resize(rec_words + 5 * (size_t)n_src);
        const size_t src_at = rec_words + (size_t)n_src;
        bool work = false;
        for (uint64_t i = 0; i < n_src; ++i) {
            const uint64_t S = plan->src[i].shard_len, len = src_lens[i];
            const uint64_t src = reinterpret_cast<uintptr_t>(srcs[i]);
            const bool mine = S != 0 && hbec::pos32_shard(S) && len != 0;  // mp_build's route
            stage[rec_words + i] = mine ? (((uint32_t)m << hbec::kMPatShift) | rec) : hbec::kSplitSkip;
            work = work || mine;
            uint32_t* d = stage.data() + src_at + 4 * i;
            d[0] = (uint32_t)src, d[1] = (uint32_t)(src >> 32), d[2] = (uint32_t)len, d[3] = (uint32_t)(len >> 32);
        }
        if (work) {
            int cus = 0;
            rc = current_cus(&cus);
            if (rc) return rc;
            rc = staged_launches(plan, stage, stream, [&](const uint32_t* d_pats) {
                return walk_chunks(kSplit, n_tiles, "launch gf_split_plan", [&](uint64_t t0, uint32_t nt) {
                    return (hipError_t)hbec::launch_split_plan(k, m, d_recs, d_tiles + t0, nt, d_pats + rec_words,
                                                               d_pats + src_at, d_pats, cus, stream, plan->shards);
                });
            });
            if (rc) return rc;
        }
    }
    // the other route, one entry at a time (any k, m, S)
    for (uint32_t i : other) {
        if (!src_lens[i]) continue;
        rc = split_other_entry(plan, i, rows, reinterpret_cast<uintptr_t>(srcs[i]), src_lens[i], stream);
        if (rc) return rc;
    }
    return HBEC_OK;
}

// ---- whole objects of a files plan into their shard files (hbec_split_plan_files) ----

int split_plan_files(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                     const uint64_t* content_lengths, uint64_t chunk_size, const void* const* object_srcs,
                     hipStream_t stream) {
    if (!codec || !plan || !content_lengths || !object_srcs) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
    if (k != plan->k || m != plan->m) return fail(HBEC_ERR_INVALID_ARG, "plan built for another (k, m)");
    const uint64_t n_src = plan->n_src;
    std::vector<const void*> srcs((size_t)std::max<uint64_t>(1, n_src), nullptr);
    std::vector<uint64_t> lens((size_t)std::max<uint64_t>(1, n_src), 0u);
    if (n_src) {
        if (const char* why = hbec::files_check_objects(object_start, n_objects, n_src))
            return fail(HBEC_ERR_INVALID_ARG, why);
        if (chunk_size == 0 || chunk_size > (uint64_t)INT64_MAX) return fail(HBEC_ERR_INVALID_ARG, "chunk_size out of range");
        for (uint32_t g = 0; g < n_objects; ++g) {
            const uint64_t L = content_lengths[g], cnt = object_start[g + 1] - object_start[g];
            if (L > (uint64_t)INT64_MAX || hbec::ec_stripe_count((int64_t)L, k, (int64_t)chunk_size) != cnt)
                return fail(HBEC_ERR_INVALID_ARG, "content length does not give the entry count (object " +
                                                      std::to_string(g) + ")");
            for (uint64_t t = 0; t < cnt; ++t) {
                const uint64_t i = object_start[g] + t;
                if (plan->src[i].shard_len != hbec::ec_stripe_shard_length((int64_t)L, k, (int64_t)chunk_size, t))
                    return fail(HBEC_ERR_INVALID_ARG, "shard length mismatch (object " + std::to_string(g) +
                                                          ", stripe " + std::to_string(t) + ")");
                uint64_t off = 0;
                hbec::glue_files_cut(L, (uint64_t)k, chunk_size, t, &off, &lens[i]);
                srcs[i] = object_srcs[g] ? static_cast<const uint8_t*>(object_srcs[g]) + off : nullptr;
            }
        }
    }
    return split_plan(codec, plan, srcs.data(), lens.data(), stream);
}

}  // namespace

extern "C" {

int hbec_reconstruct_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                                const uint32_t* pattern_of, int data_only, void* hip_stream) {
    return hbec::guarded("hbec_reconstruct_plan_mixed", [&]() -> int {
        return reconstruct_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, data_only != 0,
                                      static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_mixed_plan_stats(uint64_t* kernel_launches, uint64_t* per_stripe_calls) {
    return call_stats("hbec_mixed_plan_stats", kReconstruct, kernel_launches, per_stripe_calls);
}

// the walk kernels of all five calls code tiles of one size
int hbec_mixed_plan_tile_bytes(void) { return (int)hbec::mixed_plan_tile_bytes(); }

int hbec_set_mixed_plan_chunk_tiles(uint64_t tiles) {
    return set_chunk_tiles("hbec_set_mixed_plan_chunk_tiles", kReconstruct, tiles);
}

int hbec_verify_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                           const uint32_t* pattern_of, uint32_t* d_flags, void* hip_stream) {
    return hbec::guarded("hbec_verify_plan_mixed", [&]() -> int {
        return verify_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, d_flags,
                                 static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_verify_mixed_plan_stats(uint64_t* kernel_launches, uint64_t* per_stripe_calls) {
    return call_stats("hbec_verify_mixed_plan_stats", kVerify, kernel_launches, per_stripe_calls);
}

int hbec_verify_mixed_plan_tile_bytes(void) { return hbec_mixed_plan_tile_bytes(); }

int hbec_set_verify_mixed_plan_chunk_tiles(uint64_t tiles) {
    return set_chunk_tiles("hbec_set_verify_mixed_plan_chunk_tiles", kVerify, tiles);
}

int hbec_repair_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                           const uint32_t* pattern_of, int data_only, uint32_t* d_flags, void* hip_stream) {
    return hbec::guarded("hbec_repair_plan_mixed", [&]() -> int {
        return repair_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, data_only != 0, d_flags,
                                 static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_repair_plan_stats(uint64_t* kernel_launches, uint64_t* per_stripe_calls) {
    return call_stats("hbec_repair_plan_stats", kRepair, kernel_launches, per_stripe_calls);
}

int hbec_repair_plan_tile_bytes(void) { return hbec_mixed_plan_tile_bytes(); }

int hbec_set_repair_plan_chunk_tiles(uint64_t tiles) {
    return set_chunk_tiles("hbec_set_repair_plan_chunk_tiles", kRepair, tiles);
}

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
    return call_stats("hbec_locate_plan_stats", kLocate, kernel_launches, skipped_entries);
}

int hbec_locate_plan_tile_bytes(void) { return hbec_mixed_plan_tile_bytes(); }

int hbec_set_locate_plan_chunk_tiles(uint64_t tiles) {
    return set_chunk_tiles("hbec_set_locate_plan_chunk_tiles", kLocate, tiles);
}

int hbec_heal_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                         const uint32_t* pattern_of, const uint32_t* d_where, uint32_t* d_flags, void* hip_stream) {
    return hbec::guarded("hbec_heal_plan_mixed", [&]() -> int {
        return heal_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, d_where, d_flags,
                               static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_heal_plan_stats(uint64_t* kernel_launches, uint64_t* skipped_entries) {
    return call_stats("hbec_heal_plan_stats", kHeal, kernel_launches, skipped_entries);
}

int hbec_heal_plan_tile_bytes(void) { return hbec_mixed_plan_tile_bytes(); }

int hbec_set_heal_plan_chunk_tiles(uint64_t tiles) {
    return set_chunk_tiles("hbec_set_heal_plan_chunk_tiles", kHeal, tiles);
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
    return call_stats("hbec_hash_plan_stats", kHash, kernel_launches, chains);
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
    // a null `segments` fails with the other two: call_stats sees a null `chains`
    const int rc = call_stats("hbec_hash_files_stats", kHashFiles, kernel_launches, segments ? chains : nullptr);
    if (rc == HBEC_OK) *segments = g_hashfiles_segments.load(std::memory_order_relaxed);
    return rc;
}

int hbec_glue_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                         const uint32_t* pattern_of, void* const* dsts, const uint64_t* dst_lens, void* hip_stream) {
    return hbec::guarded("hbec_glue_plan_mixed", [&]() -> int {
        return glue_plan_mixed(codec, plan, patterns, n_patterns, pattern_of, dsts, dst_lens,
                               static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_glue_plan_files(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                         const uint64_t* content_lengths, uint64_t chunk_size, const uint8_t* patterns,
                         uint32_t n_patterns, const uint32_t* pattern_of, void* const* object_dsts, void* hip_stream) {
    return hbec::guarded("hbec_glue_plan_files", [&]() -> int {
        return glue_plan_files(codec, plan, object_start, n_objects, content_lengths, chunk_size, patterns, n_patterns,
                               pattern_of, object_dsts, static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_glue_plan_stats(uint64_t* kernel_launches, uint64_t* per_stripe_calls) {
    return call_stats("hbec_glue_plan_stats", kGlue, kernel_launches, per_stripe_calls);
}

int hbec_glue_plan_tile_bytes(void) { return hbec_mixed_plan_tile_bytes(); }

int hbec_set_glue_plan_chunk_tiles(uint64_t tiles) {
    return set_chunk_tiles("hbec_set_glue_plan_chunk_tiles", kGlue, tiles);
}

int hbec_glue_plan_range(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                         const uint32_t* pattern_of, void* const* dsts, const uint64_t* starts, const uint64_t* lens,
                         void* hip_stream) {
    return hbec::guarded("hbec_glue_plan_range", [&]() -> int {
        return glue_plan_range(codec, plan, patterns, n_patterns, pattern_of, dsts, starts, lens,
                               static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_glue_plan_files_range(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start,
                               uint32_t n_objects, const uint64_t* content_lengths, uint64_t chunk_size,
                               const uint8_t* patterns, uint32_t n_patterns, const uint32_t* pattern_of,
                               void* const* object_dsts, const uint64_t* range_starts, const uint64_t* range_ends,
                               void* hip_stream) {
    return hbec::guarded("hbec_glue_plan_files_range", [&]() -> int {
        return glue_plan_files_range(codec, plan, object_start, n_objects, content_lengths, chunk_size, patterns,
                                     n_patterns, pattern_of, object_dsts, range_starts, range_ends,
                                     static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_glue_range_stats(uint64_t* kernel_launches, uint64_t* per_stripe_calls) {
    return call_stats("hbec_glue_range_stats", kGlueRange, kernel_launches, per_stripe_calls);
}

int hbec_glue_range_tile_bytes(void) { return hbec_mixed_plan_tile_bytes(); }

int hbec_set_glue_range_chunk_tiles(uint64_t tiles) {
    return set_chunk_tiles("hbec_set_glue_range_chunk_tiles", kGlueRange, tiles);
}

int hbec_etag_plan_mixed(hbec_codec* codec, const hbec_plan* plan, const uint8_t* patterns, uint32_t n_patterns,
                         const uint32_t* pattern_of, const uint64_t* lens, const uint32_t* d_filter,
                         uint32_t filter_bits, const uint8_t* d_expected, uint8_t* d_digests, uint32_t* d_bad,
                         void* hip_stream) {
    return hbec::guarded("hbec_etag_plan_mixed", [&]() -> int {
        return etag_plan(codec, plan, patterns, n_patterns, pattern_of, lens, nullptr, 0, d_filter, filter_bits,
                         d_expected, d_digests, d_bad, static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_etag_plan_files(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                         const uint64_t* content_lengths, uint64_t chunk_size, const uint8_t* patterns,
                         uint32_t n_patterns, const uint32_t* pattern_of, const uint32_t* d_filter,
                         uint32_t filter_bits, const uint8_t* d_expected, uint8_t* d_digests, uint32_t* d_bad,
                         void* hip_stream) {
    return hbec::guarded("hbec_etag_plan_files", [&]() -> int {
        return etag_plan_files(codec, plan, object_start, n_objects, content_lengths, chunk_size, patterns,
                               n_patterns, pattern_of, d_filter, filter_bits, d_expected, d_digests, d_bad,
                               static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_etag_plan_stats(uint64_t* kernel_launches, uint64_t* chains, uint64_t* segments, uint64_t* decoded_entries) {
    // a null third or fourth fails with the other two: call_stats sees a null `chains`
    const int rc = call_stats("hbec_etag_plan_stats", kEtag, kernel_launches,
                              segments && decoded_entries ? chains : nullptr);
    if (rc == HBEC_OK) {
        *segments = g_etag_segments.load(std::memory_order_relaxed);
        *decoded_entries = g_etag_decoded.load(std::memory_order_relaxed);
    }
    return rc;
}

int hbec_split_plan(hbec_codec* codec, const hbec_plan* plan, const void* const* srcs, const uint64_t* src_lens,
                    void* hip_stream) {
    return hbec::guarded("hbec_split_plan", [&]() -> int {
        return split_plan(codec, plan, srcs, src_lens, static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_split_plan_files(hbec_codec* codec, const hbec_plan* plan, const uint32_t* object_start, uint32_t n_objects,
                          const uint64_t* content_lengths, uint64_t chunk_size, const void* const* object_srcs,
                          void* hip_stream) {
    return hbec::guarded("hbec_split_plan_files", [&]() -> int {
        return split_plan_files(codec, plan, object_start, n_objects, content_lengths, chunk_size, object_srcs,
                                static_cast<hipStream_t>(hip_stream));
    });
}

int hbec_split_plan_stats(uint64_t* kernel_launches, uint64_t* per_stripe_calls) {
    return call_stats("hbec_split_plan_stats", kSplit, kernel_launches, per_stripe_calls);
}

int hbec_split_plan_tile_bytes(void) { return hbec_mixed_plan_tile_bytes(); }

int hbec_set_split_plan_chunk_tiles(uint64_t tiles) {
    return set_chunk_tiles("hbec_set_split_plan_chunk_tiles", kSplit, tiles);
}

}  // extern "C"
