// hostpath.cpp — streaming host path: code a batch of
// HOST-resident stripes (ecSplit databuf layout, objectserver/ecutils.go:31-35,
// 55-58) through a pinned staging ring.  Per chunk of stripes:
//
//   CPU gather (thread pool) caller memory -> pinned IN slot
//   H2D IN slot -> device IN region            (copy stream)
//   gf_apply_stripes over the chunk's tiles    (compute stream)
//   D2H device OUT region -> pinned OUT slot   (copy-back stream)
//   CPU scatter pinned OUT slot -> caller memory
//
// with three slots in flight, so the CPU copies of one chunk overlap the DMA
// and kernel work of the others.  Stripes wider than a slot are cut into
// column pieces.  Everything is synchronous for the caller: when the call
// returns, parity (encode) or the rebuilt shards (reconstruct) are in the
// caller's buffers.
//
// Zero-copy: stripes that live in pinned, device-mapped host memory
// (hbec_host_alloc, or any hipHostMalloc / hipHostRegister buffer) skip the
// ring entirely.  The stripe kernel reads their data shards and writes their
// parity in place over PCIe, so there is no CPU copy and no DMA call per
// chunk; only 32-B tile records travel.
//
// What is cut where (routes, pieces, chunks, the records of a slot) is decided
// by the HIP-free rules of hostcut.h.  This file owns the ring and queues the
// work: host_run_on picks the route, zero_copy_run (over walk_slots) codes pinned
// stripes, ring_run the staged ones, verify_host_run_on serves hbec_verify_host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hbec.h"
#include "gf256.h"
#include "hostcut.h"
#include "internal.h"
#include "kernels.h"
#include "pool.h"
#include "vplan.h"

using hbec::fail;
using hbec::hip_fail;

namespace {

constexpr int kSlots = 3;

// How the host path cut its work, since load (hbec_host_run_stats): staging
// chunks queued, column pieces cut, record slots the zero-copy runners filled,
// hash arenas handed to md5_list.  One increment per event, nothing per byte.
std::atomic<uint64_t> g_ring_chunks{0}, g_ring_pieces{0}, g_zc_record_slots{0}, g_arena_flushes{0};

struct Ring {
    int dev = -1;
    int cus = 0;  // compute units of dev (grid sizing), read once
    size_t in_cap = 0, out_cap = 0, tile_cap = 0;
    hipStream_t s_h2d = nullptr, s_cmp = nullptr, s_d2h = nullptr;
    uint8_t *pin_in[kSlots] = {}, *pin_out[kSlots] = {}, *dev_in[kSlots] = {}, *dev_out[kSlots] = {};
    hbec::TileRec *pin_tiles[kSlots] = {}, *dev_tiles[kSlots] = {};
    hipEvent_t ev_h2d[kSlots] = {}, ev_cmp[kSlots] = {}, ev_done[kSlots] = {};
    // ShardHash (hbec_encode_host_md5), created on first use: n_arenas device hash arenas
    // (HBEC_HASH_ARENAS, default 2, of HBEC_HASH_ARENA_MB, default 1024; 2 x 3 GiB: pinned 4+2
    // encode+hash 1.14 x encode alone instead of 1.21 x, profiles/r02_host_md5_arenas.jsonl).  A
    // chunk's shards land in the current arena (copied D2D after the ring's kernel, or written by
    // the mirrored zero-copy kernel); a full arena is hashed by ONE md5_list launch on its own
    // stream while the next arenas fill, so hashing hides behind the PCIe stream, and the hashes
    // of several arenas may run at once.
    static constexpr int kArenas = 8;
    int n_arenas = 0;
    hipStream_t s_md5[kArenas] = {};
    uint8_t* arena[kArenas] = {};
    size_t arena_cap = 0, arena_rec_cap = 0;
    uint64_t *pin_md5rec[kArenas] = {}, *dev_md5rec[kArenas] = {};
    hipEvent_t ev_arena_copied[kArenas] = {}, ev_arena_hashed[kArenas] = {};
    std::unique_ptr<hbec::Pool> pool;

    ~Ring() {
        auto drop = [](std::initializer_list<void*> pinned, std::initializer_list<void*> device,
                       std::initializer_list<hipEvent_t> events) {
            for (void* p : pinned)
                if (p) (void)hipHostFree(p);
            for (void* p : device)
                if (p) (void)hipFree(p);
            for (hipEvent_t e : events)
                if (e) (void)hipEventDestroy(e);
        };
        for (int i = 0; i < kSlots; ++i)
            drop({pin_in[i], pin_out[i], pin_tiles[i]}, {dev_in[i], dev_out[i], dev_tiles[i]},
                 {ev_h2d[i], ev_cmp[i], ev_done[i]});
        for (int a = 0; a < kArenas; ++a)
            drop({pin_md5rec[a]}, {arena[a], dev_md5rec[a]}, {ev_arena_copied[a], ev_arena_hashed[a]});
        for (hipStream_t s : s_md5)
            if (s) (void)hipStreamDestroy(s);
        for (hipStream_t s : {s_h2d, s_cmp, s_d2h})
            if (s) (void)hipStreamDestroy(s);
    }
};

size_t env_size(const char* name, size_t dflt) {
    const long long v = hbec::env_knob(name, 0);
    return v > 0 ? (size_t)v : dflt;
}
size_t tune_size(const char* name, size_t dflt) {
    const long long v = hbec::tune_knob(name, 0);
    return v > 0 ? (size_t)v : dflt;
}

int ring_init(Ring& r, int dev) {
    r.dev = dev;
    int rc = hbec::device_cus(dev, &r.cus);
    if (rc) return rc;
    const size_t slot = env_size("HBEC_HOST_SLOT_MB", 64) << 20;  // IN bytes per slot
    r.in_cap = slot;
    r.out_cap = slot;  // outputs per piece <= inputs (R <= K) except tiny K: sized below per call
    r.tile_cap = slot / 1024 + 1024;
    hipError_t e;
#define HB_CHECK(x, what)                       \
    do {                                        \
        e = (x);                                \
        if (e != hipSuccess) return hip_fail(e, what); \
    } while (0)
    HB_CHECK(hipStreamCreateWithFlags(&r.s_h2d, hipStreamNonBlocking), "stream");
    HB_CHECK(hipStreamCreateWithFlags(&r.s_cmp, hipStreamNonBlocking), "stream");
    HB_CHECK(hipStreamCreateWithFlags(&r.s_d2h, hipStreamNonBlocking), "stream");
    for (int i = 0; i < kSlots; ++i) {
        HB_CHECK(hipHostMalloc(reinterpret_cast<void**>(&r.pin_tiles[i]), r.tile_cap * sizeof(hbec::TileRec),
                               hipHostMallocDefault),
                 "pinned tiles");
        HB_CHECK(hipMalloc(&r.dev_tiles[i], r.tile_cap * sizeof(hbec::TileRec)), "device tiles");
        HB_CHECK(hipEventCreateWithFlags(&r.ev_h2d[i], hipEventDisableTiming), "event");
        HB_CHECK(hipEventCreateWithFlags(&r.ev_cmp[i], hipEventDisableTiming), "event");
        HB_CHECK(hipEventCreateWithFlags(&r.ev_done[i], hipEventDisableTiming), "event");
    }
#undef HB_CHECK
    return HBEC_OK;
}

// The staging slots and copy threads, made on the first call that stages
// (zero-copy calls only need the tile records).
int ring_staging_init(Ring& r) {
    if (r.pool) return HBEC_OK;  // set last: everything below exists
    hipError_t e = hipSuccess;
    for (int i = 0; i < kSlots && e == hipSuccess; ++i) {  // a failed earlier attempt keeps what it got
        if (!r.pin_in[i]) e = hipHostMalloc(reinterpret_cast<void**>(&r.pin_in[i]), r.in_cap, hipHostMallocDefault);
        if (e == hipSuccess && !r.pin_out[i])
            e = hipHostMalloc(reinterpret_cast<void**>(&r.pin_out[i]), r.out_cap, hipHostMallocDefault);
        if (e == hipSuccess && !r.dev_in[i]) e = hipMalloc(&r.dev_in[i], r.in_cap);
        if (e == hipSuccess && !r.dev_out[i]) e = hipMalloc(&r.dev_out[i], r.out_cap);
    }
    if (e != hipSuccess) return hip_fail(e, "staging slots");
    r.pool.reset(new hbec::Pool(hbec::host_threads() - 1));  // + the calling thread
    return HBEC_OK;
}

int ring_md5_init(Ring& r) {
    if (r.n_arenas > 0) return HBEC_OK;  // set last: everything below exists
    const size_t cap = env_size("HBEC_HASH_ARENA_MB", 1024) << 20;
    const int n_arenas = (int)std::min<size_t>(Ring::kArenas, std::max<size_t>(2, tune_size("HBEC_HASH_ARENAS", 2)));
    r.arena_cap = std::max(cap, r.in_cap + r.out_cap);
    // MD5 records per arena (32 B pinned each; HBEC_HASH_ARENA_RECS, default
    // 256 K = 8 MiB): an arena is hashed early when its records run out, so
    // this bounds pinned memory, not batch size (one record per 16-B shard
    // would pin 2 GiB per arena)
    r.arena_rec_cap = std::min<size_t>(r.arena_cap / 16 + 1024, tune_size("HBEC_HASH_ARENA_RECS", 1u << 18));
    hipError_t e = hipSuccess;
    for (int a = 0; a < n_arenas && e == hipSuccess; ++a) {  // a failed earlier attempt keeps what it got
        if (!r.s_md5[a]) e = hipStreamCreateWithFlags(&r.s_md5[a], hipStreamNonBlocking);
        if (e == hipSuccess && !r.arena[a]) e = hipMalloc(&r.arena[a], r.arena_cap);
        if (e == hipSuccess && !r.pin_md5rec[a])
            e = hipHostMalloc(reinterpret_cast<void**>(&r.pin_md5rec[a]), r.arena_rec_cap * 32, hipHostMallocDefault);
        if (e == hipSuccess && !r.dev_md5rec[a])
            e = hipMalloc(reinterpret_cast<void**>(&r.dev_md5rec[a]), r.arena_rec_cap * 32);
        if (e == hipSuccess && !r.ev_arena_copied[a])
            e = hipEventCreateWithFlags(&r.ev_arena_copied[a], hipEventDisableTiming);
        if (e == hipSuccess && !r.ev_arena_hashed[a])
            e = hipEventCreateWithFlags(&r.ev_arena_hashed[a], hipEventDisableTiming);
    }
    if (e != hipSuccess) return hip_fail(e, "hash arena");
    r.n_arenas = n_arenas;
    return HBEC_OK;
}

// The hash arenas of one hbec_encode_host_md5 call.  Shards are appended to
// the current arena and a record per shard to its pinned record list; a full
// arena is hashed by one md5_list launch on the arena's stream, ordered after
// the work `producer` queued to fill it, and the call moves on to the next
// arena once that arena's previous hash has finished (its memory and pinned
// records are then free).
struct ArenaCursor {
    Ring* ring;
    hipStream_t producer;
    uint8_t* d_digest;
    int cur = 0;
    uint64_t used = 0, recs = 0;

    uint64_t base() const { return reinterpret_cast<uint64_t>(ring->arena[cur]) + used; }
    bool fits(uint64_t bytes, uint64_t n_recs) const {
        return used + bytes <= ring->arena_cap && recs + n_recs <= ring->arena_rec_cap;
    }
    void add(uint64_t addr, uint64_t len, uint64_t slot) {
        uint64_t* r = ring->pin_md5rec[cur] + 4 * recs++;
        r[0] = addr;
        r[1] = len;
        r[2] = slot;
        r[3] = 0;
    }
    int flush() {  // hash the current arena, move to the next free one
        if (recs == 0) return HBEC_OK;
        g_arena_flushes.fetch_add(1, std::memory_order_relaxed);
        const int a = cur;
        hipStream_t hs = ring->s_md5[a];
        hipError_t e = hipEventRecord(ring->ev_arena_copied[a], producer);
        if (e == hipSuccess) e = hipStreamWaitEvent(hs, ring->ev_arena_copied[a], 0);
        if (e == hipSuccess)
            e = hipMemcpyAsync(ring->dev_md5rec[a], ring->pin_md5rec[a], recs * 32, hipMemcpyHostToDevice, hs);
        if (e == hipSuccess) e = hbec::launch_md5_list(ring->dev_md5rec[a], recs, d_digest, true, hs);
        if (e == hipSuccess) e = hipEventRecord(ring->ev_arena_hashed[a], hs);
        if (e != hipSuccess) return hip_fail(e, "hash arena launch");
        cur = (cur + 1) % ring->n_arenas;
        used = recs = 0;
        e = hipEventSynchronize(ring->ev_arena_hashed[cur]);  // may still hash its last fill
        if (e != hipSuccess) return hip_fail(e, "hash arena wait");
        return HBEC_OK;
    }
    int finish() {  // hash the last partial arena and wait for every hash
        int rc = flush();
        if (rc) return rc;
        for (int a = 0; a < ring->n_arenas; ++a) {
            hipError_t e = hipStreamSynchronize(ring->s_md5[a]);
            if (e != hipSuccess) return hip_fail(e, "hash drain");
        }
        return HBEC_OK;
    }
};

// Rings per device are bounded (HBEC_HOST_RINGS, default 8): each staged
// ring pins 384 MiB of host memory and runs a copy pool of host_threads()
// threads, so one ring per concurrent caller (a busy object server has
// hundreds) would pin tens of GiB and spawn thousands of threads; the first
// 64-thread soak spent minutes creating them.  Callers beyond the bound wait,
// in arrival order, for a ring to come back.  No caller holds a ring while
// waiting for another, so the bound cannot deadlock.
std::mutex g_rings_mu;
std::condition_variable g_rings_cv;
std::vector<Ring*> g_free_rings;
std::map<int, int> g_rings_made;  // per device

int ring_limit() {
    static const int v = (int)env_size("HBEC_HOST_RINGS", 8);
    return v;
}

// Pooled non-blocking streams per device for short per-call work (creating
// and destroying a stream per call costs more than a small batch's copies).
std::mutex g_streams_mu;
std::vector<std::pair<int, hipStream_t>> g_free_streams;

int stream_acquire(hipStream_t* out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    {
        std::lock_guard<std::mutex> g(g_streams_mu);
        for (size_t i = 0; i < g_free_streams.size(); ++i)
            if (g_free_streams[i].first == dev) {
                *out = g_free_streams[i].second;
                g_free_streams.erase(g_free_streams.begin() + (long)i);
                return HBEC_OK;
            }
    }
    e = hipStreamCreateWithFlags(out, hipStreamNonBlocking);
    if (e != hipSuccess) return hip_fail(e, "hipStreamCreate");
    return HBEC_OK;
}

void stream_release(hipStream_t s) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    std::lock_guard<std::mutex> g(g_streams_mu);
    g_free_streams.emplace_back(dev, s);
}

int ring_acquire(Ring** out) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    {
        std::unique_lock<std::mutex> lk(g_rings_mu);
        for (;;) {
            for (size_t i = 0; i < g_free_rings.size(); ++i)
                if (g_free_rings[i]->dev == dev) {
                    *out = g_free_rings[i];
                    g_free_rings.erase(g_free_rings.begin() + (long)i);
                    return HBEC_OK;
                }
            if (g_rings_made[dev] < ring_limit()) break;
            g_rings_cv.wait(lk);
        }
        ++g_rings_made[dev];  // reserved: made below, outside the lock
    }
    std::unique_ptr<Ring> r(new (std::nothrow) Ring());
    int rc = r ? ring_init(*r, dev) : fail(HBEC_ERR_NOMEM, "ring allocation");
    if (rc) {
        {
            std::lock_guard<std::mutex> g(g_rings_mu);
            --g_rings_made[dev];
        }
        g_rings_cv.notify_one();
        return rc;
    }
    *out = r.release();
    return HBEC_OK;
}

void ring_release(Ring* r) {
    {
        std::lock_guard<std::mutex> g(g_rings_mu);
        g_free_rings.push_back(r);
    }
    g_rings_cv.notify_all();  // waiters may be on different devices
}

// ---- pinned host memory (zero-copy host path) ----
struct PinnedRange {
    uint64_t len;
    uint64_t dev;  // device address of the range's first byte
};
std::mutex g_pin_mu;
std::map<uint64_t, PinnedRange> g_pinned;  // host base -> range (hbec_host_alloc)

// Blocks per CU of the zero-copy stripes kernel (HBEC_ZC_BLOCKS_PER_CU):
// it streams over PCIe, whose latency wants more requests in flight than
// HBM's sweet spot of one 4-wave block per CU.
int zero_copy_blocks_per_cu() {
    // 1: 45.9, 2: 46.7, 4: 46.6, 8: 46.8 GiB/s (profiles/r02_zc_bpc.jsonl)
    static const int v = (int)tune_size("HBEC_ZC_BLOCKS_PER_CU", 2);
    return v;
}

// Pinned stripes that are not 16-B aligned (or S % 16 != 0): zero-copy through
// the unaligned kernel (a tuning build's HBEC_ZC_UNALIGNED=0: the staged ring).
bool zero_copy_unaligned_enabled() {
    static const bool on = hbec::tune_knob("HBEC_ZC_UNALIGNED", 1) != 0;
    return on;
}

// Grid cap of the zero-copy stripes kernel (HBEC_ZC_GRID blocks, 0 = CUs x
// blocks per CU).  64 blocks of 4 waves keep ~1 MiB of PCIe reads in flight,
// plenty for the link, where the whole chip (512 blocks) kept ~8 MiB queued
// and streamed slower: 4096 x 1 MiB 4+2 pinned stripes 48.4-48.8 -> 52.2-52.5
// GiB/s, 4 KiB stripes 42.2 -> 45.1 GiB/s; 32 and 128 blocks tie with 64
// (profiles/r02_zc_grid.jsonl).
int zero_copy_max_blocks() {
    static const int v = (int)std::max(0LL, hbec::tune_knob("HBEC_ZC_GRID", 64));
    return v;
}

bool zero_copy_enabled() {
    static const bool on = hbec::env_knob("HBEC_ZEROCOPY", 1) != 0;
    return on;
}

}  // namespace

// Device address of host range [p, p + len) when all of it lies in one
// pinned, device-mapped allocation; 0 otherwise.  hbec_host_alloc ranges are
// looked up in the registry; other pinned memory is asked of the runtime at
// both ends of the range.
bool hbec::zero_copy_any_alignment() { return zero_copy_unaligned_enabled(); }

uint64_t hbec::pinned_device_addr(const void* p, uint64_t len) {
    if (!zero_copy_enabled()) return 0;
    const uint64_t h = reinterpret_cast<uint64_t>(p);
    if (!p || len == 0) return 0;
    {
        std::lock_guard<std::mutex> g(g_pin_mu);
        auto it = g_pinned.upper_bound(h);
        if (it != g_pinned.begin()) {
            --it;
            if (h >= it->first && h + len <= it->first + it->second.len) return it->second.dev + (h - it->first);
        }
    }
    hipPointerAttribute_t a0, a1;
    if (hipPointerGetAttributes(&a0, p) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (a0.type != hipMemoryTypeHost || !a0.devicePointer) return 0;
    // memory pinned elsewhere is only trusted on the device it was pinned for
    // (hbec_host_alloc memory is portable: every device)
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || a0.device != cur) {
        (void)hipGetLastError();
        return 0;
    }
    if (hipPointerGetAttributes(&a1, reinterpret_cast<const uint8_t*>(p) + (len - 1)) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    const uint64_t d0 = reinterpret_cast<uint64_t>(a0.devicePointer);
    const uint64_t d1 = reinterpret_cast<uint64_t>(a1.devicePointer);
    if (a1.type != hipMemoryTypeHost || d1 != d0 + (len - 1)) return 0;
    return d0;
}

namespace {
using hbec::pinned_device_addr;

namespace cut = hbec::cut;
using cut::Pass;
using cut::ZcStripe;

// The slot rotation of every runner that hands a slot back when the kernel that read it is
// done (ev_cmp): wait for the slot, let body(slot, more) queue its work, kernels on s_cmp, and
// mark their end.  more: another slot follows.  There is always a first slot, so callers come
// with at least one stripe or chunk.
template <class Body>
int walk_slots(Ring* ring, const char* wait_what, const char* event_what, Body body) {
    bool more = true;
    for (int c = 0; more; ++c) {
        const int slot = c % kSlots;
        hipError_t e = hipEventSynchronize(ring->ev_cmp[slot]);  // the slot's previous kernels are done
        if (e != hipSuccess) return hip_fail(e, wait_what);
        const int rc = body(slot, more);
        if (rc) return rc;
        e = hipEventRecord(ring->ev_cmp[slot], ring->s_cmp);
        if (e != hipSuccess) return hip_fail(e, event_what);
    }
    return HBEC_OK;
}

// Records plus the slot's IN bytes to the device on the copy stream, and the
// compute stream behind them (the ring and the staged Verify).
int staged_upload(Ring* ring, int slot, size_t rec_bytes, uint64_t in_bytes, const char* what) {
    hipError_t e = hipSuccess;
    if (rec_bytes)
        e = hipMemcpyAsync(ring->dev_tiles[slot], ring->pin_tiles[slot], rec_bytes, hipMemcpyHostToDevice, ring->s_h2d);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ring->dev_in[slot], ring->pin_in[slot], in_bytes, hipMemcpyHostToDevice, ring->s_h2d);
    if (e == hipSuccess) e = hipEventRecord(ring->ev_h2d[slot], ring->s_h2d);
    if (e == hipSuccess) e = hipStreamWaitEvent(ring->s_cmp, ring->ev_h2d[slot], 0);
    return e != hipSuccess ? hip_fail(e, what) : HBEC_OK;
}

// Code pinned stripes in place: records (rings of kSlots pinned/device
// buffers; TileRec and URec are both 32 B, so the slot buffers are shared) are
// the only host->device traffic; the kernel streams the shards over PCIe.  One
// stream, so records, kernels and their reuse are ordered.  recs is the record
// kind (hostcut.h), launch its kernel.  With ps.d_digest (every stripe pinned)
// the kernel also writes every shard column it holds (inputs and outputs) to a
// device hash arena, so nothing crosses PCIe twice and no CPU copy runs; a full
// arena is hashed by one md5_list launch while the kernel fills the next ones.
template <class Recs, class Launch>
int zero_copy_run(Ring* ring, const Recs& recs, const std::vector<ZcStripe>& zs, const Pass& ps, Launch launch) {
    using Rec = typename Recs::Rec;
    static_assert(sizeof(Rec) == sizeof(hbec::TileRec), "record slots are shared");
    int rc = ps.d_digest ? ring_md5_init(*ring) : HBEC_OK;
    if (rc) return rc;
    ArenaCursor ac{ring, ring->s_cmp, ps.d_digest};
    size_t si = 0;
    uint64_t off = 0;
    rc = walk_slots(ring, "zero-copy slot wait", "zero-copy event", [&](int slot, bool& more) -> int {
        Rec* rec = reinterpret_cast<Rec*>(ring->pin_tiles[slot]);
        cut::SlotFill f;
        int frc = HBEC_OK;
        const char* refused = nullptr;
        auto flush = [&] { return (frc = ac.flush()) == HBEC_OK; };
        if (!ps.d_digest) f = cut::fill_plain(recs, zs, si, off, rec, ring->tile_cap);
        else refused = cut::fill_md5(recs, zs, si, rec, ring->tile_cap, ring->arena_cap, ps, ac, flush, f);
        if (frc || refused) return frc ? frc : fail(HBEC_ERR_INVALID_ARG, refused);
        more = si < zs.size();
        hipError_t e = hipMemcpyAsync(ring->dev_tiles[slot], rec, (f.n_main + f.n_edge) * sizeof(Rec),
                                      hipMemcpyHostToDevice, ring->s_cmp);
        if (e != hipSuccess) return hip_fail(e, "zero-copy records H2D");
        g_zc_record_slots.fetch_add(1, std::memory_order_relaxed);
        return launch(reinterpret_cast<const Rec*>(ring->dev_tiles[slot]), f);
    });
    if (!rc && ps.d_digest) rc = ac.finish();
    if (rc) return rc;
    const hipError_t e = hipStreamSynchronize(ring->s_cmp);
    return e != hipSuccess ? hip_fail(e, "zero-copy drain") : HBEC_OK;
}

// 16-B aligned stripes of S % 16 == 0: the stripes kernel (hashing: StripeArgs::mirror)
int zero_copy_aligned(Ring* ring, const std::vector<ZcStripe>& zs, const Pass& ps) {
    const cut::TileRecs recs{(uint64_t)hbec::stripes_tile_bytes(std::min((int)ps.in_idx.size(), hbec::kStripeMaxK))};
    return zero_copy_run(ring, recs, zs, ps, [&](const hbec::TileRec* d_rec, const cut::SlotFill& f) {
        return hbec::launch_stripe_passes(d_rec, f.n_main, ps.in_idx, ps.out_idx, ps.rows, 0, ring->s_cmp,
                                          zero_copy_blocks_per_cu(), ps.d_digest != nullptr, zero_copy_max_blocks());
    });
}

// Any alignment / shard length (15 object sizes in 16: ecSplit's S = ceil(len / k)):
// gf_apply_unaligned_plan records.  Hashing: the mirrored gf_odd plan kernel stores
// shard i 16-B aligned at arena + i * odd_mirror_pitch_host(S); gf_odd_mirror_copy
// adds the guard-band bytes (<= 160 per shard) afterwards.
int zero_copy_unaligned(Ring* ring, const std::vector<ZcStripe>& zs, const Pass& ps) {
    const bool mirror = ps.d_digest != nullptr;
    const cut::URecs recs{hbec::urec_tile_for(std::min((int)ps.in_idx.size(), hbec::kOddMaxK), mirror), hbec::urec_span,
                          hbec::odd_mirror_pitch_host, hbec::odd_enabled()};
    return zero_copy_run(ring, recs, zs, ps, [&](const hbec::URec* d_rec, const cut::SlotFill& f) {
        return hbec::launch_unaligned_passes(d_rec, f.n_main, ps.in_idx, ps.out_idx, ps.rows, 0, ring->s_cmp,
                                             zero_copy_max_blocks(), d_rec + f.n_main, f.n_edge, mirror);
    });
}

std::atomic<uint64_t> g_md5_zc_calls{0}, g_md5_ring_calls{0};

bool zero_copy_md5_enabled() {
    static const bool on = hbec::tune_knob("HBEC_MD5_ZEROCOPY", 1) != 0;
    return on;
}

// A call that fails part-way may leave work queued on the ring's streams
// (slot copies, kernels writing a hash arena, hashes); the next caller of
// the ring reuses slots only after their events, but starts over at hash
// arena 0, so a failed call drains every stream before the ring goes back.
void ring_drain(Ring* r) {
    for (hipStream_t s : {r->s_h2d, r->s_cmp, r->s_d2h})
        if (s) (void)hipStreamSynchronize(s);
    for (hipStream_t s : r->s_md5)
        if (s) (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
}

// A ring of the calling thread's device for the length of fn(ring).
template <class Fn>
int with_ring(Fn fn) {
    Ring* ring = nullptr;
    int rc = ring_acquire(&ring);
    if (rc) return rc;
    struct Back {
        Ring* r;
        bool ok;
        ~Back() {
            if (!ok) ring_drain(r);  // also when fn threw
            ring_release(r);
        }
    } back{ring, false};
    rc = fn(ring);
    back.ok = rc == HBEC_OK;
    return rc;
}

using Pieces = std::vector<cut::Piece>;

// The CPU copies of a chunk (thread pool): gather shards idx of the pieces into
// the pinned IN slot, packed 0.. per piece and zero-padded to lpad, or hand the
// pinned OUT slot's shards, packed likewise, back to the caller's stripes.
void ring_copy(Ring* ring, int slot, const Pieces& pieces, const hbec_stripe* stripes, const std::vector<int>& idx,
               bool gather) {
    const size_t n = idx.size();
    ring->pool->parallel_for(pieces.size() * n, [&](size_t i) {
        const cut::Piece& p = pieces[i / n];
        const size_t j = i % n;
        const hbec_stripe& st = stripes[p.stripe];
        uint8_t* mem = static_cast<uint8_t*>(st.base) + (uint64_t)idx[j] * st.shard_len + p.col;
        uint8_t* pin = (gather ? ring->pin_in[slot] + p.in_off : ring->pin_out[slot] + p.out_off) + j * p.lpad;
        std::memcpy(gather ? pin : mem, gather ? mem : pin, p.len);
        if (gather && p.lpad > p.len) std::memset(pin + p.len, 0, p.lpad - p.len);
    });
}

// the chunk's shards -> hash arena (D2D on the compute stream, before the slot is released)
int ring_hash_chunk(ArenaCursor& ac, int slot, const Pieces& pieces, uint64_t in_bytes, uint64_t out_bytes,
                    const Pass& ps) {
    Ring* ring = ac.ring;
    const size_t K = ps.in_idx.size(), R = ps.out_idx.size();
    if (!ac.fits(in_bytes + out_bytes, pieces.size() * (uint64_t)(K + R))) {
        const int rc = ac.flush();
        if (rc) return rc;
    }
    const uint64_t ain = ac.base(), aout = ain + in_bytes;
    hipError_t e = hipMemcpyAsync(reinterpret_cast<void*>(ain), ring->dev_in[slot], in_bytes, hipMemcpyDeviceToDevice,
                                  ring->s_cmp);
    if (e == hipSuccess)
        e = hipMemcpyAsync(reinterpret_cast<void*>(aout), ring->dev_out[slot], out_bytes, hipMemcpyDeviceToDevice,
                           ring->s_cmp);
    if (e != hipSuccess) return hip_fail(e, "hash arena copy");
    const uint64_t n_shards = (uint64_t)ps.n_shards;
    for (const cut::Piece& p : pieces) {
        for (size_t j = 0; j < K; ++j)
            ac.add(ain + p.in_off + (uint64_t)j * p.lpad, p.len, p.stripe * n_shards + (uint64_t)ps.in_idx[j]);
        for (size_t r = 0; r < R; ++r)
            ac.add(aout + p.out_off + (uint64_t)r * p.lpad, p.len, p.stripe * n_shards + (uint64_t)ps.out_idx[r]);
    }
    ac.used += (in_bytes + out_bytes + 255) & ~uint64_t(255);
    return HBEC_OK;
}

// The staging ring: chunks of column pieces through kSlots slots, each gathered, uploaded, coded,
// with d_digest copied to a hash arena, downloaded, and scattered when its slot comes round again.
int ring_run(Ring* ring, const hbec_stripe* stripes, uint64_t n, const Pass& ps) {
    const int K = (int)ps.in_idx.size(), R = (int)ps.out_idx.size();
    int rc = ring_staging_init(*ring);
    if (rc) return rc;
    const uint64_t tile = (uint64_t)hbec::stripes_tile_bytes(std::min(K, hbec::kStripeMaxK));
    std::vector<Pieces> chunks;
    uint64_t n_pieces = 0;
    const char* refused = cut::cut_ring(stripes, n, K, R, ring->in_cap, ring->out_cap, ring->tile_cap, tile,
                                        ps.d_digest != nullptr, chunks, n_pieces);
    g_ring_pieces.fetch_add(n_pieces, std::memory_order_relaxed);
    if (refused) return fail(HBEC_ERR_INVALID_ARG, refused);
    rc = ps.d_digest ? ring_md5_init(*ring) : HBEC_OK;
    if (rc) return rc;
    ArenaCursor ac{ring, ring->s_cmp, ps.d_digest};  // hash arenas (d_digest only)

    // in the slots inputs are packed 0..K-1 and outputs 0..R-1
    std::vector<int> slot_in(K), slot_out(R);
    for (int j = 0; j < K; ++j) slot_in[j] = j;
    for (int r = 0; r < R; ++r) slot_out[r] = r;

    // chunk c's slot is free once chunk c - kSlots is back in the caller's memory; the
    // last kSlots chunks are handed back by the turns past the end
    for (size_t c = 0; c < chunks.size() + kSlots; ++c) {
        const int slot = (int)(c % kSlots);
        if (c >= kSlots) {
            hipError_t e = hipEventSynchronize(ring->ev_done[slot]);
            if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize");
            ring_copy(ring, slot, chunks[c - kSlots], stripes, ps.out_idx, false);
        }
        if (c >= chunks.size()) continue;
        const Pieces& pieces = chunks[c];
        ring_copy(ring, slot, pieces, stripes, ps.in_idx, true);
        uint64_t nt = 0, in_bytes = 0, out_bytes = 0;
        const uint64_t din = reinterpret_cast<uint64_t>(ring->dev_in[slot]);
        const uint64_t dout = reinterpret_cast<uint64_t>(ring->dev_out[slot]);
        for (const cut::Piece& p : pieces) {
            for (uint64_t off = 0; off < p.lpad; off += tile)
                ring->pin_tiles[slot][nt++] = cut::tile_rec(din + p.in_off, dout + p.out_off, p.lpad, off, p.lpad, tile);
            in_bytes = std::max(in_bytes, p.in_off + K * p.lpad);
            out_bytes = std::max(out_bytes, p.out_off + R * p.lpad);
        }
        rc = staged_upload(ring, slot, nt * sizeof(hbec::TileRec), in_bytes, "host path H2D");
        if (!rc) rc = hbec::launch_stripe_passes(ring->dev_tiles[slot], nt, slot_in, slot_out, ps.rows, 0, ring->s_cmp);
        if (!rc && ps.d_digest) rc = ring_hash_chunk(ac, slot, pieces, in_bytes, out_bytes, ps);
        if (rc) return rc;
        hipError_t e = hipEventRecord(ring->ev_cmp[slot], ring->s_cmp);
        if (e == hipSuccess) e = hipStreamWaitEvent(ring->s_d2h, ring->ev_cmp[slot], 0);
        if (e == hipSuccess)
            e = hipMemcpyAsync(ring->pin_out[slot], ring->dev_out[slot], out_bytes, hipMemcpyDeviceToHost, ring->s_d2h);
        if (e == hipSuccess) e = hipEventRecord(ring->ev_done[slot], ring->s_d2h);
        if (e != hipSuccess) return hip_fail(e, "host path D2H");
        g_ring_chunks.fetch_add(1, std::memory_order_relaxed);
    }
    return ps.d_digest ? ac.finish() : HBEC_OK;
}

// Code every stripe by pass ps (hostcut.h).  Pinned stripes are coded in place
// (zero-copy); the rest take the ring.  Hashing needs every shard on the
// device: when every stripe is pinned, the zero-copy kernel also copies them
// to a device hash arena; otherwise the whole batch takes the ring.
int host_run_on(Ring* ring, const hbec_stripe* stripes, uint64_t n, const Pass& ps) {
    const int top = cut::top_shard(ps);
    std::vector<ZcStripe> zs, zu;  // aligned (stripes kernel) / any alignment (unaligned kernel)
    if (ps.d_digest && zero_copy_enabled() && zero_copy_md5_enabled()) {
        // the mirrored gf_odd plan is the only unaligned kernel with a mirror
        const bool any_align = hbec::zero_copy_any_alignment() && hbec::odd_enabled();
        const cut::Kind all = cut::route_hashing(stripes, n, top, any_align, pinned_device_addr, zs);
        if (all != cut::Kind::staged) {
            // the same stripe bound as the ring (hbec.h: one staging slot)
            const uint64_t max_cols =
                cut::slot_cols(ring->in_cap, ring->out_cap, (int)ps.in_idx.size(), (int)ps.out_idx.size());
            if (const char* refused = cut::hash_slot_bound(zs.data(), zs.size(), max_cols))
                return fail(HBEC_ERR_INVALID_ARG, refused);
            g_md5_zc_calls.fetch_add(1, std::memory_order_relaxed);
            return all == cut::Kind::aligned ? zero_copy_aligned(ring, zs, ps) : zero_copy_unaligned(ring, zs, ps);
        }
    }
    if (ps.d_digest) g_md5_ring_calls.fetch_add(1, std::memory_order_relaxed);
    std::vector<hbec_stripe> staged;
    if (!ps.d_digest && zero_copy_enabled()) {
        cut::route_plain(stripes, n, top, hbec::zero_copy_any_alignment(), pinned_device_addr, zs, zu, staged);
        int rc = zs.empty() ? HBEC_OK : zero_copy_aligned(ring, zs, ps);
        if (!rc && !zu.empty()) rc = zero_copy_unaligned(ring, zu, ps);
        if (rc || staged.empty()) return rc;
        stripes = staged.data();
        n = staged.size();
    }
    return ring_run(ring, stripes, n, ps);
}

int host_run(const hbec_stripe* stripes, uint64_t n, const Pass& ps) {
    if (ps.out_idx.empty() || n == 0) return HBEC_OK;
    return with_ring([&](Ring* ring) { return host_run_on(ring, stripes, n, ps); });
}

// The encode pass: data shards 0..k-1 in, parity shards k..k+m-1 out by the codec's parity rows.
int encode_host_run(hbec_codec* codec, const hbec_stripe* stripes, uint64_t n, uint8_t* d_digest = nullptr) {
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
    std::vector<uint8_t> mat((size_t)(k + m) * k);
    hbec_matrix(codec, mat.data());
    Pass ps{std::vector<int>(k), std::vector<int>(m), {mat.begin() + (size_t)k * k, mat.end()}, d_digest, k + m};
    for (int j = 0; j < k; ++j) ps.in_idx[j] = j;
    for (int r = 0; r < m; ++r) ps.out_idx[r] = k + r;
    return host_run(stripes, n, ps);
}

// ---- Verify of host stripes (hbec_verify_host) ----
// Read-only, so nothing but the flags comes back.  Pinned stripes are read in
// place over PCIe by the plan Verify kernels on records over their device
// addresses.  Every other stripe is one contiguous block of (k+m) S bytes:
// one copy into the pinned IN slot at a 16-B-aligned offset, H2D, and the
// same kernels over records of the device slot; a stripe larger than a slot
// is cut into column pieces ((k+m) copies each) that OR into its flag.  A slot
// is reused once the kernel that read it is done (ev_cmp).

// queue the Verify of v: its records, already at d_rec (VRecs, then VTiles), and its other-route stripes;
// without records d_rec may be null: verify_recs_run returns before it looks at it
int verify_queue(hbec_codec* codec, const hbec::VerifyRecs& v, const void* d_rec, const uint32_t* d_tab,
                 uint32_t* d_flags, hipStream_t st, int max_blocks = 0) {
    const uint8_t* r = static_cast<const uint8_t*>(d_rec);
    int rc = hbec::verify_recs_run(codec, reinterpret_cast<const hbec::VRec*>(r), v.recs.size(),
                                   reinterpret_cast<const hbec::VTile*>(r + v.recs.size() * sizeof(hbec::VRec)),
                                   v.tiles.size(), d_tab, d_flags, st, max_blocks);
    for (size_t i = 0; i < v.other.size() && !rc; ++i) rc = hbec::verify_other_run(codec, v.other[i], d_flags, st);
    return rc;
}

int verify_staged(Ring* ring, hbec_codec* codec, const hbec_stripe* stripes, const std::vector<uint64_t>& staged,
                  const uint32_t* d_tab, uint32_t* d_flags) {
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
    const uint64_t L = (uint64_t)(k + m);
    int rc = ring_staging_init(*ring);
    if (rc) return rc;
    std::vector<std::vector<cut::VPiece>> chunks;
    if (const char* refused = cut::cut_verify(stripes, staged, L, ring->in_cap,
                                              (uint64_t)ring->tile_cap * sizeof(hbec::TileRec), chunks))
        return fail(HBEC_ERR_INVALID_ARG, refused);
    size_t c = 0;
    return walk_slots(ring, "verify host slot wait", "verify host event", [&](int slot, bool& more) -> int {
        const auto& pieces = chunks[c++];
        more = c < chunks.size();
        ring->pool->parallel_for(pieces.size(), [&](size_t i) {
            const cut::VPiece& p = pieces[i];
            const uint8_t* src = static_cast<const uint8_t*>(stripes[p.stripe].base);
            uint8_t* dst = ring->pin_in[slot] + p.off;
            const uint64_t S = stripes[p.stripe].shard_len;
            if (p.whole) std::memcpy(dst, src, L * p.len);
            for (uint64_t j = 0; j < L && !p.whole; ++j) std::memcpy(dst + j * p.len, src + j * S + p.col, p.len);
        });
        const uint64_t din = reinterpret_cast<uint64_t>(ring->dev_in[slot]);
        hbec::VerifyRecs vr;
        uint64_t in_bytes = 0;
        for (const cut::VPiece& p : pieces) {
            (void)hbec::vp_add(vr, k, m, din + p.off, din + p.off + (uint64_t)k * p.len, p.len, p.stripe);
            in_bytes = std::max(in_bytes, p.off + L * p.len);
        }
        const size_t rb = vr.recs.size() * sizeof(hbec::VRec), tb = vr.tiles.size() * sizeof(hbec::VTile);
        uint8_t* prec = reinterpret_cast<uint8_t*>(ring->pin_tiles[slot]);
        if (rb) std::memcpy(prec, vr.recs.data(), rb);
        if (tb) std::memcpy(prec + rb, vr.tiles.data(), tb);
        const int rc = staged_upload(ring, slot, rb + tb, in_bytes, "verify host H2D");
        if (rc) return rc;
        return verify_queue(codec, vr, ring->dev_tiles[slot], d_tab, d_flags, ring->s_cmp);
    });
}

int verify_host_run_on(Ring* ring, hbec_codec* codec, const hbec_stripe* stripes, uint64_t n, uint8_t* flags) {
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
    const uint64_t L = (uint64_t)(k + m);
    hipStream_t st = ring->s_cmp;
    hbec::VerifyRecs zc;  // pinned stripes
    std::vector<uint64_t> staged;
    for (uint64_t s = 0; s < n; ++s) {
        const uint64_t S = stripes[s].shard_len;
        if (S == 0) continue;
        const uint64_t d = pinned_device_addr(stripes[s].base, L * S);
        if (!d) staged.push_back(s);
        else if (!hbec::vp_add(zc, k, m, d, d + (uint64_t)k * S, S, s))
            return fail(HBEC_ERR_INVALID_ARG, "too many tiles in one call");
    }
    // device flags, then the coefficient tables (stream-ordered scratch)
    std::vector<uint32_t> tab;
    if (hbec::vp_fast_shape(k, m)) hbec::verify_tab(codec, tab);
    const size_t flag_bytes = ((size_t)n * 4 + 15) & ~(size_t)15;
    void* d_mem = nullptr;
    int rc = hbec::scratch_alloc(flag_bytes + tab.size() * 4, st, &d_mem);
    if (rc) return rc;
    struct Scratch {
        std::vector<void*> p;
        hipStream_t s;
        ~Scratch() {
            for (void* q : p) hbec::scratch_free(q, s);
        }
    } scratch{{d_mem}, st};
    uint32_t* d_flags = static_cast<uint32_t*>(d_mem);
    const uint32_t* d_tab = reinterpret_cast<const uint32_t*>(static_cast<uint8_t*>(d_mem) + flag_bytes);
    hipError_t e = hipMemsetAsync(d_flags, 0, (size_t)n * 4, st);
    if (e == hipSuccess && !tab.empty()) e = hbec::launch_put_words(const_cast<uint32_t*>(d_tab), tab.data(), tab.size() * 4, st);
    if (e != hipSuccess) return hip_fail(e, "verify host flags");

    void* d_rec = nullptr;
    if (!zc.recs.empty()) {
        const size_t rb = zc.recs.size() * sizeof(hbec::VRec), tb = zc.tiles.size() * sizeof(hbec::VTile);
        rc = hbec::scratch_alloc(rb + tb, st, &d_rec);
        if (rc) return rc;
        scratch.p.push_back(d_rec);
        e = hipMemcpyAsync(d_rec, zc.recs.data(), rb, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && tb)
            e = hipMemcpyAsync(static_cast<uint8_t*>(d_rec) + rb, zc.tiles.data(), tb, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return hip_fail(e, "verify host records H2D");
    }
    rc = verify_queue(codec, zc, d_rec, d_tab, d_flags, st, zero_copy_max_blocks());
    if (rc) return rc;

    if (!staged.empty()) {
        rc = verify_staged(ring, codec, stripes, staged, d_tab, d_flags);
        if (rc) return rc;
    }
    std::vector<uint32_t> h(n);
    e = hipMemcpyAsync(h.data(), d_flags, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "verify host flags D2H");
    for (uint64_t s = 0; s < n; ++s) flags[s] = h[s] ? 1 : 0;
    return HBEC_OK;
}

// One process, several GPUs (how a single object server would use a node):
// stripes are cut into contiguous runs of about equal bytes, one per device,
// and each run is coded by its own host thread on its device's ring (rings
// are per device), all at once.  Stripes are independent (ecutils.go:38-70),
// so there is no exchange between devices.
template <typename Fn>
int run_on_devices(const hbec_stripe* stripes, uint64_t n, const int* devices, int n_devices, Fn fn) {
    if (n && !stripes) return fail(HBEC_ERR_INVALID_ARG, "null argument");
    std::vector<int> devs;
    if (devices) {
        if (n_devices <= 0) return fail(HBEC_ERR_INVALID_ARG, "n_devices must be > 0");
        devs.assign(devices, devices + n_devices);
    } else {
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
        for (int d = 0; d < count; ++d) devs.push_back(d);
        if (n_devices > 0 && n_devices < count) devs.resize(n_devices);
    }
    if (devs.empty()) return fail(HBEC_ERR_DEVICE, "no device");
    if (n == 0) return HBEC_OK;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) total += stripes[i].shard_len;
    // contiguous runs of ~total / D shard bytes
    std::vector<uint64_t> cut(devs.size() + 1, n);
    cut[0] = 0;
    {
        uint64_t acc = 0;
        size_t d = 1;
        for (uint64_t i = 0; i < n && d < devs.size(); ++i) {
            acc += stripes[i].shard_len;
            while (d < devs.size() && acc * devs.size() >= total * d) cut[d++] = i + 1;
        }
    }
    std::vector<int> rcs(devs.size(), HBEC_OK);
    std::vector<std::string> errs(devs.size());
    std::vector<std::thread> th;
    for (size_t d = 0; d < devs.size(); ++d) {
        if (cut[d + 1] <= cut[d]) continue;
        th.emplace_back([&, d] {
            hipError_t e = hipSetDevice(devs[d]);
            if (e != hipSuccess) {
                rcs[d] = hip_fail(e, "hipSetDevice");
            } else {
                rcs[d] = fn(stripes + cut[d], cut[d + 1] - cut[d]);
            }
            if (rcs[d]) errs[d] = hbec_last_error();
        });
    }
    for (auto& t : th) t.join();
    for (size_t d = 0; d < devs.size(); ++d)
        if (rcs[d]) return fail(rcs[d], "device " + std::to_string(devs[d]) + ": " + errs[d]);
    return HBEC_OK;
}

}  // namespace

uint64_t hbec::host_md5_max_shard(const hbec_codec* codec) {
    const uint64_t slot = env_size("HBEC_HOST_SLOT_MB", 64) << 20;  // as ring_init
    const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec);
    if (k < 1 || m < 1) return 0;
    return (std::min(slot / (uint64_t)k, slot / (uint64_t)m) / 16) * 16;
}

int hbec::host_threads() {
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t share = env_size("OMP_NUM_THREADS", 16);
    const size_t want = std::min<size_t>(env_size("HBEC_HOST_THREADS", share), hw);
    return (int)std::max<size_t>(1, want);
}

extern "C" {

int hbec_host_alloc(size_t bytes, void** out) {
    return hbec::guarded("hbec_host_alloc", [&]() -> int {
        if (!out || bytes == 0) return fail(HBEC_ERR_INVALID_ARG, "null out or zero size");
        *out = nullptr;
        void* h = nullptr;
        // portable + mapped: every device of the process may code it in place
        // (coherent or non-coherent flags measured the same: 46.2-46.4 GiB/s)
        hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocPortable | hipHostMallocMapped);
        if (e != hipSuccess) return hip_fail(e, "hipHostMalloc");
        void* d = nullptr;
        e = hipHostGetDevicePointer(&d, h, 0);
        if (e != hipSuccess || !d) {
            (void)hipHostFree(h);
            return hip_fail(e != hipSuccess ? e : hipErrorInvalidValue, "hipHostGetDevicePointer");
        }
        {
            std::lock_guard<std::mutex> g(g_pin_mu);
            g_pinned[reinterpret_cast<uint64_t>(h)] = PinnedRange{(uint64_t)bytes, reinterpret_cast<uint64_t>(d)};
        }
        *out = h;
        return HBEC_OK;
    });
}

void hbec_host_free(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_pin_mu);
        g_pinned.erase(reinterpret_cast<uint64_t>(p));
    }
    (void)hipHostFree(p);
}

int hbec_host_device_addr(const void* p, uint64_t len, uint64_t* dev) {
    return hbec::guarded("hbec_host_device_addr", [&]() -> int {
        if (!dev) return fail(HBEC_ERR_INVALID_ARG, "null out");
        *dev = pinned_device_addr(p, len);
        return HBEC_OK;
    });
}

int hbec_encode_host(hbec_codec* codec, const hbec_stripe* stripes, uint64_t n_stripes) {
    return hbec::guarded("hbec_encode_host", [&]() -> int {
        if (!codec || (n_stripes && !stripes)) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        if (hbec_parity_shards(codec) == 0) return HBEC_OK;
        return encode_host_run(codec, stripes, n_stripes);
    });
}

int hbec_encode_host_md5(hbec_codec* codec, const hbec_stripe* stripes, uint64_t n_stripes, uint8_t* digests) {
    return hbec::guarded("hbec_encode_host_md5", [&]() -> int {
        if (!codec || !digests || (n_stripes && !stripes)) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        if (n_stripes == 0) return HBEC_OK;
        const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
        if (m == 0) return fail(HBEC_ERR_INVALID_ARG, "encode_host_md5 needs parity shards");
        for (uint64_t s = 0; s < n_stripes; ++s)
            if (stripes[s].shard_len == 0) return fail(HBEC_ERR_SHARD_NO_DATA, "stripe with zero shard length");
        hipStream_t st = nullptr;
        int rc0 = stream_acquire(&st);
        if (rc0) return rc0;
        struct StreamBack {
            hipStream_t s;
            ~StreamBack() { stream_release(s); }
        } back{st};
        hipError_t e = hipSuccess;
        void* d_dig = nullptr;
        const size_t bytes = (size_t)n_stripes * n * 16;
        int rc = hbec::scratch_alloc(bytes, st, &d_dig);
        if (!rc) {
            e = hipStreamSynchronize(st);  // allocation visible to the ring's streams
            if (e != hipSuccess) rc = hip_fail(e, "scratch");
        }
        if (!rc) rc = encode_host_run(codec, stripes, n_stripes, static_cast<uint8_t*>(d_dig));
        if (!rc) {
            e = hipMemcpyAsync(digests, d_dig, bytes, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) rc = hip_fail(e, "digests D2H");
        }
        hbec::scratch_free(d_dig, st);
        (void)hipStreamSynchronize(st);
        return rc;
    });
}

int hbec_host_md5_stats(uint64_t* zero_copy_calls, uint64_t* ring_calls) {
    if (zero_copy_calls) *zero_copy_calls = g_md5_zc_calls.load(std::memory_order_relaxed);
    if (ring_calls) *ring_calls = g_md5_ring_calls.load(std::memory_order_relaxed);
    return HBEC_OK;
}

int hbec_host_run_stats(uint64_t* ring_chunks, uint64_t* ring_pieces, uint64_t* zc_record_slots,
                        uint64_t* arena_flushes) {
    if (ring_chunks) *ring_chunks = g_ring_chunks.load(std::memory_order_relaxed);
    if (ring_pieces) *ring_pieces = g_ring_pieces.load(std::memory_order_relaxed);
    if (zc_record_slots) *zc_record_slots = g_zc_record_slots.load(std::memory_order_relaxed);
    if (arena_flushes) *arena_flushes = g_arena_flushes.load(std::memory_order_relaxed);
    return HBEC_OK;
}

int hbec_device_count(int* n) {
    return hbec::guarded("hbec_device_count", [&]() -> int {
        if (!n) return fail(HBEC_ERR_INVALID_ARG, "null out");
        *n = 0;
        hipError_t e = hipGetDeviceCount(n);
        if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
        return HBEC_OK;
    });
}

int hbec_set_device(int device) {
    return hbec::guarded("hbec_set_device", [&]() -> int {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
        return HBEC_OK;
    });
}

int hbec_encode_host_devices(hbec_codec* codec, const hbec_stripe* stripes, uint64_t n_stripes, const int* devices,
                             int n_devices) {
    return hbec::guarded("hbec_encode_host_devices", [&]() -> int {
        return run_on_devices(stripes, n_stripes, devices, n_devices, [codec](const hbec_stripe* s, uint64_t n) {
            return hbec_encode_host(codec, s, n);
        });
    });
}

int hbec_reconstruct_host_devices(hbec_codec* codec, const hbec_stripe* stripes, uint64_t n_stripes,
                                  const uint8_t* present, int data_only, const int* devices, int n_devices) {
    return hbec::guarded("hbec_reconstruct_host_devices", [&]() -> int {
        if (!present) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        return run_on_devices(stripes, n_stripes, devices, n_devices, [=](const hbec_stripe* s, uint64_t n) {
            return hbec_reconstruct_host(codec, s, n, present, data_only);
        });
    });
}

int hbec_reconstruct_host(hbec_codec* codec, const hbec_stripe* stripes, uint64_t n_stripes,
                          const uint8_t* present, int data_only) {
    return hbec::guarded("hbec_reconstruct_host", [&]() -> int {
        if (!codec || !present || (n_stripes && !stripes)) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        const int k = hbec_data_shards(codec), m = hbec_parity_shards(codec), n = k + m;
        int n_present = 0, data_present = 0;
        for (int i = 0; i < n; ++i) {
            n_present += present[i] ? 1 : 0;
            if (i < k) data_present += present[i] ? 1 : 0;
        }
        if (n_present == n || (data_only && data_present == k)) return HBEC_OK;
        if (n_present < k) return fail(HBEC_ERR_TOO_FEW_SHARDS, "too few shards given");
        std::vector<int> surv(k), outs(n);
        std::vector<uint8_t> rows((size_t)n * k);
        int n_out = 0;
        int rc = hbec_decode_rows(codec, present, data_only, surv.data(), outs.data(), &n_out, rows.data());
        if (rc) return rc;
        outs.resize(n_out);
        rows.resize((size_t)n_out * k);
        return host_run(stripes, n_stripes, Pass{surv, outs, rows});
    });
}

int hbec_verify_host(hbec_codec* codec, const hbec_stripe* stripes, uint64_t n_stripes, uint8_t* flags) {
    return hbec::guarded("hbec_verify_host", [&]() -> int {
        if (!codec || (n_stripes && (!stripes || !flags))) return fail(HBEC_ERR_INVALID_ARG, "null argument");
        if (n_stripes >= (1ull << 32)) return fail(HBEC_ERR_INVALID_ARG, "too many stripes in one call");
        bool any = false;
        for (uint64_t s = 0; s < n_stripes; ++s) {
            if (stripes[s].shard_len && !stripes[s].base) return fail(HBEC_ERR_INVALID_ARG, "stripe with null base");
            any = any || stripes[s].shard_len != 0;
        }
        if (n_stripes) std::memset(flags, 0, n_stripes);
        if (hbec_parity_shards(codec) == 0 || !any) return HBEC_OK;
        return with_ring([&](Ring* ring) { return verify_host_run_on(ring, codec, stripes, n_stripes, flags); });
    });
}

}  // extern "C"
