// Host-only checks of the host path's cutting rules (csrc/hostcut.h; no GPU work
// and no libhbec): the ring's column pieces and chunks, the chunks of a staged
// Verify, the records of a zero-copy slot (plain and hashing, both record
// kinds) and the stripe classifier with its two policies, at capacities of a
// few KiB so that every seam is a few hundred bytes away.  Every property is
// checked against a restatement written here, never against the cutter's own
// output.  Built with the host compiler under AddressSanitizer + UBSan by
// tests/test_host_cut.py and run directly; the slot buffers are heap vectors
// of exactly tile_cap records, so a record too many is an ASan report.
#include <array>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../hummingbird_amd/csrc/hostcut.h"

using namespace hbec;
using namespace hbec::cut;

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static long g_cases = 0;
static const uint64_t kTile = 64, kTileCap = 8;
static uint64_t up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }
static uint64_t ceil_div(uint64_t v, uint64_t a) { return (v + a - 1) / a; }
static void* fake(uint64_t a) { return reinterpret_cast<void*>(a); }
static bool is(const char* got, const char* want) { return got && std::strcmp(got, want) == 0; }

// ---------------------------------------------------------------- ring cutter
static int ring_case(const std::vector<uint64_t>& lens, int K, int R, uint64_t in_cap, uint64_t out_cap,
                     uint64_t tile_cap, uint64_t tile, std::vector<std::vector<Piece>>* out = nullptr) {
    std::vector<hbec_stripe> st;
    for (size_t i = 0; i < lens.size(); ++i) st.push_back({lens[i] ? fake(0x1000 + 16 * i) : nullptr, lens[i]});
    const uint64_t W = std::min(in_cap / (uint64_t)K, out_cap / (uint64_t)R) / 16 * 16;
    // greedy restatement: a chunk is closed by the first piece that does not fit it
    uint64_t pieces = 0, n_chunks = 0, in_used = 0, out_used = 0, tiles = 0;
    for (uint64_t S : lens)
        for (uint64_t col = 0; col < S; col += W, ++pieces) {
            const uint64_t lpad = up(std::min(W, S - col), 16), nt = ceil_div(lpad, tile);
            if (in_used && (in_used + K * lpad > in_cap || out_used + R * lpad > out_cap || tiles + nt > tile_cap)) {
                ++n_chunks;
                in_used = out_used = tiles = 0;
            }
            in_used += K * lpad, out_used += R * lpad, tiles += nt;
        }
    n_chunks += in_used ? 1 : 0;
    uint64_t by_width = 0;
    for (uint64_t S : lens) by_width += ceil_div(S, W);

    std::vector<std::vector<Piece>> chunks;
    uint64_t n_pieces = ~0ull;
    CHECK(cut_ring(st.data(), st.size(), K, R, in_cap, out_cap, tile_cap, tile, false, chunks, n_pieces) == nullptr);
    CHECK(n_pieces == pieces && pieces == by_width && chunks.size() == n_chunks);
    std::vector<uint64_t> next(lens.size(), 0);  // every column once and in order
    uint64_t last_stripe = 0;
    for (const auto& ch : chunks) {
        CHECK(!ch.empty());
        uint64_t in_end = 0, out_end = 0, nt = 0;
        for (const Piece& p : ch) {
            CHECK(p.stripe < lens.size() && p.stripe >= last_stripe && p.col == next[p.stripe]);
            last_stripe = p.stripe;
            CHECK(p.len > 0 && p.len == std::min(W, lens[p.stripe] - p.col) && p.lpad == up(p.len, 16));
            next[p.stripe] += p.len;
            CHECK(p.in_off >= in_end && p.out_off >= out_end);  // disjoint, in order
            in_end = p.in_off + K * p.lpad, out_end = p.out_off + R * p.lpad;
            nt += ceil_div(p.lpad, tile);
        }
        CHECK(in_end <= in_cap && out_end <= out_cap && nt <= tile_cap);
    }
    for (size_t i = 0; i < lens.size(); ++i) CHECK(next[i] == lens[i]);
    if (out) *out = chunks;
    ++g_cases;
    return 0;
}

static const int kShapes[4][2] = {{4, 2}, {3, 5}, {10, 4}, {1, 1}};

static int ring_cutter() {
    for (const auto& s : kShapes) {
        const int K = s[0], R = s[1];
        const uint64_t W = std::min(4096 / K, 4096 / R) / 16 * 16;
        for (uint64_t S = 0; S <= 3 * W + 17; ++S)
            if (ring_case({S, 33, 0, S}, K, R, 4096, 4096, 200, kTile)) return 1;
    }
    std::vector<std::vector<Piece>> ch;
    // IN bytes: four stripes of 4 x 256 fill the slot exactly, the fifth opens the next
    if (ring_case(std::vector<uint64_t>(5, 256), 4, 2, 4096, 4096, 1000, kTile, &ch)) return 1;
    CHECK(ch.size() == 2 && ch[0].size() == 4 && ch[0][3].in_off + 4 * 256 == 4096);
    // OUT bytes (R > K): five stripes of 5 x 160 fill a 4000-byte OUT slot exactly
    if (ring_case(std::vector<uint64_t>(6, 160), 3, 5, 4096, 4000, 1000, kTile, &ch)) return 1;
    CHECK(ch.size() == 2 && ch[0].size() == 5 && ch[0][4].out_off + 5 * 160 == 4000);
    // tile records: one per 16-byte stripe
    if (ring_case(std::vector<uint64_t>(kTileCap + 1, 16), 4, 2, 4096, 4096, kTileCap, kTile, &ch)) return 1;
    CHECK(ch.size() == 2 && ch[0].size() == kTileCap && ch[1].size() == 1);
    // refusals
    uint64_t n_pieces = 0;
    hbec_stripe st[3] = {{fake(0x1000), 2000}, {nullptr, 5}, {fake(0x9000), 5}};
    CHECK(is(cut_ring(st, 3, 4, 2, 4096, 4096, 200, kTile, false, ch, n_pieces), "stripe with null base"));
    CHECK(n_pieces == 2);  // what was cut before it
    ++g_cases;
    CHECK(is(cut_ring(st, 1, 300, 1, 4096, 4096, 200, kTile, false, ch, n_pieces), "staging slot too small"));
    CHECK(is(cut_ring(st, 1, 1, 300, 4096, 4096, 200, kTile, false, ch, n_pieces), "staging slot too small"));
    CHECK(cut_ring(st, 1, 256, 1, 4096, 4096, 200, kTile, false, ch, n_pieces) == nullptr);  // 16 columns
    ++g_cases;
    // hashing: a stripe as wide as a piece is taken, one byte more is refused before anything is cut
    hbec_stripe w[2] = {{fake(0x1000), 1024}, {fake(0x9000), 1025}};
    CHECK(cut_ring(w, 1, 4, 2, 4096, 4096, 200, kTile, true, ch, n_pieces) == nullptr && n_pieces == 1);
    CHECK(is(cut_ring(w, 2, 4, 2, 4096, 4096, 200, kTile, true, ch, n_pieces),
             "hashing needs every stripe to fit one staging slot"));
    CHECK(n_pieces == 0);
    CHECK(slot_cols(4096, 4096, 4, 2) == 1024 && slot_cols(4096, 4000, 3, 5) == 800);
    ++g_cases;
    return 0;
}

// ------------------------------------------------------------- zero-copy fills
// toy kernels: no main record up to 40 bytes, the last 16 bytes left to the edge record
static uint64_t toy_span(uint64_t S) { return S > 40 ? S - 16 : 0; }
static uint64_t toy_pitch(uint64_t S) { return up(S, 16) + 32; }

// stripe lengths with `total` tiles of kTile bytes between them, three ways
static std::vector<uint64_t> lens_of(uint64_t total, int pattern) {
    std::vector<uint64_t> v;
    if (pattern == 0) v.push_back(kTile * total - 7);  // one ragged stripe
    for (uint64_t left = total; pattern == 1 && left;) {  // three tiles each, the last what is left
        const uint64_t t = std::min<uint64_t>(3, left);
        v.push_back(kTile * t);
        left -= t;
    }
    for (uint64_t left = total, i = 0; pattern == 2 && left; ++i) {  // 1 and 5 tiles in turn, ragged
        const uint64_t t = std::min<uint64_t>(i % 2 ? 5 : 1, left);
        v.push_back(kTile * (t - 1) + (i % 2 ? 1 : 5));
        left -= t;
    }
    return v;
}

static std::vector<ZcStripe> stripes_of(const std::vector<uint64_t>& lens) {
    std::vector<ZcStripe> zs;
    for (size_t i = 0; i < lens.size(); ++i) zs.push_back({0x10000000ull * (i + 1) + 3 * i, lens[i]});
    return zs;
}

static bool same(const TileRec& a, const TileRec& b) {
    return a.in_addr == b.in_addr && a.out_addr == b.out_addr && a.in_stride == b.in_stride &&
           a.out_stride == b.out_stride && a.valid == b.valid && a.pad_ == b.pad_;
}
static bool same(const URec& a, const URec& b) {
    return a.a == b.a && a.b == b.b && a.shard_len == b.shard_len && a.p0 == b.p0;
}

static int plain_aligned(const std::vector<uint64_t>& lens) {
    const std::vector<ZcStripe> zs = stripes_of(lens);
    std::vector<TileRec> want;
    for (const ZcStripe& z : zs)
        for (uint64_t off = 0; off < z.shard_len; off += kTile)
            want.push_back({z.dev + off, z.dev + off, (uint32_t)z.shard_len, (uint32_t)z.shard_len,
                            (uint32_t)std::min(kTile, z.shard_len - off), 0});
    const TileRecs recs{kTile};
    std::vector<TileRec> got;
    size_t si = 0, slots = 0;
    for (uint64_t off = 0; si < zs.size(); ++slots) {
        std::vector<TileRec> slot(kTileCap);
        const SlotFill f = fill_plain(recs, zs, si, off, slot.data(), kTileCap);
        CHECK(f.n_edge == 0 && f.n_main >= 1 && f.n_main <= kTileCap);
        CHECK(f.n_main == kTileCap || si == zs.size());  // every slot but the last is full
        got.insert(got.end(), slot.begin(), slot.begin() + (long)f.n_main);
    }
    CHECK(slots == ceil_div(want.size(), kTileCap) && got.size() == want.size());
    for (size_t i = 0; i < want.size(); ++i) CHECK(same(got[i], want[i]));
    ++g_cases;
    return 0;
}

static int plain_unaligned(const std::vector<uint64_t>& lens, bool edges) {
    const std::vector<ZcStripe> zs = stripes_of(lens);
    // restated: stripe i is walked in steps of kTile while below its span (once when the span is 0);
    // a step adds its main record if there is one and, the first step with edges, the edge record
    std::vector<uint64_t> weight;
    std::vector<URec> want_main, want_edge;
    for (const ZcStripe& z : zs) {
        const uint64_t span = toy_span(z.shard_len);
        for (uint64_t off = 0; off == 0 || off < span; off += kTile) {
            weight.push_back((off < span ? 1 : 0) + (off == 0 && edges ? 1 : 0));
            if (off < span) want_main.push_back({z.dev, 0, z.shard_len, off});
        }
        if (edges) want_edge.push_back({z.dev, 0, z.shard_len, 0});
    }
    size_t want_slots = 0;
    for (size_t i = 0; i < weight.size(); ++want_slots)
        for (uint64_t total = 0; i < weight.size() && total + 1 < kTileCap;) total += weight[i++];

    const URecs recs{kTile, toy_span, toy_pitch, edges};
    std::vector<URec> got_main, got_edge;
    size_t si = 0, slots = 0;
    for (uint64_t off = 0; si < zs.size(); ++slots) {
        std::vector<URec> slot(kTileCap);
        const size_t first = si + (off ? 1 : 0);  // the first stripe that can start in this slot
        const SlotFill f = fill_plain(recs, zs, si, off, slot.data(), kTileCap);
        CHECK(f.n_main + f.n_edge <= kTileCap && (edges || f.n_edge == 0));
        CHECK(f.n_main + f.n_edge + 1 >= kTileCap || si == zs.size());
        // the edge records follow the main ones and belong to the stripes that start here, in order
        const size_t started = si + (off ? 1 : 0) - first;
        CHECK(!edges || f.n_edge == started);
        for (uint64_t e = 0; e < f.n_edge; ++e) {
            const URec& r = slot[f.n_main + e];
            CHECK(r.a == zs[first + e].dev);
            bool starts_here = toy_span(r.shard_len) == 0;
            for (uint64_t i = 0; i < f.n_main; ++i) starts_here = starts_here || (slot[i].a == r.a && slot[i].p0 == 0);
            CHECK(starts_here);
        }
        got_main.insert(got_main.end(), slot.begin(), slot.begin() + (long)f.n_main);
        got_edge.insert(got_edge.end(), slot.begin() + (long)f.n_main, slot.begin() + (long)(f.n_main + f.n_edge));
    }
    CHECK(slots == want_slots && got_main.size() == want_main.size() && got_edge.size() == want_edge.size());
    for (size_t i = 0; i < want_main.size(); ++i) CHECK(same(got_main[i], want_main[i]));
    for (size_t i = 0; i < want_edge.size(); ++i) CHECK(same(got_edge[i], want_edge[i]));
    ++g_cases;
    return 0;
}

static const uint64_t kTotals = 40;                        // tile totals 1..40: on, under, over and past 2 x the slot
static const uint64_t kEdgeOnlyRuns[5] = {1, 7, 8, 9, 20};  // stripes of span 0: more of them than a slot holds

static int plain_fills() {
    for (uint64_t total = 1; total <= kTotals; ++total)
        for (int pattern = 0; pattern < 3; ++pattern) {
            const std::vector<uint64_t> lens = lens_of(total, pattern);
            if (plain_aligned(lens)) return 1;
            for (int edges = 0; edges < 2; ++edges)
                if (plain_unaligned(lens, edges != 0)) return 1;
        }
    for (uint64_t n : kEdgeOnlyRuns)
        for (int edges = 0; edges < 2; ++edges) {
            std::vector<uint64_t> lens;
            for (uint64_t i = 0; i < n; ++i) lens.push_back(5 + i % 30);
            lens.insert(lens.begin() + (long)(n / 2), 300);  // and one with main records among them
            if (plain_unaligned(lens, edges != 0)) return 1;
        }
    return 0;
}

// the record at shard position off of stripe z that mirrors to `out`
static TileRec want_rec(const TileRec*, const ZcStripe& z, uint64_t out, uint64_t off) {
    return {z.dev + off, out + off, (uint32_t)z.shard_len, (uint32_t)z.shard_len,
            (uint32_t)std::min(kTile, z.shard_len - off), 0};
}
static URec want_rec(const URec*, const ZcStripe& z, uint64_t out, uint64_t off) { return {z.dev, out, z.shard_len, off}; }

// A cursor that reproduces ArenaCursor::fits, base, add and used; flush is the caller's.
struct ToyCursor {
    uint64_t cap, rec_cap;
    uint64_t used = 0, recs = 0;
    int arena = 0;
    std::vector<std::array<uint64_t, 3>> added;
    uint64_t base() const { return 0x100000ull * (uint64_t)(arena + 1) + used; }
    bool fits(uint64_t bytes, uint64_t n) const { return used + bytes <= cap && recs + n <= rec_cap; }
    void add(uint64_t addr, uint64_t len, uint64_t slot) {
        added.push_back({addr, len, slot});
        ++recs;
    }
};

// One hashing run: the slots filled, what each holds, the order of takes (T), flushes (F) and
// closed slots (C), the MD5 records, or the refusal, against a stripe-by-stripe restatement.
template <class Recs>
static int md5_case(const Recs& recs, bool unaligned, const std::vector<uint64_t>& lens, uint64_t arena_cap,
                    uint64_t rec_cap) {
    using Rec = typename Recs::Rec;
    const std::vector<ZcStripe> zs = stripes_of(lens);
    Pass ps;
    ps.in_idx = {1, 2, 4, 5};
    ps.out_idx = {0, 3};
    ps.n_shards = 6;
    const uint64_t shards = 6, e = unaligned ? 1 : 0;
    // restatement
    std::string want_log;
    std::vector<std::vector<Rec>> want_slots(1);
    std::vector<Rec> want_edges;
    std::vector<std::array<uint64_t, 3>> want_added;
    bool want_refused = false;
    uint64_t in_slot = 0, used = 0, n_recs = 0, arena = 0;
    auto close = [&] {
        want_slots.back().insert(want_slots.back().end(), want_edges.begin(), want_edges.end());
        want_edges.clear();
        want_slots.emplace_back();
        want_log += 'C';
        in_slot = 0;
    };
    for (size_t i = 0; i < zs.size(); ++i) {
        const uint64_t S = zs[i].shard_len, span = unaligned ? toy_span(S) : S, pitch = unaligned ? toy_pitch(S) : S;
        const uint64_t tiles = ceil_div(span, kTile), bytes = up(shards * pitch, 256);
        if (tiles + 2 * e > kTileCap || bytes > arena_cap) {
            want_refused = true;
            break;
        }
        if (in_slot && in_slot + tiles + e > kTileCap) close();
        if (used + bytes > arena_cap || n_recs + shards > rec_cap) {
            if (in_slot) close();
            want_log += 'F';
            if (n_recs) ++arena;  // a flush of nothing changes nothing
            used = n_recs = 0;
        }
        const uint64_t base = 0x100000ull * (arena + 1) + used;
        for (uint64_t off = 0; off < span; off += kTile) want_slots.back().push_back(want_rec((Rec*)nullptr, zs[i], base, off));
        if (e) want_edges.push_back(want_rec((Rec*)nullptr, zs[i], base, 0));
        for (int sh : {1, 2, 4, 5, 0, 3}) want_added.push_back({base + (uint64_t)sh * pitch, S, i * shards + (uint64_t)sh});
        want_log += 'T';
        in_slot += tiles + e, used += bytes, n_recs += shards;
    }
    if (in_slot) close();
    want_slots.pop_back();

    ToyCursor ac{arena_cap, rec_cap};
    std::string log;
    auto flush = [&] {
        log += 'F';
        if (ac.recs) ++ac.arena;
        ac.used = ac.recs = 0;
        return true;
    };
    std::vector<std::vector<Rec>> slots;
    const char* refused = nullptr;
    for (size_t si = 0; si < zs.size() && !refused;) {
        std::vector<Rec> slot(kTileCap);
        SlotFill f;
        const size_t before = si;
        refused = fill_md5(recs, zs, si, slot.data(), kTileCap, arena_cap, ps, ac, flush, f);
        if (refused) break;
        CHECK(si > before && f.n_main + f.n_edge <= kTileCap && f.n_edge == e * (si - before));  // whole stripes
        log += std::string(si - before, 'T') + 'C';
        slot.resize(f.n_main + f.n_edge);
        slots.push_back(slot);
    }
    CHECK(want_refused == (refused != nullptr));
    if (refused) CHECK(is(refused, "stripe too large for a hash arena"));
    if (!refused) {
        CHECK(log == want_log && slots.size() == want_slots.size() && ac.used == used && ac.recs == n_recs);
        for (size_t s = 0; s < slots.size(); ++s) {
            CHECK(slots[s].size() == want_slots[s].size());
            for (size_t i = 0; i < slots[s].size(); ++i) CHECK(same(slots[s][i], want_slots[s][i]));
        }
        CHECK(ac.added == want_added);
    }
    ++g_cases;
    return 0;
}

static const uint64_t kMd5Sweep = 600, kMd5Lists = 30;

static int md5_fills() {
    const TileRecs tr{kTile};
    const URecs ur{kTile, toy_span, toy_pitch, true};
    uint64_t rng = 12345;
    auto rnd = [&](uint64_t n) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        return (rng >> 33) % n;
    };
    for (int unaligned = 0; unaligned < 2; ++unaligned) {
        auto run = [&](const std::vector<uint64_t>& lens, uint64_t arena_cap, uint64_t rec_cap) {
            return unaligned ? md5_case(ur, true, lens, arena_cap, rec_cap) : md5_case(tr, false, lens, arena_cap, rec_cap);
        };
        // one stripe of every length: the last that fits the arena (2048 B) and the slot (a large
        // arena) is taken, one byte more is refused
        for (uint64_t S = 1; S <= kMd5Sweep; ++S)
            for (uint64_t arena_cap : {2048ull, 1ull << 20})
                if (run({300, S, 64}, arena_cap, 1000)) return 1;
        // arenas closed by their 16 MD5 records, and by their bytes
        if (run(std::vector<uint64_t>(12, 64), 2048, 16) || run(std::vector<uint64_t>(12, 64), 2048, 1000)) return 1;
        // stripes with an edge record and no main record (unaligned), more than a slot holds
        std::vector<uint64_t> tiny;
        for (uint64_t i = 0; i < 20; ++i) tiny.push_back(5 + i % 30);
        if (run(tiny, 1 << 20, 1000)) return 1;
        for (uint64_t l = 0; l < kMd5Lists; ++l) {
            std::vector<uint64_t> lens;
            for (int i = 0; i < 20; ++i) lens.push_back(1 + rnd(i % 4 ? 120 : 300));
            if (run(lens, 2048, 16) || run(lens, 2048, 1000)) return 1;
        }
    }
    return 0;
}

// --------------------------------------------------------------- verify cutter
static uint64_t vrec_restated(uint64_t len) {
    const uint64_t main_bytes = len >= 32 ? (len - 16) / 16 * 16 : 0;
    return 24 + ceil_div(main_bytes, kVpTile) * 8;
}

static int verify_case(const std::vector<uint64_t>& lens, uint64_t L, uint64_t in_cap, uint64_t rec_cap,
                       size_t* n_chunks = nullptr) {
    std::vector<hbec_stripe> st;
    std::vector<uint64_t> staged;
    for (size_t i = 0; i < lens.size(); ++i) {
        st.push_back({fake(0x1000 + i), lens[i]});
        if (lens[i]) staged.push_back(i);
    }
    const uint64_t W = in_cap / L / 16 * 16;
    uint64_t want_chunks = 0, used = 0, rused = 0;
    for (uint64_t S : lens) {
        const uint64_t step = L * S <= in_cap ? S : W;
        for (uint64_t col = 0; col < S; col += step) {
            const uint64_t len = std::min(step, S - col), bytes = up(L * len, 16), rb = vrec_restated(len);
            if (used && (used + bytes > in_cap || rused + rb > rec_cap)) {
                ++want_chunks;
                used = rused = 0;
            }
            used += bytes, rused += rb;
        }
    }
    want_chunks += used ? 1 : 0;
    std::vector<std::vector<VPiece>> chunks;
    CHECK(cut_verify(st.data(), staged, L, in_cap, rec_cap, chunks) == nullptr);
    CHECK(chunks.size() == want_chunks);
    std::vector<uint64_t> next(lens.size(), 0);
    for (const auto& ch : chunks) {
        CHECK(!ch.empty());
        uint64_t end = 0, rb = 0;
        for (const VPiece& p : ch) {
            const uint64_t S = lens[p.stripe];
            CHECK(p.whole == (L * S <= in_cap) && p.col == next[p.stripe]);
            CHECK(p.len == (p.whole ? S : std::min(W, S - p.col)) && p.len > 0);
            next[p.stripe] += p.len;
            CHECK(p.off % 16 == 0 && p.off >= end);  // 16-B aligned blocks, disjoint
            end = p.off + up(L * p.len, 16);
            rb += vrec_restated(p.len);
        }
        CHECK(end <= in_cap && rb <= rec_cap);
    }
    for (size_t i = 0; i < lens.size(); ++i) CHECK(next[i] == lens[i]);
    if (n_chunks) *n_chunks = chunks.size();
    ++g_cases;
    return 0;
}

static const uint64_t kVerifyL[3] = {6, 3, 4};  // 4 x 1024 is exactly a slot

static int verify_cutter() {
    static_assert(sizeof(VRec) == 24 && sizeof(VTile) == 8, "restated record sizes");
    for (uint64_t L : kVerifyL) {
        const uint64_t W = 4096 / L / 16 * 16;
        for (uint64_t S = 1; S <= 3 * W + 17; ++S)
            if (verify_case({S, 40, 0, S}, L, 4096, 256)) return 1;
    }
    size_t n = 0;
    // 48-byte blocks: ten records of 24 B close a chunk long before its bytes do
    if (verify_case(std::vector<uint64_t>(40, 8), 6, 4096, 256, &n)) return 1;
    CHECK(n == 4);
    // 608-byte blocks: six fill a chunk by bytes
    if (verify_case(std::vector<uint64_t>(13, 100), 6, 4096, 1 << 20, &n)) return 1;
    CHECK(n == 3);
    std::vector<std::vector<VPiece>> chunks;
    hbec_stripe st = {fake(0x1000), 100};
    CHECK(is(cut_verify(&st, {0}, 300, 4096, 256, chunks), "staging slot too small"));
    ++g_cases;
    return 0;
}

// ------------------------------------------------------------------ classifier
struct ToyPinned {
    // [lo, hi) of host memory is pinned at device address dev
    struct Range {
        uint64_t lo, hi, dev;
    };
    std::vector<Range> ranges;
    mutable long calls = 0;
    uint64_t operator()(const void* p, uint64_t len) const {
        ++calls;
        const uint64_t h = reinterpret_cast<uint64_t>(p);
        for (const Range& r : ranges)
            if (h >= r.lo && h + len <= r.hi) return r.dev + (h - r.lo);
        return 0;
    }
};

struct ClassCase {
    uint64_t base, S;
    bool pinned, dev_aligned;
};

static const int kTop = 5;  // 4+2: shards 0..5
static const uint64_t kHuge = 1ull << 32;
// pinned x base aligned x S % 16 == 0, then: empty, null base, 2^32 bytes and more, a device
// address that is misaligned where the host address is aligned
static const ClassCase kClass[13] = {
    {0x100000, 160, true, true},  {0x110000, 161, true, true},  {0x120003, 160, true, true},
    {0x130003, 161, true, true},  {0x900000, 160, false, true}, {0x910000, 161, false, true},
    {0x920003, 160, false, true}, {0x930003, 161, false, true}, {0x140000, 0, true, true},
    {0, 160, false, true},        {0x1000000000, kHuge, true, true}, {0x1000000001, kHuge + 5, true, true},
    {0x200000, 160, true, false},
};

static Kind kind_restated(const ClassCase& c, bool any_align) {
    if (c.S == 0) return Kind::empty;
    if (!c.pinned || c.S >= kHuge) return Kind::staged;  // the 32-bit kernels stop below 2^31
    if (c.base % 16 == 0 && c.S % 16 == 0 && c.dev_aligned) return Kind::aligned;
    return any_align ? Kind::any_alignment : Kind::staged;
}

static int classifier() {
    ToyPinned pinned;
    pinned.ranges = {{0x100000, 0x1f0000, 0x7000000000ull}, {0x200000, 0x2f0000, 0x7100000007ull},
                     {0x1000000000ull, 0x1000000000ull + 8 * kHuge, 0x7200000000ull}};
    std::vector<hbec_stripe> st;
    for (const ClassCase& c : kClass) st.push_back({fake(c.base), c.S});
    for (int any_align = 0; any_align < 2; ++any_align) {
        std::vector<ZcStripe> want_zs, want_zu;
        std::vector<uint64_t> want_staged;
        for (size_t i = 0; i < st.size(); ++i) {
            const ClassCase& c = kClass[i];
            uint64_t dev = 0;
            const long before = pinned.calls;
            const Kind k = classify(st[i], kTop, any_align != 0, pinned, dev);
            CHECK(k == kind_restated(c, any_align != 0));
            const uint64_t want_dev = pinned(fake(c.base), (uint64_t)(kTop + 1) * c.S);
            if (k == Kind::aligned || k == Kind::any_alignment) CHECK(dev == want_dev && dev != 0);
            if (c.S == 0 || c.base == 0) CHECK(pinned.calls == before + 1);  // only the line above asked
            if (k == Kind::aligned) want_zs.push_back({want_dev, c.S});
            if (k == Kind::any_alignment) want_zu.push_back({want_dev, c.S});
            if (k == Kind::staged) want_staged.push_back(c.base);
            ++g_cases;
        }
        // a range must hold all of (top + 1) S: shard 5 of this stripe lies past the pinned range
        hbec_stripe cut_off = {fake(0x1f0000 - 5 * 160), 160};
        uint64_t dev = 0;
        CHECK(classify(cut_off, kTop, true, pinned, dev) == Kind::staged);
        CHECK(classify(cut_off, 4, true, pinned, dev) == Kind::aligned);
        // the plain policy: three lists, in the caller's order, empty stripes in none
        std::vector<ZcStripe> zs, zu;
        std::vector<hbec_stripe> staged;
        route_plain(st.data(), st.size(), kTop, any_align != 0, pinned, zs, zu, staged);
        CHECK(zs.size() == want_zs.size() && zu.size() == want_zu.size() && staged.size() == want_staged.size());
        for (size_t i = 0; i < zs.size(); ++i) CHECK(zs[i].dev == want_zs[i].dev && zs[i].shard_len == want_zs[i].shard_len);
        for (size_t i = 0; i < zu.size(); ++i) CHECK(zu[i].dev == want_zu[i].dev && zu[i].shard_len == want_zu[i].shard_len);
        for (size_t i = 0; i < staged.size(); ++i) CHECK(reinterpret_cast<uint64_t>(staged[i].base) == want_staged[i]);
        CHECK(want_zs.size() == 1 && want_zu.size() == (any_align ? 4u : 0u));
        ++g_cases;
    }
    // the hashing policy: all or nothing
    const std::vector<hbec_stripe> aligned = {st[0], st[0], st[0]}, mixed = {st[0], st[1], st[12], st[2]};
    const std::vector<hbec_stripe> broken = {st[0], st[4], st[1], st[0]}, empty_one = {st[0], st[8]};
    std::vector<ZcStripe> zs;
    CHECK(route_hashing(aligned.data(), 3, kTop, false, pinned, zs) == Kind::aligned && zs.size() == 3);
    zs.clear();
    CHECK(route_hashing(mixed.data(), 4, kTop, true, pinned, zs) == Kind::any_alignment && zs.size() == 4);
    for (size_t i = 0; i < 4; ++i) CHECK(zs[i].dev == pinned(mixed[i].base, 6 * mixed[i].shard_len));
    zs.clear();
    CHECK(route_hashing(mixed.data(), 4, kTop, false, pinned, zs) == Kind::staged);  // no unaligned mirror kernel
    zs.clear();
    long before = pinned.calls;
    CHECK(route_hashing(broken.data(), 4, kTop, true, pinned, zs) == Kind::staged);
    CHECK(pinned.calls == before + 2);  // it stops at the first stripe that is not pinned
    zs.clear();
    CHECK(route_hashing(empty_one.data(), 2, kTop, true, pinned, zs) == Kind::staged);
    Pass ps;
    ps.in_idx = {1, 2, 4, 5};
    ps.out_idx = {0, 3};
    CHECK(top_shard(ps) == 5);
    g_cases += 5;
    return 0;
}

int main() {
    static_assert(sizeof(TileRec) == 32 && sizeof(URec) == 32, "record slots are shared");
    if (ring_cutter() || plain_fills() || md5_fills() || verify_cutter() || classifier()) return 1;
    std::printf("host_cut ok (%ld cases)\n", g_cases);
    return 0;
}
