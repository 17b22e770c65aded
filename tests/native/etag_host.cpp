// Host-only checks of the ETag call's inline host logic (etag.h; no GPU work and
// no libhbec): the segment walk both kernels share, byte for byte against a
// brute-force model, for every (k <= 4, S <= 40, len, data mask) on slot and row
// records; the segment count; the chain list over random objects; and the
// 64-bit totals, trip counts, tails and bit lengths of objects around 2^32 and
// 2^40 bytes, which no GPU test runs.  Built with the host compiler under
// AddressSanitizer + UBSan by tests/test_etag_host.py and run directly.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hummingbird_amd/csrc/etag.h"

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

using namespace hbec;

static uint64_t g_rng = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

static const uint64_t kSlotBase = 1ull << 30, kScratch = 1ull << 40;
static uint64_t row_addr(uint32_t j) { return (1ull << 32) + ((uint64_t)j << 20) + (j & 3u); }

// every segment the walk opens for one entry, as {address, bytes}
static int walk(bool rows, uint32_t k, uint64_t S, const ERec& r, std::vector<ESeg>& segs) {
    segs.clear();
    uint32_t j = 0;
    ESeg s;
    while (rows ? etag_segment_rows(row_addr, S, r, j, &s) : etag_segment_slot(kSlotBase, S, r, j, k, &s)) {
        CHECK(s.left > 0 && s.next > j && s.next <= k);
        segs.push_back(s);
        j = s.next;
    }
    return 0;
}

static int every_entry(long* n_walks, long* n_segments) {
    for (uint32_t k = 1; k <= 4; ++k)
        for (uint64_t S = 1; S <= 40; ++S)
            for (uint64_t len = 0; len <= k * S; ++len)
                for (uint32_t mask = 0; mask < (1u << k); ++mask) {
                    uint8_t present[4];
                    for (uint32_t j = 0; j < k; ++j) present[j] = (mask >> j) & 1u;
                    // the model: the first and last missing data shard with a byte below len
                    int m0 = -1, m1 = -1;
                    for (uint32_t j = 0; j < k; ++j)
                        if (!present[j] && j * S < len) {
                            if (m0 < 0) m0 = (int)j;
                            m1 = (int)j;
                        }
                    ERec r{len, 0u, 0u, 0u};
                    const bool any = etag_span(k, S, len, present, &r.j0, &r.j1);
                    CHECK(any == (m0 >= 0));
                    uint64_t lo = 0, hi = 0;
                    if (any) {
                        CHECK((int)r.j0 == m0 && (int)r.j1 == m1);
                        lo = etag_span_lo(S, r.j0), hi = etag_span_hi(S, len, r.j1);
                        CHECK(lo == (uint64_t)m0 * S && hi == std::min<uint64_t>(len, ((uint64_t)m1 + 1) * S) && lo < hi);
                        r.red = kScratch - lo;
                    }
                    for (int rows = 0; rows < 2; ++rows) {
                        std::vector<ESeg> segs;
                        if (walk(rows != 0, k, S, r, segs)) return 1;
                        // byte for byte: D[p] is read from scratch inside the span and from its shard outside it,
                        // so no byte of a missing shard is read where it lies
                        uint64_t p = 0;
                        for (const ESeg& s : segs)
                            for (uint64_t q = 0; q < s.left; ++q, ++p) {
                                CHECK(p < len);
                                const uint64_t want = any && p >= lo && p < hi ? kScratch + (p - lo)
                                                      : rows ? row_addr((uint32_t)(p / S)) + p % S
                                                             : kSlotBase + p;
                                CHECK(s.addr + q == want);
                                if (!(any && p >= lo && p < hi)) CHECK(present[p / S]);
                            }
                        CHECK(p == len);
                        // the count: on slot records one per run, on row records one per shard outside the span
                        uint64_t model = 0;
                        if (len) {
                            if (!any) {
                                model = rows ? (len + S - 1) / S : 1;
                            } else {
                                const uint64_t tail = len > hi ? len - hi : 0;
                                model = 1 + (rows ? (uint64_t)m0 + (tail + S - 1) / S : (lo ? 1u : 0u) + (tail ? 1u : 0u));
                            }
                        }
                        CHECK(segs.size() == model && etag_entry_segments(rows != 0, k, S, r) == model);
                        *n_segments += (long)model;
                        ++*n_walks;
                    }
                }
    return 0;
}

static int chain_lists(long* n_chains) {
    for (int round = 0; round < 400; ++round) {
        const uint32_t n_obj = rnd() % 9, mixed = rnd() & 1u;
        std::vector<uint32_t> start(1, 0u);
        for (uint32_t g = 0; g < n_obj; ++g) start.push_back(start.back() + (mixed ? 1u : rnd() % 4));
        std::vector<ERec> recs(start.back());
        for (ERec& r : recs) r = ERec{rnd() % 3 ? (uint64_t)(rnd() % 200) : 0u, 0u, 0u, 0u};
        std::vector<EChain> chains;
        etag_chains(recs, mixed ? nullptr : start.data(), n_obj, chains);
        std::vector<int> seen(n_obj, 0);
        for (size_t c = 0; c < chains.size(); ++c) {
            const EChain& ch = chains[c];
            CHECK(ch.slot < n_obj && !seen[ch.slot]++);
            CHECK(ch.e0 == start[ch.slot] && ch.e1 == start[ch.slot + 1]);
            uint64_t total = 0;
            for (uint32_t e = ch.e0; e < ch.e1; ++e) total += recs[e].len;
            CHECK(total == ch.total && total > 0);
            if (c) {  // longest first, equal totals in object order
                CHECK(chains[c - 1].total >= ch.total);
                if (chains[c - 1].total == ch.total) CHECK(chains[c - 1].slot < ch.slot);
            }
        }
        for (uint32_t g = 0; g < n_obj; ++g) {  // an object without a byte has no chain
            uint64_t total = 0;
            for (uint32_t e = start[g]; e < start[g + 1]; ++e) total += recs[e].len;
            CHECK((seen[g] != 0) == (total != 0));
        }
        *n_chains += (long)chains.size();
    }
    return 0;
}

// The blocks a lane takes whole from inside a segment and the ones it gathers
// across segments, by the kernel's rule (a block lies inside when the segment
// has 64 bytes left), in segment-sized jumps so that 2^40 bytes cost nothing.
static int big_objects(long* n_big) {
    const uint64_t sizes[] = {(1ull << 32) - 65, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 1, (1ull << 32) + 55,
                              (1ull << 32) + 56, (1ull << 32) + 63, (1ull << 40) - 1, 1ull << 40, (1ull << 40) + 57,
                              (1ull << 40) + 64 + 9, (1ull << 61) + 3};
    const uint32_t k = 4;
    for (uint64_t L : sizes)
        for (uint64_t chunk : {(uint64_t)1 << 20, (uint64_t)(1 << 20) + 3, (uint64_t)1 << 33}) {
            // the object's stripes: k * chunk bytes each, a short last one, a data shard lost in every third
            std::vector<ERec> recs;
            std::vector<uint64_t> S;
            const uint64_t stripe = k * chunk, cnt = std::min<uint64_t>((L + stripe - 1) / stripe, 4096);
            uint64_t rest = L;
            for (uint64_t t = 0; t < cnt; ++t) {
                const uint64_t len = t + 1 == cnt ? rest : stripe;  // all that is left goes to the last one
                const uint64_t s = t + 1 == cnt ? (len + k - 1) / k : chunk;
                ERec r{len, 0u, 0u, 0u};
                if (t % 3 == 1) {
                    const uint8_t present[4] = {1, 0, 1, 1};
                    if (etag_span(k, s, len, present, &r.j0, &r.j1)) r.red = kScratch - etag_span_lo(s, r.j0);
                }
                recs.push_back(r);
                S.push_back(s);
                rest -= len;
            }
            CHECK(rest == 0);
            std::vector<EChain> chains;
            etag_chains(recs, nullptr, 0, chains);
            CHECK(chains.empty());
            const uint32_t start[2] = {0, (uint32_t)recs.size()};
            etag_chains(recs, start, 1, chains);
            CHECK(chains.size() == 1 && chains[0].total == L);
            const unsigned __int128 wide = L;
            CHECK(etag_blocks(L) == (uint64_t)(wide / 64) && etag_tail(L) == (uint32_t)(wide % 64));
            CHECK(etag_bits(L) == (uint64_t)(wide * 8));  // modulo 2^64, as MD5 defines its length field
            CHECK(etag_pad_blocks(L) == (wide % 64 >= 56 ? 2u : 1u));
            CHECK((uint64_t)(uint32_t)etag_blocks(L) != etag_blocks(L) || L < (1ull << 38));  // the trip count needs 64 bits
            uint64_t inside = 0, gathered = 0, carry = 0;  // carry: bytes of an open straddling block
            for (size_t e = 0; e < recs.size(); ++e) {
                std::vector<ESeg> segs;
                if (walk(false, k, S[e], recs[e], segs)) return 1;
                for (const ESeg& s : segs) {
                    uint64_t left = s.left;
                    if (carry) {  // finish the block the last segment left open
                        const uint64_t take = std::min<uint64_t>(64 - carry, left);
                        carry += take, left -= take;
                        if (carry == 64) ++gathered, carry = 0;
                    }
                    if (!carry) inside += left / 64, carry = left % 64;
                }
            }
            CHECK(inside + gathered == etag_blocks(L) && carry == etag_tail(L));
            ++*n_big;
        }
    return 0;
}

int main() {
    long walks = 0, segments = 0, chains = 0, big = 0;
    if (every_entry(&walks, &segments) || chain_lists(&chains) || big_objects(&big)) return 1;
    std::printf("etag_host ok (%ld walks, %ld segments, %ld chains, %ld big)\n", walks, segments, chains, big);
    return 0;
}
