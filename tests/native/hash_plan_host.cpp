// Host-only checks of the hash call's inline host logic (hashplan.h; no GPU work
// and no libhbec): the where word of every selection of 4+2 and 8+3 and every
// subset of it as the bad shards, decoded by loc_decode (the body of
// hbec_locate_decode) under that selection; and the chain list a call builds,
// over random lengths, selections and zero-length entries.  Built with the host
// compiler under AddressSanitizer + UBSan by tests/test_hash_plan_host.py and
// run directly.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../../hummingbird_amd/csrc/hashplan.h"
#include "../../hummingbird_amd/csrc/locate.h"

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

// One bad shard j decodes to j, two or more to kLocMultiple, none to kLocClean.
static int where_words(long* n_words) {
    using namespace hbec;
    for (auto km : {std::pair<int, int>{4, 2}, {8, 3}}) {
        const int k = km.first, m = km.second, n = k + m;
        for (uint32_t sel = 0; sel < (1u << n); ++sel) {
            uint8_t present[16] = {0};
            for (int i = 0; i < n; ++i) present[i] = (uint8_t)((sel >> i) & 1u);
            CHECK(hash_select_bits(n, present) == sel);
            // every subset of sel, the empty one last
            for (uint32_t bad = sel;; bad = (bad - 1u) & sel) {
                const uint32_t w = hash_where_word(sel, bad, (uint32_t)kVmKernel);
                const int d = loc_decode(k, m, present, w);
                const int nbad = __builtin_popcount(bad);
                if (nbad == 0)
                    CHECK(w == 0u && d == kLocClean);
                else if (nbad == 1)
                    CHECK(d == __builtin_ctz(bad) && w == (kLocBad | (sel & ~bad)));
                else
                    CHECK(d == kLocMultiple && w == (kLocBad | sel));
                CHECK((w & ~(kLocBad | kLocRuledMask)) == 0u);
                CHECK(hash_where_word(sel, bad, (uint32_t)kVmOther) == kLocSkipped);
                CHECK(hash_where_word(sel, bad, (uint32_t)kVmSkip) == 0u);
                ++*n_words;
                if (bad == 0u) break;
            }
        }
        uint8_t all[16];
        for (int i = 0; i < 16; ++i) all[i] = 1;
        CHECK(loc_decode(k, m, all, kLocSkipped) == kLocUnchecked);
    }
    // bits of shards past 15 never reach the ruled-out field
    CHECK(hash_where_word(0xFFFFFFFFu, 1u << 20, (uint32_t)kVmKernel) == (kLocBad | 0xFFFFu));
    return 0;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

// Exactly the selected shards of the non-empty entries, each once, in
// non-increasing length.
static int chain_lists(long* n_chains) {
    using namespace hbec;
    for (int round = 0; round < 200; ++round) {
        const int n = 1 + (int)(rnd() % 36);  // up to 28+8
        const uint32_t n_src = rnd() % 70, n_select = 1 + rnd() % 9;
        std::vector<MSrc> src(n_src);
        for (auto& s : src) {
            const uint32_t r = rnd() % 8;
            // zero-length entries, repeated lengths, and lengths past 32 bits
            s.shard_len = r == 0 ? 0 : r == 1 ? 4096 : r == 2 ? (1ull << 33) + rnd() % 5 : 1 + rnd() % 5000;
            s.a = 0x1000;
            s.b = 0x2000;
        }
        std::vector<uint8_t> select((size_t)n_select * n);
        for (auto& b : select) b = (uint8_t)(rnd() % 3 == 0 ? rnd() % 255 + 1 : 0);
        if (round % 5 == 0)
            for (int j = 0; j < n; ++j) select[j] = 0;  // a row with nothing set
        std::vector<uint32_t> select_of(n_src);
        for (auto& p : select_of) p = rnd() % n_select;
        std::vector<uint32_t> order;
        hash_order(src, order);
        size_t nonempty = 0;
        for (const auto& s : src) nonempty += s.shard_len != 0;
        CHECK(order.size() == nonempty);
        for (size_t i = 1; i < order.size(); ++i) {
            const uint64_t x = src[order[i - 1]].shard_len, y = src[order[i]].shard_len;
            CHECK(x > y || (x == y && order[i - 1] < order[i]));
        }
        std::vector<HChain> chains;
        hash_chains(order, n, select.data(), n_select, select_of.data(), chains);
        std::set<std::pair<uint32_t, uint32_t>> want, got;
        for (uint32_t i = 0; i < n_src; ++i)
            for (int j = 0; j < n; ++j)
                if (src[i].shard_len && select[(size_t)select_of[i] * n + j]) want.insert({i, (uint32_t)j});
        for (size_t c = 0; c < chains.size(); ++c) {
            CHECK(chains[c].entry < n_src && chains[c].shard < (uint32_t)n);
            CHECK(got.insert({chains[c].entry, chains[c].shard}).second);  // each once
            if (c) CHECK(src[chains[c - 1].entry].shard_len >= src[chains[c].entry].shard_len);
        }
        CHECK(got == want);
        *n_chains += (long)chains.size();
    }
    static_assert(sizeof(HChain) == 8 && sizeof(HRec) == 32, "device layouts");
    return 0;
}

int main() {
    long n_words = 0, n_chains = 0;
    if (where_words(&n_words) || chain_lists(&n_chains)) return 1;
    std::printf("hash_plan_host ok (%ld words, %ld chains)\n", n_words, n_chains);
    return 0;
}
