// Host-only checks of the shard-file hash call's inline host logic (hashfiles.h;
// no GPU work and no libhbec): the check of the object table on every malformed
// shape, the chain list over random objects (totals past 2^32, zero-length
// entries, empty objects, empty selection rows), and the object index of every
// entry.  Built with the host compiler under AddressSanitizer + UBSan by
// tests/test_hash_files_host.py and run directly.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../../hummingbird_amd/csrc/hashfiles.h"

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static uint64_t g_rng = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

static int object_tables(long* n_tables) {
    using namespace hbec;
    const uint32_t good[] = {0, 2, 2, 5, 7};
    CHECK(files_check_objects(good, 4, 7) == nullptr);
    const uint32_t one[] = {0, 7};
    CHECK(files_check_objects(one, 1, 7) == nullptr);
    const uint32_t empties[] = {0, 0, 0, 7, 7};
    CHECK(files_check_objects(empties, 4, 7) == nullptr);
    CHECK(files_check_objects(nullptr, 4, 7) != nullptr);
    CHECK(files_check_objects(good, 0, 7) != nullptr);  // entries but no objects: only [0] is looked at
    const uint32_t late[] = {1, 2, 5, 7};
    CHECK(files_check_objects(late, 3, 7) != nullptr);
    const uint32_t down[] = {0, 5, 4, 7};
    CHECK(files_check_objects(down, 3, 7) != nullptr);
    const uint32_t down_last[] = {0, 5, 8, 7};
    CHECK(files_check_objects(down_last, 3, 7) != nullptr);
    CHECK(files_check_objects(good, 4, 8) != nullptr);  // ends short of the entry count
    CHECK(files_check_objects(good, 4, 6) != nullptr);  // ends past it
    CHECK(files_check_objects(good, 3, 7) != nullptr);  // one word too few
    const uint32_t wrap[] = {0, 0xFFFFFFFFu, 7};
    CHECK(files_check_objects(wrap, 2, 7) != nullptr);
    CHECK(files_check_objects(good, 4, (1ull << 32) + 7) != nullptr);  // an entry count past 32 bits
    *n_tables += 13;
    // random tables: valid ones pass, and one word changed fails unless the table is still valid
    for (int round = 0; round < 300; ++round) {
        const uint32_t n_objects = 1 + rnd() % 12;
        std::vector<uint32_t> t(n_objects + 1, 0u);
        for (uint32_t g = 0; g < n_objects; ++g) t[g + 1] = t[g] + (rnd() % 3 == 0 ? 0 : rnd() % 6);
        const uint64_t n_src = t[n_objects];
        if (n_src == 0) continue;
        CHECK(files_check_objects(t.data(), n_objects, n_src) == nullptr);
        std::vector<uint32_t> u = t;
        const uint32_t at = rnd() % (n_objects + 1);
        u[at] = rnd() % 40;
        bool valid = u[0] == 0 && u[n_objects] == n_src;
        for (uint32_t g = 0; g < n_objects; ++g) valid = valid && u[g] <= u[g + 1];
        CHECK((files_check_objects(u.data(), n_objects, n_src) == nullptr) == valid);
        ++*n_tables;
    }
    return 0;
}

// Exactly the selected shard files of the objects with a byte in them, each
// once, in non-increasing total length; the object of every entry.
static int chain_lists(long* n_chains, long* n_segments) {
    using namespace hbec;
    bool past32 = false;
    for (int round = 0; round < 200; ++round) {
        const int n = 1 + (int)(rnd() % 36);  // up to 28+8
        const uint32_t n_objects = 1 + rnd() % 40, n_select = 1 + rnd() % 9;
        std::vector<uint32_t> start(n_objects + 1, 0u);
        for (uint32_t g = 0; g < n_objects; ++g) start[g + 1] = start[g] + (rnd() % 5 == 0 ? 0 : 1 + rnd() % 5);
        const uint32_t n_src = start[n_objects];
        std::vector<MSrc> src(n_src);
        for (auto& s : src) {
            const uint32_t r = rnd() % 8;
            // zero-length entries, repeated lengths, and lengths whose sum passes 32 bits
            s.shard_len = r == 0 ? 0 : r == 1 ? 4096 : r == 2 ? (1ull << 31) + rnd() % 5 : 1 + rnd() % 5000;
            s.a = 0x1000;
            s.b = 0x2000;
        }
        if (round % 7 == 0)  // an object of zero-length entries only
            for (uint32_t i = start[0]; i < start[1]; ++i) src[i].shard_len = 0;
        std::vector<uint8_t> select((size_t)n_select * n);
        for (auto& b : select) b = (uint8_t)(rnd() % 3 == 0 ? rnd() % 255 + 1 : 0);
        if (round % 5 == 0)
            for (int j = 0; j < n; ++j) select[j] = 0;  // a row with nothing set
        std::vector<uint32_t> select_of(n_objects);
        for (auto& p : select_of) p = rnd() % n_select;

        std::vector<uint32_t> object_of;
        files_entry_objects(start.data(), n_objects, object_of);
        CHECK(object_of.size() == n_src);
        for (uint32_t i = 0; i < n_src; ++i)
            CHECK(object_of[i] < n_objects && start[object_of[i]] <= i && i < start[object_of[i] + 1]);

        std::vector<uint64_t> total(n_objects, 0);
        std::vector<uint32_t> pieces(n_objects, 0);
        for (uint32_t i = 0; i < n_src; ++i) {
            total[object_of[i]] += src[i].shard_len;
            pieces[object_of[i]] += src[i].shard_len != 0;
        }
        for (uint64_t t : total) past32 = past32 || t > (1ull << 32);

        std::vector<FChain> chains;
        const uint64_t segments =
            files_chains(src, start.data(), n_objects, n, select.data(), n_select, select_of.data(), chains);
        std::set<std::pair<uint32_t, uint32_t>> want, got;
        uint64_t want_segments = 0;
        for (uint32_t g = 0; g < n_objects; ++g)
            for (int j = 0; j < n; ++j)
                if (total[g] && select[(size_t)select_of[g] * n + j]) {
                    want.insert({g, (uint32_t)j});
                    want_segments += pieces[g];
                }
        for (size_t c = 0; c < chains.size(); ++c) {
            CHECK(chains[c].object < n_objects && chains[c].shard < (uint32_t)n);
            CHECK(got.insert({chains[c].object, chains[c].shard}).second);  // each once
            if (c) {
                const uint64_t x = total[chains[c - 1].object], y = total[chains[c].object];
                CHECK(x > y || (x == y && chains[c - 1].object <= chains[c].object));  // 64-bit order, stable
            }
        }
        CHECK(got == want);
        CHECK(segments == want_segments);
        *n_chains += (long)chains.size();
        *n_segments += (long)segments;
    }
    CHECK(past32);
    static_assert(sizeof(FChain) == 8 && sizeof(HRec) == 32, "device layouts");
    return 0;
}

int main() {
    long n_tables = 0, n_chains = 0, n_segments = 0;
    if (object_tables(&n_tables) || chain_lists(&n_chains, &n_segments)) return 1;
    std::printf("hash_files_host ok (%ld tables, %ld chains, %ld segments)\n", n_tables, n_chains, n_segments);
    return 0;
}
