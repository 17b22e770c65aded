// glue_host.cpp — the host arithmetic of the glue calls (csrc/glue.h) alone, for
// a run under AddressSanitizer + UBSan: the bytes of each data shard inside a
// prefix, the tiles with something to do, the cut of an object into its entries'
// destinations and the overlap of a destination with a shard, each against a
// bytewise restatement.  Links no libhbec and touches no device.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../hummingbird_amd/csrc/glue.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main(int argc, char** argv) {
    // "cuts k chunk max_L": the cut of every object of 0..max_L bytes, a line
    // "L t offset length" per entry, for a comparison with the reference's sizes
    if (argc == 5 && std::string(argv[1]) == "cuts") {
        const uint64_t k = std::strtoull(argv[2], nullptr, 10), chunk = std::strtoull(argv[3], nullptr, 10);
        const uint64_t max_l = std::strtoull(argv[4], nullptr, 10);
        if (k < 1 || chunk < 1) return 2;
        for (uint64_t L = 0; L <= max_l; ++L) {
            const uint64_t n = hbec::ec_stripe_count((int64_t)L, (int64_t)k, (int64_t)chunk);
            for (uint64_t t = 0; t < n; ++t) {
                uint64_t off = 0, len = 0;
                hbec::glue_files_cut(L, k, chunk, t, &off, &len);
                std::printf("%llu %llu %llu %llu\n", (unsigned long long)L, (unsigned long long)t,
                            (unsigned long long)off, (unsigned long long)len);
            }
        }
        return 0;
    }
    // clamp and needed tiles: D = k shards of S bytes, its first len bytes wanted
    uint64_t clamps = 0, tiles = 0, needed = 0;
    for (int it = 0; it < 200000; ++it) {
        const uint64_t k = 1 + rnd() % 12, S = rnd() % 41, len = rnd() % (k * S + 4);
        std::vector<uint64_t> in_shard((size_t)k + 2, 0);     // wanted bytes per shard, counted one by one
        std::vector<uint8_t> pos_wanted((size_t)S + 1, 0);    // shard position p has a wanted byte in some shard
        for (uint64_t b = 0; b < len && b < k * S; ++b) {
            ++in_shard[(size_t)(b / S)];
            pos_wanted[(size_t)(b % S)] = 1;
        }
        // (a length past k S is refused by the call; the clamp still holds for the k shards)
        for (uint64_t j = 0; j < (len <= k * S ? k + 2 : k); ++j)
            CHECK(hbec::glue_valid(len, j, S) == in_shard[(size_t)j]);
        ++clamps;
        const uint64_t T = 1 + rnd() % 9;
        if (len <= k * S) {
            uint64_t span = 0;
            for (uint64_t p = 0; p < S; ++p) span += pos_wanted[(size_t)p];
            CHECK(hbec::glue_span(S, len) == span);  // the wanted positions are [0, span)
            for (uint64_t p = 0; p < span; ++p) CHECK(pos_wanted[(size_t)p]);
            for (uint64_t ti = 0; ti * T < S + 2 * T; ++ti) {
                bool want = false;
                for (uint64_t p = ti * T; p < (ti + 1) * T && p < S; ++p) want = want || pos_wanted[(size_t)p];
                CHECK(hbec::glue_tile_needed(S, len, ti, T) == want);
                needed += want;
                ++tiles;
            }
        }
    }
    CHECK(needed > 100000 && tiles > needed + 100000);
    // no overflow at the top of the range
    CHECK(hbec::glue_valid(~0ull, 255, ~0ull) == 0);
    CHECK(hbec::glue_valid(~0ull, 0, ~0ull) == ~0ull);
    CHECK(hbec::glue_valid(~0ull, 1, 1ull << 63) == (1ull << 63) - 1);
    CHECK(!hbec::glue_tile_needed(~0ull, ~0ull, ~0ull, ~0ull));
    CHECK(hbec::glue_tile_needed(~0ull, ~0ull, 1, ~0ull - 1));

    // the files cut: every byte of [0, L) in exactly one entry, in order, and
    // each entry's length the smaller of k S_t and what is left
    uint64_t cuts = 0;
    const uint64_t ks[] = {1, 2, 3, 4, 8, 12};
    const uint64_t chunks[] = {1, 2, 5, 64};
    for (uint64_t k : ks)
        for (uint64_t chunk : chunks)
            for (uint64_t L = 0; L <= 3 * k * chunk + k; ++L) {
                std::vector<uint8_t> seen((size_t)L, 0);
                const uint64_t n = hbec::ec_stripe_count((int64_t)L, (int64_t)k, (int64_t)chunk);
                uint64_t next = 0;
                for (uint64_t t = 0; t < n; ++t) {
                    uint64_t off = ~0ull, len = ~0ull;
                    hbec::glue_files_cut(L, k, chunk, t, &off, &len);
                    const uint64_t S = hbec::ec_stripe_shard_length((int64_t)L, (int64_t)k, (int64_t)chunk, t);
                    CHECK(off == next && len >= 1 && len <= k * S && len + k > k * S);
                    CHECK(len == (k * S < L - off ? k * S : L - off));
                    for (uint64_t b = off; b < off + len; ++b) {
                        CHECK(b < L && !seen[(size_t)b]);
                        seen[(size_t)b] = 1;
                    }
                    next = off + len;
                    ++cuts;
                }
                CHECK(next == L);
            }
    {
        uint64_t off = 0, len = 0;
        hbec::glue_files_cut(~0ull, 255, 1ull << 56, 0, &off, &len);
        CHECK(off == 0 && len == 255 * (1ull << 56));
        hbec::glue_files_cut(~0ull, 255, 1ull << 56, 1, &off, &len);
        CHECK(off == 255 * (1ull << 56) && len == ~0ull - off);
    }

    // overlap: two byte ranges in a small window, byte by byte
    uint64_t overlaps = 0, touching = 0, pairs = 0;
    for (int it = 0; it < 200000; ++it) {
        const uint64_t dst = 4096 + rnd() % 64, len = rnd() % 24, sh = 4096 + rnd() % 64, S = rnd() % 24;
        bool share = false;
        for (uint64_t b = dst; b < dst + len; ++b) share = share || (b >= sh && b < sh + S);
        CHECK(hbec::glue_overlaps(dst, len, sh, S) == share);
        overlaps += share;
        touching += !share && len && S && (dst + len == sh || sh + S == dst);
        ++pairs;
    }
    CHECK(overlaps > 20000 && touching > 1000);
    CHECK(!hbec::glue_overlaps(~0ull - 7, 8, 0, 8));  // no wrap: the top of the address space is not address 0
    CHECK(hbec::glue_overlaps(~0ull - 7, 8, ~0ull, 1));
    CHECK(!hbec::glue_overlaps(16, 0, 0, 64) && !hbec::glue_overlaps(16, 8, 0, 0));
    std::printf("glue_host ok (%llu clamps, %llu tiles, %llu cuts, %llu pairs)\n", (unsigned long long)clamps,
                (unsigned long long)tiles, (unsigned long long)cuts, (unsigned long long)pairs);
    return 0;
}
