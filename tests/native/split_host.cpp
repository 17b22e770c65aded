// split_host.cpp — the host arithmetic of the split calls (csrc/splitplan.h)
// alone, for a run under AddressSanitizer + UBSan: which piece lengths fill
// shards of S bytes, the bytes of each data shard that come from the piece and
// the pad behind them, the tiles with work, and the pieces of a files plan's
// objects, each against a bytewise restatement of ecSplit's stripe
// (ecutils.go:26-72).  Links no libhbec and touches no device.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../hummingbird_amd/csrc/splitplan.h"

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

// ecSplit's stripe of a piece of len bytes, restated: pad with zeros to a
// multiple of k, then cut into k.  from[j] = bytes of shard j that are the
// piece's, by walking the padded stripe byte by byte.
static uint64_t stripe_of(uint64_t len, uint64_t k, std::vector<uint64_t>& from, uint64_t* pad) {
    uint64_t padded = len;
    while (padded % k) ++padded;
    const uint64_t S = padded / k;
    from.assign((size_t)k, 0);
    for (uint64_t b = 0; b < len; ++b) ++from[(size_t)(b / S)];
    *pad = padded - len;
    return S;
}

int main(int argc, char** argv) {
    // "lens k chunk max_L": for every object of 0..max_L bytes and every entry of
    // it, a line "L t offset length shard_length ok": the piece, the shard length
    // the length rule gives it, and whether the rule accepts it for the entry's own
    // shard length; for a comparison with the reference's sizes
    if (argc == 5 && std::string(argv[1]) == "lens") {
        const uint64_t k = std::strtoull(argv[2], nullptr, 10), chunk = std::strtoull(argv[3], nullptr, 10);
        const uint64_t max_l = std::strtoull(argv[4], nullptr, 10);
        if (k < 1 || chunk < 1) return 2;
        for (uint64_t L = 0; L <= max_l; ++L) {
            const uint64_t n = hbec::ec_stripe_count((int64_t)L, (int64_t)k, (int64_t)chunk);
            for (uint64_t t = 0; t < n; ++t) {
                uint64_t off = 0, len = 0;
                hbec::glue_files_cut(L, k, chunk, t, &off, &len);
                const uint64_t S = hbec::ec_stripe_shard_length((int64_t)L, (int64_t)k, (int64_t)chunk, t);
                std::printf("%llu %llu %llu %llu %llu %d\n", (unsigned long long)L, (unsigned long long)t,
                            (unsigned long long)off, (unsigned long long)len,
                            (unsigned long long)hbec::split_shard_length(len, k), hbec::split_len_ok(len, k, S) ? 1 : 0);
            }
        }
        return 0;
    }
    // the length rule, the bytes per shard and the pad
    uint64_t rules = 0, whole_pad_shards = 0, accepted = 0;
    for (int it = 0; it < 200000; ++it) {
        const uint64_t k = 1 + rnd() % 12, len = 1 + rnd() % 200;
        std::vector<uint64_t> from;
        uint64_t pad = 0;
        const uint64_t S = stripe_of(len, k, from, &pad);
        CHECK(hbec::split_shard_length(len, k) == S);
        CHECK(hbec::split_len_ok(len, k, S));
        CHECK(!hbec::split_len_ok(len, k, S + 1) && !hbec::split_len_ok(len, k, S - 1));
        CHECK(!hbec::split_len_ok(0, k, S) && !hbec::split_len_ok(0, k, 0) && !hbec::split_len_ok(len, k, 0));
        CHECK(hbec::split_pad(len, k, S) == pad && pad < k);
        uint64_t sum = 0;
        for (uint64_t j = 0; j < k; ++j) {
            CHECK(hbec::split_valid(len, j, S) == from[(size_t)j]);
            whole_pad_shards += from[(size_t)j] == 0;
            sum += from[(size_t)j];
        }
        CHECK(sum == len && hbec::split_valid(len, k, S) == 0);
        // any other shard length is refused, any length of this one's range accepted
        const uint64_t S2 = rnd() % 60, len2 = rnd() % (k * S2 + k + 1);
        const bool ok = len2 > 0 && len2 <= k * S2 && len2 + k > k * S2;
        CHECK(hbec::split_len_ok(len2, k, S2) == ok);
        accepted += ok;
        ++rules;
    }
    CHECK(whole_pad_shards > 1000 && accepted > 1000);
    // no overflow at the top of the range
    CHECK(hbec::split_shard_length(~0ull, 1) == ~0ull);
    CHECK(hbec::split_shard_length(~0ull, 2) == (1ull << 63));
    CHECK(hbec::split_len_ok(~0ull, 2, 1ull << 63) && hbec::split_pad(~0ull, 2, 1ull << 63) == 1);
    CHECK(!hbec::split_len_ok(~0ull, 2, (1ull << 63) - 1));
    CHECK(hbec::split_valid(~0ull, 1, 1ull << 63) == (1ull << 63) - 1);

    // tiles: every tile with a position below S has work, no other
    uint64_t tiles = 0;
    for (int it = 0; it < 100000; ++it) {
        const uint64_t S = rnd() % 200, T = 1 + rnd() % 40;
        uint64_t n = 0;
        for (uint64_t ti = 0; ti * T < S + 2 * T; ++ti) {
            bool want = false;
            for (uint64_t p = ti * T; p < (ti + 1) * T; ++p) want = want || p < S;
            CHECK(hbec::split_tile_needed(S, ti, T) == want);
            n += want;
            ++tiles;
        }
        CHECK(hbec::split_tiles(S, T) == n);
    }
    CHECK(!hbec::split_tile_needed(~0ull, ~0ull, ~0ull));
    CHECK(hbec::split_tile_needed(~0ull, 1, ~0ull - 1));
    CHECK(hbec::split_tiles(~0ull, ~0ull) == 1 && hbec::split_tiles(~0ull, 1) == ~0ull);

    // the pieces of a files plan: each passes the length rule for its entry's
    // shard length, and they tile [0, L) in order
    uint64_t cuts = 0;
    const uint64_t ks[] = {1, 2, 3, 4, 8, 12};
    const uint64_t chunks[] = {1, 2, 5, 64};
    for (uint64_t k : ks)
        for (uint64_t chunk : chunks)
            for (uint64_t L = 0; L <= 3 * k * chunk + k; ++L) {
                const uint64_t n = hbec::ec_stripe_count((int64_t)L, (int64_t)k, (int64_t)chunk);
                uint64_t next = 0;
                for (uint64_t t = 0; t < n; ++t) {
                    uint64_t off = ~0ull, len = ~0ull;
                    hbec::glue_files_cut(L, k, chunk, t, &off, &len);
                    const uint64_t S = hbec::ec_stripe_shard_length((int64_t)L, (int64_t)k, (int64_t)chunk, t);
                    CHECK(off == next && hbec::split_len_ok(len, k, S));
                    CHECK(t + 1 == n || hbec::split_pad(len, k, S) == 0);  // ecSplit pads its last stripe alone
                    next = off + len;
                    ++cuts;
                }
                CHECK(next == L);
            }
    std::printf("split_host ok (%llu rules, %llu tiles, %llu cuts)\n", (unsigned long long)rules,
                (unsigned long long)tiles, (unsigned long long)cuts);
    return 0;
}
