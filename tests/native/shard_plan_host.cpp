// shard_plan_host.cpp — the host logic of shards plans (csrc/shardplan.h) alone,
// for a run under AddressSanitizer + UBSan: the check of an entry's row of shard
// addresses against a pairwise restatement, and ecSplit's stripe arithmetic
// against the loop of ecutils.go:38-58 with the shard size of :85-92.  Links no
// libhbec and touches no device.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../hummingbird_amd/csrc/shardplan.h"

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

int main() {
    // rows: n shards of S bytes dropped at random into a small window, so that
    // overlaps, touching ranges and null pointers all occur
    std::vector<uint64_t> tmp;
    uint64_t rows = 0, bad_null = 0, bad_overlap = 0, good = 0;
    for (int it = 0; it < 200000; ++it) {
        const int n = 1 + (int)(rnd() % 16);
        const uint64_t S = 1 + rnd() % 40;
        const uint64_t window = S * (uint64_t)n * (1 + rnd() % 4) + 1;
        std::vector<uint64_t> row((size_t)n);
        if (it % 3 == 0) {  // packed back to back in a random order: ranges touch, none overlap
            std::vector<int> order((size_t)n);
            for (int i = 0; i < n; ++i) order[i] = i;
            for (int i = n - 1; i > 0; --i) std::swap(order[i], order[rnd() % (uint64_t)(i + 1)]);
            for (int i = 0; i < n; ++i) row[order[i]] = 4096 + (uint64_t)i * S;
        } else {
            for (int i = 0; i < n; ++i) row[i] = rnd() % 7 == 0 && it % 5 == 0 ? 0 : 4096 + rnd() % window;
        }
        bool has_null = false, overlap = false;
        for (int i = 0; i < n; ++i) has_null = has_null || row[i] == 0;
        for (int i = 0; i < n && !has_null; ++i)
            for (int j = i + 1; j < n; ++j)
                overlap = overlap || (row[i] < row[j] + S && row[j] < row[i] + S);
        const std::vector<uint64_t> before(row);
        const char* why = hbec::shards_check_row(row.data(), n, S, tmp);
        CHECK(row == before);  // the caller's row is not reordered
        if (has_null) {
            CHECK(why && std::strstr(why, "null"));
            ++bad_null;
        } else if (overlap) {
            CHECK(why && std::strstr(why, "overlap"));
            ++bad_overlap;
        } else {
            CHECK(why == nullptr);
            ++good;
        }
        if (it % 3 == 0) CHECK(why == nullptr);
        ++rows;
    }
    CHECK(bad_null > 100 && bad_overlap > 1000 && good > 60000);

    // stripe arithmetic: ecSplit's loop, restated
    uint64_t lengths = 0;
    const int64_t ks[] = {1, 2, 3, 4, 8, 12, 200};
    const int64_t chunks[] = {1, 2, 5, 64, 1000};
    for (int64_t k : ks)
        for (int64_t chunk : chunks)
            for (int64_t L = -2; L <= 3 * k * chunk + k; ++L) {
                std::vector<uint64_t> want;
                for (int64_t done = 0; done < L;) {
                    int64_t expect = k * chunk;
                    if (L - done < expect) expect = L - done;
                    done += expect;
                    while (expect % k) ++expect;  // zero padding to a multiple of k
                    want.push_back((uint64_t)(expect / k));
                }
                CHECK(hbec::ec_stripe_count(L, k, chunk) == want.size());
                uint64_t sum = 0;
                for (size_t t = 0; t < want.size(); ++t) {
                    CHECK(hbec::ec_stripe_shard_length(L, k, chunk, t) == want[t]);
                    sum += want[t];
                }
                CHECK(sum == (L <= 0 ? 0u : (uint64_t)((L + k - 1) / k)));
                ++lengths;
            }
    // no overflow at the top of the range
    const int64_t big = INT64_MAX;
    CHECK(hbec::ec_stripe_count(big, 200, big) == 1);
    CHECK(hbec::ec_stripe_shard_length(big, 200, big, 0) == (uint64_t)((big - 1) / 200 + 1));
    CHECK(hbec::ec_stripe_count(big, 1, 1) == (uint64_t)big);
    CHECK(hbec::ec_stripe_shard_length(big, 1, 1, (uint64_t)big - 1) == 1);
    std::printf("shard_plan_host ok (%llu rows, %llu lengths)\n", (unsigned long long)rows,
                (unsigned long long)lengths);
    return 0;
}
