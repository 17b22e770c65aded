// Host-only checks of correct.h (no GPU work, no libhbec): cor_classify against
// a brute force over every (shard, error byte) pair, and cor_pattern's inverse
// tables read back.  One all-present mask per r: 4+2 and 8+3 with every
// syndrome there is, 12+4 with every single error and 2^22 random syndromes.
// Built with -fsanitize=address,undefined by tests/test_correct_host.py.
#include <algorithm>
#include <cstdio>
#include <unordered_map>
#include <vector>

#include "../../hummingbird_amd/csrc/correct.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// every shard present: survivors 0..k-1, checked k..k+r-1, rows = the parity rows
static int rule(int k, int r) {
    using namespace hbec;
    const Field& F = field();
    std::vector<uint8_t> mat;
    CHECK(build_matrix(k, r, mat));
    const uint8_t* rows = mat.data() + (size_t)k * k;
    std::vector<int> shard(k + r);
    for (int j = 0; j < k + r; ++j) shard[j] = j;
    const int *surv = shard.data(), *checked = shard.data() + k;
    auto pack = [&](const uint8_t* s) { return s[0] | s[1] << 8 | s[2] << 16 | (uint32_t)s[3] << 24; };
    // the brute force: every (shard, error byte) pair and the syndrome it leaves
    std::unordered_map<uint32_t, uint32_t> single;  // syndrome -> shard << 8 | e
    uint8_t s[4] = {0, 0, 0, 0}, err = 0;
    for (int j = 0; j < k + r; ++j)
        for (int e = 1; e < 256; ++e) {
            for (int q = 0; q < r; ++q) s[q] = j < k ? F.mul((uint8_t)e, rows[(size_t)q * k + j]) : (j - k == q ? e : 0);
            CHECK(single.emplace(pack(s), (uint32_t)j << 8 | (uint32_t)e).second);  // no two alike
            CHECK(cor_classify(k, r, rows, s, surv, checked, &err) == j && err == e);
        }
    uint32_t seed = 2468u;
    for (uint64_t w = 0; w < (r <= 3 ? 1ull << (8 * r) : 1ull << 22); ++w) {
        for (int q = 0; q < r; ++q) {
            seed = seed * 1664525u + 1013904223u;
            s[q] = r <= 3 ? (uint8_t)(w >> (8 * q)) : ((seed >> 28) < 4u ? 0 : (uint8_t)(seed >> 16));
        }
        err = 0x55;
        const int got = cor_classify(k, r, rows, s, surv, checked, &err);
        const auto it = single.find(pack(s));
        if (it == single.end())
            CHECK(got == -1 && err == 0);
        else
            CHECK(got == (int)(it->second >> 8) && err == (uint8_t)it->second);
    }
    // the record: Verify's words, then the tables of 1 / rows[0][t]
    std::vector<uint32_t> buf(8, 0u), ref(8, 0u);  // a record that does not start at 0
    CHECK(cor_pattern(buf, k, surv, checked, r, rows) == 2 && loc_pattern(ref, k, surv, checked, r, rows) == 2);
    CHECK(buf.size() == 8 + cor_pattern_words(k, r) && std::equal(ref.begin(), ref.end(), buf.begin()));
    for (int t = 0; t < k; ++t) {
        uint32_t tab[5];
        perm_table(cor_pattern_inverse(buf.data() + 8, k, r, t), tab);
        CHECK(F.mul(cor_pattern_inverse(buf.data() + 8, k, r, t), rows[t]) == 1);
        CHECK(std::equal(tab, tab + 5, buf.data() + 8 + cor_inverse_at(k, r) + 5 * t));
    }
    return 0;
}

int main() {
    if (rule(4, 2) || rule(8, 3) || rule(12, 4)) return 1;
    std::puts("correct_host ok");
    return 0;
}
