// Host-only checks of gluewide.h (no GPU work and no libhbec): the gather record, the
// records of one to four missing data shards, the per-entry word and the gather
// refinement.  Built under ASan + UBSan by tests/test_glue_wide_host.py and run directly.
#include <cstdio>
#include <vector>

#include "../../hummingbird_amd/csrc/gluewide.h"

#define CHECK(c) \
    do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using namespace hbec;

// r = 0: the gather record; r >= 1: the first r of every other data shard lost.  The middle
// record of three, `stride` apart.
static int record(int k, int r, uint32_t stride) {
    std::vector<int> surv(k), outs(r);
    for (int q = 0; q < r; ++q) outs[q] = 2 * q;
    for (int j = 0; j < k; ++j) surv[j] = j < r ? 2 * j + 1 : j + r;
    std::vector<uint8_t> rows((size_t)r * k);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (uint8_t)(7 * i + 3);
    std::vector<uint32_t> buf(3 * (size_t)stride, 0u);
    uint32_t* p = buf.data() + stride;
    if (r == 0)
        gw_gather_pattern(p, k);
    else
        gw_pattern(p, k, surv.data(), outs.data(), r, rows.data());
    const uint32_t used = r ? rw_record_words(k, r) : kRwSurvWords;  // a gather record: no rows, no tables
    for (size_t i = 0; i < buf.size(); ++i)
        if (i < stride || i >= stride + used) CHECK(buf[i] == 0u);
    for (int j = 0; j < kRwMaxK; ++j) CHECK(((p[j >> 2] >> (8 * (j & 3))) & 0xFFu) == (j < k ? (uint32_t)surv[j] : 0u));
    for (int q = 0; q < 4; ++q) CHECK(((p[kRwRowsWord] >> (8 * q)) & 0xFFu) == (q < r ? (uint32_t)outs[q] : 0u));
    for (int j = 0; j < k; ++j)
        for (int q = 0; q < r; ++q) {
            uint32_t t[5];
            perm_table(rows[(size_t)q * k + j], t);
            for (int z = 0; z < 5; ++z) CHECK(p[kRwHdr + 5 * (j * r + q) + z] == t[z]);
        }
    return 0;
}

// the word around the cut: r = 0 exactly when every missing data shard has no byte below len
static int words(int* n) {
    const int lost[][4] = {{0, 0, 0, 0}, {3, 0, 0, 0}, {0, 3, 0, 0}, {2, 3, 0, 0}, {1, 2, 3, 0}, {0, 1, 2, 3}};
    const int count[] = {0, 1, 2, 2, 3, 4};
    for (uint64_t S : {1ull, 16ull, 993ull, (1ull << 31) - 65537})
        for (int m = 0; m < 6; ++m)
            for (int s = 0; s <= 4; ++s)
                for (int d = -1; d <= 1; ++d, ++*n) {
                    const uint64_t at = (uint64_t)s * S;
                    if (d < 0 && at == 0) continue;
                    const uint64_t len = at + (uint64_t)d;  // just before, at and just past the start of shard s
                    bool all_beyond = true;
                    for (int q = 0; q < count[m]; ++q) all_beyond = all_beyond && glue_valid(len, (uint64_t)lost[m][q], S) == 0;
                    CHECK(gw_gathers(S, len, lost[m], count[m]) == all_beyond);
                    const uint32_t w = gw_word(S, len, lost[m], count[m], 7u, 9u);
                    if (len == 0) {
                        CHECK(w == 0u);
                        continue;
                    }
                    CHECK(w != 0u && rw_word_chk(w) == 0u);
                    CHECK((rw_word_out(w) == 0u) == all_beyond);
                    CHECK(all_beyond ? rw_word_pat(w) == 9u : rw_word_out(w) == (uint32_t)count[m] && rw_word_pat(w) == 7u);
                }
    CHECK(gw_word(0, 0, lost[1], 1, 7u, 9u) == 0u);  // a zero-length entry
    for (int r = 0; r <= kMaxR; ++r)
        for (uint32_t pat : {0u, 1u, 255u, 256u, 65534u, 65535u}) {
            const uint32_t w = rw_word(r, 0, pat);
            CHECK(w != 0u && rw_word_out(w) == (uint32_t)r && rw_word_chk(w) == 0u && rw_word_pat(w) == pat);
        }
    return 0;
}

int main() {
    int n_rec = 0, n_words = 0;
    for (int k : {1, 12, 13, 32})
        for (int r = 0; r <= 4 && r <= k; ++r, ++n_rec)  // at its own size and at a four-row call's stride
            if (gw_stride(k, 0) != kRwHdr || record(k, r, gw_stride(k, r)) || record(k, r, gw_stride(k, 4))) return 1;
    if (words(&n_words)) return 1;
    std::printf("glue_wide_host ok (%d records, %d words)\n", n_rec, n_words);
    return 0;
}
