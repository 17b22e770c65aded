// Host-only checks of splitwide.h (no GPU, no libhbec): the record, the word and the three-phase
// cut.  Built under ASan + UBSan by tests/test_split_wide_host.py and run directly.
#include <cstdio>
#include <vector>

#include "../../hummingbird_amd/csrc/splitwide.h"

#define CHECK(c) \
    do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using namespace hbec;

// the record of k + m against rw_pattern's layout, between two guard records
static int record(int k, int m) {
    std::vector<uint8_t> rows((size_t)m * k);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (uint8_t)(11 * i + 5);
    const uint32_t words = rw_record_words(k, m);
    std::vector<uint32_t> buf(3 * (size_t)words, 0u);
    uint32_t* p = buf.data() + words;
    sw_pattern(p, k, m, rows.data());
    for (size_t i = 0; i < buf.size(); ++i)
        if (i < words || i >= 2 * (size_t)words) CHECK(buf[i] == 0u);
    for (int j = 0; j < kRwMaxK; ++j) CHECK(((p[j >> 2] >> (8 * (j & 3))) & 0xFFu) == (j < k ? (uint32_t)j : 0u));
    for (int q = 0; q < 4; ++q) CHECK(((p[kRwRowsWord] >> (8 * q)) & 0xFFu) == (q < m ? (uint32_t)(k + q) : 0u));
    for (uint32_t i = kRwRowsWord + 1; i < kRwHdr; ++i) CHECK(p[i] == 0u);
    for (int j = 0; j < k; ++j)
        for (int q = 0; q < m; ++q) {
            uint32_t t[5];
            perm_table(rows[(size_t)q * k + j], t);
            for (int z = 0; z < 5; ++z) CHECK(p[kRwHdr + 5 * (j * m + q) + z] == t[z]);
        }
    return 0;
}

// every legal length of (k, S) against V_j = clamp(len - j S, 0, S) taken input by input
static int cuts(int* n) {
    for (uint32_t k : {13u, 32u})
        for (uint32_t S : {1u, 5u, 16u, 993u})
            for (uint64_t len = (uint64_t)k * S - k + 1; len <= (uint64_t)k * S; ++len, ++*n) {
                CHECK(split_len_ok(len, k, S));
                const SwCut c = sw_cut(len, S, k);
                CHECK(c.whole >= 1u && c.whole <= k && c.partial < S);
                CHECK(c.pad_from == c.whole + (c.partial ? 1u : 0u) && c.pad_from <= k);
                for (uint32_t j = 0; j < k; ++j) {
                    const uint64_t v = split_valid(len, j, S);
                    CHECK(v == (j < c.whole ? S : (j == c.whole ? c.partial : 0u)));
                    CHECK((v == 0) == (j >= c.pad_from));
                }
            }
    return 0;
}

int main() {
    int n_rec = 0, n_cut = 0;
    for (int k : {1, 12, 13, 32})
        for (int m = 1; m <= 4; ++m, ++n_rec)
            if (record(k, m)) return 1;
    for (int m = 1; m <= kMaxR; ++m) {  // the word: m rows to code, none checked, record 0
        const uint32_t w = sw_word(m, 17, 17 * 13 - 2);
        CHECK(sw_word(m, 0, 0) == 0u && sw_word(m, 17, 0) == 0u && w == rw_word(m, 0, 0) && w != 0u);
        CHECK(rw_word_out(w) == (uint32_t)m && rw_word_chk(w) == 0u && rw_word_pat(w) == 0u);
    }
    if (cuts(&n_cut)) return 1;
    std::printf("split_wide_host ok (%d records, %d cuts)\n", n_rec, n_cut);
    return 0;
}
