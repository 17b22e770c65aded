// Host-only checks of the wide repair call's inline host logic (repairwide.h; no
// GPU work and no libhbec): record sizes and strides, the per-entry word, and
// where the survivor and row indices and the tables land.  Built under
// AddressSanitizer + UBSan by tests/test_repair_wide_host.py and run directly.
#include <cstdio>
#include <vector>

#include "../../hummingbird_amd/csrc/repairwide.h"

#define CHECK(c) \
    do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

using namespace hbec;

static int sizes_and_words() {
    for (int k : {1, 12, 13, 32})
        for (int a = 1; a <= kMaxR; ++a) {
            const uint32_t w = rw_record_words(k, a);
            CHECK(w % 4 == 0 && w >= kRwHdr + 5u * k * a && w < kRwHdr + 5u * k * a + 4);
        }
    CHECK(rw_record_words(1, 1) == 20 && rw_record_words(12, 4) == 252 && rw_record_words(13, 1) == 80);
    CHECK(rw_record_words(32, 4) == 652 && kRwHdr % 4 == 0 && kRwHdr > kRwRowsWord && kRwSurvWords * 4 == kRwMaxK);
    CHECK(rw_shape(1, 1) && rw_shape(32, 4) && !rw_shape(33, 4) && !rw_shape(4, 5) && !rw_shape(0, 1) && !rw_shape(4, 0));
    for (int ro = 0; ro <= kMaxR; ++ro)
        for (int rc = 0; ro + rc <= kMaxR; ++rc)
            for (uint32_t pat : {0u, 1u, 255u, 256u, 65534u, 65535u}) {
                const uint32_t w = rw_word(ro, rc, pat);
                CHECK(w != 0u && rw_word_out(w) == (uint32_t)ro && rw_word_chk(w) == (uint32_t)rc && rw_word_pat(w) == pat);
            }
    return 0;
}

// `ro` shards lost among the first: the middle record of three, `stride` apart
static int record(int k, int ro, int rc, uint32_t stride) {
    const int a = ro + rc;
    std::vector<int> surv(k), outs(ro), chk(rc);
    for (int q = 0; q < ro; ++q) outs[q] = 2 * q;
    for (int j = 0; j < k; ++j) surv[j] = j < ro ? 2 * j + 1 : j + ro;
    for (int q = 0; q < rc; ++q) chk[q] = k + ro + q;
    std::vector<uint8_t> orows((size_t)ro * k), crows((size_t)rc * k);
    for (size_t i = 0; i < orows.size(); ++i) orows[i] = (uint8_t)(7 * i + 3);
    for (size_t i = 0; i < crows.size(); ++i) crows[i] = (uint8_t)(11 * i + 5);
    std::vector<uint32_t> buf(3 * (size_t)stride, 0u);
    uint32_t* p = buf.data() + stride;
    rw_pattern(p, k, surv.data(), outs.data(), ro, orows.data(), chk.data(), rc, crows.data());
    for (size_t i = 0; i < buf.size(); ++i)
        if (i < stride || i >= stride + rw_record_words(k, a)) CHECK(buf[i] == 0u);
    for (int j = 0; j < kRwMaxK; ++j)  // as the kernel's in_base(j) reads it
        CHECK(((p[j >> 2] >> (8 * (j & 3))) & 0xFFu) == (j < k ? (uint32_t)surv[j] : 0u));
    for (int q = 0; q < 4; ++q)
        CHECK(((p[kRwRowsWord] >> (8 * q)) & 0xFFu) == (q < ro ? (uint32_t)outs[q] : q < a ? (uint32_t)chk[q - ro] : 0u));
    for (int j = 0; j < k; ++j)
        for (int q = 0; q < a; ++q) {
            uint32_t t[5];
            perm_table(q < ro ? orows[(size_t)q * k + j] : crows[(size_t)(q - ro) * k + j], t);
            for (int z = 0; z < 5; ++z) CHECK(p[kRwHdr + 5 * (j * a + q) + z] == t[z]);
        }
    return 0;
}

int main() {
    if (sizes_and_words()) return 1;
    int n = 0;
    for (int k : {1, 12, 13, 32})
        for (int ro = 0; ro <= 4 && ro <= k; ++ro)
            for (int rc = ro ? 0 : 1; ro + rc <= 4; ++rc, ++n)  // at its own size and at a four-row call's stride
                if (record(k, ro, rc, rw_record_words(k, ro + rc)) || record(k, ro, rc, rw_record_words(k, 4))) return 1;
    std::printf("repair_wide_host ok (%d records)\n", n);
    return 0;
}
