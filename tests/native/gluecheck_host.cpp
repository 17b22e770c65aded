// gluecheck_host.cpp — csrc/gluecheck.h alone under AddressSanitizer + UBSan: gc_record of every mask of
// 4+2 and 3+2 with at most m shards missing and 300 each of 8+3 and 12+4 against a brute-force model.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../hummingbird_amd/csrc/gluecheck.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint8_t gmul(uint8_t a, uint8_t b) { return hbec::field().mul(a, b); }
static bool table_is(const uint32_t* t, uint8_t c) {  // the five words at t are the v_perm tables of c
    uint32_t want[5];
    hbec::perm_table(c, want);
    return std::memcmp(t, want, sizeof want) == 0 && (uint8_t)(t[0] >> 8) == c;
}

static uint64_t g_records = 0;

static int check_mask(int k, int m, const std::vector<uint8_t>& enc, const std::vector<uint8_t>& mask) {
    std::vector<int> surv, chk, outs;  // the model: by walking the mask
    for (int i = 0; i < k + m; ++i) {
        if (mask[i])
            ((int)surv.size() < k ? surv : chk).push_back(i);
        else if (i < k)
            outs.push_back(i);
    }
    const int r = (int)chk.size(), o = (int)outs.size(), A = r + o;
    CHECK((int)surv.size() == k && A <= m);
    // the rows handed in: shard x over the survivors is enc[x] * inverse(enc[survivors])
    std::vector<uint8_t> sub((size_t)k * k), inv((size_t)k * k), rows((size_t)(A > 0 ? A : 1) * k, 0);
    for (int t = 0; t < k; ++t)
        for (int c = 0; c < k; ++c) sub[(size_t)t * k + c] = enc[(size_t)surv[t] * k + c];
    CHECK(hbec::invert(k, sub.data(), inv.data()));
    for (int q = 0; q < A; ++q)
        for (int t = 0; t < k; ++t)
            for (int c = 0; c < k; ++c)
                rows[(size_t)q * k + t] ^= gmul(enc[(size_t)(q < r ? chk[q] : outs[q - r]) * k + c], inv[(size_t)c * k + t]);

    std::vector<uint32_t> buf(12, 0xDEADBEEFu);  // a record is appended, at a 16-B unit
    CHECK(hbec::gc_record(buf, k, surv.data(), chk.data(), r, rows.data(), outs.data(), o, rows.data() + (size_t)r * k) == 3 &&
          buf[11] == 0xDEADBEEFu);
    const uint32_t words = (uint32_t)buf.size() - 12, tables = hbec::kGcHdr + 5u * (uint32_t)(k * A);
    const uint32_t inv_at = hbec::gc_inverse_at(k, A);
    CHECK(words == hbec::gc_record_words(k, r, o) && words % 4 == 0 && inv_at % 4 == 0 && inv_at >= tables && inv_at < tables + 4);
    CHECK(hbec::gc_word(A, 3) == (((uint32_t)A << 28) | 3u) && hbec::kGlueSkip >> 28 > 4u);  // no instance's row count
    const uint32_t* p = buf.data() + 12;
    uint32_t hdr[8] = {0, 0, 0, 0, (uint32_t)r | ((uint32_t)o << 8), 0, 0, 0};
    for (int j = 0; j < k; ++j) hdr[j / 4] |= (uint32_t)surv[j] << (8 * (j % 4));
    for (int q = 0; q < A; ++q) hdr[3] |= (uint32_t)(q < r ? chk[q] : outs[q - r]) << (8 * q);
    for (int w = 0; w < 8; ++w) CHECK(p[w] == hdr[w]);
    for (int t = 0; t < k; ++t)
        for (int q = 0; q < A; ++q) {
            const uint32_t* tab = p + hbec::kGcHdr + 5 * (t * A + q);
            CHECK(table_is(tab, rows[(size_t)q * k + t]) && hbec::gc_record_coef(p, A, q, t) == rows[(size_t)q * k + t]);
        }
    for (uint32_t w = tables; w < inv_at; ++w) CHECK(p[w] == 0);  // the padding
    if (r) {
        for (int t = 0; t < k; ++t) {
            const uint8_t i = hbec::gc_record_inverse(p, k, A, t);
            CHECK(gmul(i, rows[t]) == 1 && table_is(p + inv_at + 5 * t, i));
        }
        for (uint32_t w = inv_at + 5u * (uint32_t)k; w < words; ++w) CHECK(p[w] == 0);
    }
    ++g_records;
    return 0;
}

int main() {
    const int shapes[4][3] = {{4, 2, 0}, {3, 2, 0}, {8, 3, 300}, {12, 4, 300}};  // k, m, sample (0: every mask)
    for (const auto& sh : shapes) {
        const int k = sh[0], m = sh[1], n = k + m;
        std::vector<uint8_t> enc;
        CHECK(hbec::build_matrix(k, m, enc));
        const uint32_t count = sh[2] ? (uint32_t)sh[2] : 1u << n;
        for (uint32_t i = 0; i < count; ++i) {
            std::vector<uint8_t> mask((size_t)n, 1);
            if (sh[2]) {
                for (uint32_t lost = i % (uint32_t)(m + 1); lost; --lost) mask[(i * 2654435761u >> (7 + 5 * lost)) % (uint32_t)n] = 0;
            } else {
                int gone = 0;
                for (int j = 0; j < n; ++j) gone += (mask[j] = (i >> j) & 1u) ? 0 : 1;
                if (gone > m) continue;
            }
            if (check_mask(k, m, enc, mask)) return 1;
        }
    }
    std::printf("gluecheck_host ok (%llu records)\n", (unsigned long long)g_records);
    return 0;
}
