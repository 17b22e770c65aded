// Host-only checks of the locate call's inline host logic (locate.h; no GPU work
// and no libhbec): the per-byte rule loc_classify, the decode of a word, the
// coefficient read back from a pattern record, and the routing.  For every mask
// of 4+2 and 8+3 with two or more checked shards, every single-shard error
// value 1..255 must locate its shard, and random syndromes must agree with a
// brute-force search over the columns of [rows | I] written here.  Built with
// the host compiler under AddressSanitizer + UBSan by tests/test_locate_host.py
// and run directly.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hummingbird_amd/csrc/locate.h"

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

namespace {

// shift-and-xor product, independent of gf256.h's log tables
uint8_t slow_mul(uint8_t a, uint8_t b) {
    unsigned r = 0, x = a;
    for (int i = 0; i < 8; ++i) {
        if (b & (1u << i)) r ^= x;
        x <<= 1;
        if (x & 0x100u) x ^= 0x11Du;
    }
    return (uint8_t)r;
}

struct Mask {
    int k = 0, r = 0;
    std::vector<int> surv, checked;
    std::vector<uint8_t> rows;  // r x k
    uint32_t present = 0;
};

// the decode rows of one mask: row q = M[checked q] x inverse(M[survivors])
bool resolve(int k, int m, const uint8_t* present, Mask& o) {
    using namespace hbec;
    const int n = k + m;
    o.k = k;
    o.surv.assign(k, 0);
    o.checked.assign(n, 0);
    if (!vm_select(k, n, present, o.surv.data(), o.checked.data(), &o.r)) return false;
    o.checked.resize(o.r);
    std::vector<uint8_t> mat, sub((size_t)k * k), inv((size_t)k * k);
    if (!build_matrix(k, m, mat)) return false;
    for (int j = 0; j < k; ++j)
        for (int c = 0; c < k; ++c) sub[(size_t)j * k + c] = mat[(size_t)o.surv[j] * k + c];
    if (!invert(k, sub.data(), inv.data())) return false;
    o.rows.assign((size_t)o.r * k, 0);
    for (int q = 0; q < o.r; ++q)
        for (int t = 0; t < k; ++t) {
            uint8_t v = 0;
            for (int i = 0; i < k; ++i) v ^= slow_mul(mat[(size_t)o.checked[q] * k + i], inv[(size_t)i * k + t]);
            o.rows[(size_t)q * k + t] = v;
        }
    o.present = loc_present_bits(k, o.surv.data(), o.r, o.checked.data());
    return true;
}

// bit j for every present shard j whose column has a multiple equal to s
uint32_t brute_candidates(const Mask& mk, const uint8_t* s) {
    uint32_t cand = 0;
    for (int j = 0; j < mk.k + mk.r; ++j)
        for (int e = 1; e < 256; ++e) {
            bool eq = true;
            for (int q = 0; q < mk.r && eq; ++q) {
                const uint8_t c = j < mk.k ? mk.rows[(size_t)q * mk.k + j] : (uint8_t)(j - mk.k == q ? 1 : 0);
                eq = slow_mul((uint8_t)e, c) == s[q];
            }
            if (eq) {
                cand |= 1u << (j < mk.k ? mk.surv[j] : mk.checked[j - mk.k]);
                break;
            }
        }
    return cand;
}

int every_mask(int k, int m, uint32_t* seed) {
    using namespace hbec;
    const int n = k + m;
    int n_masks = 0;
    for (uint32_t bits = 0; bits < (1u << n); ++bits) {
        if (__builtin_popcount(bits) < k + 2) continue;
        uint8_t present[16];
        for (int i = 0; i < n; ++i) present[i] = (bits >> i) & 1u ? (uint8_t)(1 + i) : 0;  // any non-zero byte
        Mask mk;
        CHECK(resolve(k, m, present, mk) && mk.r >= 2 && mk.present == bits);
        ++n_masks;
        for (size_t i = 0; i < mk.rows.size(); ++i) CHECK(mk.rows[i] != 0);
        // the record holds the raw coefficients
        std::vector<uint32_t> buf(8, 0u);  // a record that does not start at 0
        const uint32_t off = loc_pattern(buf, k, mk.surv.data(), mk.checked.data(), mk.r, mk.rows.data());
        CHECK(off == 2);
        for (int q = 0; q < mk.r; ++q)
            for (int t = 0; t < k; ++t)
                CHECK(loc_pattern_coef(buf.data() + 4 * off, mk.r, t, q) == mk.rows[(size_t)q * k + t]);
        // one corrupt shard, every error value: exactly that shard is left
        uint8_t s[4];
        for (int j = 0; j < k + mk.r; ++j) {
            const int shard = j < k ? mk.surv[j] : mk.checked[j - k];
            for (int e = 1; e < 256; ++e) {
                for (int q = 0; q < mk.r; ++q)
                    s[q] = j < k ? slow_mul((uint8_t)e, mk.rows[(size_t)q * k + j]) : (uint8_t)(j - k == q ? e : 0);
                const uint32_t w = loc_classify(k, mk.r, mk.rows.data(), s, mk.present, mk.surv.data(),
                                                mk.checked.data());
                CHECK(w == (kLocBad | (mk.present & ~(1u << shard))));
                CHECK(loc_decode(k, m, present, w) == shard);
            }
        }
        // random syndromes, some components forced to zero: the brute-force column search
        for (int it = 0; it < 200; ++it) {
            uint32_t any = 0;
            for (int q = 0; q < mk.r; ++q) {
                *seed = *seed * 1664525u + 1013904223u;
                s[q] = (*seed >> 28) < 5u ? 0 : (uint8_t)(*seed >> 16);
                any |= s[q];
            }
            const uint32_t w = loc_classify(k, mk.r, mk.rows.data(), s, mk.present, mk.surv.data(),
                                            mk.checked.data());
            if (!any) {
                CHECK(w == 0u);
                continue;
            }
            const uint32_t cand = brute_candidates(mk, s);
            CHECK(__builtin_popcount(cand) <= 1);  // the columns are pairwise independent
            CHECK(w == (kLocBad | (mk.present & ~cand)));
        }
        // two corrupt shards at one position, r >= 3: never attributed to one
        if (mk.r >= 3)
            for (int it = 0; it < 60; ++it) {
                *seed = *seed * 1664525u + 1013904223u;
                const int j1 = (int)((*seed >> 8) % (uint32_t)(k + mk.r));
                const int j2 = (j1 + 1 + (int)((*seed >> 16) % (uint32_t)(k + mk.r - 1))) % (k + mk.r);
                const uint8_t e1 = (uint8_t)(1 + (*seed >> 24) % 255u), e2 = (uint8_t)(1 + (*seed >> 3) % 255u);
                for (int q = 0; q < mk.r; ++q) {
                    const uint8_t c1 = j1 < k ? mk.rows[(size_t)q * k + j1] : (uint8_t)(j1 - k == q);
                    const uint8_t c2 = j2 < k ? mk.rows[(size_t)q * k + j2] : (uint8_t)(j2 - k == q);
                    s[q] = slow_mul(e1, c1) ^ slow_mul(e2, c2);
                }
                const uint32_t w = loc_classify(k, mk.r, mk.rows.data(), s, mk.present, mk.surv.data(),
                                                mk.checked.data());
                CHECK(w == (kLocBad | mk.present) && loc_decode(k, m, present, w) == kLocMultiple);
            }
    }
    CHECK(n_masks == (n == 6 ? 1 : 1 + 11));  // all present; 8+3 also one lost
    return 0;
}

int one_checked() {
    using namespace hbec;
    // r = 1: nothing is ruled out, whatever the byte
    const uint8_t present[6] = {1, 0, 1, 1, 1, 1};
    Mask mk;
    CHECK(resolve(4, 2, present, mk) && mk.r == 1 && mk.present == 0x3Du);
    for (int e = 0; e < 256; ++e) {
        const uint8_t s[1] = {(uint8_t)e};
        const uint32_t w = loc_classify(4, 1, mk.rows.data(), s, mk.present, mk.surv.data(), mk.checked.data());
        CHECK(w == (e ? kLocBad : 0u));
    }
    CHECK(loc_decode(4, 2, present, kLocBad) == kLocAmbiguous);
    return 0;
}

int decode() {
    using namespace hbec;
    const uint8_t full[6] = {1, 1, 1, 1, 1, 1}, lost[6] = {1, 1, 0, 1, 9, 1};
    CHECK(loc_decode(4, 2, full, 0u) == kLocClean);
    CHECK(loc_decode(4, 2, full, 0x3Fu) == kLocClean);  // no kLocBad: bits of the caller's own
    for (int j = 0; j < 6; ++j) CHECK(loc_decode(4, 2, full, kLocBad | (0x3Fu & ~(1u << j))) == j);
    CHECK(loc_decode(4, 2, full, kLocBad | 0x3Fu) == kLocMultiple);
    CHECK(loc_decode(4, 2, full, kLocBad) == kLocAmbiguous);
    CHECK(loc_decode(4, 2, full, kLocBad | 0x0Fu) == kLocAmbiguous);
    // a missing shard is never a candidate, ruled out or not
    CHECK(loc_decode(4, 2, lost, kLocBad | 0x33u) == 3);
    CHECK(loc_decode(4, 2, lost, kLocBad | 0x3Bu) == kLocMultiple);
    CHECK(loc_decode(4, 2, full, kLocSkipped) == kLocUnchecked);
    CHECK(loc_decode(4, 2, full, kLocNothing) == kLocUnchecked);
    CHECK(loc_decode(4, 2, full, kLocBad | kLocSkipped | 0x3Eu) == kLocUnchecked);
    // 12+4: bit 15
    uint8_t wide[16];
    for (int i = 0; i < 16; ++i) wide[i] = 1;
    CHECK(loc_decode(12, 4, wide, kLocBad | 0x7FFFu) == 15);
    return 0;
}

int routing() {
    using namespace hbec;
    CHECK(loc_route(4, 2, 0) == kVmSkip && loc_route(13, 2, 0) == kVmSkip);
    for (uint64_t s : {(uint64_t)1, (uint64_t)3968, kPos32MaxShard}) {
        CHECK(loc_route(4, 2, s) == kVmKernel && loc_route(12, 4, s) == kVmKernel);
        CHECK(loc_route(13, 2, s) == kVmOther && loc_route(4, 5, s) == kVmOther);
    }
    CHECK(loc_route(4, 2, kPos32MaxShard + 1) == kVmOther);
    CHECK((kLocBad & kLocSkipped) == 0u && (kLocBad | kLocSkipped | kLocNothing | kLocRuledMask) == 0xE000FFFFu);
    return 0;
}

}  // namespace

int main() {
    uint32_t seed = 12345u;
    if (every_mask(4, 2, &seed) || every_mask(8, 3, &seed) || one_checked() || decode() || routing()) return 1;
    std::puts("locate_host ok");
    return 0;
}
