// Host-only checks of the heal call's inline host logic (heal.h; no GPU work and
// no libhbec): the rule that turns a locate word into the shard to rewrite,
// against loc_decode (the body of hbec_locate_decode) for every mask of 4+2 and
// 8+3 with at least k present, every 16-bit ruled-out set and every combination
// of the status bits; and the staging heal_build makes.  With a file name as its
// argument the program reads what hbec_decode_rows and hbec_check_rows answered
// for every mask of 4+2 and 8+3 with something missing, one mask a line:
//   k m 0  mask[k+m]  surv[k]  r_o outs[r_o] rows[r_o k]  r_c checked[r_c] rows[r_c k]
// stages every mask p of those shapes, and checks that the word of (p, j) is 0
// exactly where it must be and otherwise names the record rp_pattern builds from
// the library's rows of p \ {j}, word for word.  Built with the host compiler
// under AddressSanitizer + UBSan by tests/test_heal_host.py and run directly.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../hummingbird_amd/csrc/heal.h"

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

// The pick is hbec_locate_decode's rule: a shard exactly when decode names one,
// unnamed exactly when decode says AMBIGUOUS or MULTIPLE, not the call's
// business exactly when it says CLEAN or UNCHECKED.
static int pick(long* n_words) {
    using namespace hbec;
    const uint32_t status[3] = {kLocBad, kLocSkipped, kLocNothing};
    for (auto km : {std::pair<int, int>{4, 2}, {8, 3}}) {
        const int k = km.first, m = km.second, n = k + m;
        for (uint32_t bits = 0; bits < (1u << n); ++bits) {
            if (__builtin_popcount(bits) < k) continue;
            uint8_t present[16] = {0};
            for (int i = 0; i < n; ++i) present[i] = (uint8_t)((bits >> i) & 1u);
            CHECK(heal_mask_bits(n, present) == bits);
            for (uint32_t st = 0; st < 8; ++st) {
                uint32_t hi = (st & 4u) ? 1u << 20 : 0u;  // a bit of the caller's own rides along
                for (int b = 0; b < 3; ++b) hi |= ((st >> b) & 1u) ? status[b] : 0u;
                for (uint32_t ruled = 0; ruled < 65536u; ++ruled) {
                    const uint32_t w = hi | ruled;
                    const int d = loc_decode(k, m, present, w);
                    const bool ex = heal_examined(w);
                    const int j = heal_pick(bits, w);
                    if (d >= 0)
                        CHECK(ex && j == d);
                    else if (d == kLocAmbiguous || d == kLocMultiple)
                        CHECK(ex && j == -1);
                    else
                        CHECK(!ex && (d == kLocClean || d == kLocUnchecked));
                    CHECK(j == -1 || (j < n && ((bits >> j) & 1u) && !((w >> j) & 1u)));
                    ++*n_words;
                }
            }
        }
    }
    CHECK(!heal_examined(0u) && !heal_examined(kLocBad | kLocSkipped) && !heal_examined(kLocBad | kLocNothing));
    CHECK(heal_examined(kLocBad) && heal_pick(0x3Fu, kLocBad | 0x3Bu) == 2 && heal_pick(0x3Fu, kLocBad) == -1);
    CHECK(kHealDone == 4u && kHealUnnamed == 8u && kHealNone != 0u && kHealRow == 16);
    return 0;
}

struct Rows {
    std::vector<int> surv, outs, chk;
    std::vector<uint8_t> orows, crows;
};
typedef std::map<std::pair<int, uint32_t>, Rows> Library;  // (k, mask bits) -> the library's answers

static int read_library(const char* path, Library& lib) {
    using namespace hbec;
    std::ifstream f(path);
    CHECK(f.good());
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        int k = 0, m = 0, data_only = 0, ro = 0, rc = 0;
        in >> k >> m >> data_only;
        CHECK(in && k >= 1 && k <= kOddMaxK && m >= 1 && m <= kMaxR && data_only == 0);
        const int n = k + m;
        Rows r;
        std::vector<int> mask;
        auto ints = [&](std::vector<int>& v, int c) {
            v.resize(c);
            for (int& x : v) in >> x;
        };
        auto bytes = [&](std::vector<uint8_t>& v, int c) {
            v.resize(c);
            for (uint8_t& x : v) {
                int t = -1;
                in >> t;
                x = (uint8_t)t;
            }
        };
        ints(mask, n);
        ints(r.surv, k);
        in >> ro;
        CHECK(in && ro >= 1 && ro <= m);
        ints(r.outs, ro);
        bytes(r.orows, ro * k);
        in >> rc;
        CHECK(in && rc >= 0 && ro + rc == m);
        ints(r.chk, rc);
        bytes(r.crows, rc * k);
        CHECK(!in.fail());
        uint32_t bits = 0;
        for (int i = 0; i < n; ++i) bits |= mask[i] ? 1u << i : 0u;
        CHECK(lib.emplace(std::make_pair(k, bits), r).second);
    }
    return 0;
}

static int staging(const Library& lib, int* n_pairs) {
    using namespace hbec;
    for (auto km : {std::pair<int, int>{4, 2}, {8, 3}}) {
        const int k = km.first, m = km.second, n = k + m;
        std::vector<uint32_t> masks;
        for (uint32_t bits = 0; bits < (1u << n); ++bits)
            if (__builtin_popcount(bits) >= k) masks.push_back(bits);
        masks.push_back(masks[3]);  // a mask listed twice shares its records
        int asked = 0;
        auto rows_of = [&](const uint8_t* mask, int* surv, int* outs, int* n_out, uint8_t* orows, int* chk,
                           int* n_chk, uint8_t* crows) {
            ++asked;
            auto it = lib.find(std::make_pair(k, heal_mask_bits(n, mask)));
            if (it == lib.end()) return false;
            const Rows& r = it->second;
            std::copy(r.surv.begin(), r.surv.end(), surv);
            std::copy(r.outs.begin(), r.outs.end(), outs);
            std::copy(r.orows.begin(), r.orows.end(), orows);
            std::copy(r.chk.begin(), r.chk.end(), chk);
            std::copy(r.crows.begin(), r.crows.end(), crows);
            *n_out = (int)r.outs.size();
            *n_chk = (int)r.chk.size();
            return true;
        };
        HealStage h;
        CHECK(heal_build(h, k, m, masks, rows_of) && !h.overflow);
        // one record per distinct mask with >= k present and something missing: each asked for once
        size_t distinct = 0;
        for (uint32_t bits = 0; bits < (1u << n); ++bits)
            distinct += __builtin_popcount(bits) >= k && __builtin_popcount(bits) < n;
        CHECK((size_t)asked == distinct && h.rec_of.size() == distinct);
        CHECK(h.n_rows == masks.size() && h.present_at == h.words_at + masks.size() * kHealRow);
        CHECK(h.index_at == h.present_at + masks.size() && h.stage.size() == h.index_at);
        CHECK(h.words_at % 4 == 0);  // records are whole 16-B units
        for (size_t row = 0; row < masks.size(); ++row) {
            const uint32_t bits = masks[row];
            CHECK(h.stage[h.present_at + row] == bits);
            const int present = __builtin_popcount(bits);
            for (int j = 0; j < kHealRow; ++j) {
                const uint32_t w = h.stage[h.words_at + row * kHealRow + j];
                const bool named = j < n && ((bits >> j) & 1u) && present - 1 >= k;
                CHECK((w != 0u) == named);  // 0 exactly where no record may be chosen
                if (!named) continue;
                CHECK(w != kRpNothing && (int)rp_word_out(w) == n - present + 1 &&
                      (int)rp_word_chk(w) == present - 1 - k && rp_word_out(w) + rp_word_chk(w) == (uint32_t)m);
                const Rows& r = lib.at(std::make_pair(k, bits & ~(1u << j)));
                // shard j is an output and no survivor or checked shard: it is never read
                bool out_j = false;
                for (int o : r.outs) out_j |= o == j;
                CHECK(out_j);
                for (int s : r.surv) CHECK(s != j && ((bits >> s) & 1u));
                for (int c : r.chk) CHECK(c != j && ((bits >> c) & 1u));
                std::vector<uint32_t> want;
                rp_pattern(want, k, r.surv.data(), r.outs.data(), (int)r.outs.size(), r.orows.data(), r.chk.data(),
                           (int)r.chk.size(), r.crows.data());
                const size_t at = (size_t)rp_word_rec(w) * 4;
                CHECK(at + want.size() <= h.words_at);
                for (size_t q = 0; q < want.size(); ++q) CHECK(h.stage[at + q] == want[q]);
                ++*n_pairs;
            }
        }
        const size_t last = masks.size() - 1;
        for (int j = 0; j < kHealRow; ++j)
            CHECK(h.stage[h.words_at + last * kHealRow + j] == h.stage[h.words_at + 3 * kHealRow + j]);
        // a failing rows_of fails the build
        HealStage bad;
        CHECK(!heal_build(bad, k, m, masks, [](const uint8_t*, int*, int*, int*, uint8_t*, int*, int*, uint8_t*) {
            return false;
        }));
        CHECK(!bad.overflow);
        // records past rp_word's 22-bit offset: refused, not wrapped
        HealStage big;
        big.stage.assign((size_t)kRpNothing * 4 - 8, 0u);
        CHECK(!heal_build(big, k, m, masks, rows_of) && big.overflow);
    }
    return 0;
}

static int routing() {
    using namespace hbec;
    for (uint64_t s : {(uint64_t)1, (uint64_t)3967, (uint64_t)3968, kPos32MaxShard}) {
        CHECK(heal_route(4, 2, s) == kVmKernel && heal_route(12, 4, s) == kVmKernel);
        CHECK(heal_route(13, 2, s) == kVmOther && heal_route(4, 5, s) == kVmOther);
    }
    CHECK(heal_route(4, 2, 0) == kVmSkip && heal_route(4, 2, kPos32MaxShard + 1) == kVmOther);
    return 0;
}

int main(int argc, char** argv) {
    long n_words = 0;
    if (pick(&n_words) || routing()) return 1;
    int n_pairs = 0;
    if (argc > 1) {
        Library lib;
        if (read_library(argv[1], lib) || staging(lib, &n_pairs)) return 1;
    }
    std::printf("heal_host ok (%ld words, %d records of a mask with one shard left out)\n", n_words, n_pairs);
    return 0;
}
