// Host-only checks of the repair call's inline host logic (repair.h; no GPU work
// and no libhbec): the per-entry word for every (r_o, r_c), the pattern record's
// layout (outputs first, then checked shards) and the routing of sizes and
// shapes.  With a file name as its argument the program also reads what
// hbec_decode_rows and hbec_check_rows answered for a list of masks, one mask a
// line:
//   k m data_only  mask[k+m]  surv[k]  r_o outs[r_o] rows[r_o k]  r_c checked[r_c] rows[r_c k]
// and checks the record rp_pattern builds from them word by word.  Built with
// the host compiler under AddressSanitizer + UBSan by
// tests/test_repair_mixed_host.py and run directly.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../hummingbird_amd/csrc/repair.h"

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static int words() {
    using namespace hbec;
    int pairs = 0;
    for (int ro = 0; ro <= kMaxR; ++ro)
        for (int rc = 0; ro + rc <= kMaxR; ++rc) {
            if (ro + rc == 0) continue;
            ++pairs;
            for (uint32_t rec : {0u, 1u, 11u, kRpRecMask - 1u, kRpRecMask}) {
                const uint32_t w = rp_word(ro, rc, rec);
                CHECK(w != 0u && w != kRpNothing);
                CHECK(rp_word_out(w) == (uint32_t)ro && rp_word_chk(w) == (uint32_t)rc && rp_word_rec(w) == rec);
            }
        }
    CHECK(pairs == 14);
    // exactly k present and nothing to rebuild: no record, told apart from "no
    // tiles" (0) and from every word with a count
    CHECK(rp_word(0, 0, 0) == kRpNothing && rp_word(0, 0, 77) == kRpNothing && kRpNothing != 0u);
    CHECK(rp_word_out(kRpNothing) == 0u && rp_word_chk(kRpNothing) == 0u);
    // no record starts at the offset kRpNothing carries: 65536 of the largest fit below it
    CHECK((uint64_t)65536 * mp_pattern_words(kOddMaxK, kMaxR) / 4 < kRpNothing);
    CHECK(kRpOutShift + 3 <= 32 && kRpChkShift + 3 == kRpOutShift);
    return 0;
}

static int records() {
    using namespace hbec;
    std::vector<uint32_t> buf;
    // 4+2, shard 1 lost: survivors 0 2 3 4, shard 1 rebuilt, shard 5 checked
    const int sv[4] = {0, 2, 3, 4}, out[1] = {1}, chk[1] = {5};
    const uint8_t orow[4] = {0x1b, 0x02, 0xd7, 0x8e}, crow[4] = {0x03, 0x55, 0xa0, 0x01};
    CHECK(rp_pattern(buf, 4, sv, out, 1, orow, chk, 1, crow) == 0);
    CHECK(buf.size() == mp_pattern_words(4, 2) && buf.size() % 4 == 0);
    CHECK(buf[0] == 0x04030200u && buf[1] == 0 && buf[2] == 0 && buf[3] == 0x0501u);
    for (int j = 0; j < 4; ++j) {
        uint32_t t[5];
        perm_table(orow[j], t);
        for (int q = 0; q < 5; ++q) CHECK(buf[kMPatHdr + 5 * (j * 2 + 0) + q] == t[q]);
        perm_table(crow[j], t);
        for (int q = 0; q < 5; ++q) CHECK(buf[kMPatHdr + 5 * (j * 2 + 1) + q] == t[q]);
    }
    // nothing checked: the record of the mixed plan reconstruct; nothing rebuilt: Verify's
    std::vector<uint32_t> a, b;
    CHECK(rp_pattern(a, 4, sv, out, 1, orow, nullptr, 0, nullptr) == 0 && mp_pattern(b, 4, sv, out, 1, orow) == 0);
    CHECK(a == b);
    a.clear();
    b.clear();
    CHECK(rp_pattern(a, 4, sv, nullptr, 0, nullptr, chk, 1, crow) == 0 && vm_pattern(b, 4, sv, chk, 1, crow) == 0);
    CHECK(a == b);
    // a second record starts where the first ends, in 16-B units
    const uint32_t off = rp_pattern(buf, 4, sv, out, 1, orow, chk, 1, crow);
    CHECK(off * 4 == mp_pattern_words(4, 2) && buf.size() == 2 * mp_pattern_words(4, 2));
    return 0;
}

static int routing() {
    using namespace hbec;
    const uint64_t T = 3968;  // mixed_plan_tile_bytes(): kUnalignedU windows of kUnalignedWindow
    CHECK(rp_route(4, 2, 0) == kVmSkip && rp_route(13, 4, 0) == kVmSkip);
    for (uint64_t s : {(uint64_t)1, T - 1, T, T + 1, kPos32MaxShard}) {
        CHECK(rp_route(4, 2, s) == kVmKernel && rp_route(12, 4, s) == kVmKernel && rp_route(1, 1, s) == kVmKernel);
        CHECK(rp_route(13, 2, s) == kVmOther && rp_route(16, 4, s) == kVmOther && rp_route(4, 5, s) == kVmOther);
    }
    CHECK(rp_route(4, 2, kPos32MaxShard + 1) == kVmOther && rp_route(8, 3, 1ull << 33) == kVmOther);
    // the same entries mp_build gives tiles to: the plan's list is shared
    std::vector<MSrc> src;
    for (uint64_t s : {(uint64_t)0, (uint64_t)1, T - 1, T, T + 1, kPos32MaxShard, kPos32MaxShard + 1})
        src.push_back(MSrc{4096, 1u << 20, s});
    for (auto km : {std::pair<int, int>{4, 2}, {13, 2}, {16, 4}, {4, 5}}) {
        MixedPlanRecs r;
        CHECK(mp_build(r, km.first, km.second, src, (uint32_t)T));
        size_t n_other = 0;
        for (size_t i = 0; i < src.size(); ++i) {
            const VmRoute v = rp_route(km.first, km.second, src[i].shard_len);
            CHECK((r.recs[i].shard_len != 0) == (v == kVmKernel));
            CHECK(r.recs[i].pad_ == 0u);  // the zero the kernel's output rows start from
            if (v == kVmOther) CHECK(n_other < r.other.size() && r.other[n_other++] == i);
        }
        CHECK(n_other == r.other.size());
    }
    return 0;
}

// One line of the file: the record built from the library's answers has the
// survivors in words 0..2, outputs then checked shards in word 3, and the table
// of row q x survivor j at word kMPatHdr + 5 (j R + q), R = r_o + r_c.
static int from_library(const char* path, int* n_lines) {
    using namespace hbec;
    std::ifstream f(path);
    CHECK(f.good());
    std::string line;
    std::vector<uint32_t> buf;
    while (std::getline(f, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        int k = 0, m = 0, data_only = 0, ro = 0, rc = 0;
        in >> k >> m >> data_only;
        CHECK(in && k >= 1 && k <= kOddMaxK && m >= 1 && m <= kMaxR);
        const int n = k + m;
        std::vector<int> mask(n), sv(k), outs, chk;
        std::vector<uint8_t> orows, crows;
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
        ints(sv, k);
        in >> ro;
        CHECK(in && ro >= 0 && ro <= m);
        ints(outs, ro);
        bytes(orows, ro * k);
        in >> rc;
        CHECK(in && rc >= 0 && ro + rc <= m);
        ints(chk, rc);
        bytes(crows, rc * k);
        CHECK(!in.fail());
        // the library's sets are the mask's: survivors the first k present,
        // outputs missing, checked the other present shards
        std::vector<uint8_t> present(n);
        for (int i = 0; i < n; ++i) present[i] = (uint8_t)mask[i];
        std::vector<int> wsv(k), wchk(n);
        int wnc = -1;
        CHECK(vm_select(k, n, present.data(), wsv.data(), wchk.data(), &wnc) && wnc == rc);
        for (int j = 0; j < k; ++j) CHECK(sv[j] == wsv[j]);
        for (int q = 0; q < rc; ++q) CHECK(chk[q] == wchk[q]);
        int missing = 0;
        for (int i = 0; i < n; ++i) missing += !mask[i] && (i < k || !data_only);
        CHECK(missing == ro);
        for (int q = 0; q < ro; ++q) CHECK(!mask[outs[q]] && (q == 0 || outs[q] > outs[q - 1]));
        if (ro + rc == 0) {
            CHECK(rp_word(ro, rc, 5) == kRpNothing);
            ++*n_lines;
            continue;
        }
        const size_t at = buf.size();
        const uint32_t off = rp_pattern(buf, k, sv.data(), outs.data(), ro, orows.data(), chk.data(), rc, crows.data());
        CHECK(off == at / 4 && off <= kRpRecMask && buf.size() == at + mp_pattern_words(k, ro + rc));
        const uint32_t* p = buf.data() + at;
        const int R = ro + rc;
        for (int j = 0; j < 12; ++j) CHECK(((p[j / 4] >> (8 * (j % 4))) & 0xFFu) == (j < k ? (uint32_t)sv[j] : 0u));
        for (int q = 0; q < 4; ++q)
            CHECK(((p[3] >> (8 * q)) & 0xFFu) == (q < ro ? (uint32_t)outs[q] : q < R ? (uint32_t)chk[q - ro] : 0u));
        for (int q = 0; q < R; ++q)
            for (int j = 0; j < k; ++j) {
                uint32_t t[5];
                perm_table(q < ro ? orows[(size_t)q * k + j] : crows[(size_t)(q - ro) * k + j], t);
                for (int z = 0; z < 5; ++z) CHECK(p[kMPatHdr + 5 * (j * R + q) + z] == t[z]);
            }
        const uint32_t w = rp_word(ro, rc, off);
        CHECK(rp_word_out(w) == (uint32_t)ro && rp_word_chk(w) == (uint32_t)rc && rp_word_rec(w) == off);
        ++*n_lines;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (words() || records() || routing()) return 1;
    int n_lines = 0;
    if (argc > 1 && from_library(argv[1], &n_lines)) return 1;
    std::printf("repair_host ok (%d masks)\n", n_lines);
    return 0;
}
