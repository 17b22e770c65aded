// Host-only checks of the degraded plan Verify's inline host logic (vmixed.h;
// no GPU work and no libhbec): which shards a mask reads and checks, the record
// words of 4+2 and 12+4 masks against hand-computed indices, the per-entry word
// packing, and the routing of sizes and shapes.  Built with the host compiler
// under AddressSanitizer + UBSan by tests/test_verify_mixed_host.py and run
// directly.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hummingbird_amd/csrc/vmixed.h"

#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static int selection() {
    using namespace hbec;
    int sv[12], ck[16], nc = -1;
    // 4+2, shard 1 lost: survivors 0 2 3 4, parity 5 checked
    const uint8_t a[6] = {1, 0, 1, 1, 1, 1};
    CHECK(vm_select(4, 6, a, sv, ck, &nc) && nc == 1);
    CHECK(sv[0] == 0 && sv[1] == 2 && sv[2] == 3 && sv[3] == 4 && ck[0] == 5);
    // all present: Encoder.Verify's data shards and parity shards
    const uint8_t full[6] = {1, 1, 1, 1, 1, 1};
    CHECK(vm_select(4, 6, full, sv, ck, &nc) && nc == 2 && sv[3] == 3 && ck[0] == 4 && ck[1] == 5);
    // a parity shard lost: the other one is checked; any non-zero byte is "present"
    const uint8_t p[6] = {1, 7, 1, 255, 0, 1};
    CHECK(vm_select(4, 6, p, sv, ck, &nc) && nc == 1 && sv[1] == 1 && ck[0] == 5);
    // exactly k present: nothing to check
    const uint8_t two[6] = {0, 1, 1, 0, 1, 1};
    CHECK(vm_select(4, 6, two, sv, ck, &nc) && nc == 0 && sv[0] == 1 && sv[1] == 2 && sv[2] == 4 && sv[3] == 5);
    // fewer than k present
    const uint8_t few[6] = {1, 1, 1, 0, 0, 0};
    CHECK(!vm_select(4, 6, few, sv, ck, &nc));
    // 12+4 with data shards 3 and 9 lost: survivors run into the parity, 14 and 15 checked
    uint8_t w[16];
    for (int i = 0; i < 16; ++i) w[i] = (i == 3 || i == 9) ? 0 : 1;
    CHECK(vm_select(12, 16, w, sv, ck, &nc) && nc == 2 && ck[0] == 14 && ck[1] == 15);
    const int want[12] = {0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13};
    for (int j = 0; j < 12; ++j) CHECK(sv[j] == want[j]);
    return 0;
}

static int records() {
    using namespace hbec;
    std::vector<uint32_t> buf;
    // 4+2, shard 1 lost
    const int sv4[4] = {0, 2, 3, 4}, ck4[1] = {5};
    const uint8_t rows4[4] = {0x1b, 0x02, 0xd7, 0x8e};
    CHECK(vm_pattern(buf, 4, sv4, ck4, 1, rows4) == 0);
    CHECK(buf.size() == mp_pattern_words(4, 1) && buf.size() % 4 == 0);
    CHECK(buf[0] == 0x04030200u && buf[1] == 0 && buf[2] == 0 && buf[3] == 5u);
    for (int j = 0; j < 4; ++j) {
        uint32_t t[5];
        perm_table(rows4[j], t);
        for (int q = 0; q < 5; ++q) CHECK(buf[kMPatHdr + 5 * j + q] == t[q]);
    }
    // 12+4, shards 3 and 9 lost: the record starts where the first one ends
    const int sv[12] = {0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12, 13}, ck[2] = {14, 15};
    std::vector<uint8_t> rows(2 * 12);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (uint8_t)(i * 29 + 3);
    const uint32_t off = vm_pattern(buf, 12, sv, ck, 2, rows.data());
    CHECK(off * 4 == mp_pattern_words(4, 1) && buf.size() == off * 4 + mp_pattern_words(12, 2));
    const uint32_t* p = buf.data() + off * 4;
    CHECK(p[0] == 0x04020100u && p[1] == 0x08070605u && p[2] == 0x0d0c0b0au && p[3] == 0x00000f0eu);
    for (int r = 0; r < 2; ++r)
        for (int j = 0; j < 12; ++j) {
            uint32_t t[5];
            perm_table(rows[(size_t)r * 12 + j], t);
            for (int q = 0; q < 5; ++q) CHECK(p[kMPatHdr + 5 * (j * 2 + r) + q] == t[q]);
        }
    return 0;
}

static int words() {
    using namespace hbec;
    for (int r = 1; r <= kMaxR; ++r)
        for (uint32_t rec : {0u, 1u, 11u, (1u << 22) - 1u}) {
            const uint32_t w = vm_word(r, rec);
            CHECK(w != 0u && w != kVmNothing && vm_word_r(w) == (uint32_t)r && vm_word_rec(w) == rec);
        }
    // nothing to check: r = 0, told apart from "no tiles" (0) and from every record offset
    CHECK(vm_word(0, 0) == kVmNothing && vm_word(0, 77) == kVmNothing && kVmNothing != 0u);
    CHECK(vm_word_r(kVmNothing) == 0u);
    CHECK((uint64_t)65536 * mp_pattern_words(kOddMaxK, kMaxR) / 4 < kVmNothing);
    return 0;
}

static int routing() {
    using namespace hbec;
    const uint64_t T = 3968;  // mixed_plan_tile_bytes(): kUnalignedU windows of kUnalignedWindow
    CHECK(vm_route(4, 2, 0) == kVmSkip && vm_route(13, 4, 0) == kVmSkip);
    for (uint64_t s : {(uint64_t)1, T - 1, T, T + 1, kPos32MaxShard}) {
        CHECK(vm_route(4, 2, s) == kVmKernel && vm_route(12, 4, s) == kVmKernel && vm_route(1, 1, s) == kVmKernel);
        CHECK(vm_route(13, 4, s) == kVmOther && vm_route(4, 5, s) == kVmOther && vm_route(4, 0, s) == kVmOther);
    }
    CHECK(vm_route(4, 2, kPos32MaxShard + 1) == kVmOther && vm_route(8, 3, 1ull << 33) == kVmOther);
    // the same entries mp_build gives tiles to: the plan's list is shared
    std::vector<MSrc> src;
    for (uint64_t s : {(uint64_t)0, (uint64_t)1, T - 1, T, T + 1, kPos32MaxShard, kPos32MaxShard + 1})
        src.push_back(MSrc{4096, 1u << 20, s});
    for (auto km : {std::pair<int, int>{4, 2}, {13, 4}, {4, 5}}) {
        MixedPlanRecs r;
        CHECK(mp_build(r, km.first, km.second, src, (uint32_t)T));
        size_t n_other = 0;
        for (size_t i = 0; i < src.size(); ++i) {
            const VmRoute v = vm_route(km.first, km.second, src[i].shard_len);
            CHECK((r.recs[i].shard_len != 0) == (v == kVmKernel));
            if (v == kVmOther) CHECK(n_other < r.other.size() && r.other[n_other++] == i);
        }
        CHECK(n_other == r.other.size());
    }
    return 0;
}

int main() {
    if (selection() || records() || words() || routing()) return 1;
    std::puts("verify_mixed_host ok");
    return 0;
}
