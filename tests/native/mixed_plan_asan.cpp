// Host-only checks of the mixed plan reconstruct under AddressSanitizer +
// UBSan (no GPU work): the routing of a plan's source entries to records and
// tiles (mixedplan.h mp_build), the pattern records (mp_pattern), and every
// argument check of hbec_reconstruct_plan_mixed / hbec_mixed_plan_stats, which
// answer before a device is touched.  Linked against the sanitized libhbec
// (build.py build_asan).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hummingbird_amd/csrc/mixedplan.h"
#include "../../include/hbec.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                 \
        }                                                             \
    } while (0)

static int records() {
    using namespace hbec;
    const uint32_t T = 3968;
    const uint64_t sizes[] = {0, 1, 15, 16, 991, 992, 993, T - 1, T, T + 1, 0, 2 * T + 17, 300001, kPos32MaxShard,
                              kPos32MaxShard + 1, 0};
    std::vector<MSrc> src;
    uint64_t want_tiles = 0, want_other = 0;
    for (uint64_t s : sizes) {
        src.push_back(s ? MSrc{4096 + src.size(), (1u << 20) + src.size(), s} : MSrc{0, 0, 0});
        if (s && pos32_shard(s)) want_tiles += (s + T - 1) / T;
        if (s && !pos32_shard(s)) ++want_other;
    }
    MixedPlanRecs r;
    CHECK(mp_build(r, 8, 3, src, T));
    CHECK(r.recs.size() == src.size() && r.tiles.size() == want_tiles && r.other.size() == want_other);
    size_t t = 0;
    for (size_t i = 0; i < src.size(); ++i) {
        const bool kernel = src[i].shard_len && pos32_shard(src[i].shard_len);
        CHECK(r.recs[i].shard_len == (kernel ? src[i].shard_len : 0));
        if (!kernel) continue;
        CHECK(r.recs[i].a == src[i].a && r.recs[i].b == src[i].b);
        const uint64_t nt = (src[i].shard_len + T - 1) / T;
        // the tiles of an entry cover [0, S) exactly, in order, under its caller index
        CHECK((nt - 1) * T < src[i].shard_len && nt * T >= src[i].shard_len);
        for (uint64_t q = 0; q < nt; ++q, ++t) CHECK(r.tiles[t].rec == i && r.tiles[t].ti == q);
    }
    CHECK(t == r.tiles.size());
    CHECK(r.other.size() == 1 && r.other[0] == 14);
    // shapes outside the kernel: every non-empty entry to the other route
    for (auto km : {std::pair<int, int>{13, 4}, {4, 5}, {16, 4}}) {
        MixedPlanRecs w;
        CHECK(mp_build(w, km.first, km.second, src, T));
        CHECK(w.tiles.empty() && w.other.size() == 13 && w.other[0] == 1 && w.other.back() == 14);
        for (const MRec& m : w.recs) CHECK(m.shard_len == 0);
    }
    CHECK(mp_fast_shape(12, 4) && !mp_fast_shape(13, 4) && !mp_fast_shape(12, 5));
    // an empty plan
    MixedPlanRecs none;
    CHECK(mp_build(none, 4, 2, {}, T) && none.recs.empty() && none.tiles.empty() && none.other.empty());
    return 0;
}

static int patterns() {
    using namespace hbec;
    // 12 survivors, 4 outputs: every index byte and table slot in its place
    const int k = 12;
    int surv[12], outs[4] = {3, 7, 14, 15};
    for (int j = 0; j < k; ++j) surv[j] = j < 3 ? j : (j < 6 ? j + 1 : j + 2);
    std::vector<uint8_t> rows(4 * k);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (uint8_t)(i * 37 + 1);
    std::vector<uint32_t> buf;
    // a short record first (4 inputs, 1 output), so the long one starts at an offset
    CHECK(mp_pattern(buf, 4, surv, outs, 1, rows.data()) == 0);
    CHECK(buf.size() == mp_pattern_words(4, 1) && buf.size() % 4 == 0 && buf.size() >= kMPatHdr + 20);
    CHECK(buf[0] == 0x04020100u && buf[1] == 0 && buf[2] == 0 && buf[3] == 3u);
    const uint32_t off = mp_pattern(buf, k, surv, outs, 4, rows.data());
    CHECK(off * 4 == mp_pattern_words(4, 1) && buf.size() == off * 4 + mp_pattern_words(k, 4));
    CHECK(mp_pattern_words(12, 4) == 244 && mp_pattern_words(4, 2) == 44);
    const uint32_t* p = buf.data() + off * 4;
    for (int j = 0; j < k; ++j) CHECK(((p[j / 4] >> (8 * (j % 4))) & 0xFF) == (uint32_t)surv[j]);
    for (int r = 0; r < 4; ++r) CHECK(((p[3] >> (8 * r)) & 0xFF) == (uint32_t)outs[r]);
    for (int r = 0; r < 4; ++r)
        for (int j = 0; j < k; ++j) {
            uint32_t t[5];
            perm_table(rows[(size_t)r * k + j], t);
            for (int q = 0; q < 5; ++q) CHECK(p[kMPatHdr + 5 * (j * 4 + r) + q] == t[q]);
        }
    // the largest record offset of a call fits the per-entry word
    CHECK((uint64_t)65536 * mp_pattern_words(kOddMaxK, kMaxR) / 4 <= kMPatMask);
    return 0;
}

static int arguments() {
    hbec_codec *c42 = nullptr, *c83 = nullptr;
    CHECK(hbec_new(4, 2, &c42) == HBEC_OK && hbec_new(8, 3, &c83) == HBEC_OK);
    std::vector<hbec_stripe> st(5);  // zero-length: planned on the host alone
    std::vector<hbec_object> ob(5);
    hbec_plan *ps = nullptr, *po = nullptr, *p0 = nullptr;
    CHECK(hbec_plan_stripes(c42, st.data(), st.size(), &ps) == HBEC_OK);
    CHECK(hbec_plan_objects(c42, ob.data(), ob.size(), &po) == HBEC_OK);
    CHECK(hbec_plan_stripes(c42, nullptr, 0, &p0) == HBEC_OK);
    const uint8_t pats[3][6] = {{0, 1, 1, 1, 1, 1}, {1, 1, 1, 1, 1, 1}, {1, 1, 1, 0, 0, 0}};
    const uint32_t idx[5] = {0, 1, 0, 1, 0}, bad[5] = {0, 1, 0, 1, 2}, none[1] = {0};
    for (hbec_plan* p : {ps, po}) {
        CHECK(hbec_reconstruct_plan_mixed(nullptr, p, pats[0], 2, idx, 0, nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_reconstruct_plan_mixed(c42, nullptr, pats[0], 2, idx, 0, nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_reconstruct_plan_mixed(c42, p, nullptr, 2, idx, 0, nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_reconstruct_plan_mixed(c42, p, pats[0], 2, nullptr, 0, nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_reconstruct_plan_mixed(c83, p, pats[0], 2, idx, 0, nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_reconstruct_plan_mixed(c42, p, pats[0], 0, idx, 0, nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_reconstruct_plan_mixed(c42, p, pats[0], 65537, idx, 0, nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_reconstruct_plan_mixed(c42, p, pats[0], 2, bad, 0, nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_reconstruct_plan_mixed(c42, p, pats[0], 3, idx, 0, nullptr) == HBEC_ERR_TOO_FEW_SHARDS);
        CHECK(hbec_reconstruct_plan_mixed(c42, p, pats[0], 3, idx, 1, nullptr) == HBEC_ERR_TOO_FEW_SHARDS);
        CHECK(hbec_reconstruct_plan_mixed(c42, p, pats[0], 2, idx, 0, nullptr) == HBEC_OK);
        CHECK(hbec_reconstruct_plan_mixed(c42, p, pats[0], 2, idx, 1, nullptr) == HBEC_OK);
    }
    CHECK(hbec_reconstruct_plan_mixed(c42, p0, pats[0], 1, none, 0, nullptr) == HBEC_OK);
    CHECK(hbec_reconstruct_plan_mixed(c42, p0, pats[0], 0, none, 0, nullptr) == HBEC_OK);

    uint64_t a = 1, b = 1;
    CHECK(hbec_mixed_plan_stats(nullptr, &b) == HBEC_ERR_INVALID_ARG);
    CHECK(hbec_mixed_plan_stats(&a, nullptr) == HBEC_ERR_INVALID_ARG);
    CHECK(hbec_mixed_plan_stats(&a, &b) == HBEC_OK && a == 0 && b == 0);
    CHECK(hbec_mixed_plan_tile_bytes() == 3968);
    CHECK(hbec_set_mixed_plan_chunk_tiles(3) == HBEC_OK && hbec_set_mixed_plan_chunk_tiles(0) == HBEC_OK);
    for (hbec_plan* p : {ps, po, p0}) hbec_plan_free(p);
    hbec_free(c42);
    hbec_free(c83);
    return 0;
}

int main() {
    if (records() || patterns() || arguments()) return 1;
    std::puts("mixed_plan_asan ok");
    return 0;
}
