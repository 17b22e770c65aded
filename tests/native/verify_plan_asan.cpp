// Host-only checks of the plan Verify under AddressSanitizer + UBSan (no GPU
// work): the routing of stripes to Verify records and their flag indices
// (vplan.h vp_add), and every argument check of hbec_verify_plan /
// hbec_verify_host / hbec_verify_plan_stats / hbec_verify_route_stats, which answer before a device is
// touched.  Linked against the sanitized libhbec (build.py build_asan).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hummingbird_amd/csrc/vplan.h"
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
    const uint64_t sizes[] = {1, 31, 32, 33, kVpTile + 15, kVpTile + 16, kVpTile + 17, 3 * kVpTile, 300001,
                              kPos32MaxShard, kPos32MaxShard + 1};
    VerifyRecs v;
    uint64_t idx = 5, want_tiles = 0, want_recs = 0, want_other = 0;
    for (uint64_t s : sizes) {
        CHECK(vp_add(v, 8, 3, 4096 + idx, 1 << 20, s, idx));
        if (pos32_shard(s)) {
            const VRec& r = v.recs.back();
            CHECK(r.flag == idx && r.shard_len == s && r.a == 4096 + idx && r.b == (1u << 20));
            const uint64_t nt = (vp_main_bytes((uint32_t)s) + kVpTile - 1) / kVpTile;
            // the tiles cover exactly the main bytes; the tail is shorter than its slots
            CHECK(nt * kVpTile >= vp_main_bytes((uint32_t)s) && (nt == 0 || (nt - 1) * kVpTile < vp_main_bytes((uint32_t)s)));
            CHECK(s - vp_main_bytes((uint32_t)s) < kVpTailSlots && vp_main_bytes((uint32_t)s) % 16 == 0);
            CHECK(s < 32 ? vp_main_bytes((uint32_t)s) == 0 : vp_main_bytes((uint32_t)s) + 16 <= s);
            for (uint64_t t = 0; t < nt; ++t) {
                const VTile& e = v.tiles[want_tiles + t];
                CHECK(e.rec == want_recs && e.ti == t);
            }
            want_tiles += nt;
            ++want_recs;
        } else {
            CHECK(v.other.back().idx == idx && v.other.back().shard_len == s);
            ++want_other;
        }
        idx += 3;  // zero-length stripes in between shift nothing: the index is the caller's
    }
    CHECK(v.recs.size() == want_recs && v.tiles.size() == want_tiles && v.other.size() == want_other);
    // shapes outside the plan kernels: every stripe to the other route
    VerifyRecs w;
    CHECK(vp_add(w, 13, 4, 64, 128, 100, 0) && vp_add(w, 4, 5, 64, 128, 100, 1) && vp_add(w, 16, 4, 64, 128, 100, 2));
    CHECK(w.recs.empty() && w.tiles.empty() && w.other.size() == 3 && w.other[2].idx == 2);
    CHECK(vp_fast_shape(12, 4) && !vp_fast_shape(12, 0) && vp_tiles_shape(8, 4) && !vp_tiles_shape(9, 4));
    return 0;
}

static int arguments() {
    hbec_codec *c42 = nullptr, *c83 = nullptr, *c40 = nullptr;
    CHECK(hbec_new(4, 2, &c42) == HBEC_OK && hbec_new(8, 3, &c83) == HBEC_OK && hbec_new(4, 0, &c40) == HBEC_OK);
    std::vector<hbec_stripe> st(5);  // zero-length: planned on the host alone
    std::vector<hbec_object> ob(5);
    hbec_plan *ps = nullptr, *po = nullptr, *p0 = nullptr, *pm = nullptr;
    CHECK(hbec_plan_stripes(c42, st.data(), st.size(), &ps) == HBEC_OK);
    CHECK(hbec_plan_objects(c42, ob.data(), ob.size(), &po) == HBEC_OK);
    CHECK(hbec_plan_stripes(c42, nullptr, 0, &p0) == HBEC_OK);
    CHECK(hbec_plan_stripes(c40, st.data(), st.size(), &pm) == HBEC_OK);
    std::vector<uint32_t> flags(5, 0xABCDu);  // host memory: never dereferenced by these calls
    for (hbec_plan* p : {ps, po}) {
        CHECK(hbec_verify_plan(nullptr, p, flags.data(), nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_verify_plan(c42, nullptr, flags.data(), nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_verify_plan(c42, p, nullptr, nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_verify_plan(c83, p, flags.data(), nullptr) == HBEC_ERR_INVALID_ARG);
        CHECK(hbec_verify_plan(c42, p, flags.data(), nullptr) == HBEC_OK);
    }
    CHECK(hbec_verify_plan(c42, p0, nullptr, nullptr) == HBEC_OK);
    CHECK(hbec_verify_plan(c40, pm, flags.data(), nullptr) == HBEC_OK);
    for (uint32_t f : flags) CHECK(f == 0xABCDu);

    std::vector<uint8_t> hf(5, 9);
    CHECK(hbec_verify_host(nullptr, st.data(), st.size(), hf.data()) == HBEC_ERR_INVALID_ARG);
    CHECK(hbec_verify_host(c42, nullptr, st.size(), hf.data()) == HBEC_ERR_INVALID_ARG);
    CHECK(hbec_verify_host(c42, st.data(), st.size(), nullptr) == HBEC_ERR_INVALID_ARG);
    st[3].shard_len = 77;  // null base
    CHECK(hbec_verify_host(c42, st.data(), st.size(), hf.data()) == HBEC_ERR_INVALID_ARG);
    for (uint8_t f : hf) CHECK(f == 9);
    st[3].shard_len = 0;
    CHECK(hbec_verify_host(c42, st.data(), st.size(), hf.data()) == HBEC_OK);
    for (uint8_t f : hf) CHECK(f == 0);
    CHECK(hbec_verify_host(c42, nullptr, 0, nullptr) == HBEC_OK);
    uint8_t one = 7;
    hbec_stripe s1 = {&one, 64};
    CHECK(hbec_verify_host(c40, &s1, 1, &one) == HBEC_OK && one == 0);  // m = 0: nothing read

    uint64_t a = 1, b = 1;
    CHECK(hbec_verify_plan_stats(nullptr, &b) == HBEC_ERR_INVALID_ARG);
    CHECK(hbec_verify_plan_stats(&a, nullptr) == HBEC_ERR_INVALID_ARG);
    CHECK(hbec_verify_plan_stats(&a, &b) == HBEC_OK && a == 0 && b == 0);
    hbec_verify_routes vr;
    CHECK(hbec_verify_route_stats(nullptr) == HBEC_ERR_INVALID_ARG);
    CHECK(hbec_verify_route_stats(&vr) == HBEC_OK);
    CHECK(vr.packed + vr.pipe + vr.records + vr.odd + vr.wide + vr.unaligned + vr.scratch == 0);  // nothing reached a route
    hbec_apply_routes ar;
    CHECK(hbec_apply_route_stats(nullptr) == HBEC_ERR_INVALID_ARG);
    CHECK(hbec_apply_route_stats(&ar) == HBEC_OK);
    CHECK(ar.packed + ar.vec + ar.odd + ar.unaligned + ar.wide == 0);  // nothing reached a pass
    CHECK(hbec_verify_plan_tile_bytes(8) == (int)hbec::kVpTile);
    for (hbec_plan* p : {ps, po, p0, pm}) hbec_plan_free(p);
    hbec_free(c42);
    hbec_free(c83);
    hbec_free(c40);
    return 0;
}

int main() {
    if (records() || arguments()) return 1;
    std::puts("verify_plan_asan ok");
    return 0;
}
