// gluerange_host.cpp — the arithmetic of the ranged glue calls (csrc/gluerange.h)
// alone, for a run under AddressSanitizer + UBSan: the window of each data shard,
// where its bytes land, the wanted shard positions as at most two intervals, the
// tile predicates (live, coded, read by a gather), the bytes of a 16-B block a
// lane owns, the range check and the cut of an object's range into its entries',
// each against a byte-by-byte model.  The kernel runs this same text.  Links no
// libhbec and touches no device.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../hummingbird_amd/csrc/gluerange.h"

typedef unsigned __int128 u128;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// entry t of an object of L bytes cut k * chunk bytes at a time: its own model
static void entry_of(uint64_t L, uint64_t k, uint64_t chunk, uint64_t t, uint64_t* off, uint64_t* len) {
    *off = t * k * chunk;
    *len = L - *off < k * chunk ? L - *off : k * chunk;
}

int main(int argc, char** argv) {
    // "cuts k chunk L": for every 0 <= start <= end <= L a line
    // "start end t entry_start entry_len dst_off" per entry with a byte of the range
    if (argc == 5 && std::string(argv[1]) == "cuts") {
        const uint64_t k = std::strtoull(argv[2], nullptr, 10), chunk = std::strtoull(argv[3], nullptr, 10);
        const uint64_t L = std::strtoull(argv[4], nullptr, 10);
        if (k < 1 || chunk < 1) return 2;
        const uint64_t n = (L + k * chunk - 1) / (k * chunk);
        for (uint64_t start = 0; start <= L; ++start)
            for (uint64_t end = start; end <= L; ++end)
                for (uint64_t t = 0; t < n; ++t) {
                    uint64_t off, len, es, el, d;
                    entry_of(L, k, chunk, t, &off, &len);
                    hbec::gr_files_cut(off, len, start, end, &es, &el, &d);
                    if (el)
                        std::printf("%llu %llu %llu %llu %llu %llu\n", (unsigned long long)start,
                                    (unsigned long long)end, (unsigned long long)t, (unsigned long long)es,
                                    (unsigned long long)el, (unsigned long long)d);
                }
        return 0;
    }

    // every (S, k, s, e), S <= 40 and k <= 4: windows, landing addresses, wanted
    // positions and the tile predicates, each from the bytes of D[s, e) one by one
    uint64_t windows = 0, tiles = 0, live = 0, coded = 0, two = 0;
    const uint64_t dsts[] = {4096, 4099, ~0ull - 50, 7};  // near the top of the address space too: modulo 2^64
    const uint64_t Ts[] = {1, 3, 8, 16, 41};
    for (uint64_t S = 1; S <= 40; ++S)
        for (uint64_t k = 1; k <= 4; ++k)
            for (uint64_t s = 0; s <= k * S; ++s)
                for (uint64_t e = s; e <= k * S; ++e) {
                    uint8_t want[4][40] = {};
                    uint8_t pos[40] = {};
                    for (uint64_t b = s; b < e; ++b) want[b / S][b % S] = 1, pos[b % S] = 1;
                    const uint64_t dst = dsts[(s + 3 * e + S) % 4];
                    uint64_t total = 0;
                    for (uint64_t j = 0; j < k; ++j) {
                        const hbec::GrWin w = hbec::gr_window(S, s, e, j);
                        CHECK(w.lo <= S && w.hi <= S);
                        for (uint64_t p = 0; p < S; ++p) {
                            CHECK((p >= w.lo && p < w.hi) == (want[j][p] != 0));
                            // position p of shard j is byte j S + p of D, byte j S + p - s of the destination
                            if (want[j][p]) CHECK(hbec::gr_base(dst, S, s, j) + p == dst + (j * S + p - s));
                        }
                        CHECK(hbec::gr_empty(w) == !(w.lo < w.hi));
                        total += hbec::gr_empty(w) ? 0 : w.hi - w.lo;
                        ++windows;
                    }
                    CHECK(total == e - s);
                    const hbec::GrSpan P = hbec::gr_positions(S, s, e);
                    for (uint64_t p = 0; p < S; ++p)
                        CHECK(((p >= P.a.lo && p < P.a.hi) || (p >= P.b.lo && p < P.b.hi)) == (pos[p] != 0));
                    if (!hbec::gr_empty(P.b)) {  // two intervals: apart, in order, a from 0 and b to S
                        CHECK(!hbec::gr_empty(P.a) && P.a.lo == 0 && P.a.hi < P.b.lo && P.b.hi == S);
                        ++two;
                    }
                    if ((s + e) % 3) continue;  // the tile predicates on a third of the cases
                    for (uint64_t T : Ts)
                        for (uint64_t p0 = 0; p0 < S + T; p0 += T) {
                            const uint64_t p1 = p0 + T;
                            bool any = false, in_shard[4] = {};
                            for (uint64_t p = p0; p < p1 && p < S; ++p) {
                                any = any || pos[p];
                                for (uint64_t j = 0; j < k; ++j) in_shard[j] = in_shard[j] || want[j][p];
                            }
                            CHECK(hbec::gr_tile_live(P, p0, p1) == any);
                            for (uint64_t j = 0; j < k; ++j)
                                CHECK(hbec::gr_shard_in_tile(S, s, e, j, p0, p1) == in_shard[j]);
                            // every set of missing data shards, packed as the pattern record packs it
                            for (uint32_t lostset = 0; lostset < (1u << k); ++lostset) {
                                uint32_t packed = 0;
                                int r = 0;
                                bool must = false;
                                for (uint64_t j = 0; j < k; ++j)
                                    if (lostset >> j & 1u) {
                                        packed |= (uint32_t)j << (8 * r++);
                                        must = must || in_shard[j];
                                    }
                                CHECK(hbec::gr_tile_coded(S, s, e, p0, p1, packed, r) == must);
                                coded += must;
                            }
                            live += any;
                            ++tiles;
                        }
                }
    CHECK(two > 1000 && live > 100000 && tiles > live + 100000 && coded > 100000);

    // who writes which byte: one shard's window [lo, hi), its blocks e bytes into
    // the columns, 64-lane windows modelled with nl storing lanes.  Every window
    // that holds a wanted position stores; each wanted position must be written
    // exactly once, nothing else at all, and sixteen bytes at once only inside.
    uint64_t blocks = 0, whole = 0, heads = 0;
    for (uint64_t nl = 1; nl <= 3; ++nl)
        for (uint32_t e = 0; e < 16; ++e)
            for (uint64_t lo = 0; lo < 72; ++lo)
                for (uint64_t hi = lo + 1; hi <= 72; ++hi) {
                    const hbec::GrWin w = {lo, hi};
                    const uint64_t Wn = 16 * nl;
                    int written[72 + 64] = {};
                    for (uint64_t c0 = 0; c0 < 72 + 16; c0 += Wn) {
                        if (!hbec::gr_meets(w, c0, c0 + Wn)) continue;
                        uint32_t b0, b1;
                        for (uint64_t l = 0; l < nl; ++l) {
                            const uint64_t q = c0 + 16 * l + e;
                            if (!hbec::gr_block_bytes(w, q, &b0, &b1)) continue;
                            CHECK(b0 < b1 && b1 <= 16);
                            for (uint32_t b = b0; b < b1; ++b) ++written[q + b];
                            whole += b1 - b0 == 16;
                            ++blocks;
                        }
                        if (hbec::gr_head_bytes(w, c0, e, &b0, &b1)) {
                            CHECK(b0 <= b1 && b1 <= e);
                            for (uint32_t b = b0; b < b1; ++b) ++written[c0 + b];
                            heads += b0 < b1;
                        }
                    }
                    for (uint64_t p = 0; p < 72 + 64; ++p) CHECK(written[p] == (p >= lo && p < hi ? 1 : 0));
                }
    CHECK(whole > 50000 && blocks > whole + 50000 && heads > 10000);  // whole blocks, cut blocks and heads all occur

    // large values: k S up to the top of 64 bits, addresses anywhere
    uint64_t randoms = 0;
    for (int it = 0; it < 200000; ++it) {
        const uint64_t k = 1 + rnd() % 12;
        const uint64_t S = it % 4 == 0 ? ~0ull / k : 1 + rnd() % (~0ull / k);
        const u128 kS = (u128)k * S;
        uint64_t s = (uint64_t)(((u128)rnd() << 64 | rnd()) % (kS + 1)), e = (uint64_t)(((u128)rnd() << 64 | rnd()) % (kS + 1));
        if (s > e) std::swap(s, e);
        if (it % 3 == 0 && e - s > 100000) e = s + rnd() % 100000;  // short ranges too
        const uint64_t dst = rnd();
        u128 total = 0;
        const uint64_t probe = rnd() % S, T = 1 + rnd() % (S / 2 + 1), p0 = probe - probe % T;
        const uint64_t p1 = p0 + T < p0 ? ~0ull : p0 + T;
        bool probe_in = false, tile_any = false;
        for (uint64_t j = 0; j < k; ++j) {
            const u128 off = (u128)j * S;
            const u128 lo = (u128)s <= off ? 0 : ((u128)s - off < S ? (u128)s - off : S);
            const u128 hi = (u128)e <= off ? 0 : ((u128)e - off < S ? (u128)e - off : S);
            const hbec::GrWin w = hbec::gr_window(S, s, e, j);
            CHECK(w.lo == (uint64_t)lo && w.hi == (uint64_t)hi);
            if (lo < hi) {
                total += hi - lo;
                CHECK(hbec::gr_base(dst, S, s, j) + w.lo == dst + (uint64_t)(off + lo - s));
                probe_in = probe_in || (probe >= lo && probe < hi);
                const bool meets = lo < p1 && p0 < hi;
                tile_any = tile_any || meets;
                CHECK(hbec::gr_shard_in_tile(S, s, e, j, p0, p1) == meets);
                CHECK(hbec::gr_tile_coded(S, s, e, p0, p1, (uint32_t)j << 8 | (uint32_t)((j + 1) % k), 2) ==
                      (meets || hbec::gr_shard_in_tile(S, s, e, (j + 1) % k, p0, p1)));
            } else {
                CHECK(hbec::gr_empty(w) && !hbec::gr_shard_in_tile(S, s, e, j, p0, p1));
            }
        }
        CHECK(total == (u128)e - s);
        const hbec::GrSpan P = hbec::gr_positions(S, s, e);
        CHECK(((probe >= P.a.lo && probe < P.a.hi) || (probe >= P.b.lo && probe < P.b.hi)) == probe_in);
        CHECK(hbec::gr_tile_live(P, p0, p1) == tile_any);
        // the range check, at and around the limit and where s + len wraps
        const uint64_t len = rnd() >> (rnd() % 64);
        CHECK(hbec::gr_range_ok(s, len, k, S) == ((u128)s + len <= kS));
        CHECK(hbec::gr_range_ok(s, e - s, k, S));
        ++randoms;
    }
    CHECK(!hbec::gr_range_ok(~0ull, 1, 1, ~0ull) && hbec::gr_range_ok(~0ull, 0, 1, ~0ull));
    CHECK(!hbec::gr_range_ok(1, ~0ull, 1, ~0ull) && hbec::gr_range_ok(1, ~0ull, 2, ~0ull));
    CHECK(!hbec::gr_range_ok(0, 1, 12, 0) && hbec::gr_range_ok(0, 0, 12, 0));  // a zero-length entry takes no byte

    // the files cut: every (start, end) of every L, byte by byte
    uint64_t cuts = 0;
    const uint64_t ks[] = {1, 2, 3, 4};
    const uint64_t chunks[] = {1, 2, 5};
    for (uint64_t k : ks)
        for (uint64_t chunk : chunks)
            for (uint64_t L = 0; L <= 3 * k * chunk + k; ++L) {
                const uint64_t n = (L + k * chunk - 1) / (k * chunk);
                for (uint64_t start = 0; start <= L; ++start)
                    for (uint64_t end = start; end <= L; ++end) {
                        uint64_t next = start;  // the pieces tile [start, end) in order
                        for (uint64_t t = 0; t < n; ++t) {
                            uint64_t off, len, es = ~0ull, el = ~0ull, d = ~0ull;
                            entry_of(L, k, chunk, t, &off, &len);
                            hbec::gr_files_cut(off, len, start, end, &es, &el, &d);
                            uint64_t cnt = 0, first = 0;
                            for (uint64_t b = start; b < end; ++b)
                                if (b >= off && b < off + len && cnt++ == 0) first = b;
                            CHECK(el == cnt);
                            if (cnt) {
                                CHECK(es == first - off && d == first - start && first == next && es + el <= len);
                                next = first + cnt;
                            } else {
                                CHECK(es == 0 && d == 0);
                            }
                            ++cuts;
                        }
                        CHECK(next == end || start == end);
                    }
            }
    {
        uint64_t es, el, d;
        hbec::gr_files_cut(~0ull - 9, 10, 0, ~0ull, &es, &el, &d);  // off + len = 2^64: no wrap
        CHECK(es == 0 && el == 9 && d == ~0ull - 9);
        hbec::gr_files_cut(~0ull - 9, 10, ~0ull - 3, ~0ull, &es, &el, &d);
        CHECK(es == 6 && el == 3 && d == 0);
    }
    std::printf("gluerange_host ok (%llu windows, %llu tiles, %llu blocks, %llu randoms, %llu cuts)\n",
                (unsigned long long)windows, (unsigned long long)tiles, (unsigned long long)blocks,
                (unsigned long long)randoms, (unsigned long long)cuts);
    return 0;
}
