// splitselect_host.cpp — csrc/splitselect.h alone under AddressSanitizer + UBSan:
// for every mask of 4+2, 3+2 and 4+0 and a sample of 8+3 and 12+4 the record's
// masks, row list, table offsets and length, and the inputs a tile walks in their
// order, against a brute-force model of ecSplit with nil writers (ecutils.go:63).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../hummingbird_amd/csrc/splitselect.h"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() { return (rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull) >> 33; }

#define CHECK(c) \
    do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// GF(2^8) product, poly 0x11D, bit by bit: no table of gf256.h
static uint8_t gmul(uint8_t a, uint8_t b) {
    unsigned acc = 0, x = a;
    for (int i = 0; i < 8; ++i, x = (x << 1) ^ ((x & 0x80u) ? 0x11Du : 0u))
        if (b & (1u << i)) acc ^= x;
    return (uint8_t)acc;
}

// the five words at t are the v_perm tables of c: c * b, c * (b << 3), c * (b << 6)
static bool table_is(const uint32_t* t, uint8_t c) {
    bool ok = true;
    for (int b = 0; b < 8; ++b) {
        ok = ok && (uint8_t)(t[b / 4] >> (8 * (b % 4))) == gmul(c, (uint8_t)b);
        ok = ok && (uint8_t)(t[2 + b / 4] >> (8 * (b % 4))) == gmul(c, (uint8_t)(b << 3));
        ok = ok && (b >= 4 || (uint8_t)(t[4] >> (8 * b)) == gmul(c, (uint8_t)(b << 6)));
    }
    return ok;
}

static uint64_t g_records = 0, g_walks = 0;

static int check_mask(int k, int m, const std::vector<uint8_t>& enc, const std::vector<uint8_t>& mask) {
    std::vector<int> rows;  // the model: what is written and which parity rows, by walking the mask
    uint32_t store = 0, list = 0;
    for (int j = 0; j < k; ++j) store |= mask[j] ? 1u << j : 0u;
    for (int r = 0; r < m; ++r)
        if (mask[k + r]) rows.push_back(r);
    const int R = (int)rows.size();
    for (int q = 0; q < R; ++q) list |= (uint32_t)(k + rows[q]) << (8 * q);

    std::vector<uint32_t> buf(8, 0xDEADBEEFu);  // a record is appended, at a 16-B unit
    int got_R = -1;
    CHECK(hbec::ss_record(buf, k, m, mask.data(), enc.data(), &got_R) == 2 && got_R == R && buf[7] == 0xDEADBEEFu);
    const uint32_t words = (uint32_t)buf.size() - 8, tables = 4u + 5u * (uint32_t)(k * R);
    CHECK(words == hbec::ss_record_words(k, R) && words % 4 == 0 && words >= tables && words < tables + 4);
    const uint32_t* p = buf.data() + 8;
    CHECK(p[0] == store && p[1] == (R ? (1u << k) - 1u : store) && p[2] == list && p[3] == (uint32_t)R);
    // only the selected rows' tables, the R of one input together
    for (int j = 0; j < k; ++j)
        for (int q = 0; q < R; ++q) {
            const uint32_t t = hbec::ss_table_at(R, j, q);
            CHECK(t == 4u + 5u * (uint32_t)(j * R + q) && t + 5 <= words);
            CHECK(table_is(p + t, enc[(size_t)rows[q] * k + j]));
        }
    for (uint32_t w = tables; w < words; ++w) CHECK(p[w] == 0);  // the padding
    ++g_records;

    const uint64_t shard_lens[] = {1, 2, 5, 16, 17};
    for (uint64_t S : shard_lens)
        for (uint64_t len = S * k - k + 1; len <= S * k; ++len) {
            std::vector<uint32_t> want, got;
            for (int j = 0; j < k; ++j) {
                uint64_t V = 0;  // bytes of the piece in shard j, byte by byte
                for (uint64_t b = (uint64_t)j * S; b < (uint64_t)(j + 1) * S; ++b) V += b < len;
                if (mask[j] || (R > 0 && V > 0)) want.push_back((uint32_t)j);  // stored, or read with a byte in it
            }
            uint32_t rest = hbec::ss_needed_inputs(p[0], p[1], (uint32_t)k, len, S);
            while (rest) got.push_back(hbec::ss_next_input(rest));
            CHECK(got == want && (R == 0 || got[0] == 0));  // in order; a coded tile reads input 0
            ++g_walks;
        }
    return 0;
}

int main() {
    const int shapes[][2] = {{4, 2}, {3, 2}, {4, 0}, {8, 3}, {12, 4}};
    for (const auto& sh : shapes) {
        const int k = sh[0], m = sh[1], n = k + m;
        std::vector<uint8_t> mat;
        CHECK(hbec::build_matrix(k, m, mat));
        const std::vector<uint8_t> enc(mat.begin() + (size_t)k * k, mat.end());
        const uint32_t all = 1u << n;
        const bool every = n <= 6;  // every mask of the small shapes, a sample of the others
        for (uint32_t it = 0; it < (every ? all : 300u); ++it) {
            const uint32_t bits = every ? it : (it == 0 ? all - 1u : (uint32_t)(rnd() % all));
            std::vector<uint8_t> mask((size_t)n);
            for (int i = 0; i < n; ++i) mask[i] = (bits >> i) & 1u ? (uint8_t)(1 + rnd() % 255) : 0;  // any non-zero byte
            if (check_mask(k, m, enc, mask)) return 1;
        }
    }
    std::printf("splitselect_host ok (%llu records, %llu walks)\n", (unsigned long long)g_records,
                (unsigned long long)g_walks);
    return 0;
}
