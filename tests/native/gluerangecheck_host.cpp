// The byte mask of the examined positions (csrc/gluerangecheck.h grc_live_mask)
// against a brute force, for every (S <= 40, k <= 4, s, e) and every dword of
// every 16-B block up to one block past S.  A program of its own: it links no
// libhbec and is built with AddressSanitizer + UBSan by
// tests/test_glue_range_checked_host.py.
#include <cstdio>

#include "../../hummingbird_amd/csrc/gluerangecheck.h"

int main() {
    using namespace hbec;
    unsigned long long masks = 0;
    for (uint64_t S = 1; S <= 40; ++S)
        for (uint64_t k = 1; k <= 4; ++k)
            for (uint64_t s = 0; s <= k * S; ++s)
                for (uint64_t e = s; e <= k * S; ++e) {
                    const GrSpan P = gr_positions(S, s, e);
                    for (uint64_t pos = 0; pos < S + 16; pos += 4, ++masks) {
                        uint32_t want = 0;
                        for (uint32_t b = 0; b < 4; ++b)
                            for (uint64_t j = 0; j < k; ++j) {
                                const uint64_t x = pos + b, at = j * S + x;
                                if (x < S && s <= at && at < e) want |= 0xFFu << (8 * b);
                            }
                        const uint32_t got = grc_live_mask(P, pos);
                        if (got != want) {
                            std::printf("S %llu k %llu [%llu, %llu) pos %llu: %08x, expected %08x\n",
                                        (unsigned long long)S, (unsigned long long)k, (unsigned long long)s,
                                        (unsigned long long)e, (unsigned long long)pos, got, want);
                            return 1;
                        }
                    }
                }
    // the word: A for a checked mask, kGrcPlain | o for exactly k present, never kGlueSkip's 15
    for (int r = 0; r <= 4; ++r)
        for (int o = 0; r + o <= 4; ++o) {
            const uint32_t bits = grc_word(r, o, 0x0ABCDEFu) >> kGrcShift;
            if ((grc_word(r, o, 0x0ABCDEFu) & kGrcMask) != 0x0ABCDEFu || bits == 15u ||
                bits != (r ? (uint32_t)(r + o) : kGrcPlain | (uint32_t)o) || grc_rows(r, o) != (r ? r + o : o)) {
                std::printf("word of r %d o %d\n", r, o);
                return 1;
            }
        }
    std::printf("gluerangecheck_host ok (%llu masks)\n", masks);
    return 0;
}
