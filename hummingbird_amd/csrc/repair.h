// repair.h — rebuild the missing shards of a plan and check its surplus ones in
// one pass (hbec_repair_plan_mixed): the per-call words and pattern records of
// gf_repair_mixed_plan (repair.hip) and the routing of a plan's source entries
// to it.  The device records and the static {entry, tile} list are the mixed
// plan reconstruct's (mixedplan.h); a pattern record is mp_pattern's with the
// rows of the outputs first and those of the checked shards after them.
// Everything inline here needs no device, so it compiles alone
// (tests/native/repair_host.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "mixedplan.h"
#include "vmixed.h"

namespace hbec {

// Per-call word of a source entry: (r_o << kRpOutShift) | (r_c << kRpChkShift) |
// record offset in 16-B units; r_o the shards it rebuilds, r_c the shards it
// checks, r_o + r_c <= kMaxR.  The offset has kRpChkShift = 22 bits: 65536
// records of 976 B (12+4, four rows) are just below 2^22 units.  r_c == 0 says
// that exactly k shards are present (every present shard beyond the first k is
// checked), which the kernel reports as flag bit 1.  An entry with exactly k
// present and nothing to rebuild (data_only with its data complete) has no
// record: kRpNothing, both counts 0 and every offset bit set; no record starts
// there.  0: no tiles (zero-length, or the other route).
constexpr uint32_t kRpChkShift = 22;
constexpr uint32_t kRpOutShift = 25;
constexpr uint32_t kRpRecMask = (1u << kRpChkShift) - 1u;
constexpr uint32_t kRpNothing = kRpRecMask;
inline uint32_t rp_word(int r_out, int r_chk, uint32_t rec) {
    return r_out + r_chk > 0 ? ((uint32_t)r_out << kRpOutShift) | ((uint32_t)r_chk << kRpChkShift) | rec : kRpNothing;
}
inline uint32_t rp_word_out(uint32_t w) { return (w >> kRpOutShift) & 7u; }
inline uint32_t rp_word_chk(uint32_t w) { return (w >> kRpChkShift) & 7u; }
inline uint32_t rp_word_rec(uint32_t w) { return w & kRpRecMask; }

// Where a source entry of shard length S goes: mp_build's rule, as vm_route.
inline VmRoute rp_route(int k, int m, uint64_t shard_len) { return vm_route(k, m, shard_len); }

// Append the record of one mask with r_out + r_chk >= 1 rows: the shard indices
// of word 3 and the tables are those of the outputs (out_rows: r_out x k, the
// decode rows) followed by those of the checked shards (chk_rows: r_chk x k).
// Returns its offset in 16-B units.
inline uint32_t rp_pattern(std::vector<uint32_t>& buf, int k, const int* survivors, const int* outs, int r_out,
                           const uint8_t* out_rows, const int* checked, int r_chk, const uint8_t* chk_rows) {
    int idx[kMaxR];
    std::vector<uint8_t> rows((size_t)(r_out + r_chk) * k);
    for (int q = 0; q < r_out; ++q) idx[q] = outs[q];
    for (int q = 0; q < r_chk; ++q) idx[r_out + q] = checked[q];
    for (int i = 0; i < r_out * k; ++i) rows[i] = out_rows[i];
    for (int i = 0; i < r_chk * k; ++i) rows[(size_t)r_out * k + i] = chk_rows[i];
    return mp_pattern(buf, k, survivors, idx, r_out + r_chk, rows.data());
}

// Tiles [0, n_tiles) of `tiles`: every tile whose entry's word has 1..r rows in
// total (r >= 1: the largest total in the call) rebuilds its r_o outputs and
// ORs 1 into flags[entry] when one of its r_c checked shards differs from what
// the survivors imply; tile 0 of an entry whose word has r_c == 0 ORs 2.
// rows: the records are a shards plan's (a = the entry's address row, shardplan.h).
hipError_t launch_repair_mixed_plan(int k, int r, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                                    const uint32_t* pat_of, const uint32_t* pats, uint32_t* flags, int cus,
                                    hipStream_t stream, bool rows = false);

}  // namespace hbec
