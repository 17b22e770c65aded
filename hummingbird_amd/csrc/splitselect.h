// splitselect.h — chosen shards of a plan's entries from their object bytes
// (hbec_split_plan_select, hbec_split_plan_files_select): ecSplit's loop
// (ecutils.go:26-72) with its writers.  ecSplit writes shard i of a stripe only
// where writers[i] != nil && !failed[i] (ecutils.go:63); here entry i of the
// plan has a row of k + m bytes, and shard j of it is written whole if and
// only if its byte is set.  The cut and the pad are splitplan.h's.
//
// Here: the host arithmetic of the call.  The record of one distinct mask as
// the kernels read it, and which inputs a tile needs and in which order.
// Everything is inline and needs neither HIP nor a
// device, so it compiles alone (tests/native/splitselect_host.cpp).  The
// kernels are gf_split_select_plan and gf_split_select_plan_rows
// (splitselect.hip, splitselect_tile.h).
#pragma once
#include <stdint.h>

#include <vector>

#include "gf256.h"
#include "splitplan.h"

#if defined(__HIPCC__)
#define HBEC_SS_HD __host__ __device__
#else
#define HBEC_SS_HD
#endif

namespace hbec {

// Per-call word of a source entry: (R << kSsShift) | record offset in 16-B
// units, as mixedplan.h's word; R = the entry's count of selected parity rows,
// 0..4 (0: a partial scatter).  kSsSkip says the entry is not the kernel's
// (nothing selected, no bytes given, or the per-entry route); its R reads as
// 15: above every instance's largest.
constexpr uint32_t kSsShift = 28;
constexpr uint32_t kSsMask = (1u << kSsShift) - 1u;
constexpr uint32_t kSsSkip = 0xFFFFFFFFu;

// The record of one distinct mask, as words:
//   [0] store mask: bit j set where data shard j is written
//   [1] read mask:  the data shards the tile reads; all k when a parity row is
//       selected (every input goes into every row), else the store mask
//   [2] the selected parity shards' indices k + r, a byte each, ascending
//   [3] R, their count (the kernel takes it from the entry's word)
// then, for R > 0, the v_perm tables (gf256.h perm_table) of selected row r x
// data shard j at word kSsHdr + 5 (j R + r): the R rows of one input lie
// together, and an unselected row has no table.  Padded to 16 B; a record is
// as long as its mask needs (no parity: 16 B; 4+2 with one row: 96 B; 12+4
// with all four: 976 B).
constexpr uint32_t kSsHdr = 4;
inline uint32_t ss_record_words(int k, int R) { return (kSsHdr + 5u * (uint32_t)(k * R) + 3u) & ~3u; }
inline uint32_t ss_table_at(int R, int j, int r) { return kSsHdr + 5u * (uint32_t)(j * R + r); }

// Selected parity rows of a mask of k + m bytes.
inline int ss_parity_count(int k, int m, const uint8_t* mask) {
    int R = 0;
    for (int r = 0; r < m; ++r) R += mask[k + r] ? 1 : 0;
    return R;
}
inline uint32_t ss_store_mask(int k, const uint8_t* mask) {
    uint32_t s = 0;
    for (int j = 0; j < k; ++j) s |= mask[j] ? 1u << j : 0u;
    return s;
}

// Append the record of `mask` (k <= 12, at most 4 parity rows selected;
// enc_rows: rows k..k+m-1 of the coding matrix, m x k coefficients); returns
// its offset in 16-B units and the count of selected rows in *R_out.
inline uint32_t ss_record(std::vector<uint32_t>& buf, int k, int m, const uint8_t* mask, const uint8_t* enc_rows,
                          int* R_out) {
    const int R = ss_parity_count(k, m, mask);
    const size_t at = buf.size();
    buf.resize(at + ss_record_words(k, R), 0u);
    uint32_t* p = buf.data() + at;
    p[0] = ss_store_mask(k, mask);
    p[1] = R > 0 ? (1u << k) - 1u : p[0];
    p[3] = (uint32_t)R;
    int q = 0;
    for (int r = 0; r < m; ++r) {
        if (!mask[k + r]) continue;
        p[2] |= (uint32_t)(k + r) << (8 * q);
        for (int j = 0; j < k; ++j) perm_table(enc_rows[(size_t)r * k + j], p + ss_table_at(R, j, q));
        ++q;
    }
    *R_out = R;
    return (uint32_t)(at / 4);
}

// The inputs a tile of an entry walks, as bits: a data shard it stores (an
// all-pad one too: it is written as zeros), and a data shard it reads that has
// a byte of the piece (V_j > 0: j S < len).  An input read for the parity
// alone that is all pad adds nothing to any row and is left out.  They are
// walked in ascending order, ss_next_input by ss_next_input.
HBEC_SS_HD inline uint32_t ss_needed_inputs(uint32_t store, uint32_t read, uint32_t k, uint64_t len, uint64_t S) {
    uint32_t need = store;
    for (uint32_t j = 0; j < k; ++j)
        if ((uint64_t)j * S < len) need |= read & (1u << j);  // j < 12 and S < 2^31 on the device
    return need;
}
// The lowest input of `rest` (not 0), which it leaves.
HBEC_SS_HD inline uint32_t ss_next_input(uint32_t& rest) {
    const uint32_t j = (uint32_t)__builtin_ctz(rest);
    rest &= rest - 1u;
    return j;
}

// Tiles [0, n_tiles) of `tiles`: splits every tile whose entry's word is not
// kSsSkip.  rmax: the largest count of selected parity rows in the call,
// 0..kMaxR.  srcs: per source entry {address lo, hi, length lo, hi}.  rows: the
// records are a shards plan's.  stream: a hipStream_t; returns a hipError_t
// (both as plain types, so this header stays free of HIP).
int launch_split_select_plan(int k, int rmax, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                             const uint32_t* words, const uint32_t* srcs, const uint32_t* pats, int cus, void* stream,
                             bool rows);

}  // namespace hbec
