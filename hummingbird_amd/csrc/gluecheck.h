// gluecheck.h — the object bytes of a plan's entries from their shards, with the
// surplus shards checked and bad bytes corrected on the way
// (hbec_glue_plan_checked, hbec_glue_plan_files_checked): the record of one
// present mask and the per-entry word of gf_glue_checked (gluecheck.hip,
// gluecheck_tile.h).  The call is hbec_glue_plan_mixed's (glue.h: lengths,
// destinations, the files cut) with correct.h's rule applied to what is read,
// and it stores nothing into any shard.  Everything inline here needs neither
// HIP nor a device, so it compiles alone (tests/native/gluecheck_host.cpp).
//
// One multiply.  A mask with r checked shards and o missing data shards has
// r + o <= m <= kMaxR, both counts coming out of the same m.  The kernel keeps
// A = r + o accumulator rows per column: rows 0..r-1 start as the stored
// columns of the checked shards and end as the syndrome (check row q of
// hbec_check_rows), rows r..A-1 start as zero and end as the missing data
// shards (decode row of hbec_decode_rows, data_only).  Both row sets are over
// the same k survivors, so survivor t has one block of A tables and is loaded
// once.
//
// The caveat is correct.h's: at r = 2 two bad bytes in one column can imitate a
// third shard, and the object then holds a consistent but wrong column; only a
// check outside the code (the ETag, etag.h) catches it.
#pragma once
#include <stdint.h>

#include <vector>

#include "gf256.h"
#include "glue.h"

#if defined(__HIPCC__)
#define HBEC_GC_HD __host__ __device__
#else
#define HBEC_GC_HD
#endif

namespace hbec {

// the word's layout is mixedplan.h's (kMPatShift), spelt out so that this header needs no HIP
constexpr uint32_t kGcShift = 28;
constexpr uint32_t kGcMask = (1u << kGcShift) - 1u;

// The record of one mask, as words:
//   0..2  the k survivors, a byte each (survivor j in word j / 4, bits 8 (j % 4))
//   3     the rows' shards, a byte each: checked shards 0..r-1, then the missing data shards
//   4     r | o << 8
//   5..7  zero
//   kGcHdr + 5 (t A + q)         perm_table(coefficient of row q at survivor t), A = r + o
//   gc_inverse_at(k, A) + 5 t    perm_table(1 / rows[0][t]), only with r >= 1 (correct.h cor_pattern)
// padded to 16 B.
constexpr uint32_t kGcHdr = 8;
HBEC_GC_HD inline uint32_t gc_inverse_at(int k, int A) { return (kGcHdr + 5u * (uint32_t)(k * A) + 3u) & ~3u; }
inline uint32_t gc_record_words(int k, int r, int o) {
    return gc_inverse_at(k, r + o) + (r > 0 ? (5u * (uint32_t)k + 3u) & ~3u : 0u);
}

// Per-call word of a source entry: (A << kGcShift) | record offset in 16-B
// units; kGlueSkip (glue.h) for an entry that is not the kernel's.  The counts
// r and o are the record's: an entry with exactly k present (r = 0) still needs
// its survivors and decode tables, so "nothing to check" is read there.
inline uint32_t gc_word(int A, uint32_t rec) { return ((uint32_t)A << kGcShift) | rec; }

// Append the record of one mask.  survivors: k; checked / chk_rows: r shards and
// their r x k check rows; outs / out_rows: o missing data shards and their o x k
// decode rows.  Returns its offset in 16-B units.
inline uint32_t gc_record(std::vector<uint32_t>& buf, int k, const int* survivors, const int* checked, int r,
                          const uint8_t* chk_rows, const int* outs, int o, const uint8_t* out_rows) {
    const int A = r + o;
    const size_t at = buf.size();
    buf.resize(at + gc_record_words(k, r, o), 0u);
    uint32_t* p = buf.data() + at;
    for (int j = 0; j < k; ++j) p[j / 4] |= (uint32_t)survivors[j] << (8 * (j % 4));
    for (int q = 0; q < A; ++q) {
        p[3] |= (uint32_t)(q < r ? checked[q] : outs[q - r]) << (8 * q);
        const uint8_t* row = q < r ? chk_rows + (size_t)q * k : out_rows + (size_t)(q - r) * k;
        for (int t = 0; t < k; ++t) perm_table(row[t], p + kGcHdr + 5 * (t * A + q));
    }
    p[4] = (uint32_t)r | ((uint32_t)o << 8);
    if (r > 0)
        for (int t = 0; t < k; ++t) perm_table(field().div(1, chk_rows[t]), p + gc_inverse_at(k, A) + 5 * t);
    return (uint32_t)(at / 4);
}
// read back from a record (perm_table's word 0 holds c * {0, 1, 2, 3}: byte 1 is c itself)
inline uint8_t gc_record_coef(const uint32_t* p, int A, int q, int t) { return (uint8_t)(p[kGcHdr + 5 * (t * A + q)] >> 8); }
inline uint8_t gc_record_inverse(const uint32_t* p, int k, int A, int t) {
    return (uint8_t)(p[gc_inverse_at(k, A) + 5 * t] >> 8);
}

struct MRec;
struct MTile;
// Tiles [0, n_tiles) of `tiles`: glues every tile whose entry's word is not
// kGlueSkip (A <= amax, the largest row count in the call, 0..kMaxR) as
// launch_glue_plan does, with the bytes correct.h's rule finds wrong replaced,
// and ORs the entry's word of `fixed`.  dsts: per source entry {address lo, hi,
// length lo, hi}.  rows: the records are a shards plan's.  stream: a
// hipStream_t; returns a hipError_t (plain types: this header stays free of HIP).
int launch_glue_checked(int k, int amax, const MRec* recs, const MTile* tiles, uint32_t n_tiles, const uint32_t* words,
                        const uint32_t* dsts, const uint32_t* pats, uint32_t* fixed, int cus, void* stream, bool rows);

}  // namespace hbec
