// gluerangecheck.h — any byte range of a plan's entries from ALL their present
// shards, with the surplus shards checked and bad bytes corrected on the way
// (hbec_glue_plan_range_checked, hbec_glue_plan_files_range_checked): the
// per-entry word of gf_range_checked (gluerangecheck.hip, gluerangecheck_tile.h)
// and the byte mask of the examined positions.  The call is hbec_glue_plan_range's
// (gluerange.h: windows, bases, the files cut) with correct.h's rule applied at
// the shard positions P = gr_positions(S, s, e), and it stores nothing into any
// shard.  Everything inline here needs neither HIP nor a device, so it compiles
// alone (tests/native/gluerangecheck_host.cpp).
//
// The caveat is correct.h's: at r = 2 two bad bytes in one column can imitate a
// third shard, and the range then holds a consistent but wrong column; only a
// check outside the code (the ETag, etag.h) catches it.
#pragma once
#include <stdint.h>

#include "gluerange.h"

namespace hbec {

// Per-call word of a source entry: four bits over the record's offset in 16-B
// units (the layout is mixedplan.h's kMPatShift, spelt out so that this header
// needs no HIP).  A mask with r >= 1 checked shards has a gc_record (gluecheck.h)
// and the bits hold A = r + o, 1..kMaxR.  A mask with exactly k present has
// nothing to check and is glued exactly as gf_range_plan glues it: its record is
// that kernel's mp_pattern (mixedplan.h) and the bits hold kGrcPlain | o.
// kGlueSkip (glue.h) reads as 15, which is neither.
constexpr uint32_t kGrcShift = 28;
constexpr uint32_t kGrcMask = (1u << kGrcShift) - 1u;
constexpr uint32_t kGrcPlain = 8u;
inline uint32_t grc_word(int r, int o, uint32_t rec) {
    return ((r > 0 ? (uint32_t)(r + o) : kGrcPlain | (uint32_t)o) << kGrcShift) | rec;
}
// the accumulator rows an entry's tile keeps: what the instance's AMAX must cover
inline int grc_rows(int r, int o) { return r > 0 ? r + o : o; }

// 0xFF in byte b of the result where shard position pos + b lies in w, b = 0..3.
HBEC_GR_FN uint32_t grc_window_mask(GrWin w, uint64_t pos) {
    if (!(w.lo < w.hi && pos < w.hi && w.lo < pos + 4u)) return 0u;
    const uint32_t b0 = w.lo > pos ? (uint32_t)(w.lo - pos) : 0u;        // 0..3
    const uint32_t b1 = w.hi - pos < 4u ? (uint32_t)(w.hi - pos) : 4u;  // b0 < b1 <= 4
    return (0xFFFFFFFFu >> (8u * (4u - b1))) & (0xFFFFFFFFu << (8u * b0));
}

// The examined bytes of the dword at shard positions [pos, pos + 4): those in P
// (gr_positions).  Both ends of both intervals may fall inside one dword.
HBEC_GR_FN uint32_t grc_live_mask(GrSpan P, uint64_t pos) {
    return grc_window_mask(P.a, pos) | grc_window_mask(P.b, pos);
}

struct MRec;
struct MTile;
// Tiles [0, n_tiles) of `tiles`: glues the range of every tile whose entry's
// word is not kGlueSkip (grc_rows <= amax, the largest in the call, 0..kMaxR) as
// launch_glue_range does, from every present shard, with the bytes correct.h's
// rule finds wrong at the positions P replaced, and ORs the entry's word of
// `fixed`.  ranges: per source entry {address, start, length}, 64 bits each,
// low word first.  rows: the records are a shards plan's.  stream: a
// hipStream_t; returns a hipError_t (plain types: this header stays free of HIP).
int launch_glue_range_checked(int k, int amax, const MRec* recs, const MTile* tiles, uint32_t n_tiles,
                              const uint32_t* words, const uint32_t* ranges, const uint32_t* pats, uint32_t* fixed,
                              int cus, void* stream, bool rows);

}  // namespace hbec
