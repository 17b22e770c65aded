// etag.h — the ETag of a plan's objects from their shards, degraded or not
// (hbec_etag_plan_mixed, hbec_etag_plan_files).  The ETag is the MD5 of the
// object's own bytes, carried in every shard's metadata (ecengine.go:320-321,
// indexdb.go:739-740,768-769, ecobj.go:415-417), and the object's bytes are its
// stripes' data shards 0..k-1 back to back, cut at its length (ecGlue,
// ecutils.go:171-183): a chain runs over (entry, data shard j), j innermost,
// for lens[entry] bytes of each entry, and is hashed as one stream.
//
// A chain is walked as a list of segments.  On a slot-record plan (stripes=,
// objects=) an entry's data shards lie back to back at `a`, so a run of present
// data shards is ONE segment: a healthy entry is one segment, and no 64-B block
// straddles a shard junction.  On a row-record plan (shards=, files=) every
// shard is a segment at its own address.  Missing data shards with a byte below
// the entry's length are decoded before the chain kernel runs, by the ranged
// glue (gluerange.h), into scratch: the decoded SPAN of an entry is D[j0 S,
// min(len, (j1 + 1) S)), j0 / j1 its first / last such shard, present shards
// between them copied along, and the chain reads the whole span from scratch as
// one segment (ERec::red is the address D's byte 0 would have there).
//
// Here: the per-entry and per-chain records a call stages, the rule that gives
// the segment that starts at a data shard (shared by the kernels, etag.hip, and
// the host, which counts segments with it), and the chain list.  Everything
// needs no device and no HIP, so it compiles alone (tests/native/etag_host.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define HBEC_ETAG_FN __host__ __device__ inline
#else
#define HBEC_ETAG_FN inline
#endif

namespace hbec {

// What a call says of one source entry: the bytes of D hashed, and its span.
struct ERec {
    uint64_t len;     // D[0, len) belongs to the chain; 0: the entry has no byte in it
    uint64_t red;     // 0: nothing decoded; else D[p] of the span lies at red + p (wraps)
    uint32_t j0, j1;  // the span's first and last data shard (red != 0)
};

// One chain of a call: the entries [e0, e1), `total` bytes, digest slot `slot`.
struct EChain {
    uint64_t total;
    uint32_t e0, e1, slot, pad_;
};

// A segment of a chain: `left` bytes at `addr`; the next one starts at data shard `next`.
struct ESeg {
    uint64_t addr, left;
    uint32_t next;
};

// The first and last MISSING data shard of an entry with a byte below len (a
// shard j has one when j S < len).  present: the entry's mask, k bytes of it
// looked at.  False: nothing of the entry needs decoding.
inline bool etag_span(uint32_t k, uint64_t S, uint64_t len, const uint8_t* present, uint32_t* j0, uint32_t* j1) {
    bool any = false;
    for (uint32_t j = 0; j < k && (uint64_t)j * S < len; ++j) {
        if (present[j]) continue;
        if (!any) *j0 = j;
        *j1 = j;
        any = true;
    }
    return any;
}

// D's positions [lo, hi) of the span of shards j0..j1 in an entry of len bytes.
HBEC_ETAG_FN uint64_t etag_span_lo(uint64_t S, uint32_t j0) { return (uint64_t)j0 * S; }
HBEC_ETAG_FN uint64_t etag_span_hi(uint64_t S, uint64_t len, uint32_t j1) {
    const uint64_t hi = ((uint64_t)j1 + 1u) * S;
    return hi < len ? hi : len;
}

// The segment of an entry that starts at data shard j, or false when the entry
// has no byte there (j S >= len: the entry is over).  Slot records: data shard
// j at a + j S.  k S >= len, so `next` = k ends the entry.
HBEC_ETAG_FN bool etag_segment_slot(uint64_t a, uint64_t S, const ERec& r, uint32_t j, uint32_t k, ESeg* s) {
    const uint64_t pos = (uint64_t)j * S;
    if (pos >= r.len) return false;
    if (r.red != 0u && j < r.j0) {  // the present run in front of the span
        s->addr = a + pos, s->left = etag_span_lo(S, r.j0) - pos, s->next = r.j0;
    } else if (r.red != 0u && j <= r.j1) {
        s->addr = r.red + pos, s->left = etag_span_hi(S, r.len, r.j1) - pos, s->next = r.j1 + 1u;
    } else {  // the present run to the entry's end
        s->addr = a + pos, s->left = r.len - pos, s->next = k;
    }
    return true;
}

// Row records: data shard j at row(j), read only for a shard that is a segment.
template <class Row>
HBEC_ETAG_FN bool etag_segment_rows(Row&& row, uint64_t S, const ERec& r, uint32_t j, ESeg* s) {
    const uint64_t pos = (uint64_t)j * S;
    if (pos >= r.len) return false;
    if (r.red != 0u && j >= r.j0 && j <= r.j1) {
        s->addr = r.red + pos, s->left = etag_span_hi(S, r.len, r.j1) - pos, s->next = r.j1 + 1u;
    } else {
        const uint64_t rest = r.len - pos;
        s->addr = row(j), s->left = rest < S ? rest : S, s->next = j + 1u;
    }
    return true;
}

// The segments an entry is walked in (what the kernels' cursors open).
inline uint32_t etag_entry_segments(bool rows, uint32_t k, uint64_t S, const ERec& r) {
    uint32_t n = 0, j = 0;
    ESeg s;
    while (rows ? etag_segment_rows([](uint32_t) { return (uint64_t)0; }, S, r, j, &s)
                : etag_segment_slot(0u, S, r, j, k, &s)) {
        ++n;
        j = s.next;
    }
    return n;
}

// The chain list of one call: an object (entries [object_start[g],
// object_start[g + 1]); object_start == nullptr: every entry is its own
// object) with a byte in it is one chain, longest first (equal totals in object
// order): the 64 lanes of a wave run similar trip counts.  Totals are 64-bit.
inline void etag_chains(const std::vector<ERec>& recs, const uint32_t* object_start, uint32_t n_objects,
                        std::vector<EChain>& chains) {
    chains.clear();
    for (uint32_t g = 0; g < n_objects; ++g) {
        const uint32_t e0 = object_start ? object_start[g] : g, e1 = object_start ? object_start[g + 1] : g + 1u;
        uint64_t total = 0;
        for (uint32_t e = e0; e < e1; ++e) total += recs[e].len;
        if (total) chains.push_back(EChain{total, e0, e1, g, 0u});
    }
    std::stable_sort(chains.begin(), chains.end(), [](const EChain& x, const EChain& y) { return x.total > y.total; });
}

// Whole 64-B blocks of a chain (a lane's trip count), the bytes behind them,
// and the blocks of the MD5 pad (1, or 2 when the tail leaves no room for 0x80
// and the 64-bit length).  The bit length is total * 8 modulo 2^64, as MD5 has it.
HBEC_ETAG_FN uint64_t etag_blocks(uint64_t total) { return total / 64u; }
HBEC_ETAG_FN uint32_t etag_tail(uint64_t total) { return (uint32_t)(total - etag_blocks(total) * 64u); }
HBEC_ETAG_FN uint32_t etag_pad_blocks(uint64_t total) { return etag_tail(total) >= 56u ? 2u : 1u; }
HBEC_ETAG_FN uint64_t etag_bits(uint64_t total) { return total * 8u; }

// Chains [0, n_chains), one lane each (etag.hip): the MD5 of the chain's bytes
// when any of its entries passes the filter (filter == nullptr, or
// filter[entry] & filter_bits); digest to digests + slot 16 when digests is
// given; bad[slot] |= 1 when expected is given and differs there.  recs: the
// plan's hash records (HRec, hashplan.h); rows: they are a shards plan's.
// stream: a hipStream_t; returns a hipError_t (both as plain types, so this
// header stays free of HIP).
int launch_etag_chains(const void* recs, const ERec* erecs, const EChain* chains, uint64_t n_chains, int k,
                       const uint32_t* filter, uint32_t filter_bits, const uint8_t* expected, uint8_t* digests,
                       uint32_t* bad, void* stream, bool rows);

}  // namespace hbec
