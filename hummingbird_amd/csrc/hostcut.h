// hostcut.h — how the host path (hostpath.cpp) cuts a batch of host stripes: which stripes
// are coded in place and which are staged, the column pieces and chunks of the staging ring,
// the chunks of a staged Verify, and the records of one slot of a zero-copy run.  No HIP call
// and no global: capacities, tile sizes and whatever depends on the kernels (urec_span, the
// mirror pitch, edge records, the pinned-memory lookup) are arguments, so the rules link
// against nothing and run on a CPU (tests/native/host_cut.cpp).  A refusal is returned as its
// text (all are HBEC_ERR_INVALID_ARG), nullptr for none.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/hbec.h"
#include "kernels.h"
#include "vplan.h"

namespace hbec {
namespace cut {

// One pass over every stripe: outputs = shards out_idx from inputs = shards in_idx by
// `rows`.  With d_digest (device, n * n_shards * 16 B) every input and output shard
// is hashed too: digest of shard i of stripe s at (s * n_shards + i) * 16.
struct Pass {
    std::vector<int> in_idx, out_idx;
    std::vector<uint8_t> rows;
    uint8_t* d_digest = nullptr;
    int n_shards = 0;
};

// the highest shard index the pass touches: a stripe is pinned when [base, base + (top + 1) S) is
inline int top_shard(const Pass& ps) {
    int top = 0;
    for (int i : ps.in_idx) top = std::max(top, i);
    for (int i : ps.out_idx) top = std::max(top, i);
    return top;
}

// ---- which path a stripe takes ----
// aligned: pinned, host and device base 16-B aligned, S % 16 == 0 (the stripes kernel);
// any_alignment: pinned otherwise, where any_align allows it and the 32-bit positions of
// gf_odd reach (the unaligned kernel); staged: the ring, which is also where a null base goes
// to be refused.  pinned(p, len) is the device address of [p, p + len) or 0, and becomes dev.
enum class Kind { empty, aligned, any_alignment, staged };
template <class Pinned>
inline Kind classify(const hbec_stripe& st, int top, bool any_align, Pinned&& pinned, uint64_t& dev) {
    const uint64_t S = st.shard_len;
    if (S == 0) return Kind::empty;
    const bool aligned = (reinterpret_cast<uintptr_t>(st.base) & 15u) == 0 && S % 16 == 0 && S < (1ull << 32);
    const bool any = any_align && pos32_shard(S);
    if (!st.base || (!aligned && !any)) return Kind::staged;
    dev = pinned(st.base, (uint64_t)(top + 1) * S);
    if (!dev) return Kind::staged;
    if (aligned && (dev & 15u) == 0) return Kind::aligned;
    return any ? Kind::any_alignment : Kind::staged;
}

struct ZcStripe {
    uint64_t dev;  // device address of the stripe base
    uint64_t shard_len;
};

// A plain call: every stripe on its own, pinned ones in place, the rest staged.
template <class Pinned>
inline void route_plain(const hbec_stripe* stripes, uint64_t n, int top, bool any_align, Pinned&& pinned,
                        std::vector<ZcStripe>& aligned, std::vector<ZcStripe>& any, std::vector<hbec_stripe>& staged) {
    for (uint64_t s = 0; s < n; ++s) {
        uint64_t dev = 0;
        const Kind kind = classify(stripes[s], top, any_align, pinned, dev);
        if (kind == Kind::aligned) aligned.push_back({dev, stripes[s].shard_len});
        else if (kind == Kind::any_alignment) any.push_back({dev, stripes[s].shard_len});
        else if (kind == Kind::staged) staged.push_back(stripes[s]);
    }
}

// A hashing call is all or nothing: Kind::staged (the ring takes the whole
// batch) at the first stripe that is not pinned, Kind::aligned (the mirror
// kernel) when every stripe is aligned, else Kind::any_alignment for all.
template <class Pinned>
inline Kind route_hashing(const hbec_stripe* stripes, uint64_t n, int top, bool any_align, Pinned&& pinned,
                          std::vector<ZcStripe>& zs) {
    Kind all = Kind::aligned;
    zs.reserve(n);
    for (uint64_t s = 0; s < n; ++s) {
        uint64_t dev = 0;
        const Kind kind = classify(stripes[s], top, any_align, pinned, dev);
        if (kind != Kind::aligned && kind != Kind::any_alignment) return Kind::staged;
        if (kind == Kind::any_alignment) all = kind;
        zs.push_back({dev, stripes[s].shard_len});
    }
    return all;
}

// ---- the staging ring: column pieces in chunks of one slot ----
// One column piece of one stripe: columns [col, col+len) of its K inputs / R outputs.
struct Piece {
    uint64_t stripe, col;
    uint64_t len;   // bytes (<= shard_len - col)
    uint64_t lpad;  // len rounded up to 16
    uint64_t in_off, out_off;  // offsets of this piece in the slot's IN / OUT regions
};

// max columns per piece so that K*lpad fits the IN slot and R*lpad the OUT slot
inline uint64_t slot_cols(uint64_t in_cap, uint64_t out_cap, int K, int R) {
    return (std::min(in_cap / (uint64_t)K, out_cap / (uint64_t)R) / 16) * 16;
}

// Hashing hashes whole shards where they lie in a slot (hbec.h: one staging
// slot), on the ring and, for the same bound, in place.
template <class Stripe>
inline const char* hash_slot_bound(const Stripe* stripes, uint64_t n, uint64_t max_cols) {
    for (uint64_t s = 0; s < n; ++s)
        if (stripes[s].shard_len > max_cols) return "hashing needs every stripe to fit one staging slot";
    return nullptr;
}

// Cut the batch into chunks of pieces that fit a slot; whole_stripes: a
// hashing call.  n_pieces counts the pieces cut, also those before a refusal.
inline const char* cut_ring(const hbec_stripe* stripes, uint64_t n, int K, int R, uint64_t in_cap, uint64_t out_cap,
                            uint64_t tile_cap, uint64_t tile, bool whole_stripes,
                            std::vector<std::vector<Piece>>& chunks, uint64_t& n_pieces) {
    n_pieces = 0;
    chunks.assign(1, {});
    const uint64_t max_cols = slot_cols(in_cap, out_cap, K, R);
    if (max_cols < 16) return "staging slot too small";
    if (const char* err = whole_stripes ? hash_slot_bound(stripes, n, max_cols) : nullptr) return err;
    uint64_t in_used = 0, out_used = 0, tiles_used = 0;
    for (uint64_t s = 0; s < n; ++s) {
        const uint64_t S = stripes[s].shard_len;
        if (S == 0) continue;
        if (!stripes[s].base) return "stripe with null base";
        for (uint64_t col = 0; col < S; col += max_cols, ++n_pieces) {
            const uint64_t len = std::min(max_cols, S - col), lpad = (len + 15) / 16 * 16;
            const uint64_t nt = (lpad + tile - 1) / tile;
            if (in_used + K * lpad > in_cap || out_used + R * lpad > out_cap || tiles_used + nt > tile_cap) {
                chunks.emplace_back();
                in_used = out_used = tiles_used = 0;
            }
            chunks.back().push_back({s, col, len, lpad, in_used, out_used});
            in_used += K * lpad;
            out_used += R * lpad;
            tiles_used += nt;
        }
    }
    if (chunks.back().empty()) chunks.pop_back();
    return nullptr;
}

// ---- staged Verify: blocks of (k+m) x len bytes in chunks of one IN slot ----
struct VPiece {
    uint64_t stripe, col, len, off;  // off: the piece's (k+m) x len block in the slot
    bool whole;                      // col == 0 and len == S: one copy
};

// bytes of the Verify records (vp_add) of a piece of len columns
inline uint64_t vrec_bytes(uint64_t len) {
    return sizeof(VRec) + (uint64_t)((vp_main_bytes((uint32_t)len) + kVpTile - 1) / kVpTile) * sizeof(VTile);
}

// staged: the non-empty stripes to stage, L = k + m.  A stripe that fits a
// slot is one block, a larger one is cut into column pieces; blocks start 16-B
// aligned, and a chunk's records fit rec_cap bytes.
inline const char* cut_verify(const hbec_stripe* stripes, const std::vector<uint64_t>& staged, uint64_t L,
                              uint64_t in_cap, uint64_t rec_cap, std::vector<std::vector<VPiece>>& chunks) {
    chunks.assign(1, {});
    const uint64_t max_cols = (in_cap / L / 16) * 16;
    if (max_cols < 16) return "staging slot too small";
    uint64_t used = 0, rused = 0;
    for (uint64_t s : staged) {
        const uint64_t S = stripes[s].shard_len;
        const bool whole = L * S <= in_cap;
        for (uint64_t col = 0; col < S; col += whole ? S : max_cols) {
            const uint64_t len = whole ? S : std::min(max_cols, S - col);
            const uint64_t bytes = (L * len + 15) & ~(uint64_t)15, rb = vrec_bytes(len);
            if (used + bytes > in_cap || rused + rb > rec_cap) {
                chunks.emplace_back();
                used = rused = 0;
            }
            chunks.back().push_back({s, col, len, used, whole});
            used += bytes;
            rused += rb;
        }
    }
    return nullptr;
}

// ---- records ----
// Tile `off` of a block of len columns: inputs from `in`, outputs from `out`,
// shards `stride` bytes apart in both.
inline TileRec tile_rec(uint64_t in, uint64_t out, uint64_t stride, uint64_t off, uint64_t len, uint64_t tile) {
    return {in + off, out + off, (uint32_t)stride, (uint32_t)stride, (uint32_t)std::min(tile, len - off), 0};
}

// The two record kinds of a zero-copy run.  rec(z, out, off): the record at
// shard position off of stripe z that writes (plain: in_place) or mirrors
// (hashing: the arena) to out.  TileRec of the stripes kernel: one per tile of
// S, shards S apart in the arena.
struct TileRecs {
    using Rec = TileRec;
    static constexpr uint64_t kEdge = 0;  // edge records per stripe
    static constexpr bool edges = false;
    uint64_t tile;
    uint64_t span(uint64_t S) const { return S; }
    uint64_t pitch(uint64_t S) const { return S; }
    uint64_t in_place(uint64_t dev) const { return dev; }
    Rec rec(const ZcStripe& z, uint64_t out, uint64_t off) const {
        return tile_rec(z.dev, out, z.shard_len, off, z.shard_len, tile);
    }
};
// URec of the unaligned kernels: one per tile below span(S) (none when it is
// 0) and, with gf_odd (edges), one edge record per stripe for the rest; shards
// pitch(S) apart in the arena.
struct URecs {
    using Rec = URec;
    static constexpr uint64_t kEdge = 1;
    uint64_t tile;
    uint64_t (*span)(uint64_t);
    uint64_t (*pitch)(uint64_t);
    bool edges;
    uint64_t in_place(uint64_t) const { return 0; }
    Rec rec(const ZcStripe& z, uint64_t out, uint64_t off) const { return {z.dev, out, z.shard_len, off}; }
};

// What a record slot holds: n_main records, then n_edge edge records.
struct SlotFill {
    uint64_t n_main = 0, n_edge = 0;
};

// A plain run fills every slot but the last: a stripe may straddle slots, off (the next
// shard position of stripe si) carries over.  An edge record goes to the slot its stripe
// starts in, and a slot closes while one more main and edge record would still fit.
template <class Recs>
inline SlotFill fill_plain(const Recs& p, const std::vector<ZcStripe>& zs, size_t& si, uint64_t& off,
                           typename Recs::Rec* rec, uint64_t tile_cap) {
    SlotFill f;
    std::vector<typename Recs::Rec> edges;
    while (si < zs.size() && f.n_main + edges.size() + Recs::kEdge < tile_cap) {
        const ZcStripe& z = zs[si];
        const uint64_t span = p.span(z.shard_len);
        if (p.edges && off == 0) edges.push_back(p.rec(z, p.in_place(z.dev), 0));
        if (off < span) rec[f.n_main++] = p.rec(z, p.in_place(z.dev), off);
        off += p.tile;
        if (off >= span) {
            off = 0;
            ++si;
        }
    }
    std::copy(edges.begin(), edges.end(), rec + f.n_main);
    f.n_edge = edges.size();
    return f;
}

// A hashing run keeps whole stripes in a slot and mirrors each to the hash arena of cursor ac
// (ArenaCursor: fits, base, add, used): shard i of stripe s at base + i * pitch(S), its MD5
// record for digest s * n_shards + i, the stripe's arena bytes rounded to 256.  A stripe the
// arena cannot take closes the slot (the arena is hashed after the slot's kernels); when the
// slot is still empty the caller's flush() hashes the arena now (false: it failed).
template <class Recs, class Cursor, class Flush>
inline const char* fill_md5(const Recs& p, const std::vector<ZcStripe>& zs, size_t& si, typename Recs::Rec* rec,
                            uint64_t tile_cap, uint64_t arena_cap, const Pass& ps, Cursor& ac, Flush&& flush,
                            SlotFill& f) {
    std::vector<typename Recs::Rec> edges;  // one per stripe of this slot
    for (; si < zs.size(); ++si) {
        const ZcStripe& z = zs[si];
        const uint64_t S = z.shard_len, span = p.span(S), pitch = p.pitch(S);
        const uint64_t tiles = (span + p.tile - 1) / p.tile;
        const uint64_t bytes = ((uint64_t)ps.n_shards * pitch + 255) & ~uint64_t(255);
        if (tiles + 2 * Recs::kEdge > tile_cap || bytes > arena_cap) return "stripe too large for a hash arena";
        // a stripe may add an edge record and no main record, so either kind fills the slot
        const bool any = f.n_main > 0 || !edges.empty();
        if (any && f.n_main + edges.size() + tiles + Recs::kEdge > tile_cap) break;
        if (!ac.fits(bytes, (uint64_t)(ps.in_idx.size() + ps.out_idx.size()))) {
            if (any) break;
            if (!flush()) return nullptr;
        }
        const uint64_t mbase = ac.base();  // 256-B aligned
        for (uint64_t off = 0; off < span; off += p.tile) rec[f.n_main++] = p.rec(z, mbase, off);
        if (Recs::kEdge) edges.push_back(p.rec(z, mbase, 0));
        for (const std::vector<int>* idx : {&ps.in_idx, &ps.out_idx})
            for (int i : *idx) ac.add(mbase + (uint64_t)i * pitch, S, (uint64_t)si * (uint64_t)ps.n_shards + (uint64_t)i);
        ac.used += bytes;
    }
    std::copy(edges.begin(), edges.end(), rec + f.n_main);
    f.n_edge = edges.size();
    return nullptr;
}

}  // namespace cut
}  // namespace hbec
