// splitselect_tile.h — the wave tile of gf_split_select_plan (splitselect.hip):
// the selected shards of one entry from its object piece [src, src + len), an
// unselected shard left as it is (ecSplit's writers, ecutils.go:26-72, line
// 63).  The cut, the pad rule, the junction rule, the 16-B-store-only-inside-
// own-shard rule and the bytewise head and tail are split_tile.h's, and its
// split_store and split_pad_mask are used as they stand.  What differs:
//   1. The input loop runs over the needed inputs only (splitselect.h
//      ss_needed_inputs), lowest first, not over 0..k-1: the data shards the
//      mask stores and, where a parity row is selected, every data shard with
//      a byte of the piece.  The one-ahead prefetch targets the next needed
//      input, so a skipped shard leaves no bubble and costs no load.
//   2. Input j is stored to data shard j only where the store mask has bit j
//      (wave-uniform).  With R = 0 the tile is a partial scatter: it reads the
//      pieces of the selected data shards and nothing else.
//   3. R counts the selected parity rows, not m.  The record holds their R
//      tables per input and their shard indices; an unselected row is neither
//      multiplied nor stored.
// An input with V_j = 0 is not loaded (split_tile.h's first difference); it is
// in the loop only where it is stored, as zeros.
// Everything of the record is read through the wave-uniform __restrict__
// pointer p (scalar loads): no LDS, no per-lane gather.  Every write is a
// per-lane vector store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.h"
#include "kernels.h"
#include "shard_rows.h"
#include "split_tile.h"
#include "splitselect.h"
#include "unaligned_tile.h"

namespace hbec {

// One wave tile: U windows from shard position p0 < S of one entry with R
// selected parity rows.  p: the record of the entry's mask (splitselect.h).
// Every argument but lane is wave-uniform.  U: the windows coded together,
// kUnalignedU (the list's tile) or a part of it (R = 4 in two halves).
template <int R, bool ROWS, int U = kUnalignedU>
__device__ __forceinline__ void split_select_tile(int K, uint64_t a, uint64_t b, uint64_t S, uint64_t p0, uint64_t src,
                                                  uint64_t len, const uint32_t* __restrict__ p, uint32_t lane) {
    constexpr uint32_t W = kUnalignedWindow;
    constexpr int RA = R > 0 ? R : 1;
    const uint32_t k = (uint32_t)K;
    const uint32_t store = p[0];
    uint32_t rest = ss_needed_inputs(store, p[1], k, len, S);
    if (rest == 0u) return;  // never with a word the host built: R = 0 has a bit stored, R > 0 reads input 0
    // bytes of virtual shard i inside the piece: clamp(len - i S, 0, S)
    auto valid = [=](uint32_t i) {
        const uint64_t off = (uint64_t)i * S;  // i < k <= 12, S < 2^31
        return len <= off ? (uint64_t)0 : (len - off < S ? len - off : S);
    };

    uint64_t col[U];
    bool live[U];  // window-uniform
#pragma unroll
    for (int u = 0; u < U; ++u) {
        col[u] = p0 + (uint64_t)u * W + lane * 16u;
        live[u] = p0 + (uint64_t)u * W < S;
    }
    u32x4 acc[RA][U];
#pragma unroll
    for (int r = 0; r < RA; ++r)
#pragma unroll
        for (int u = 0; u < U; ++u) acc[r][u] = u32x4{0, 0, 0, 0};
    u32x4 clo[U], chi[U];
    uint32_t j = ss_next_input(rest);  // the first needed input
    uint64_t cV = valid(j);
    UView cv = uview(src + (uint64_t)j * S, cV);
    if (cV > 0u) {  // wave-uniform
#pragma unroll
        for (int u = 0; u < U; ++u) uload(clo[u], chi[u], cv, col[u]);  // clamped: no branch
    } else {  // all pad, stored as zeros
#pragma unroll
        for (int u = 0; u < U; ++u) clo[u] = chi[u] = u32x4{0, 0, 0, 0};
    }
#pragma unroll 1
    for (;;) {
        const bool more = rest != 0u;  // wave-uniform
        u32x4 nlo[U], nhi[U];
        UView nv = cv;
        uint64_t nV = cV;
        uint32_t nj = j;
        if (more) {
            nj = ss_next_input(rest);
            nV = valid(nj);
            nv = uview(src + (uint64_t)nj * S, nV);
            if (nV > 0u) {  // wave-uniform
#pragma unroll
                for (int u = 0; u < U; ++u) uload(nlo[u], nhi[u], nv, col[u]);
            } else {  // all pad: nothing of the piece is there to load
#pragma unroll
                for (int u = 0; u < U; ++u) nlo[u] = nhi[u] = u32x4{0, 0, 0, 0};
            }
        }
        uint32_t tb[RA][5];
        if constexpr (R > 0) {
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int q = 0; q < 5; ++q) tb[r][q] = (p + kSsHdr + 5u * (j * (uint32_t)R + (uint32_t)r))[q];
        }
        const bool stored = ((store >> j) & 1u) != 0u;  // wave-uniform
        const uint64_t db = stored ? shard_at<ROWS>(a, b, S, k, j) : 0u;  // data shard j
        const uint32_t de = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(db & 15u)) & 15u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u32x4 x = realign16(clo[u], upper(clo[u], chi[u]), cv.d);
            if (cV < S) x = split_pad_mask(x, col[u], cV);  // wave-uniform: the pad is zero
            if constexpr (R > 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const Sel sx = selectors(x[e]);
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        acc[r][u][e] ^= gf_mul_sel(sx, tb[r][0], tb[r][1], tb[r][2], tb[r][3], tb[r][4]);
                }
            }
            if (stored && live[u]) split_store(db, S, de, x, col[u], lane);
        }
        if (!more) break;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            clo[u] = nlo[u];
            chi[u] = nhi[u];
        }
        cv = nv;
        cV = nV;
        j = nj;
    }
    if constexpr (R > 0) {
        const uint32_t prow = p[2];  // the selected parity shards' indices
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t ob = shard_at<ROWS>(a, b, S, k, (prow >> (8 * r)) & 0xFFu);
            const uint32_t e = __builtin_amdgcn_readfirstlane((16u - (uint32_t)(ob & 15u)) & 15u);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!live[u]) continue;  // window-uniform: every lane takes part in the shuffle
                split_store(ob, S, e, acc[r][u], col[u], lane);
            }
        }
    }
}

}  // namespace hbec
