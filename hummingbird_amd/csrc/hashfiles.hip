// hashfiles.hip — md5_files: the ShardHash of the selected shard FILES of a
// plan's objects, one LANE per chain (hashfiles.h).  A shard file is shard j of
// each of the object's entries back to back (ecSplit appends it stripe by
// stripe, ecutils.go:38-70), hashed as one stream: one pad, one 64-bit length.
// The compression is md5_device.h's and the schedule md5_plan's (hashplan.hip):
// a wave-uniform trip count from the wave's longest chain, counted in blocks of
// the TOTAL length, two load groups of HBEC_MD5_DEPTH_LIST blocks ping-ponged,
// lanes past their own end keeping their state with a select.
//
// What differs is that a lane walks a list of segments, not one address.  It
// keeps two cursors {entry, address, bytes left in the segment}: one for the
// loads running ahead, one for the block being compressed.  Both take the same
// steps, so the block a slot was loaded for is the block the other cursor
// stands on when the slot is compressed.  A 64-B block that lies wholly inside
// a segment takes md5_plan's loader: dword-aligned 16-B groups from addr & ~3
// plus one dword, shifted into place with 16 v_alignbyte_b32.  The shift comes
// from that block's own address, since it changes at every segment boundary and
// after every block that straddles one; shift 0 re-reads the block's last dword,
// so no load touches a dword that holds no byte of the segment.  A block that
// straddles a boundary (a short last piece, or pieces so small that one block
// spans three or more of them) is put together bytewise from the segments it
// spans, in a branch a wave enters only when one of its lanes needs it; its
// prefetch slot loads the zero block.  So do the slots of lanes past their end.
//
// The filter is read on the device: a lane scans its object's entries for a
// passing word before any shard load (a shard file can only be hashed whole),
// and a wave with no examined lane returns at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.h"
#include "hashfiles.h"
#include "kernels.h"
#include "md5_device.h"

namespace hbec {

namespace {

// load target of straddling blocks and of lanes past their end
__device__ __attribute__((aligned(16))) uint8_t kFilesZeroBlock[64];

typedef __attribute__((address_space(1))) const uint32_t fu32_c;
typedef __attribute__((address_space(1))) const uint8_t fu8_c;
// 16 B at a dword-aligned address: one global_load_dwordx4
typedef uint32_t fu32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(1))) const fu32x4_a4 fu32x4_a4_c;

// Where a lane stands in its chain: on byte `addr` of entry `e`'s shard, with
// `left` bytes of that shard to go.
struct FCursor {
    uint32_t e;
    uint64_t addr, left;
};

}  // namespace

__global__ __launch_bounds__(64) void md5_files(const HRec* __restrict__ recs,
                                                const uint32_t* __restrict__ object_start,
                                                const FChain* __restrict__ chains, uint64_t n_chains, uint32_t k,
                                                uint32_t n, const uint32_t* __restrict__ filter, uint32_t filter_bits,
                                                const uint8_t* __restrict__ expected, uint8_t* digests,
                                                uint32_t* bad) {
    constexpr int D = HBEC_MD5_DEPTH_LIST;
    const uint64_t c = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    FChain ch{0, 0};
    uint32_t e0 = 0, e1 = 0;
    uint64_t total = 0;
    bool examined = false;
    if (c < n_chains) {
        ch = chains[c];
        e0 = object_start[ch.object];
        e1 = object_start[ch.object + 1];
        examined = filter == nullptr;
        for (uint32_t e = e0; e < e1; ++e) {
            total += recs[e].len;
            if (filter && (filter[e] & filter_bits) != 0u) examined = true;
        }
    }
    if (__ballot(examined) == 0ull) return;  // nothing of this wave's objects is loaded
    if (!examined) {
        e0 = e1 = 0;
        total = 0;
    }
    const uint32_t shard = ch.shard;
    // integer addresses + address_space(1) loads, as md5_plan: no flat loads
    auto open = [&](FCursor& p) {  // on the first byte of shard `shard` of entry p.e
        const HRec* r = recs + p.e;
        const uint64_t len = r->len;
        p.left = len;
        p.addr = shard < k ? r->a + (uint64_t)shard * len : r->b + (uint64_t)(shard - k) * len;
    };
    auto settle = [&](FCursor& p) {  // on a byte, unless the chain is over
        while (p.left == 0 && p.e + 1 < e1) {
            ++p.e;
            open(p);
        }
    };
    FCursor lc{e0, 0, 0}, cc;
    if (examined) open(lc);  // e0 < e1: the host lists no chain of an object without a byte
    cc = lc;

    uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    const uint64_t nb = total / 64u;
    uint64_t nb_max = nb;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)nb_max, off, 64);
        nb_max = o > nb_max ? o : nb_max;
    }
    nb_max = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(nb_max >> 32)) << 32) |
             __builtin_amdgcn_readfirstlane((uint32_t)nb_max);

    // The next `count` bytes of the chain from p, bytewise across segments, as
    // a block: the pad byte after them when pad, zeros behind.  Words enter at
    // m[15] and move down, so every index is a constant.
    auto gather = [&](FCursor& p, uint32_t (&m)[16], uint32_t count, bool pad) {
#pragma unroll 1
        for (uint32_t w = 0; w < 16; ++w) {
            uint32_t x = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t q = 4 * w + j;
                uint32_t byte = 0;
                if (q < count) {
                    settle(p);
                    byte = *reinterpret_cast<fu8_c*>(p.addr);
                    p.addr += 1;
                    p.left -= 1;
                } else if (pad && q == count) {
                    byte = 0x80u;
                }
                x |= byte << (8 * j);
            }
#pragma unroll
            for (int i = 0; i < 15; ++i) m[i] = m[i + 1];
            m[15] = x;
        }
    };

    if (nb_max > 0) {
        const uint64_t zero = reinterpret_cast<uint64_t>(kFilesZeroBlock);
        const uint64_t groups = (nb_max + D - 1) / D;
        uint64_t lblk = 0;  // the block the next slot is loaded for: uniform
        auto load_group = [&](u32x4 (&dst)[D][4], uint32_t (&ext)[D]) {
#pragma unroll
            for (int j = 0; j < D; ++j, ++lblk) {
                settle(lc);
                const bool live = lblk < nb;
                const bool inside = live && lc.left >= 64u;
                const bool cut = live && !inside;
                uint64_t bp = zero;  // a straddling block, or past this lane's end
                uint32_t extra = 60u;
                if (inside) {
                    const uint32_t sh = (uint32_t)lc.addr & 3u;
                    bp = lc.addr - sh;
                    extra = sh ? 64u : 60u;  // shift 0: the block's last dword again
                    lc.addr += 64u;
                    lc.left -= 64u;
                }
                if (__ballot(cut) != 0ull) {
                    if (cut) {  // step over the 64 bytes the compress cursor will gather
                        uint32_t need = 64u;
                        while (need) {
                            settle(lc);
                            const uint32_t take = lc.left < need ? (uint32_t)lc.left : need;
                            lc.addr += take;
                            lc.left -= take;
                            need = take ? need - take : 0u;  // take 0 is not reached: a live block has its 64 bytes
                        }
                    }
                }
#pragma unroll
                for (int w = 0; w < 4; ++w) dst[j][w] = *reinterpret_cast<fu32x4_a4_c*>(bp + 16 * w);
                ext[j] = *reinterpret_cast<fu32_c*>(bp + extra);
            }
        };
        auto step = [&](const u32x4 (&q)[4], uint32_t e, uint64_t blk) {
            uint32_t d[17], m[16];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                d[4 * w + 0] = q[w].x;
                d[4 * w + 1] = q[w].y;
                d[4 * w + 2] = q[w].z;
                d[4 * w + 3] = q[w].w;
            }
            d[16] = e;
            settle(cc);
            const bool live = blk < nb;
            const bool cut = live && cc.left < 64u;
            const uint32_t sh = (uint32_t)cc.addr & 3u;  // this block's own shift
#pragma unroll
            for (int w = 0; w < 16; ++w) m[w] = __builtin_amdgcn_alignbyte(d[w + 1], d[w], sh);
            if (live && !cut) {
                cc.addr += 64u;
                cc.left -= 64u;
            }
            if (__ballot(cut) != 0ull) {
                if (cut) gather(cc, m, 64u, false);
            }
            uint32_t t[4] = {h[0], h[1], h[2], h[3]};
            md5_compress(t, m);
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = live ? t[i] : h[i];
        };
        u32x4 ga[D][4], gb[D][4];
        uint32_t ea[D], eb[D];
        load_group(ga, ea);
        for (uint64_t g = 0; g < groups; g += 2) {  // uniform: groups from the wave maximum
            load_group(gb, eb);
#pragma unroll
            for (int j = 0; j < D; ++j)
                if (g * D + j < nb_max) step(ga[j], ea[j], g * D + j);
            load_group(ga, ea);
#pragma unroll
            for (int j = 0; j < D; ++j)
                if ((g + 1) * D + j < nb_max) step(gb[j], eb[j], (g + 1) * D + j);
        }
    }
    if (!examined) return;
    // the compress cursor stands behind the last whole block
    const uint32_t rv = (uint32_t)(total - nb * 64u);
    uint32_t m[16] = {0};
    gather(cc, m, rv, true);
    if (rv >= 56) {
        md5_compress(h, m);
#pragma unroll
        for (int w = 0; w < 14; ++w) m[w] = 0;
    }
    const uint64_t bits = total * 8u;
    m[14] = (uint32_t)bits;
    m[15] = (uint32_t)(bits >> 32);
    md5_compress(h, m);
    const uint64_t slot = ((uint64_t)ch.object * n + ch.shard) * 16u;
    if (digests) {
        uint32_t* out = reinterpret_cast<uint32_t*>(digests + slot);
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = h[i];
    }
    if (expected) {
        const uint32_t* want = reinterpret_cast<const uint32_t*>(expected + slot);
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) diff |= want[i] ^ h[i];
        if (diff) atomicOr(bad + ch.object, 1u << ch.shard);
    }
}

__global__ __launch_bounds__(256) void hash_files_where(const HRec* __restrict__ recs, uint32_t n_src,
                                                        const uint32_t* __restrict__ object_of,
                                                        const uint32_t* __restrict__ sel,
                                                        const uint32_t* __restrict__ filter, uint32_t filter_bits,
                                                        const uint32_t* __restrict__ bad, uint32_t* where) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_src) return;
    const HRec r = recs[i];
    if (r.len == 0) return;
    uint32_t w = kLocSkipped;  // the other route, filtered or not
    if (r.route == (uint32_t)kVmKernel) {
        if (filter && !(filter[i] & filter_bits)) return;
        const uint32_t g = object_of[i];
        w = hash_where_word(sel[g], bad[g], r.route);
    }
    if (w) atomicOr(where + i, w);
}

hipError_t launch_md5_files(const HRec* recs, const uint32_t* object_start, const FChain* chains, uint64_t n_chains,
                            int k, int n, const uint32_t* filter, uint32_t filter_bits, const uint8_t* expected,
                            uint8_t* digests, uint32_t* bad, hipStream_t stream) {
    if (n_chains == 0) return hipSuccess;
    const dim3 grid((unsigned)((n_chains + 63) / 64));
    hipLaunchKernelGGL(md5_files, grid, dim3(64), 0, stream, recs, object_start, chains, n_chains, (uint32_t)k,
                       (uint32_t)n, filter, filter_bits, expected, digests, bad);
    return hipGetLastError();
}

hipError_t launch_hash_files_where(const HRec* recs, uint32_t n_src, const uint32_t* object_of, const uint32_t* sel,
                                   const uint32_t* filter, uint32_t filter_bits, const uint32_t* bad, uint32_t* where,
                                   hipStream_t stream) {
    if (n_src == 0) return hipSuccess;
    const dim3 grid((unsigned)(((uint64_t)n_src + 255) / 256));
    hipLaunchKernelGGL(hash_files_where, grid, dim3(256), 0, stream, recs, n_src, object_of, sel, filter, filter_bits,
                       bad, where);
    return hipGetLastError();
}

}  // namespace hbec
