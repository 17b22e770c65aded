// etag_kernel.inc — the text of md5_etag (etag.hip), included once per kernel:
// HBEC_ETAG_KERNEL names it, and with HBEC_ETAG_ROWS the records are a shards
// plan's, whose `a` is the address of the entry's row of 64-bit shard addresses
// (shardplan.h), read for every shard a lane opens as a segment.  The schedule
// is md5_files' (hashfiles_kernel.inc); the segment walk is etag.h's.
__global__ __launch_bounds__(64) void HBEC_ETAG_KERNEL(const HRec* __restrict__ recs,
                                                       const ERec* __restrict__ erecs,
                                                       const EChain* __restrict__ chains, uint64_t n_chains,
                                                       uint32_t k, const uint32_t* __restrict__ filter,
                                                       uint32_t filter_bits, const uint8_t* __restrict__ expected,
                                                       uint8_t* digests, uint32_t* bad) {
    constexpr int D = HBEC_MD5_DEPTH_LIST;
    const uint64_t c = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    EChain ch{0, 0, 0, 0, 0};
    bool examined = false;
    if (c < n_chains) {
        ch = chains[c];
        examined = filter == nullptr;
        for (uint32_t e = ch.e0; filter && e < ch.e1; ++e)
            if ((filter[e] & filter_bits) != 0u) examined = true;
    }
    if (__ballot(examined) == 0ull) return;  // nothing of this wave's objects is loaded
    const uint32_t e1 = examined ? ch.e1 : 0u;
    const uint64_t total = examined ? ch.total : 0u;
    // integer addresses + address_space(1) loads, as md5_plan: no flat loads
    auto settle = [&](ECursor& p) {  // on a byte, unless the chain is over
        while (p.left == 0 && p.e < e1) {
            const HRec* r = recs + p.e;
            const ERec er = erecs[p.e];
            const uint64_t S = r->len;
            ESeg s;
#if HBEC_ETAG_ROWS
            const uint64_t row = r->a;  // read only where the entry has a byte: then it has a row
            const bool open = etag_segment_rows(
                [row](uint32_t j) { return reinterpret_cast<eu64_c*>(row)[j]; }, S, er, p.j, &s);
#else
            const bool open = etag_segment_slot(r->a, S, er, p.j, k, &s);
#endif
            if (open) {
                p.addr = s.addr;
                p.left = s.left;
                p.j = s.next;
            } else {  // the entry is over, or has no byte in the chain
                ++p.e;
                p.j = 0;
            }
        }
    };
    ECursor lc{examined ? ch.e0 : 0u, 0, 0, 0}, cc;
    settle(lc);
    cc = lc;

    uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    const uint64_t nb = etag_blocks(total);
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
    auto gather = [&](ECursor& p, uint32_t (&m)[16], uint32_t count, bool pad) {
#pragma unroll 1
        for (uint32_t w = 0; w < 16; ++w) {
            uint32_t x = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t q = 4 * w + j;
                uint32_t byte = 0;
                if (q < count) {
                    settle(p);
                    byte = *reinterpret_cast<eu8_c*>(p.addr);
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
        const uint64_t zero = reinterpret_cast<uint64_t>(kEtagZeroBlock);
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
                for (int w = 0; w < 4; ++w) dst[j][w] = *reinterpret_cast<eu32x4_a4_c*>(bp + 16 * w);
                ext[j] = *reinterpret_cast<eu32_c*>(bp + extra);
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
    const uint32_t rv = etag_tail(total);
    uint32_t m[16] = {0};
    gather(cc, m, rv, true);
    if (etag_pad_blocks(total) == 2u) {
        md5_compress(h, m);
#pragma unroll
        for (int w = 0; w < 14; ++w) m[w] = 0;
    }
    const uint64_t bits = etag_bits(total);
    m[14] = (uint32_t)bits;
    m[15] = (uint32_t)(bits >> 32);
    md5_compress(h, m);
    const uint64_t slot = (uint64_t)ch.slot * 16u;
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
        if (diff) atomicOr(bad + ch.slot, 1u);
    }
}
