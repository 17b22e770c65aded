// hashfiles_kernel.inc — the text of md5_files (hashfiles.hip), included once per
// kernel: HBEC_MD5_FILES_KERNEL names it, and with HBEC_MD5_FILES_ROWS the records
// are a shards plan's, whose `a` is the address of the entry's row of 64-bit shard
// addresses (shardplan.h), read again at every segment a lane opens.  Two kernels
// from one text, as hashplan_kernel.inc and for its reason: md5_files compiles to
// the instructions it had.
__global__ __launch_bounds__(64) void HBEC_MD5_FILES_KERNEL(const HRec* __restrict__ recs,
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
#if HBEC_MD5_FILES_ROWS
        // the lane's own shard of the entry's row; a zero-length entry has no row (a = 0)
        p.addr = len ? reinterpret_cast<fu64_c*>(r->a)[shard] : 0u;
#else
        p.addr = shard < k ? r->a + (uint64_t)shard * len : r->b + (uint64_t)(shard - k) * len;
#endif
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
