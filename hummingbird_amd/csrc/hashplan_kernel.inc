// hashplan_kernel.inc — the text of md5_plan (hashplan.hip), included once per
// kernel: HBEC_MD5_PLAN_KERNEL names it, and with HBEC_MD5_PLAN_ROWS the records
// are a shards plan's, whose `a` is the address of the entry's row of 64-bit shard
// addresses (shardplan.h).  Two kernels from one text, and not one function
// called by both: with the body in a function md5_plan itself went from 92 to 96
// VGPRs, and its figures are pinned.
__global__ __launch_bounds__(64) void HBEC_MD5_PLAN_KERNEL(const HRec* __restrict__ recs, const HChain* __restrict__ chains,
                                               uint64_t n_chains, uint32_t k, uint32_t n,
                                               const uint32_t* __restrict__ filter, uint32_t filter_bits,
                                               const uint8_t* __restrict__ expected, uint8_t* digests,
                                               uint32_t* bad) {
    constexpr int D = HBEC_MD5_DEPTH_LIST;
    const uint64_t c = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    HChain ch{0, 0};
    bool examined = c < n_chains;
    if (examined) {
        ch = chains[c];
        if (filter) examined = (filter[ch.entry] & filter_bits) != 0u;
    }
    if (__ballot(examined) == 0ull) return;  // nothing of this wave's entries is loaded
    uint64_t addr = 0, len = 0;
    if (examined) {
        const HRec r = recs[ch.entry];
        len = r.len;
#if HBEC_MD5_PLAN_ROWS
        // the lane's own shard of the entry's row; a zero-length entry has no row (a = 0)
        addr = len ? reinterpret_cast<gu64_c*>(r.a)[ch.shard] : 0u;
#else
        addr = ch.shard < k ? r.a + (uint64_t)ch.shard * len : r.b + (uint64_t)(ch.shard - k) * len;
#endif
    }
    uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    const uint64_t nb = len / 64u;
    uint64_t nb_max = nb;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((long long)nb_max, off, 64);
        nb_max = o > nb_max ? o : nb_max;
    }
    nb_max = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(nb_max >> 32)) << 32) |
             __builtin_amdgcn_readfirstlane((uint32_t)nb_max);
    // integer addresses + address_space(1) loads, as md5_list: no flat loads
    constexpr bool kBytes = HBEC_HASH_PLAN_BYTE_LOADER != 0;  // the A/B partner: md5_list's byte loader
    const uint32_t sh = nb > 0 && !kBytes ? (uint32_t)addr & 3u : 0u;
    const uint64_t base = nb > 0 ? addr - sh : reinterpret_cast<uint64_t>(kHashZeroBlock);
    const uint64_t last = nb > 0 ? nb - 1 : 0;
    const uint32_t extra = sh ? 64u : 60u;  // shift 0: the block's last dword again
    if (nb_max > 0) {
        const uint64_t groups = (nb_max + D - 1) / D;
        auto load_group = [&](u32x4 (&dst)[D][4], uint32_t (&ext)[D], uint64_t g) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                uint64_t blk = g * D + j;
                blk = blk < last ? blk : last;  // clamp to this lane's chain
                const uint64_t bp = base + 64u * blk;
                if (kBytes) {
                    typedef __attribute__((address_space(1))) const uint8_t gu8_c;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        uint32_t e[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            gu8_c* q = reinterpret_cast<gu8_c*>(bp + 16 * w + 4 * i);
                            e[i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) |
                                   ((uint32_t)q[3] << 24);
                        }
                        dst[j][w] = u32x4{e[0], e[1], e[2], e[3]};
                    }
                    ext[j] = 0u;
                    continue;
                }
#pragma unroll
                for (int w = 0; w < 4; ++w) dst[j][w] = *reinterpret_cast<gu32x4_a4_c*>(bp + 16 * w);
                ext[j] = *reinterpret_cast<gu32_c*>(bp + extra);
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
#pragma unroll
            for (int w = 0; w < 16; ++w) m[w] = __builtin_amdgcn_alignbyte(d[w + 1], d[w], sh);
            uint32_t t[4] = {h[0], h[1], h[2], h[3]};
            md5_compress(t, m);
            const bool keep = blk < nb;
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = keep ? t[i] : h[i];
        };
        u32x4 ga[D][4], gb[D][4];
        uint32_t ea[D], eb[D];
        load_group(ga, ea, 0);
        for (uint64_t g = 0; g < groups; g += 2) {  // uniform: groups from the wave maximum
            load_group(gb, eb, g + 1 < groups ? g + 1 : g);
#pragma unroll
            for (int j = 0; j < D; ++j)
                if (g * D + j < nb_max) step(ga[j], ea[j], g * D + j);
            load_group(ga, ea, g + 2 < groups ? g + 2 : groups - 1);
#pragma unroll
            for (int j = 0; j < D; ++j)
                if ((g + 1) * D + j < nb_max) step(gb[j], eb[j], (g + 1) * D + j);
        }
    }
    if (!examined) return;
    const uint32_t rv = (uint32_t)(len - nb * 64u);
    const Pending pend{nullptr, reinterpret_cast<const uint8_t*>(addr), 0};
    uint32_t m[16];
    assemble(m, pend, nb * 64u, rv, true);
    if (rv >= 56) {
        md5_compress(h, m);
#pragma unroll
        for (int w = 0; w < 14; ++w) m[w] = 0;
    }
    const uint64_t bits = len * 8u;
    m[14] = (uint32_t)bits;
    m[15] = (uint32_t)(bits >> 32);
    md5_compress(h, m);
    const uint64_t slot = ((uint64_t)ch.entry * n + ch.shard) * 16u;
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
        if (diff) atomicOr(bad + ch.entry, 1u << ch.shard);
    }
}
