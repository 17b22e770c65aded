// md5_device.h — the MD5 (RFC 1321) block compression and the bytewise block
// assembly shared by the hash kernels (md5.hip: md5_chains, md5_list;
// hashplan.hip: md5_plan).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.h"

namespace hbec {

__device__ constexpr uint32_t kMd5K[64] = {
    0xd76aa478, 0xe8c7b756, 0x242070db, 0xc1bdceee, 0xf57c0faf, 0x4787c62a, 0xa8304613, 0xfd469501,
    0x698098d8, 0x8b44f7af, 0xffff5bb1, 0x895cd7be, 0x6b901122, 0xfd987193, 0xa679438e, 0x49b40821,
    0xf61e2562, 0xc040b340, 0x265e5a51, 0xe9b6c7aa, 0xd62f105d, 0x02441453, 0xd8a1e681, 0xe7d3fbc8,
    0x21e1cde6, 0xc33707d6, 0xf4d50d87, 0x455a14ed, 0xa9e3e905, 0xfcefa3f8, 0x676f02d9, 0x8d2a4c8a,
    0xfffa3942, 0x8771f681, 0x6d9d6122, 0xfde5380c, 0xa4beea44, 0x4bdecfa9, 0xf6bb4b60, 0xbebfbc70,
    0x289b7ec6, 0xeaa127fa, 0xd4ef3085, 0x04881d05, 0xd9d4d039, 0xe6db99e5, 0x1fa27cf8, 0xc4ac5665,
    0xf4292244, 0x432aff97, 0xab9423a7, 0xfc93a039, 0x655b59c3, 0x8f0ccc92, 0xffeff47d, 0x85845dd1,
    0x6fa87e4f, 0xfe2ce6e0, 0xa3014314, 0x4e0811a1, 0xf7537e82, 0xbd3af235, 0x2ad7d2bb, 0xeb86d391};

__device__ constexpr int md5_shift(int i) {
    constexpr int s[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
    return s[(i >> 4) * 4 + (i & 3)];
}

__device__ constexpr int md5_word(int i) {
    return i < 16 ? i : i < 32 ? (5 * i + 1) & 15 : i < 48 ? (3 * i + 5) & 15 : (7 * i) & 15;
}

__device__ __forceinline__ uint32_t rotl(uint32_t x, int s) { return __builtin_amdgcn_alignbit(x, x, 32 - s); }

// One 64-byte block.  Plain C logic: the compiler maps F/G and I to
// v_bitop3_b32 (gfx950) and a + f + (m + K) to v_add3_u32; H is written as an
// explicit XOR3 (the compiler emitted two v_xor_b32 for b ^ c ^ d).
__device__ __forceinline__ void md5_compress(uint32_t (&h)[4], const uint32_t (&m)[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        uint32_t f;
        if (i < 16)
            f = d ^ (b & (c ^ d));
        else if (i < 32)
            f = c ^ (d & (b ^ c));
        else if (i < 48)
            f = xor3(b, c, d);  // one v_bitop3 (plain C became two v_xor_b32)
        else
            f = c ^ (b | ~d);
        const uint32_t t = a + f + (m[md5_word(i)] + kMd5K[i]);
        a = d;
        d = c;
        c = b;
        b = b + rotl(t, md5_shift(i));
    }
    h[0] += a;
    h[1] += b;
    h[2] += c;
    h[3] += d;
}

__device__ __forceinline__ void md5_compress4(uint32_t (&h)[4], const u32x4 (&q)[4]) {
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[4 * j + 0] = q[j].x;
        m[4 * j + 1] = q[j].y;
        m[4 * j + 2] = q[j].z;
        m[4 * j + 3] = q[j].w;
    }
    md5_compress(h, m);
}

// Byte q (< carry + len) of the pending stream = carried tail ++ this call's data.
struct Pending {
    const uint8_t* tail;  // carried bytes (state), may be null when carry == 0
    const uint8_t* data;
    uint32_t carry;
    __device__ __forceinline__ uint32_t at(uint64_t q) const { return q < carry ? tail[q] : data[q - carry]; }
};

// Block of 16 words from pending bytes [off, off + n) followed by the MD5 pad
// byte 0x80 at n (when pad) and zeros; bit length in words 14-15 when len_words.
__device__ __forceinline__ void assemble(uint32_t (&m)[16], const Pending& p, uint64_t off, uint32_t n, bool pad) {
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        uint32_t x = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t q = 4 * w + j;
            const uint32_t byte = q < n ? p.at(off + q) : (pad && q == n ? 0x80u : 0u);
            x |= byte << (8 * j);
        }
        m[w] = x;
    }
}

}  // namespace hbec
