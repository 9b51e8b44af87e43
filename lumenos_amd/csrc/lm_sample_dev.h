// The ChaCha20 keystream, the Gaussian table and the two small-coefficient rules of the deterministic samplers
// (lm_sample.hip), shared bit for bit with the CPU checker (oracle/lo_encdet.c):
//     keystream(I, s) = ChaCha20(key = seed, nonce = LE64(I) || LE32(s), counter = block)
#pragma once
#include "lm_arith.h"
#include "lm_common.h"

struct enc_seed_t {
    u32 k[8];
};
struct enc_cdt_t {
    u64 t[19];
};
static const u64 H_GAUSS_CDT[19] = {
    0x0ff52b40a5917f1dull, 0x2e5a25d4bf0e400eull, 0x489ae26955b04bd6ull, 0x5d2bc20f621bf185ull,
    0x6bc8694c3cc80ff4ull, 0x7532d89ac6ba7dceull, 0x7ab396cb74436798ull, 0x7d9e4e916643eb07ull,
    0x7f05495819eb2051ull, 0x7fa1ce9c0039a957ull, 0x7fdfb3f212e8c4e8ull, 0x7ff5e6f9d2314fccull,
    0x7ffd1f97bc4406a2ull, 0x7fff40fa0088d11dull, 0x7fffd2e835e1c57dull, 0x7ffff6524386ff1eull,
    0x7ffffe1db4769da5ull, 0x7fffffac0a1dcb08ull, 0x7ffffff428673853ull};

#define LM_QR(a, b, c, d)                    \
    a += b, d ^= a, d = (d << 16) | (d >> 16); \
    c += d, b ^= c, b = (b << 12) | (b >> 20); \
    a += b, d ^= a, d = (d << 8) | (d >> 24);  \
    c += d, b ^= c, b = (b << 7) | (b >> 25);

// RFC 8439 block function
__device__ __forceinline__ void chacha20_block(const enc_seed_t &key, u32 counter, u32 n0, u32 n1, u32 n2,
                                               u32 out[16]) {
    u32 s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.k[0], key.k[1], key.k[2], key.k[3],
                 key.k[4],    key.k[5],    key.k[6],    key.k[7],    counter,  n0,       n1,       n2};
    u32 x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = s[i];
#pragma unroll
    for (int r = 0; r < 10; r++) {
        LM_QR(x[0], x[4], x[8], x[12])
        LM_QR(x[1], x[5], x[9], x[13])
        LM_QR(x[2], x[6], x[10], x[14])
        LM_QR(x[3], x[7], x[11], x[15])
        LM_QR(x[0], x[5], x[10], x[15])
        LM_QR(x[1], x[6], x[11], x[12])
        LM_QR(x[2], x[7], x[8], x[13])
        LM_QR(x[3], x[4], x[9], x[14])
    }
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = x[i] + s[i];
}

// 16 ternary coefficients of one block: word w -> ((w * 3) >> 32) - 1
__device__ __forceinline__ uint4 lm_ternary16(const u32 w[16]) {
    union {
        int8_t b[16];
        uint4 v;
    } r;
#pragma unroll
    for (int i = 0; i < 16; i++) r.b[i] = (int8_t)((int)(((u64)w[i] * 3) >> 32) - 1);
    return r.v;
}
// 8 Gaussian coefficients of one block: x = w0 | w1 << 32, m = x >> 1, |e| = #{ i : m >= CDT[i] }, sign = x & 1
__device__ __forceinline__ uint2 lm_gauss8(const u32 w[16], const enc_cdt_t &cdt) {
    union {
        int8_t b[8];
        uint2 v;
    } r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 x = (u64)w[2 * i] | ((u64)w[2 * i + 1] << 32), m = x >> 1;
        int a = 0;
#pragma unroll
        for (int t = 0; t < 19; t++) a += m >= cdt.t[t];
        r.b[i] = (int8_t)((x & 1) ? -a : a);
    }
    return r.v;
}

// ---- uniform residues: streams 16 + m
#define LM_UNIFORM_STREAM 16u
struct kg_lim_t {
    u64 t[LM_MAX_LIMBS]; // 2^64 - (2^64 mod q_m): words below it are kept
};
// RUN consecutive coefficients from i0 (a multiple of RUN) of the limb whose stream is `stream`: RUN = 8 is one
// ChaCha20 block per attempt, RUN = 4 the half of it that i0 lies in.  Attempt t of coefficients 8 blk .. 8 blk + 7 is
// the words of block t * N/8 + blk; a coefficient keeps its first word below `bound`, reduced modulo q.
template <int RUN>
__device__ __forceinline__ void lm_uniform_run(const enc_seed_t &seed, u64 I, u32 stream, uint32_t logN, uint32_t i0, u64 q,
                                               u64 qinv64, u64 bound, u64 *r) {
    static_assert(RUN == 8 || RUN == 4, "a block of the keystream or half of one");
    const uint32_t N = 1u << logN, blk = i0 >> 3;
    const u32 upper = RUN == 4 && (i0 & 4) ? ~0u : 0u; // a mask, not a branch: the block's words stay in registers
    uint32_t pending = (1u << RUN) - 1;
    for (uint32_t t = 0; pending; t++) {
        u32 w[16];
        chacha20_block(seed, t * (N >> 3) + blk, (u32)I, (u32)(I >> 32), stream, w);
#pragma unroll
        for (int i = 0; i < RUN; i++) {
            u32 lo = w[2 * i], hi = w[2 * i + 1];
            if (RUN == 4) lo ^= (lo ^ w[8 + 2 * i]) & upper, hi ^= (hi ^ w[9 + 2 * i]) & upper;
            const u64 x = (u64)lo | ((u64)hi << 32);
            if (((pending >> i) & 1u) && x < bound) {
                r[i] = lm_reduce(x, q, qinv64);
                pending &= ~(1u << i);
            }
        }
    }
}
