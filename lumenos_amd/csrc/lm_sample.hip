// The deterministic samplers of the client side: the small polynomials (ternary u and s, Gaussian e) and the uniform
// masks of the public-key encryptor (lm_encrypt.hip), the secret-key encryptor (lm_encrypt_sk.hip) and key generation
// (lm_keygen.hip).  One definition, shared bit for bit with the CPU checkers (oracle/lo_encdet.c, tests/keygen_model.py,
// tests/encrypt_sk_model.py):
//     keystream(I, s) = ChaCha20(key = seed, nonce = LE64(I) || LE32(s), counter = 0, 1, ...)      (lm_sample_dev.h)
//     stream 0         ternary: word k -> coefficient k = ((w * 3) >> 32) - 1                       (lm_ternary16)
//     streams 1 ..     Gaussian: words 2k, 2k+1 -> coefficient k by the CDT rule                    (lm_gauss8)
//     streams 16 + m   uniform mod q_m: little-endian 64-bit words; attempt t = 0, 1, ... for coefficient k is word
//                      number t * N + k, the first x < 2^64 - (2^64 mod q_m) is kept and a[k] = x mod q_m
// Who draws what: the public-key encryptor streams 0-2 of a ciphertext's index, the secret-key encryptor stream 3 and
// the masks, key generation stream 0 (secrets), stream 1 (errors) and the masks of its own indices.
//
// The sample index of item i is index[i] where a table is given (key generation: several keys in one launch are not
// one run) and base + i otherwise, in 64 bits; its high word is the nonce's second word.
#include <cstring>

#include "lm_enc_host.h"
#include "lm_sample_dev.h"

// out: [nitems][ns][N] int8, streams s0 .. s0 + ns - 1 of every item.  One thread per ChaCha20 block: per item the N/16
// blocks of stream 0 (when s0 = 0), then the N/8 blocks of each Gaussian stream.
__global__ __launch_bounds__(256) void k_sample_small(int8_t *__restrict__ out, const u64 *__restrict__ index, u64 base,
                                                      uint32_t nitems, uint32_t s0, uint32_t ns, uint32_t logN,
                                                      enc_seed_t seed, enc_cdt_t cdt) {
    const uint32_t N = 1u << logN, nt = s0 ? 0 : N >> 4, per = nt + (ns - (s0 ? 0 : 1)) * (N >> 3);
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (size_t)nitems * per) return;
    const uint32_t it = (uint32_t)(g / per), j = (uint32_t)(g % per);
    uint32_t stream = 0, blk = j;
    if (j >= nt) stream = (s0 ? s0 : 1) + ((j - nt) >> (logN - 3)), blk = (j - nt) & ((N >> 3) - 1);
    const u64 I = index ? index[it] : base + it;
    u32 w[16];
    chacha20_block(seed, blk, (u32)I, (u32)(I >> 32), stream, w);
    int8_t *o = out + ((size_t)it * ns + (stream - s0)) * N;
    if (stream == 0)
        *reinterpret_cast<uint4 *>(o + (size_t)blk * 16) = lm_ternary16(w);
    else
        *reinterpret_cast<uint2 *>(o + (size_t)blk * 8) = lm_gauss8(w, cdt);
}

// The `a` half of every entry: a is the first of them, [LK][N] per item and item_stride words from one item to the next
// (a key's [nitems][b|a][LK][N]: out + LK * N, 2 * LK * N apart; the secret-key encryptor's c1 halves alike, or a plain
// [nitems][L][N] block).  blockIdx.y = item * LK + limb, one thread per block of 8 coefficients.  Attempt t of
// coefficients 8 blk .. 8 blk + 7 is words of block t * N/8 + blk.
__global__ __launch_bounds__(256) void k_sample_uniform(u64 *__restrict__ a, size_t item_stride, const u64 *__restrict__ index,
                                                        u64 base, uint32_t LK, uint32_t logN, lm_mods mods, kg_lim_t lim,
                                                        enc_seed_t seed) {
    const uint32_t N = 1u << logN, blk = blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= (N >> 3)) return;
    const uint32_t it = blockIdx.y / LK, m = blockIdx.y % LK;
    const u64 I = index ? index[it] : base + it, q = mods.m[m].q, qinv64 = mods.m[m].qinv64, bound = lim.t[m];
    u64 r[8];
    lm_uniform_run<8>(seed, I, LM_UNIFORM_STREAM + m, logN, blk * 8, q, qinv64, bound, r);
    lm_store_run(a + (size_t)it * item_stride + (size_t)m * N, blk * 8, r, 8);
}

enc_seed_t lm_sample_seed(const uint8_t seed[32]) {
    enc_seed_t k;
    memcpy(k.k, seed, 32); // little-endian words, as RFC 8439 reads the key
    return k;
}
static enc_cdt_t sample_cdt() {
    enc_cdt_t c;
    memcpy(c.t, H_GAUSS_CDT, sizeof(c.t));
    return c;
}
kg_lim_t lm_sample_lim(const lumen_ctx *ctx, uint32_t LK) {
    kg_lim_t lim;
    for (uint32_t t = 0; t < LM_MAX_LIMBS; t++) lim.t[t] = 0 - h_r64_mod(ctx->mod[t < LK ? t : 0]);
    return lim;
}

int lm_sample_small(lumen_ctx *ctx, int8_t *out, const u64 *d_index, u64 base, uint32_t nitems, uint32_t s0, uint32_t ns,
                    const uint8_t seed[32]) {
    const size_t per = (size_t)(ctx->N >> 4) * (2 * ns - (s0 ? 0 : 1));
    return lm_launch_flat(ctx, k_sample_small, nitems * per, out, d_index, base, nitems, s0, ns, ctx->logN, lm_sample_seed(seed),
                          sample_cdt());
}

int lm_sample_uniform(lumen_ctx *ctx, u64 *a, size_t item_stride, const u64 *d_index, u64 base, uint32_t nitems,
                      uint32_t LK, const uint8_t seed[32]) {
    const uint32_t nb = ctx->N >> 3, bs = nb < 256 ? nb : 256;
    hipLaunchKernelGGL(k_sample_uniform, dim3(nb / bs, nitems * LK), dim3(bs), 0, ctx->stream, a, item_stride, d_index, base, LK,
                       ctx->logN, ctx->mods, lm_sample_lim(ctx, LK), lm_sample_seed(seed));
    LM_HIP(ctx, hipGetLastError());
    return 0;
}
