// Device helpers of the lazy inner products over F_T (lm_polyeval.hip: P(z); lm_verify.hip: the verifier's two checks):
// one workgroup per column, products summed in 128 bits, one Montgomery reduction per group of products.
#pragma once
#include "lm_common.h"

constexpr uint32_t PE_THREADS = 256;
constexpr uint32_t PE_UNROLL = 4; // 16-byte loads in flight per thread and iteration
// products summed in 128 bits before one reduction: 8 * 2^64 * T < 2^128 and lm_mont_reduce_wide's 8 * T < 2^63
constexpr uint64_t PE_MAX_T = 1ull << 60;

__device__ __forceinline__ u64 pe_mont_mul(u64 a, u64 b, const mod_t &m) {
    const u128 p = (u128)a * b;
    return lm_mont_reduce((u64)p, (u64)(p >> 64), m.q, m.qneg);
}

// sum of a workgroup's values mod q; the result is valid in thread 0.  A kernel that sums twice puts a
// __syncthreads() between the two calls (they share the staging words).
__device__ __forceinline__ u64 pe_block_sum(u64 acc, const mod_t &m) {
    __shared__ u64 wsum[PE_THREADS / 64];
    for (int off = 32; off; off >>= 1) acc = lm_addmod(acc, __shfl_xor(acc, off), m.q);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t k = 1; k < PE_THREADS / 64; k++) acc = lm_addmod(acc, wsum[k], m.q);
    return acc;
}

// out[i] = base^(e0 + i) * 2^64 mod T for i < n, on the context's stream (k_poly_pow_table, lm_polyeval.hip);
// baseM = base * 2^64 mod T
int lm_poly_pow_table(lumen_ctx *ctx, u64 *out, uint32_t n, uint64_t baseM, uint64_t e0);
