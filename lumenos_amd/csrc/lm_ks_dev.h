// Device-side pieces of the hybrid key switch shared by the Galois (lm_keyswitch.hip, lm_ks_key.hip), the
// ring-switch (lm_ringswitch.hip) and the plaintext-product (lm_mulplain.hip) paths.
#pragma once
#include "lm_ntt_dev.h"

// constants of one basis extension (sources m_0..m_{ns-1} -> target t).
// The source-side factors y_a = x_a * (M/m_a)^-1 mod m_a do not depend on the target: they are
// produced once, fused into the N^-1 scaling of the INTT that brings the sources to the
// coefficient domain.  For a two-limb group k_pack_v then replaces (y_0, y_1) by the two words of the
// exact integer W = y_0*m_1 + y_1*m_0 + (2 - v)*M  (v: the reference's float64 correction term,
// 0 <= W < 4M < 2^118), split as W = hi * 2^57 + lo.  The extension to t is then ONE multiplication:
//     x mod t  ==  hi * (2^57 mod t) + lo + (t - 2M mod t)        (lazily, < 5t + 2^57)
struct bx_t {
    tw_t b57;     // 2^57 mod t (two-limb groups)
    u64 c_t;      // t - (2M mod t)
    uint32_t ns;  // 1: plain reduction, 2: reconstruction from (hi, lo)
    uint32_t own; // target limb belongs to the digit: no extension
};
#define LM_W_SPLIT 57

// lazy value congruent to the extension of the digit to modulus t
__device__ __forceinline__ u64 bx_apply(const bx_t &c, u64 a, u64 b, const lm_qc &qc) {
    if (c.ns == 1) return lm_shoup3<true>(a, 1ull, qc.qinv64, qc.nq); // x mod t, lazily
    return lm_shoup3<true>(a, c.b57.w, c.b57.wp, qc.nq, b + c.c_t);
}

// Layout of the key switch's three big streams, in limbs of N words: LIMB-MAJOR (round 6).  The gadget product walks
// ONE modulus t at a time over every (column, digit); with the modulus outermost everything one of its workgroups
// touches -- 4 columns x beta digits of `ext`, the 2 beta key limbs, its 8 output limbs -- sits in a few MB of
// contiguous addresses (a handful of 2 MB translations), and the chip as a whole streams one 48 MB region of `ext`
// and one 16 MB region of `u` at a time.  Rounds 1-5 kept the column outermost ([b][d][t], [b][w][t], [d][w][t]:
// 36 + 8 blocks 1.75 MB apart per workgroup): the gadget product took 5-8 % longer and the extension kernel, which
// writes `ext`, 3.7 % (profiles/r06_exp_ks_layout.txt; same residues).
// limb t of digit d of column b in the extended-digit buffer: [L+K][B][beta]
__host__ __device__ __forceinline__ size_t ks_ext_at(uint32_t b, uint32_t d, uint32_t t, uint32_t B, uint32_t beta) {
    return ((size_t)t * B + b) * beta + d;
}
// limb t of polynomial pw = 2 b + w of the gadget product's output u: the Q limbs [L][2B], behind them the limbs
// modulo P as [2B][K] -- the K limbs of one polynomial stay adjacent (their inverse transform, the packing pass and
// ModDown's lift read them as a pair)
__host__ __device__ __forceinline__ size_t ks_u_at(uint32_t pw, uint32_t t, uint32_t B, uint32_t L, uint32_t K) {
    return t < L ? (size_t)t * 2 * B + pw : (size_t)L * 2 * B + (size_t)pw * K + (t - L);
}
// limb t of polynomial w of digit d of a switching key as the gadget product reads it: [L+K][beta][2]
// (lumen_load_galois_key takes the caller's [beta][2][L+K] and k_key_prepare permutes)
__host__ __device__ __forceinline__ size_t ks_key_at(uint32_t d, uint32_t w, uint32_t t, uint32_t beta) {
    return ((size_t)t * beta + d) * 2 + w;
}

// The key switch at a level of nl <= L limbs works on nl + K POSITIONS: the level's Q limbs, then the K limbs modulo P.
// The context's tables (moduli, twiddles, inverse-transform scales, key limbs) hold the limbs modulo P behind ALL L
// Q limbs, so position t is modulus t for t < nl and t + (L - nl) behind them; pshift = L - nl is 0 at the top level,
// where the map is the identity.
__host__ __device__ __forceinline__ uint32_t ks_mod_at(uint32_t t, uint32_t nl, uint32_t pshift) {
    return t < nl ? t : t + pshift;
}

// 64 x 64 -> 128-bit product as four 32x32+64 multiply-adds (the compiler's __int128 multiply goes
// through v_mul_lo/hi_u32, twice as slow each)
__device__ __forceinline__ void mul128(u64 a, u64 b, u64 &lo, u64 &hi) {
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), b0 = (u32)b, b1 = (u32)(b >> 32);
    const u64 p0 = (u64)a0 * b0;
    const u64 p1 = lm_keep((u64)a0 * b1 + (p0 >> 32));
    const u64 p2 = lm_keep((u64)a1 * b0 + (u32)p1);
    hi = (u64)a1 * b1 + (p1 >> 32) + (p2 >> 32);
    lo = (p2 << 32) | (u32)p0;
}

// host-side view of the per-context key-switch tables (owned by lm_keyswitch.hip)
struct lm_ks_view {
    const bx_t *d_bxp;      // [L]: lift of the P limbs into q_t
    const tw_t *d_pinv;     // [L]: P^-1 mod q_t
    const lm_ninv_t *yscale; // per modulus: N^-1 * (M/m)^-1 of its source group
};
int lm_ks_tables_view(lumen_ctx *ctx, lm_ks_view *out);
// (y0, y1) -> (hi, lo) of the exact reconstruction for every two-limb source group (see k_pack_v)
int lm_launch_pack_v(lumen_ctx *ctx, u64 *y, size_t poly_stride, uint32_t npoly, uint32_t ngroups,
                     uint32_t group_limbs, uint32_t first_mod, uint32_t nlimbs_total);
