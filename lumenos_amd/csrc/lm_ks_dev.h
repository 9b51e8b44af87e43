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

// ---- the c0 fold of matrixInnerSumEval's doublings (k_ks_mac_fold, k_lift_fold, k_ks_close): the lifts of polynomial 0
// are summed per coefficient as ONE signed integer S, whatever the Q limb, in three 64-bit words, two's complement.
struct lm_s192 {
    u64 a, b, c; // weights 1, 2^64, 2^128
};
__host__ __device__ __forceinline__ lm_s192 lm_s192_add(const lm_s192 &x, const lm_s192 &y) {
    lm_s192 r;
    r.a = x.a + y.a;
    const u64 c0 = r.a < x.a ? 1u : 0u;
    r.b = x.b + y.b;
    u64 c1 = r.b < x.b ? 1u : 0u;
    r.b += c0;
    c1 += r.b < c0 ? 1u : 0u; // (at most one of the two additions of the middle word wraps)
    r.c = x.c + y.c + c1;
    return r;
}
__host__ __device__ __forceinline__ lm_s192 lm_s192_neg(const lm_s192 &x) {
    return lm_s192_add(lm_s192{~x.a, ~x.b, ~x.c}, lm_s192{1, 0, 0});
}
// S mod q_t at the close: with s2' = (top word) xor 2^63 the integer is s0 + s1 2^64 + (s2' - 2^63) 2^128, every term
// unsigned, so S == s0 + s1 r64 + s2' r128 + off (mod q), off = q - (2^63 r128 mod q): the sign is a multiple of q away
struct sfold_t {
    tw_t r64, r128; // 2^64 mod q_t, 2^128 mod q_t
    u64 off, pad;
};
// lazily, below 10q < 2^64 (q < 2^60)
__device__ __forceinline__ u64 lm_s192_mod(const sfold_t &f, u64 s0, u64 s1, u64 s2, const lm_qc &qc) {
    const u64 r0 = lm_shoup3<true>(s0, 1ull, qc.qinv64, qc.nq);
    const u64 r1 = lm_shoup3<true>(s1, f.r64.w, f.r64.wp, qc.nq);
    const u64 r2 = lm_shoup3<true>(s2 ^ (1ull << 63), f.r128.w, f.r128.wp, qc.nq);
    return r0 + r1 + r2 + f.off;
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
