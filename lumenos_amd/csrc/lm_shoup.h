// The hand-scheduled Shoup multiplication of gfx950 and what the lazy butterflies build on it (structure: lm_ntt_dev.h).
#pragma once
#include "lm_common.h"

// ---- Shoup multiplication as a chain of 32x32+64 multiply-adds (v_mad_u64_u32: 4.9 cycles per
// wave-op on MI355X against 8-10 for v_mul_lo/hi_u32, profiles/r01_ubench_int_valu.txt).
// Written in plain C so the scheduler can interleave independent butterflies and place
// wave-uniform operands (twiddles of uniform stages, the modulus) in SGPRs; lm_keep() is an empty
// asm that marks all 64 bits of a partial sum as used, which stops the compiler from narrowing the
// low-word products back to the slower v_mul_lo_u32.
__device__ __forceinline__ u64 lm_keep(u64 x) {
    asm("" : "+v"(x));
    return x;
}

// a*w mod q, lazily, for ANY a < 2^64: result in [0, 3q).  nq = 2^64 - q (wave-uniform).
// t ~ floor(a*wp / 2^64) from three partial products (the a0*wp0 term and its
// carry are dropped: t is exact or one short), then r = a*w + t*nq mod 2^64.
// UW documents that the twiddle (w, wp) is wave-uniform (it then lives in SGPRs).
// x is an optional addend: the result is x + a*w (lazily reduced a*w) mod 2^64, for free, because
// the first multiply-add of the low chain has an empty addend slot.
//
// The compiler's rendering of this chain costs ~19 instructions: every time the HIGH word of one
// product feeds the next multiply-add it copies that word into a zero-extended, 64-bit-aligned
// register pair (gfx950 only takes even-aligned VGPR tuples) and then adds pairs.  LM_ASM_SHOUP
// writes the chain by hand on eight fixed temporaries: 10 multiply-adds and 2 adds.
//   * "x += zext(hi word)" is itself a multiply-add by the inline constant 1 (the word is read as a
//     32-bit source, so its alignment does not matter);
//   * S = a1*p0 + m1 is a 65-bit sum: its carry-out (an SGPR pair) is added to the upper word of t;
//   * the upper result word only matters mod 2^32, so it is accumulated apart (4 multiply-adds),
//     added into the upper word of lo' = a0*w0 + x, and the last multiply-add t0*n0 + {lo', upper}
//     writes the result.
// gfx950 needs two wait states between a VALU write of an SGPR (the carry) and a VALU read of it:
// three independent instructions sit in between.
#ifndef LM_ASM_SHOUP
#define LM_ASM_SHOUP 1
#endif
// the eight temporaries: v[80:87]
#define LM_T(i) LM_T##i
#define LM_T0 "80"
#define LM_T1 "81"
#define LM_T2 "82"
#define LM_T3 "83"
#define LM_T4 "84"
#define LM_T5 "85"
#define LM_T6 "86"
#define LM_T7 "87"
#define LM_V(i) "v" LM_T(i)
#define LM_VP(i, j) "v[" LM_T(i) ":" LM_T(j) "]"
#define LM_SHOUP_CLOBBERS LM_V(0), LM_V(1), LM_V(2), LM_V(3), LM_V(4), LM_V(5), LM_V(6), LM_V(7), "s96", "s97", "s98", "s99"
// v[0:1]: m1, later `up`;  v[2:3]: S;  v[4:5]: t;  v[6:7]: lo'
#define LM_SHOUP_BODY(ADDEND)                                                                                   \
    "v_mad_u64_u32 " LM_VP(0, 1) ", s[96:97], %[a0], %[p1], 0\n\t"                 /* m1 = a0*p1           */ \
    "v_mad_u64_u32 " LM_VP(2, 3) ", s[98:99], %[a1], %[p0], " LM_VP(0, 1) "\n\t"   /* S, carry -> s[98:99] */ \
    "v_mad_u64_u32 " LM_VP(4, 5) ", s[96:97], %[a1], %[p1], 0\n\t"                 /* t = a1*p1            */ \
    "v_mad_u64_u32 " LM_VP(6, 7) ", s[96:97], %[a0], %[w0], " ADDEND "\n\t"        /* lo' = a0*w0 + x      */ \
    "v_mad_u64_u32 " LM_VP(4, 5) ", s[96:97], " LM_V(3) ", 1, " LM_VP(4, 5) "\n\t" /* t += hi(S)           */ \
    "v_mad_u64_u32 " LM_VP(0, 1) ", s[96:97], %[a0], %[w1], 0\n\t"                 /* up = a0*w1           */ \
    "v_addc_co_u32_e64 " LM_V(5) ", s[96:97], " LM_V(5) ", 0, s[98:99]\n\t"        /* t += carry << 32     */ \
    "v_mad_u64_u32 " LM_VP(0, 1) ", s[96:97], %[a1], %[w0], " LM_VP(0, 1) "\n\t"   /* up += a1*w0          */ \
    "v_mad_u64_u32 " LM_VP(0, 1) ", s[96:97], " LM_V(4) ", %[n1], " LM_VP(0, 1) "\n\t" /* up += t0*n1      */ \
    "v_mad_u64_u32 " LM_VP(0, 1) ", s[96:97], " LM_V(5) ", %[n0], " LM_VP(0, 1) "\n\t" /* up += t1*n0      */ \
    "v_add_u32 " LM_V(7) ", " LM_V(7) ", " LM_V(0) "\n\t"                          /* hi(lo') += up        */ \
    "v_mad_u64_u32 %[o], s[96:97], " LM_V(4) ", %[n0], " LM_VP(6, 7)                /* {lo', upper} + t0*n0 */

// compiler-scheduled form of the same chain (no pinned registers): for kernels whose occupancy must
// not be tied to the v[80:89] temporaries of the hand-scheduled one
__device__ __forceinline__ u64 lm_shoup3_c(u64 a, u64 w, u64 wp, u64 nq, u64 x = 0) {
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), p0 = (u32)wp, p1 = (u32)(wp >> 32);
    const u32 w0 = (u32)w, w1 = (u32)(w >> 32), n0 = (u32)nq, n1 = (u32)(nq >> 32);
    const u64 m1 = (u64)a0 * p1;
    const u64 m2 = lm_keep((u64)a1 * p0 + (u32)m1);
    const u64 t = (u64)a1 * p1 + (m1 >> 32) + (m2 >> 32);
    const u32 t0 = (u32)t, t1 = (u32)(t >> 32);
    // everything below is arithmetic mod 2^64: partial sums may wrap
    const u64 lo = lm_keep((u64)a0 * w0 + x) + (u64)t0 * n0;
    u64 acc = (u64)a0 * w1 + (lo >> 32);
    acc += (u64)a1 * w0;
    acc += (u64)t0 * n1;
    acc += (u64)t1 * n0;
    acc = lm_keep(acc);
    return (acc << 32) | (u32)lo;
}

template <bool UW>
__device__ __forceinline__ u64 lm_shoup3(u64 a, u64 w, u64 wp, u64 nq, u64 x) {
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), p0 = (u32)wp, p1 = (u32)(wp >> 32);
    const u32 w0 = (u32)w, w1 = (u32)(w >> 32), n0 = (u32)nq, n1 = (u32)(nq >> 32);
#if LM_ASM_SHOUP
    u64 o;
    if (UW)
        asm(LM_SHOUP_BODY("%[x]")
            : [o] "=v"(o)
            : [a0] "v"(a0), [a1] "v"(a1), [p0] "s"(p0), [p1] "s"(p1), [w0] "s"(w0), [w1] "s"(w1), [n0] "s"(n0),
              [n1] "s"(n1), [x] "v"(x)
            : LM_SHOUP_CLOBBERS);
    else
        asm(LM_SHOUP_BODY("%[x]")
            : [o] "=v"(o)
            : [a0] "v"(a0), [a1] "v"(a1), [p0] "v"(p0), [p1] "v"(p1), [w0] "v"(w0), [w1] "v"(w1), [n0] "s"(n0),
              [n1] "s"(n1), [x] "v"(x)
            : LM_SHOUP_CLOBBERS);
    return o;
#else
    return lm_shoup3_c(a, w, wp, nq, x);
#endif
}
template <bool UW>
__device__ __forceinline__ u64 lm_shoup3(u64 a, u64 w, u64 wp, u64 nq) {
#if LM_ASM_SHOUP
    const u32 a0 = (u32)a, a1 = (u32)(a >> 32), p0 = (u32)wp, p1 = (u32)(wp >> 32);
    const u32 w0 = (u32)w, w1 = (u32)(w >> 32), n0 = (u32)nq, n1 = (u32)(nq >> 32);
    u64 o;
    if (UW)
        asm(LM_SHOUP_BODY("0")
            : [o] "=v"(o)
            : [a0] "v"(a0), [a1] "v"(a1), [p0] "s"(p0), [p1] "s"(p1), [w0] "s"(w0), [w1] "s"(w1), [n0] "s"(n0),
              [n1] "s"(n1)
            : LM_SHOUP_CLOBBERS);
    else
        asm(LM_SHOUP_BODY("0")
            : [o] "=v"(o)
            : [a0] "v"(a0), [a1] "v"(a1), [p0] "v"(p0), [p1] "v"(p1), [w0] "v"(w0), [w1] "v"(w1), [n0] "s"(n0),
              [n1] "s"(n1)
            : LM_SHOUP_CLOBBERS);
    return o;
#else
    return lm_shoup3<UW>(a, w, wp, nq, 0);
#endif
}
// canonical a*w mod q for a constant multiplier held in SGPRs
__device__ __forceinline__ u64 lm_shoup_cs(u64 a, tw_t W, u64 q, u64 nq) {
    u64 r = lm_shoup3<true>(a, W.w, W.wp, nq);
    r = lm_csub(r, 2 * q);
    return lm_csub(r, q);
}
// x mod q for any x < 2^64 (mad-chain form of lm_reduce): Shoup step with w = 1
__device__ __forceinline__ u64 lm_reduce_s(u64 x, u64 q, u64 nq, u64 qinv64) {
    u64 r = lm_shoup3<true>(x, 1ull, qinv64, nq);
    r = lm_csub(r, 2 * q);
    return lm_csub(r, q);
}

// (2x + 3q) - s, the difference branch of the forward butterfly, as exactly three instructions.  Left
// to the compiler the expression is re-associated into (3q - s) + 2x with the wave-uniform 3q as the
// minuend: v_subb_co_u32 cannot take an SGPR there, so every butterfly pays a v_mov of q3's upper word
// (94 of them in k_modup_ntt<14>) -- and each VALU instruction of these kernels costs its SIMD about
// five cycles whatever it does (tools/ubench_bfly.hip).  q3 = 3q lives in an SGPR pair.
__device__ __forceinline__ u64 lm_bfly_diff(u64 x, u64 q3, u64 s) {
#if LM_ASM_SHOUP
    u32 lo, hi;
    asm("v_lshl_add_u64 " LM_VP(0, 1) ", %[x], 1, %[q3]\n\t"
        "v_sub_co_u32_e32 %[lo], vcc, " LM_V(0) ", %[slo]\n\t"
        "v_subb_co_u32_e32 %[hi], vcc, " LM_V(1) ", %[shi], vcc"
        : [lo] "=&v"(lo), [hi] "=v"(hi)
        : [x] "v"(x), [q3] "s"(q3), [slo] "v"((u32)s), [shi] "v"((u32)(s >> 32))
        : LM_V(0), LM_V(1), "vcc");
    return ((u64)hi << 32) | lo;
#else
    return ((x << 1) + q3) - s;
#endif
}

struct lm_qc { // per-modulus constants of the lazy butterflies
    u64 q, nq, q3, qinv64;
};
__device__ __forceinline__ lm_qc lm_make_qc(const mod_t &m) {
    lm_qc c;
    c.q = m.q;
    c.nq = 0 - m.q;
    c.q3 = 3 * m.q;
    c.qinv64 = m.qinv64;
    return c;
}
