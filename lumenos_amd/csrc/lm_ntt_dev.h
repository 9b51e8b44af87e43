// LDS-resident limb NTT building blocks for gfx950 (design notes: lm_ntt.hip).
//
// v3 structure.  A transform of N = 2^logN coefficients runs in one workgroup of NT = N/16 threads
// (64 <= NT <= 1024), i.e. NW = NT/64 waves, 16 coefficients per lane, as a list of passes of
// R <= 4 butterfly stages; a work item keeps 2^R coefficients in VGPRs for the R stages of a pass.
//   * The CROSS-WAVE pass does log2(NW) stages (the ones whose butterflies span more than N/NW
//     coefficients): it is the first pass of the forward transform, which reads its coefficients
//     straight from global memory through a caller-supplied loader (fusing e.g. an RNS basis
//     extension into the load), and the last pass of the inverse.
//   * Every other stage only touches one block of N/NW = 1024 consecutive coefficients, and each
//     block is owned by ONE wave for the rest of the transform: work items are dealt so that wave j
//     handles block j in every pass.  Those passes exchange coefficients through LDS without
//     workgroup barriers (a wave's LDS operations execute in order), so a transform has ONE
//     s_barrier instead of one per pass and the waves of a CU drift apart -- which is what keeps
//     the VALU fed: a single wave can issue a VALU instruction only every ~8 cycles
//     (profiles/r01_ubench_mad_latency.txt), so each SIMD needs two of its four waves runnable.
//   * The forward transform's last pass hands runs of 8 finished coefficients to a
//     caller-supplied storer (final reduction, rescale combine, ... fused) that writes global memory.
// Multiplications by twiddles are Shoup multiplications written as explicit v_mad_u64_u32 chains
// with the quotient estimate truncated to three partial products: the result is in [0, 3q).
// Twiddles of stages whose block index is wave-uniform are fetched with scalar loads.
#pragma once
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "lm_common.h"

// LDS layout: one pad slot per 8 coefficients.  Conflict-free for the stride-8 items and the runs of 8 of the last two
// passes; 64 consecutive coefficients (first two passes) straddle pad slots: a 2-way conflict on 4 of every 32 lanes
// (measured: a third of the LDS cycles are conflict cycles, the LDS busy 17 % of a launch).
#define LM_PAD(i) ((i) + ((i) >> 3))
// Padded index of element base + (k << LOG_STRIDE): for strides of at least 8 the pad term is affine in k --
// (base + 8m) >> 3 = (base >> 3) + m whatever the low bits of base -- so the 2^R elements of a work item sit at
// ONE padded base plus compile-time constants that the ds_read / ds_write offset field takes (the compiler does
// not see this by itself and builds a separate address register per element).  Smaller strides (runs of
// consecutive coefficients starting at a multiple of 8) fold already.
template <int LOG_STRIDE>
__device__ __forceinline__ uint32_t lm_pad_at(uint32_t base, uint32_t pbase, int k) {
    if constexpr (LOG_STRIDE >= 3)
        return pbase + (uint32_t)k * ((1u << LOG_STRIDE) + (1u << (LOG_STRIDE - 3)));
    else
        return LM_PAD(base + ((uint32_t)k << LOG_STRIDE));
}
#define LM_MAX_PASSES 8

struct lm_ninv_t {
    tw_t t[LM_MAX_LIMBS];
};

__host__ __device__ constexpr int lm_ilog2(int x) { return x <= 1 ? 0 : 1 + lm_ilog2(x >> 1); }
__host__ __device__ constexpr size_t lm_lds_for(uint32_t n) { return (size_t)(n + (n >> 3) + 2) * sizeof(u64); }
// Launch geometry of a limb-transform kernel.  A kernel's __launch_bounds__ (LM_GEOM_BOUNDS), its launches
// (lm_launch) and any occupancy query all read the SAME one of the two functions below.
struct lm_geom {
    int threads; // workgroup size
    int waves;   // second __launch_bounds__ argument (waves per SIMD); 1 = no constraint
    size_t lds;  // dynamic LDS bytes
};
#define LM_GEOM_BOUNDS(g) __launch_bounds__((g).threads, (g).waves)
// the LDS-resident form (lm_ntt_forward, lm_ntt_inverse): 16 coefficients per lane, at least one wave, at most
// 1024 threads, the whole limb in LDS
__host__ __device__ constexpr lm_geom lm_geom_lds(int logN) {
    const int nt = (1 << logN) / 16;
    return lm_geom{nt < 64 ? 64 : (nt > 1024 ? 1024 : nt), 1, lm_lds_for(1u << logN)};
}
// workgroup size the dealing templates assume (lm_deal, lm_fwd_first, lm_inv_last, lm_linear_out)
__host__ __device__ constexpr int lm_nthreads(int logN) { return lm_geom_lds(logN).threads; }
__host__ __device__ constexpr int lm_log_epl(int logN) { // log2 coefficients a work item keeps in VGPRs: at most 16
    return logN - lm_ilog2(lm_nthreads(logN)) > 4 ? 4 : logN - lm_ilog2(lm_nthreads(logN));
}
__host__ __device__ constexpr int lm_cross_r(int logN) { return lm_ilog2(lm_nthreads(logN) / 64); }   // stages of the cross-wave pass
// Pass plan in forward order: [cross-wave pass,] then the wave-local stages in as few passes of
// at most log2(coefficients per lane) stages as possible, bigger passes first (14 -> 4 | 4 3 3).
__host__ __device__ constexpr int lm_local_passes(int logN) {
    return (logN - lm_cross_r(logN) + lm_log_epl(logN) - 1) / lm_log_epl(logN);
}
__host__ __device__ constexpr int lm_npasses(int logN) { return (lm_cross_r(logN) > 0 ? 1 : 0) + lm_local_passes(logN); }
__host__ __device__ constexpr int lm_pass_r(int logN, int i) {
    const int ra = lm_cross_r(logN);
    if (ra > 0) {
        if (i == 0) return ra;
        i--;
    }
    int n = lm_local_passes(logN), rem = logN - ra, r = 0;
    for (int k = 0; k <= i; k++) {
        const int left = n - k;
        r = (rem + left - 1) / left;
        rem -= r;
    }
    return r;
}
// ring degrees the kernels are instantiated for
#define LM_FOR_EACH_LOGN(X) X(8) X(10) X(11) X(12) X(13) X(14)
// run-time ring degree -> compile-time: f(std::integral_constant<int, n>{}) for the instantiated n
template <class F>
static inline int lm_for_logn(lumen_ctx *ctx, uint32_t logN, F &&f) {
    switch (logN) {
#define LM_X(n) \
    case n: return f(std::integral_constant<int, n>{});
        LM_FOR_EACH_LOGN(LM_X)
#undef LM_X
    default: return lm_fail(ctx, "ring degree 2^%u has no kernel instantiation", logN);
    }
}
static inline bool lm_logn_supported(uint32_t logN) {
#define LM_X(n) if (logN == n) return true;
    LM_FOR_EACH_LOGN(LM_X)
#undef LM_X
    return false;
}
// ---- split degrees.  Above 2^14 a limb no longer fits a CU's LDS (lm_lds_for(2^15) = 288 KB of 160).  A transform of
// such a degree is ONE outer radix-2 stage and two half transforms of LOGN - 1, each of which is the LDS-resident code
// above with an adapted loader / storer (lm_split_fwd_loader, lm_ntt_inverse_split below, DESIGN.md section 3 "the
// split transform").  Only the kernels of the server's path and of the key switch are instantiated for these degrees
// (lm_for_logn_split); every other entry point keeps lm_for_logn and refuses them.
#define LM_FOR_EACH_SPLIT_LOGN(X) X(15)
__host__ __device__ constexpr bool lm_is_split(int logN) { return logN > 14; }
// degree of the transform a workgroup runs: the half transform of a split degree, the degree itself otherwise
__host__ __device__ constexpr int lm_tlog(int logN) { return lm_is_split(logN) ? logN - 1 : logN; }
static inline bool lm_logn_split_supported(uint32_t logN) {
#define LM_X(n) if (logN == n) return true;
    LM_FOR_EACH_SPLIT_LOGN(LM_X)
#undef LM_X
    return false;
}
// lm_for_logn plus the split degrees: for the launches whose kernels are instantiated for both lists
template <class F>
static inline int lm_for_logn_split(lumen_ctx *ctx, uint32_t logN, F &&f) {
    switch (logN) {
#define LM_X(n) \
    case n: return f(std::integral_constant<int, n>{});
        LM_FOR_EACH_SPLIT_LOGN(LM_X)
#undef LM_X
    default: return lm_for_logn(ctx, logN, std::forward<F>(f));
    }
}
// first statement (behind LM_ENTER) of the entry points that have no kernel for the split degrees: refused before
// anything is drawn, allocated or launched
#define LM_REFUSE_SPLIT(ctx, what)                                                                                      \
    LM_CHECK(ctx, !lm_logn_split_supported((ctx)->logN), "%s: ring degree 2^%u has no kernel instantiation (split degree: " \
             "transforms, rescale, products and the key switch only)", what, (ctx)->logN)
// Sub-tables of a split degree, in place of a modulus's table of N entries (forward or inverse, lm_build_tw's order:
// the stage with m groups reads tw[m + i]): half h in [h N/2, (h + 1) N/2), sub_h[m' + i] = tw[2m' + h m' + i] for
// m' = 1, 2, .., N/4 -- the table a transform of N/2 points expects, for the stages behind (forward) or before
// (inverse) the outer one -- and slot 0 of both, which no stage reads, the outer twiddle tw[1].
static inline void lm_split_tw(tw_t *tw, uint32_t logN) {
    const uint32_t H = 1u << (logN - 1);
    std::vector<tw_t> sub((size_t)2 * H);
    for (uint32_t h = 0; h < 2; h++) {
        sub[(size_t)h * H] = tw[1];
        for (uint32_t m = 1; m < H; m <<= 1)
            for (uint32_t i = 0; i < m; i++) sub[(size_t)h * H + m + i] = tw[2 * m + h * m + i];
    }
    memcpy(tw, sub.data(), sub.size() * sizeof(tw_t));
}
// a table of [count][2^logN] entries as the kernels of degree logN read it
static inline void lm_layout_tw(std::vector<tw_t> &tw, uint32_t logN) {
    if (!lm_logn_split_supported(logN)) return;
    for (size_t at = 0; at + ((size_t)1 << logN) <= tw.size(); at += (size_t)1 << logN) lm_split_tw(tw.data() + at, logN);
}
// Which half a workgroup of a forward-bearing kernel owns, and which logical block (what blockIdx.x is below the split
// degrees).  The grid of a split degree is twice the logical one, the halves of block k at k and k + gridDim.x / 2: a
// host-built work list keeps its XCD order when its length is a multiple of 8.
template <int LOGN>
struct lm_half {
    uint32_t block, h, off; // off = h * N/2: first coefficient of the half
};
template <int LOGN>
__device__ __forceinline__ lm_half<LOGN> lm_half_of_block() {
    if constexpr (lm_is_split(LOGN)) {
        const uint32_t nb = gridDim.x >> 1, h = blockIdx.x >= nb ? 1u : 0u;
        return {blockIdx.x - h * nb, h, h << (LOGN - 1)};
    } else {
        return {blockIdx.x, 0u, 0u};
    }
}
// position inside its half of NTT-domain position p (where the half's workgroup keeps it in LDS)
template <int LOGN>
__device__ __forceinline__ uint32_t lm_half_local(uint32_t p) {
    if constexpr (lm_is_split(LOGN))
        return p & ((1u << (LOGN - 1)) - 1);
    else
        return p;
}
// grid of a forward-bearing kernel with `blocks` logical workgroups
template <int LOGN>
static inline uint32_t lm_fwd_grid(uint32_t blocks) { return lm_is_split(LOGN) ? 2 * blocks : blocks; }

// Launches a kernel with dynamic LDS on the context's stream: raises the kernel's dynamic-LDS limit once per
// context (hipFuncSetAttribute is not free on the launch path), fails through lm_fail.
template <class... P, class... A>
static inline int lm_launch(lumen_ctx *ctx, void (*kernel)(P...), const lm_geom &g, dim3 grid, A &&...args) {
    const void *fp = reinterpret_cast<const void *>(kernel);
    if (!ctx->lds_attr_done.count(fp)) {
        LM_HIP(ctx, hipFuncSetAttribute(fp, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        ctx->lds_attr_done.insert(fp);
    }
    hipLaunchKernelGGL(kernel, grid, dim3(g.threads), g.lds, ctx->stream, std::forward<A>(args)...);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

static inline lm_ninv_t lm_ninv_of(const lumen_ctx *ctx) {
    lm_ninv_t n;
    for (uint32_t i = 0; i < LM_MAX_LIMBS; i++) n.t[i] = ctx->ninv[i];
    return n;
}

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

// Butterflies (written out stage by stage in lm_fwd_stages / lm_inv_stages):
//   forward (Cooley-Tukey), fully lazy:   s = x + w*y (x rides in the multiplication's addend slot),
//       y' = (2x + 3q) - s, x' = s: both outputs grow by < 3q per stage;
//   inverse (Gentleman-Sande), lazy inside a pass: in stage st of a pass both inputs are below
//       C = 3q * 2^st; x' = x + y is left to grow (< 2C), y' = w * (x + C - y) goes through the Shoup
//       multiplication (any input below 2^64) and lands in [0, 3q); lm_inv_stages brings the sums
//       back under 3q once per pass instead of once per butterfly.

template <bool UW>
__device__ __forceinline__ tw_t lm_tw_load(const tw_t *__restrict__ tw, uint32_t idx) {
    if (UW) idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx); // -> scalar load
    return tw[idx];
}

// Twiddles of R forward stages starting at stage s0 for block blk: W[(1 << st) - 1 + g], g < 2^st.
// Loaded apart from the stages that use them so that a pass can fetch the NEXT work item's (or the next
// pass's) twiddles before it starts computing: the per-lane table reads of the last stages are L2 round
// trips of about a thousand cycles, and with four waves per SIMD nothing else hides them.
template <int R, bool UW>
struct lm_twset {
    tw_t w[(1 << R) - 1];
    __device__ __forceinline__ void load(const tw_t *__restrict__ tw, uint32_t s0, uint32_t blk) {
#pragma unroll
        for (int st = 0; st < R; st++)
#pragma unroll
            for (int g = 0; g < (1 << st); g++) w[(1 << st) - 1 + g] = lm_tw_load<UW>(tw, ((1u << s0) << st) + (blk << st) + g);
    }
};

// R forward stages on e[0 .. 2^R) with preloaded twiddles
// (tools/exp_no_butterflies.patch makes the stages return at once: a transform kernel's memory-side floor,
// profiles/r05_exp_no_butterflies_floor.txt)
template <int R, bool UW>
__device__ __forceinline__ void lm_fwd_stages(u64 *e, const lm_twset<R, UW> &T, const lm_qc &c) {
#pragma unroll
    for (int st = 0; st < R; st++) {
        const int span = (1 << R) >> st, half = span >> 1;
        // all sums x + w*y of the stage first (x rides in the multiplication's addend slot), then all
        // differences (2x + 3q) - sum: measured 1-2 % faster than butterfly by butterfly
        u64 sum[(1 << R) / 2];
#pragma unroll
        for (int g = 0; g < (1 << st); g++) {
            const tw_t W = T.w[(1 << st) - 1 + g];
#pragma unroll
            for (int k = 0; k < half; k++)
                sum[g * half + k] = lm_shoup3<UW>(e[g * span + k + half], W.w, W.wp, c.nq, e[g * span + k]);
        }
#pragma unroll
        for (int g = 0; g < (1 << st); g++)
#pragma unroll
            for (int k = 0; k < half; k++) {
                u64 &x = e[g * span + k];
                e[g * span + k + half] = lm_bfly_diff(x, c.q3, sum[g * half + k]);
                x = sum[g * half + k];
            }
    }
}

// Twiddles of R inverse stages (first stage at butterfly distance 2^log_t0) for block blk, loaded apart from
// the stages that use them: stage st takes 2^(R-st-1) of them.  Left inside the stage loop, the compiler
// requests some of a pass's per-lane table words only when their stage comes up (two of the seven in the
// second pass at N = 2^14, each followed by s_waitcnt vmcnt(0): an L2 round trip in the middle of the
// butterflies); fetched as a set they are all in flight before the pass's LDS reads, and a pass with several
// work items per lane can request the next item's set before it computes the current one (LM_INV_TW_PREFETCH).
// N = 2^14: 9.4 -> 10.1 M inverse transforms/s.  (FIRST marks the first pass's sets: a transposed [g][w] table
// layout for them -- every load instruction one contiguous kilobyte instead of lanes 64 / 32 bytes apart --
// was measured and changes nothing, 9.35 against 9.40: the loads wait on L2 latency, not on request count.)
template <int R, bool UW, bool FIRST>
struct lm_inv_twset {
    tw_t w[(1 << R) - 1];
    static constexpr int off(int st) { return (1 << R) - (1 << (R - st)); } // stages 0..st-1 hold 2^R - 2^(R-st)
    __device__ __forceinline__ void load(const tw_t *__restrict__ tw, uint32_t logN, uint32_t log_t0, uint32_t blk) {
#pragma unroll
        for (int st = 0; st < R; st++) {
            const uint32_t m = 1u << (logN - log_t0 - st - 1);
#pragma unroll
            for (int g = 0; g < (1 << (R - st - 1)); g++)
                w[off(st) + g] = lm_tw_load<UW>(tw, m + (blk << (R - st - 1)) + g);
        }
    }
};

// R inverse stages on inputs in [0, 3q) with preloaded twiddles.
// Output e[i] has taken the sum branch in its last k stages (k = R for i = 0, else R-1-floor(log2 i))
// and is below 3q * 2^k <= 48q.  Unless this is the transform's last pass (whose storer multiplies by
// N^-1 and takes any value below 2^64) the outputs are brought back under 3q: k conditional
// subtractions, or one multiplication-free Shoup reduction when k >= 3.
template <int R, bool UW, bool LAST, bool FIRST>
__device__ __forceinline__ void lm_inv_stages(u64 *e, const lm_inv_twset<R, UW, FIRST> &T, const lm_qc &c) {
    static_assert(R <= 4, "3q * 2^R must stay below 2^64");
#pragma unroll
    for (int st = 0; st < R; st++) {
        const int half = 1 << st, span = half << 1;
        const u64 C = c.q3 << st;
        // all sums and differences of the stage first, then the multiplications (as in the forward stages)
        u64 dif[(1 << R) / 2];
#pragma unroll
        for (int g = 0; g < ((1 << R) / span); g++)
#pragma unroll
            for (int k = 0; k < half; k++) {
                u64 &x = e[g * span + k], &y = e[g * span + k + half];
                dif[g * half + k] = x + C - y;
                x = x + y;
            }
#pragma unroll
        for (int g = 0; g < ((1 << R) / span); g++) {
            const tw_t W = T.w[lm_inv_twset<R, UW, FIRST>::off(st) + g];
#pragma unroll
            for (int k = 0; k < half; k++)
                e[g * span + k + half] = lm_shoup3<UW>(dif[g * half + k], W.w, W.wp, c.nq);
        }
    }
    if (!LAST) {
#pragma unroll
        for (int i = 0; i < (1 << R) / 2; i++) {
            const int k = i == 0 ? R : R - 1 - lm_ilog2(i);
            if (k >= 3) {
                e[i] = lm_shoup3<true>(e[i], 1ull, c.qinv64, c.nq);
            } else {
#pragma unroll
                for (int j = k - 1; j >= 0; j--) e[i] = lm_csub(e[i], c.q3 << j);
            }
        }
    }
}

// Work-item dealing.  Cross-wave pass: item = tid + m*nthreads.  Wave-local passes: the items of
// a pass are split evenly over the waves in order, so that wave j always covers coefficients
// [j*N/NW, (j+1)*N/NW); within its share lane l takes items l, l+64, ...
template <int LOGN, int R>
struct lm_deal {
    static constexpr uint32_t items = 1u << (LOGN - R);
    static constexpr uint32_t per_wave = items / (lm_nthreads(LOGN) / 64);
    static constexpr uint32_t reps = per_wave / 64 ? per_wave / 64 : 1;
    static __device__ __forceinline__ uint32_t local(uint32_t tid, uint32_t m) {
        return (tid >> 6) * per_wave + (tid & 63) + 64 * m;
    }
    static __device__ __forceinline__ bool valid(uint32_t tid) { return per_wave >= 64 || (tid & 63) < per_wave; }
};
// orders a wave's LDS writes before its later LDS reads of other lanes' slots: the hardware keeps
// one wave's LDS operations in order, this only pins the compiler
__device__ __forceinline__ void lm_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------ forward
// Loader: u64 operator()(uint32_t i) -> coefficient i in [0, 7q)
// Storer: void operator()(uint32_t i0, const u64 *v, int count) -> `count` consecutive lazy
//         results (values < (3*logN+7)*q) starting at coefficient i0
//         (as a half of a split degree the loader's values are below 10q, not 7q, and the bound is the whole degree's:
//         (3*(logN+1)+7)*q -- lm_split_fwd_loader)
#ifndef LM_TW_PREFETCH
#define LM_TW_PREFETCH 1 // fetch the next work item's twiddles before computing the current one
#endif
template <int LOGN, int R, bool CROSS, class Loader>
__device__ __forceinline__ void lm_fwd_first(u64 *s, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld) {
    constexpr uint32_t log_tl = LOGN - R, items = 1u << log_tl, NT = lm_nthreads(LOGN);
    constexpr uint32_t reps = items / NT ? items / NT : 1;
    lm_twset<R, true> T;
    T.load(tw, 0, 0);
#pragma unroll 1
    for (uint32_t m = 0; m < reps; m++) {
        const uint32_t w = tid + m * NT;
        if (items < NT && w >= items) break;
        u64 e[1 << R];
#pragma unroll
        for (int k = 0; k < (1 << R); k++) e[k] = ld(w + ((uint32_t)k << log_tl));
        lm_fwd_stages<R, true>(e, T, c);
#pragma unroll
        for (int k = 0; k < (1 << R); k++) s[lm_pad_at<log_tl>(w, LM_PAD(w), k)] = e[k];
    }
}

// the wave-local passes: D::reps work items per lane; the twiddles of item m+1 are requested before
// item m is computed (two sets alive: (2^R - 1) * 4 VGPRs each when they are per-lane)
template <int LOGN, int R, int S0>
__device__ __forceinline__ void lm_fwd_mid(u64 *s, const tw_t *tw, const lm_qc &c, uint32_t tid) {
    constexpr uint32_t log_tl = LOGN - S0 - R;
    constexpr bool UW = log_tl >= 6;
    using D = lm_deal<LOGN, R>;
    if (!D::valid(tid)) return;
    lm_twset<R, UW> T[2];
    T[0].load(tw, S0, D::local(tid, 0) >> log_tl);
#pragma unroll
    for (uint32_t m = 0; m < D::reps; m++) {
        const uint32_t w = D::local(tid, m);
        const uint32_t blk = w >> log_tl, off = w & ((1u << log_tl) - 1);
        const uint32_t base = (blk << (log_tl + R)) + off;
        u64 e[1 << R];
        const uint32_t pb = LM_PAD(base);
#pragma unroll
        for (int k = 0; k < (1 << R); k++) e[k] = s[lm_pad_at<log_tl>(base, pb, k)];
        if (LM_TW_PREFETCH && m + 1 < D::reps) T[(m + 1) & 1].load(tw, S0, D::local(tid, m + 1) >> log_tl);
        if (!LM_TW_PREFETCH && m) T[m & 1].load(tw, S0, blk);
        lm_fwd_stages<R, UW>(e, T[m & 1], c);
#pragma unroll
        for (int k = 0; k < (1 << R); k++) s[lm_pad_at<log_tl>(base, pb, k)] = e[k];
    }
}

// A storer may have a member `void pre(uint32_t i0)`: it is called with the first coefficient of a run
// BEFORE the run's butterflies are computed, so that whatever the store phase reads from global memory
// (the gadget product and the accumulator in the ModDown kernel) is requested a whole pass body early.
template <class S, class = void>
struct lm_has_pre : std::false_type {};
template <class S>
struct lm_has_pre<S, std::void_t<decltype(std::declval<S &>().pre(0u))>> : std::true_type {};

template <int LOGN, int R, class Storer>
__device__ __forceinline__ void lm_fwd_last(const u64 *s, const tw_t *tw, const lm_qc &c, uint32_t tid, Storer &st) {
    constexpr uint32_t s0 = LOGN - R;
    using D = lm_deal<LOGN, R>;
    if (!D::valid(tid)) return;
    // a storer with its own prefetch keeps its registers: no second twiddle set then
    constexpr bool TWPF = LM_TW_PREFETCH && !lm_has_pre<Storer>::value;
    lm_twset<R, false> T[2];
    T[0].load(tw, s0, D::local(tid, 0));
#pragma unroll
    for (uint32_t m = 0; m < D::reps; m++) {
        const uint32_t w = D::local(tid, m);
        const uint32_t base = w << R;
        u64 e[1 << R];
#pragma unroll
        for (int k = 0; k < (1 << R); k++) e[k] = s[LM_PAD(base + k)];
        if constexpr (lm_has_pre<Storer>::value) st.pre(base);
        if (TWPF && m + 1 < D::reps) T[(m + 1) & 1].load(tw, s0, D::local(tid, m + 1));
        if (!TWPF && m) T[0].load(tw, s0, w);
        lm_fwd_stages<R, false>(e, T[TWPF ? (m & 1) : 0], c);
        st(base, e, 1 << R);
    }
}

template <int LOGN, int P, int S0, class Loader, class Storer>
__device__ __forceinline__ void lm_fwd_rec(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld,
                                           Storer &st) {
    constexpr int NP = lm_npasses(LOGN), R = lm_pass_r(LOGN, P);
    constexpr bool cross = lm_cross_r(LOGN) > 0;
    if constexpr (P == 0)
        lm_fwd_first<LOGN, R, cross>(sm, tw, c, tid, ld);
    else if constexpr (P == NP - 1)
        lm_fwd_last<LOGN, R>(sm, tw, c, tid, st);
    else
        lm_fwd_mid<LOGN, R, S0>(sm, tw, c, tid);
    if constexpr (P + 1 < NP) {
        if constexpr (P == 0 && cross)
            __syncthreads();
        else
            lm_wave_sync();
        lm_fwd_rec<LOGN, P + 1, S0 + R>(sm, tw, c, tid, ld, st);
    }
}
// coefficients per run the forward transform hands to its storer (2^R of the last pass)
template <int LOGN>
__host__ __device__ constexpr int lm_fwd_run() {
    return 1 << lm_pass_r(LOGN, lm_npasses(LOGN) - 1);
}
struct lm_no_after {
    __device__ __forceinline__ void operator()(uint32_t, uint32_t) const {}
};

// Forward transform.  `after(i0, n)` runs once the storer has seen coefficients [i0, i0+n) (the
// whole transform) -- NOT behind a barrier: other waves may still be in their last pass.
// N = 2^14 (pass plan 4 | 4 3 3) with every twiddle set requested a whole work item -- or a barrier wait --
// before its butterflies, ACROSS the passes: pass 1's wave-uniform set (SGPRs) before the barrier, the two
// per-lane sets of pass 2 under pass 1's butterflies, those of pass 3 in the registers pass 2 frees item
// by item.  (The generic passes only look one item ahead inside a pass: the first item of every pass
// waits a whole L2 round trip for its table words.)
#ifndef LM_TW_XPASS
#define LM_TW_XPASS 1
#endif
template <int LOGN, int R, int S0, bool UW>
__device__ __forceinline__ void lm_fwd_mid_item(u64 *s, const lm_twset<R, UW> &T, const lm_qc &c, uint32_t w) {
    constexpr uint32_t log_tl = LOGN - S0 - R;
    const uint32_t blk = w >> log_tl, off = w & ((1u << log_tl) - 1);
    const uint32_t base = (blk << (log_tl + R)) + off;
    u64 e[1 << R];
    const uint32_t pb = LM_PAD(base);
#pragma unroll
    for (int k = 0; k < (1 << R); k++) e[k] = s[lm_pad_at<log_tl>(base, pb, k)];
    lm_fwd_stages<R, UW>(e, T, c);
#pragma unroll
    for (int k = 0; k < (1 << R); k++) s[lm_pad_at<log_tl>(base, pb, k)] = e[k];
}
template <class Loader, class Storer>
__device__ __forceinline__ void lm_fwd14_xpass(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld,
                                               Storer &st) {
    constexpr int LOGN = 14;
    static_assert(lm_npasses(LOGN) == 4 && lm_pass_r(LOGN, 0) == 4 && lm_pass_r(LOGN, 1) == 4 &&
                      lm_pass_r(LOGN, 2) == 3 && lm_pass_r(LOGN, 3) == 3,
                  "written for the pass plan 4 | 4 3 3");
    using D4 = lm_deal<LOGN, 4>;
    using D3 = lm_deal<LOGN, 3>;
    static_assert(D4::reps == 1 && D3::reps == 2, "one item in pass 1, two in passes 2 and 3");
    lm_fwd_first<LOGN, 4, true>(sm, tw, c, tid, ld);
    lm_twset<4, true> T1;
    T1.load(tw, 4, D4::local(tid, 0) >> (LOGN - 8));
    __syncthreads();
    lm_twset<3, false> A, B;
    A.load(tw, 8, D3::local(tid, 0) >> (LOGN - 11));
    B.load(tw, 8, D3::local(tid, 1) >> (LOGN - 11));
    lm_fwd_mid_item<LOGN, 4, 4, true>(sm, T1, c, D4::local(tid, 0));
    lm_wave_sync();
    lm_fwd_mid_item<LOGN, 3, 8, false>(sm, A, c, D3::local(tid, 0));
    A.load(tw, 11, D3::local(tid, 0));
    lm_fwd_mid_item<LOGN, 3, 8, false>(sm, B, c, D3::local(tid, 1));
    B.load(tw, 11, D3::local(tid, 1));
    lm_wave_sync();
#pragma unroll
    for (uint32_t m = 0; m < 2; m++) {
        const uint32_t base = D3::local(tid, m) << 3;
        u64 e[8];
#pragma unroll
        for (int k = 0; k < 8; k++) e[k] = sm[LM_PAD(base + k)];
        lm_fwd_stages<3, false>(e, m ? B : A, c);
        st(base, e, 8);
    }
}

// XPASS = false: the generic passes also at N = 2^14 (a kernel whose storer needs the registers the second
// twiddle set of the last pass would take)
template <int LOGN, bool XPASS = true, class Loader, class Storer, class After = lm_no_after>
__device__ __forceinline__ void lm_ntt_forward(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld,
                                               Storer &st, After after = After()) {
    static_assert(lm_npasses(LOGN) >= 2, "a transform needs a loading and a storing pass");
    // (not with a storer that prefetches for itself -- ModDown: its pre() words and two live twiddle sets
    // make 119 VGPRs and the kernel 3 % slower, measured)
    if constexpr (LOGN == 14 && XPASS && LM_TW_XPASS && !lm_has_pre<Storer>::value)
        lm_fwd14_xpass(sm, tw, c, tid, ld, st);
    else
        lm_fwd_rec<LOGN, 0, 0>(sm, tw, c, tid, ld, st);
    after(0u, 1u << LOGN);
}

// ------------------------------------------------------------------ forward, N = 2^14, limb in registers
// Two workgroups per CU.  lm_ntt_forward<14> keeps the whole limb in LDS (144 KB of the CU's 160 KB): one 16-wave
// workgroup per CU, whose waves load, meet at the barrier and multiply together.  Here 512 threads (8 waves) keep
// 32 coefficients per lane in VGPRs and LDS is only a transit buffer for half a limb: one slot of 1024 words per
// wave, lm_lds_for(8192) = 73 744 B, so two workgroups fit on a CU and four waves share a SIMD.
// Coefficient index i = bits 13..0.  Pass plan (stage s works on index bit 13 - s):
//   pass 1  stages 0-4   (bits 13..9)  i = r << 9 | tid                      twiddles: constant indices (SGPRs)
//   pass 2  stages 5-7   (bits 8..6)   i = w << 11 | r << 6 | l             wave-uniform (SGPRs), 4 items of 8
//   pass 3  stages 8-10  (bits 5..3)   i = w << 11 | r4 r3 << 9 | l5..3 << 6 | r2..0 << 3 | l2..0    per lane
//   pass 4  stages 11-13 (bits 2..0)   i = w << 11 | r4 r3 << 9 | l << 3 | r2..0                    per lane
// (r: the lane's register index 0..31, w: wave, l: lane).  From pass 2 on wave w owns bits 13..11 = w.
// Every exchange goes in two halves split by index bit 10: a register bit of every pass from 2 on and a stage
// bit of none, so each lane writes 16 and reads 16 words per half and every work item lies in one half.  In
// every layout bit 10 is the top register bit (pass 1: r bit 1), the half of coefficient i sits at slot word
// (i >> 11) << 10 | (i & 1023): wave w's slot holds exactly the words wave w reads.  The cross-wave exchange
// (pass 1 -> 2) needs barriers between its halves; after it each wave only touches its own slot and the
// wave-local exchanges are ordered by lm_wave_sync alone.
// Bank conflicts: pass 1 and 2 lanes move consecutive words; pass 3 runs of 8 lanes on consecutive words, runs
// 64 words apart (72 padded: the second 16-lane group of a ds_write_b64 on the other 16 banks); pass 4 lanes
// 8 words apart (9 padded).
// Every stage is one lazy butterfly as in lm_ntt_forward, so the storer's (3*logN+7)*q bound holds unchanged.
#define LM_W14_THREADS 512
// scheduling fence between the work items of passes 3 and 4: left alone the scheduler hoists later items'
// twiddle loads over the current item and runs out of the 128 VGPRs
#ifndef LM_W14_SCHED_FENCE
#define LM_W14_SCHED_FENCE 1
#endif
#if LM_W14_SCHED_FENCE
#define LM_W14_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define LM_W14_FENCE() ((void)0)
#endif
// LM_W14_PF3 / LM_W14_PF4: request the next work item's per-lane twiddle set (28 VGPRs) before computing the current
// one in pass 3 / 4, as lm_fwd_mid does.  With the limb in 64 VGPRs either one spills under the 128-VGPR cap
// (15-37 VGPRs), so each set is requested right before its item and four waves per SIMD cover the wait.
#ifndef LM_W14_PF3
#define LM_W14_PF3 0
#endif
#ifndef LM_W14_PF4
#define LM_W14_PF4 0
#endif
struct lm_w14_plan { // stages per pass
    static constexpr int R1 = 5, R2 = 3, R3 = 3, R4 = 3;
};
static_assert(lm_w14_plan::R1 + lm_w14_plan::R2 + lm_w14_plan::R3 + lm_w14_plan::R4 == 14, "the four passes cover the 14 stages once");
static_assert((1 << lm_w14_plan::R1) == 32 && (1 << lm_w14_plan::R2) * 4 == 32 && (1 << lm_w14_plan::R3) * 4 == 32 &&
                  (1 << lm_w14_plan::R4) * 4 == 32,
              "pass 1 is one item of 32 coefficients per lane, passes 2-4 four items of 8");
static_assert(LM_W14_THREADS * 32 == 1 << 14 && LM_W14_THREADS / 64 == 8, "8 waves x 64 lanes x 32 coefficients");
__device__ __forceinline__ uint32_t lm_w14_pos(uint32_t i) { return LM_PAD(((i >> 11) << 10) | (i & 1023u)); }
// padded slot word of base | k for a compile-time k whose bits are disjoint from base's, base & 7 == 0 or k & 7 == 0
__device__ __forceinline__ uint32_t lm_w14_at(uint32_t pbase, uint32_t k) { return pbase + k + (k >> 3); }

// R stages on e[0 .. 2^R) whose twiddles are the same for every lane (the transform's first R stages: table
// indices 1 .. 2^R - 1), fetched stage by stage with scalar loads.  Sums before differences as in lm_fwd_stages,
// in chunks of at most 8 butterflies (a whole stage of sums would take 32 more VGPRs).
template <int R>
__device__ __forceinline__ void lm_fwd_stages_first(u64 *e, const tw_t *tw, const lm_qc &c) {
#pragma unroll
    for (int st = 0; st < R; st++) {
        const int span = (1 << R) >> st, half = span >> 1, CH = half < 8 ? half : 8;
#pragma unroll
        for (int g = 0; g < (1 << st); g++) {
            const tw_t W = lm_tw_load<true>(tw, (1u << st) + g);
#pragma unroll
            for (int k0 = 0; k0 < half; k0 += CH) {
                u64 sum[CH];
#pragma unroll
                for (int k = 0; k < CH; k++)
                    sum[k] = lm_shoup3<true>(e[g * span + k0 + k + half], W.w, W.wp, c.nq, e[g * span + k0 + k]);
#pragma unroll
                for (int k = 0; k < CH; k++) {
                    u64 &x = e[g * span + k0 + k];
                    e[g * span + k0 + k + half] = lm_bfly_diff(x, c.q3, sum[k]);
                    x = sum[k];
                }
            }
        }
    }
}

// Loader / Storer / pre as lm_ntt_forward (runs of 8).  after(i0, n) runs once per half: every wave's storer
// has then seen offsets [i0, i0 + n) of the wave's block of 2048 coefficients (NOT behind a workgroup barrier).
template <class Loader, class Storer, class After = lm_no_after>
__device__ __forceinline__ void lm_ntt_forward_w14(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld,
                                                   Storer &st, After after = After()) {
    const uint32_t w = tid >> 6, l = tid & 63;
    u64 e[32];
    // pass 1
#pragma unroll
    for (int r = 0; r < 32; r++) e[r] = ld(((uint32_t)r << 9) | tid);
    lm_fwd_stages_first<5>(e, tw, c);
    // cross-wave exchange into pass 2's layout: pass 1 holds bit 10 in r bit 1, pass 2 in r bit 4
    const uint32_t p1 = LM_PAD(tid), p2 = LM_PAD((w << 10) | l);
    lm_twset<3, true> T2[2];
    T2[0].load(tw, 5, (w << 2) | 0);
    // (half 0 lands in e[0..15] only once pass 1's half-1 words there have left: they are spread over all of e)
    u64 e0[16];
#pragma unroll
    for (int h = 0; h < 2; h++) {
#pragma unroll
        for (int r = 0; r < 32; r++)
            if (((r >> 1) & 1) == h) sm[lm_w14_at(p1, (uint32_t)((r >> 2) << 10 | (r & 1) << 9))] = e[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; r++) (h ? e[16 + r] : e0[r]) = sm[lm_w14_at(p2, (uint32_t)r << 6)];
        if (h == 0) __syncthreads(); // every wave has read half 0 before half 1 overwrites it
    }
#pragma unroll
    for (int r = 0; r < 16; r++) e[r] = e0[r];
    // pass 2: items gq = r >> 3 (bits 10, 9), wave-uniform twiddle sets, the next one requested before each item
#pragma unroll
    for (int gq = 0; gq < 4; gq++) {
        if (gq + 1 < 4) T2[(gq + 1) & 1].load(tw, 5, (w << 2) | (uint32_t)(gq + 1));
        lm_fwd_stages<3, true>(e + 8 * gq, T2[gq & 1], c);
    }
    // wave-local exchange into pass 3's layout (bit 10: r bit 4 on both sides)
    const uint32_t p3 = LM_PAD((w << 10) | ((l >> 3) << 6) | (l & 7));
    lm_twset<3, false> T3[2];
    T3[0].load(tw, 8, (w << 5) | (l >> 3));
#pragma unroll
    for (int h = 0; h < 2; h++) {
        lm_wave_sync();
#pragma unroll
        for (int r = 16 * h; r < 16 * h + 16; r++) sm[lm_w14_at(p2, (uint32_t)(r & 15) << 6)] = e[r];
        lm_wave_sync();
#pragma unroll
        for (int r = 16 * h; r < 16 * h + 16; r++)
            e[r] = sm[lm_w14_at(p3, (uint32_t)(((r >> 3) & 1) << 9 | (r & 7) << 3))];
    }
    // pass 3: items m = r >> 3 (bits 10, 9), per-lane twiddle sets, the next one requested before each item
#pragma unroll
    for (int m = 0; m < 4; m++) {
        LM_W14_FENCE();
        if (LM_W14_PF3 && m + 1 < 4) T3[(m + 1) & 1].load(tw, 8, (w << 5) | ((uint32_t)(m + 1) << 3) | (l >> 3));
        if (!LM_W14_PF3 && m) T3[0].load(tw, 8, (w << 5) | ((uint32_t)m << 3) | (l >> 3));
        lm_fwd_stages<3, false>(e + 8 * m, T3[LM_W14_PF3 ? (m & 1) : 0], c);
    }
    // wave-local exchange into pass 4's layout
    const uint32_t p4 = LM_PAD((w << 10) | (l << 3));
    lm_twset<3, false> T4[2];
    T4[0].load(tw, 11, (w << 8) | l);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        lm_wave_sync();
#pragma unroll
        for (int r = 16 * h; r < 16 * h + 16; r++)
            sm[lm_w14_at(p3, (uint32_t)(((r >> 3) & 1) << 9 | (r & 7) << 3))] = e[r];
        lm_wave_sync();
#pragma unroll
        for (int r = 16 * h; r < 16 * h + 16; r++)
            e[r] = sm[lm_w14_at(p4, (uint32_t)(((r >> 3) & 1) << 9 | (r & 7)))];
    }
    // pass 4: items m = r >> 3, runs of 8 consecutive coefficients to the storer; after() once per half
    constexpr bool TWPF = LM_W14_PF4 && !lm_has_pre<Storer>::value;
    lm_wave_sync();
#pragma unroll
    for (int m = 0; m < 4; m++) {
        LM_W14_FENCE();
        const uint32_t i0 = (w << 11) | ((uint32_t)m << 9) | (l << 3);
        if constexpr (lm_has_pre<Storer>::value) st.pre(i0);
        if (TWPF && m + 1 < 4) T4[(m + 1) & 1].load(tw, 11, (w << 8) | ((uint32_t)(m + 1) << 6) | l);
        if (!TWPF && m) T4[0].load(tw, 11, (w << 8) | ((uint32_t)m << 6) | l);
        lm_fwd_stages<3, false>(e + 8 * m, T4[TWPF ? (m & 1) : 0], c);
        st(i0, e + 8 * m, 8);
        if (m & 1) {
            lm_wave_sync();
            after((uint32_t)(m >> 1) << 10, 1024u);
            lm_wave_sync();
        }
    }
}
// Storer of lm_ntt_forward_w14 that parks the runs in the wave's slot (the extension kernel's and ModDown's), and the
// coalesced output of one half from there (the counterparts of lm_lds_runs / lm_linear_out): f(j, v0, v1) gets
// coefficients j, j + 1 of the limb, lanes on consecutive pairs, one contiguous kilobyte per store instruction.
struct lm_w14_runs {
    u64 *sm;
    __device__ __forceinline__ void operator()(uint32_t i0, const u64 *v, int count) const {
        const uint32_t pb = lm_w14_pos(i0);
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < count) sm[pb + k] = v[k];
    }
};
template <class F>
__device__ __forceinline__ void lm_w14_linear_out(const u64 *sm, uint32_t tid, uint32_t i0, F f) {
    const uint32_t w = tid >> 6, lane = tid & 63;
    const uint32_t pb = LM_PAD((w << 10) | (2 * lane));
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t j = (w << 11) | i0 | (2 * lane + 128 * k);
        f(j, sm[lm_w14_at(pb, 128 * k)], sm[lm_w14_at(pb, 128 * k) + 1]);
    }
}

// Geometry of the forward kernels that run lm_ntt_forward_w14 at N = 2^14 (k_limb_ntt<14, false>, k_modup_ntt<14>,
// k_moddown_ntt<14>)
// and lm_ntt_forward below it (a split degree: the LDS-resident half transform, lm_tlog).  4 waves per SIMD caps the
// N = 2^14 kernels at 128 VGPRs, so that two workgroups of 8 waves fit on a CU.
__host__ __device__ constexpr lm_geom lm_geom_fwd(int logN) {
    return logN == 14 ? lm_geom{LM_W14_THREADS, 4, lm_lds_for(1u << 13)} : lm_geom_lds(lm_tlog(logN));
}

// ------------------------------------------------------------------ inverse
// Loader: void operator()(uint32_t i0, u64 *v, int count) -> `count` consecutive coefficients in [0, q)
// Storer: void operator()(uint32_t i, u64 v) -> lazy result (any value below 2^64, before the N^-1 scaling)
template <int LOGN, int R, class Loader>
__device__ __forceinline__ void lm_inv_first(u64 *s, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld) {
    using D = lm_deal<LOGN, R>;
    if (!D::valid(tid)) return;
    // (requesting run m+1 while run m is computed was measured and is slower: 9.09 against 9.41 M
    // transforms/s at N = 2^14 -- the loads of sixteen waves then bunch up in front of the first pass)
#pragma unroll 1
    for (uint32_t m = 0; m < D::reps; m++) {
        const uint32_t w = D::local(tid, m);
        const uint32_t base = w << R;
        u64 e[1 << R];
        lm_inv_twset<R, false, true> T;
        T.load(tw, LOGN, 0, w);
        ld(base, e, 1 << R);
        lm_inv_stages<R, false, false, true>(e, T, c);
#pragma unroll
        for (int k = 0; k < (1 << R); k++) s[LM_PAD(base + k)] = e[k];
    }
}

#ifndef LM_INV_TW_PREFETCH
#define LM_INV_TW_PREFETCH 1 // wave-local inverse passes: request work item m+1's twiddles before computing item m
#endif
template <int LOGN, int R, int LT>
__device__ __forceinline__ void lm_inv_mid(u64 *s, const tw_t *tw, const lm_qc &c, uint32_t tid) {
    using D = lm_deal<LOGN, R>;
    if (!D::valid(tid)) return;
    constexpr bool UW = LT >= 6;
    lm_inv_twset<R, UW, false> T[2];
    T[0].load(tw, LOGN, LT, D::local(tid, 0) >> LT);
#pragma unroll
    for (uint32_t m = 0; m < D::reps; m++) {
        const uint32_t w = D::local(tid, m);
        const uint32_t blk = w >> LT, off = w & ((1u << LT) - 1);
        const uint32_t base = (blk << (LT + R)) + off;
        u64 e[1 << R];
        const uint32_t pb = LM_PAD(base);
#pragma unroll
        for (int k = 0; k < (1 << R); k++) e[k] = s[lm_pad_at<LT>(base, pb, k)];
        if (LM_INV_TW_PREFETCH && m + 1 < D::reps) T[(m + 1) & 1].load(tw, LOGN, LT, D::local(tid, m + 1) >> LT);
        if (!LM_INV_TW_PREFETCH && m) T[0].load(tw, LOGN, LT, blk);
        lm_inv_stages<R, UW, false, false>(e, T[LM_INV_TW_PREFETCH ? (m & 1) : 0], c);
#pragma unroll
        for (int k = 0; k < (1 << R); k++) s[lm_pad_at<LT>(base, pb, k)] = e[k];
    }
}

// a storer may take a third argument: the position k < 2^R of the value in its work item (a compile-time
// constant at every call site, so that it can index what pre() fetched without a dynamic register index)
template <class S, class = void>
struct lm_has_slot : std::false_type {};
template <class S>
struct lm_has_slot<S, std::void_t<decltype(std::declval<S &>()(0u, (u64)0, 0))>> : std::true_type {};

template <int LOGN, int R, class Storer>
__device__ __forceinline__ void lm_inv_last(const u64 *s, const tw_t *tw, const lm_qc &c, uint32_t tid, Storer &st) {
    constexpr uint32_t log_t0 = LOGN - R, items = 1u << log_t0, NT = lm_nthreads(LOGN);
    constexpr uint32_t reps = items / NT ? items / NT : 1;
    lm_inv_twset<R, true, false> T; // wave-uniform (block 0 for every item): scalar loads, once
    T.load(tw, LOGN, log_t0, 0);
#pragma unroll 1
    for (uint32_t m = 0; m < reps; m++) {
        const uint32_t w = tid + m * NT;
        if (items < NT && w >= items) break;
        u64 e[1 << R];
#pragma unroll
        for (int k = 0; k < (1 << R); k++) e[k] = s[lm_pad_at<log_t0>(w, LM_PAD(w), k)];
        // a storer with a member pre(w) is told the work item before its butterflies run: whatever it
        // reads from global memory for coefficients w + (k << log_t0), k < 2^R, is then in flight under them
        if constexpr (lm_has_pre<Storer>::value) st.pre(w);
        lm_inv_stages<R, true, true, false>(e, T, c);
#pragma unroll
        for (int k = 0; k < (1 << R); k++) {
            if constexpr (lm_has_slot<Storer>::value)
                st(w + ((uint32_t)k << log_t0), e[k], k);
            else
                st(w + ((uint32_t)k << log_t0), e[k]);
        }
    }
}

// the inverse runs the pass list backwards: wave-local passes first, the cross-wave pass last
template <int LOGN, int P, int LT, class Loader, class Storer>
__device__ __forceinline__ void lm_inv_rec(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld,
                                           Storer &st) {
    constexpr int NP = lm_npasses(LOGN), R = lm_pass_r(LOGN, NP - 1 - P);
    constexpr bool cross = lm_cross_r(LOGN) > 0;
    if constexpr (P == 0)
        lm_inv_first<LOGN, R>(sm, tw, c, tid, ld);
    else if constexpr (P == NP - 1)
        lm_inv_last<LOGN, R>(sm, tw, c, tid, st);
    else
        lm_inv_mid<LOGN, R, LT>(sm, tw, c, tid);
    if constexpr (P + 1 < NP) {
        if constexpr (P + 2 == NP && cross)
            __syncthreads();
        else
            lm_wave_sync();
        lm_inv_rec<LOGN, P + 1, LT + R>(sm, tw, c, tid, ld, st);
    }
}
// (Requests ACROSS the inverse's passes, as lm_fwd14_xpass does for the forward transform -- the second pass's
// first set under the first pass, the wave-uniform sets before the fences and the barrier -- were measured at
// N = 2^14: 10.14 against 10.17 M transforms/s with the first pass left as the rolled loop, 9.48 with its two
// work items unrolled.  Not kept.)
template <int LOGN, class Loader, class Storer>
__device__ __forceinline__ void lm_ntt_inverse(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld,
                                               Storer &st) {
    static_assert(lm_npasses(LOGN) >= 2, "a transform needs a loading and a storing pass");
    lm_inv_rec<LOGN, 0, 0>(sm, tw, c, tid, ld, st);
}

// ---- stock loaders / storers
// consecutive coefficients move as 16-byte vectors
__device__ __forceinline__ void lm_load_run(const u64 *p, uint32_t i0, u64 *v, int count) {
    if (count == 2) {
        const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(p + i0);
        v[0] = a.x, v[1] = a.y;
    } else {
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            if (k < count) {
                const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(p + i0 + k);
                v[k] = a.x, v[k + 1] = a.y;
            }
        }
    }
}
// ---- coalesced output of a forward transform (round 5).  The last pass finishes runs of 2^R <= 8 consecutive coefficients
// per lane; stored from there (lm_store_run) a wave's 16-byte stores sit 64 bytes apart -- four partial writes per 128-byte
// line, and the extension kernel's store phase is sensitive to exactly that (profiles/r05_exp_linear_store.txt: -3.5 % on
// k_modup_ntt<14>).  Instead the runs go back to the slots their lane has just consumed (lm_lds_runs as the Storer; a wave's
// LDS operations execute in order and every slot of a wave's block is written by that wave) and lm_linear_out hands every
// lane PAIRS of consecutive coefficients, lanes on consecutive addresses: one contiguous kilobyte per store instruction.
struct lm_lds_runs {
    u64 *sm;
    __device__ __forceinline__ void operator()(uint32_t i0, const u64 *v, int count) const {
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < count) sm[LM_PAD(i0 + k)] = v[k];
    }
};
// f(j, v0, v1): coefficients j, j + 1 of the limb (after the wave's own last pass; no workgroup barrier)
template <int LOGN, class F>
__device__ __forceinline__ void lm_linear_out(const u64 *sm, uint32_t tid, F f) {
    constexpr uint32_t NW = lm_nthreads(LOGN) / 64, BLK = (1u << LOGN) / NW, IT = BLK / 128 ? BLK / 128 : 1;
    const uint32_t wave = tid >> 6, lane = tid & 63;
    lm_wave_sync();
#pragma unroll
    for (uint32_t k = 0; k < IT; k++) {
        const uint32_t j = wave * BLK + 2 * lane + k * 128;
        if (BLK >= 128 || 2 * lane < BLK) f(j, sm[LM_PAD(j)], sm[LM_PAD(j + 1)]);
    }
}

__device__ __forceinline__ void lm_store_run(u64 *p, uint32_t i0, const u64 *v, int count) {
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        if (k < count) {
            ulonglong2 a;
            a.x = v[k], a.y = v[k + 1];
            *reinterpret_cast<ulonglong2 *>(p + i0 + k) = a;
        }
    }
}

// ------------------------------------------------------------------ the split transform (LM_FOR_EACH_SPLIT_LOGN)
// `tw` below is a modulus's table in the split layout (lm_split_tw): half h's sub-table at tw + h N/2, the outer
// twiddle in its slot 0.
//
// Forward.  lo[j] = x[j] + w x[j + N/2], hi[j] = x[j] - w x[j + N/2] with w = tw[1], then half h is an ordinary
// transform of N/2 points whose outputs are NTT-domain positions [h N/2, (h + 1) N/2).  Two workgroups per limb, one
// per half (lm_half_of_block): the loader of half h calls the kernel's own loader at j and j + N/2 and does the outer
// butterfly -- no scratch and no extra launch, but whatever is fused into the load (the basis extensions of the key
// switch) runs twice per coefficient.  The storer sees indices of the HALF: the kernel offsets its pointers by
// lm_half::off.  Bounds: the kernel's loader gives x < 7q; the lazy butterfly adds less than 3q to either output, so
// the half transform starts below 10q and its storer gets values below (3 (LOGN - 1) + 10) q = (3 LOGN + 7) q, the
// bound of a one-piece transform of LOGN stages (52q at 2^15, under the context's (3 LOGN + 8) q < 2^64).
template <class Loader>
struct lm_split_fwd_loader {
    Loader &ld;
    const lm_qc &c;
    tw_t W;
    uint32_t h, half_n;
    __device__ __forceinline__ u64 operator()(uint32_t j) {
        const u64 x = ld(j), y = ld(j + half_n);
        const u64 s = lm_shoup3<true>(y, W.w, W.wp, c.nq, x);
        return h ? lm_bfly_diff(x, c.q3, s) : s;
    }
};
template <int LOGN, class Loader, class Storer, class After = lm_no_after>
__device__ __forceinline__ void lm_ntt_forward_split(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid,
                                                     const lm_half<LOGN> &hf, Loader &ld, Storer &st, After after = After()) {
    static_assert(lm_is_split(LOGN), "degrees up to 2^14 run lm_ntt_forward / lm_ntt_forward_w14");
    const tw_t *twh = tw + hf.off;
    lm_split_fwd_loader<Loader> wld{ld, c, lm_tw_load<true>(twh, 0), hf.h, 1u << (LOGN - 1)};
    lm_ntt_forward<LOGN - 1>(sm, twh, c, tid, wld, st, after);
}
// The same in ONE workgroup, for a kernel that may run in place (k_limb_ntt: a second workgroup would read input words
// the first has already overwritten): the loader of the first run forms both outputs of the outer butterfly, keeps lo[j]
// and parks hi[j], as it is (below 10q), in `park` (N/2 words of global memory: the second half of the kernel's own
// output, which the second run's storer overwrites); the second run's loader reads it back -- the first pass deals the
// same indices to a lane in both runs, so a lane reads what it wrote itself.  Every input word is read once.  In place:
// x[j + N/2] is read by the lane that overwrites it, right before; x[j]'s slot is written by the first run's last
// pass, behind the barrier that follows every read of the first run.  The storer gets indices of the whole limb.
template <int LOGN, class Loader, class Storer>
__device__ __forceinline__ void lm_ntt_forward_split_parked(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld,
                                                            u64 *park, Storer &st) {
    static_assert(lm_is_split(LOGN), "degrees up to 2^14 run lm_ntt_forward / lm_ntt_forward_w14");
    constexpr uint32_t H = 1u << (LOGN - 1);
    const tw_t W = lm_tw_load<true>(tw, 0);
    auto ld0 = [&](uint32_t j) {
        const u64 x = ld(j), y = ld(j + H);
        const u64 s = lm_shoup3<true>(y, W.w, W.wp, c.nq, x);
        park[j] = lm_bfly_diff(x, c.q3, s);
        return s;
    };
    // (the generic passes: the first run's loader holds two words per coefficient, the registers lm_fwd14_xpass spends
    // on twiddle sets requested across the passes)
    lm_ntt_forward<LOGN - 1, false>(sm, tw, c, tid, ld0, st);
    __syncthreads(); // the second half transform reuses the LDS
    uint32_t tid1 = tid; // nothing derived from the lane index is carried over from the first run (as in k_intt_pack)
    asm volatile("" : "+v"(tid1));
    auto ld1 = [&](uint32_t j) { return park[j]; };
    auto st1 = [&](uint32_t i0, const u64 *v, int count) { st(i0 + H, v, count); };
    lm_ntt_forward<LOGN - 1, false>(sm, tw + H, c, tid1, ld1, st1);
}

// Inverse, the mirror image: half h of the NTT-domain input is inverse-transformed on its own with its sub-table (A from
// half 0, B from half 1, unscaled), then out[j] = (A[j] + B[j]) N^-1 and out[j + N/2] = (A[j] - B[j]) inv[1] N^-1.
// ONE workgroup runs the two half transforms back to back.  The first parks A, canonical, in `park` (N/2 words of
// global memory: the kernel's own output, whose first half the join overwrites); the storer of the second reads A[j]
// back when B[j] leaves its registers -- in the cross-wave last pass a lane sees the same indices in both runs, so it
// reads what it wrote itself (the read-back of k_intt_pack) -- and hands the kernel's storer the two joined values,
// which the storer scales by N^-1 as it would a one-piece transform's.  The inverse's storer receives "any value
// below 2^64" (up to 48q at 2^14): B is brought under 3q first, so A + B < 4q and A + 3q - B < 4q cannot wrap, and the
// difference leaves its multiplication by inv[1] in [0, 3q).
// In place (park == the loader's source) is safe as it is for a one-piece transform: every global read of a half
// transform sits before the barrier in front of its last pass, every write behind it.
template <int LOGN, class Loader, class Storer>
__device__ __forceinline__ void lm_ntt_inverse_split(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld,
                                                     u64 *park, Storer &st) {
    static_assert(lm_is_split(LOGN), "degrees up to 2^14 run lm_ntt_inverse");
    constexpr uint32_t H = 1u << (LOGN - 1);
    {
        auto st0 = [&](uint32_t i, u64 v) { park[i] = lm_reduce_s(v, c.q, c.nq, c.qinv64); };
        lm_ntt_inverse<LOGN - 1>(sm, tw, c, tid, ld, st0);
    }
    __syncthreads(); // the second half transform reuses the LDS
    const tw_t W = lm_tw_load<true>(tw + H, 0);
    auto ld1 = [&](uint32_t i0, u64 *v, int count) { ld(i0 + H, v, count); };
    auto st1 = [&](uint32_t i, u64 v) {
        const u64 a = park[i];
        const u64 b = lm_shoup3<true>(v, 1ull, c.qinv64, c.nq);
        st(i, a + b);
        st(i + H, lm_shoup3<true>(a + c.q3 - b, W.w, W.wp, c.nq));
    };
    uint32_t tid1 = tid; // nothing derived from the lane index is carried over from the first run (as in k_intt_pack)
    asm volatile("" : "+v"(tid1));
    lm_ntt_inverse<LOGN - 1>(sm, tw + H, c, tid1, ld1, st1);
}
