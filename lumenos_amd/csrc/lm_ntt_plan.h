// Plan of the limb transforms (design notes: lm_ntt.hip, structure: lm_ntt_dev.h): the LDS layout and budget, the launch
// geometry, the pass plan, the ring degrees with their dispatchers, the launch, the host-side table layout of the split
// degrees and the modulus bound.  Host and constexpr code only -- no device code: what a translation unit without a
// transform (lm_ctx.hip) needs of them.
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
#define LM_MAX_PASSES 8

struct lm_ninv_t {
    tw_t t[LM_MAX_LIMBS];
};

__host__ __device__ constexpr int lm_ilog2(int x) { return x <= 1 ? 0 : 1 + lm_ilog2(x >> 1); }
__host__ __device__ constexpr size_t lm_lds_for(uint32_t n) { return (size_t)(n + (n >> 3) + 2) * sizeof(u64); }
// LDS of a gfx950 CU: what a workgroup's transform has to fit (the reason for the split degrees below) and the dynamic-LDS
// limit every transform kernel is raised to
constexpr size_t LM_CU_LDS_BYTES = 160 * 1024;
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
// with an adapted loader / storer (lm_split_fwd_loader, lm_ntt_inverse_split: lm_ntt_split.h, DESIGN.md section 3 "the
// split transform").  Only the kernels of the server's path and of the key switch are instantiated for these degrees
// (lm_for_any_logn); every other entry point keeps lm_for_logn and refuses them.
#define LM_FOR_EACH_SPLIT_LOGN(X) X(15)
// THE question "is this a split degree", at compile time and -- for a context's degree, which lumen_ctx_create has found
// on one of the two lists -- at run time
__host__ __device__ constexpr bool lm_is_split(int logN) { return logN > 14; }
// degree of the transform a workgroup runs: the half transform of a split degree, the degree itself otherwise
__host__ __device__ constexpr int lm_tlog(int logN) { return lm_is_split(logN) ? logN - 1 : logN; }
// the two lists against the predicate, and both against the LDS budget that is the reason for splitting
#define LM_X(n)                                                                                                         \
    static_assert(!lm_is_split(n), "a degree of LM_FOR_EACH_LOGN runs one-piece transforms");                            \
    static_assert(lm_lds_for(1u << lm_tlog(n)) <= LM_CU_LDS_BYTES, "the transform of a workgroup must fit a CU's LDS");
LM_FOR_EACH_LOGN(LM_X)
#undef LM_X
#define LM_X(n)                                                                                                         \
    static_assert(lm_is_split(n), "a degree of LM_FOR_EACH_SPLIT_LOGN runs half transforms");                            \
    static_assert(lm_lds_for(1u << lm_tlog(n)) <= LM_CU_LDS_BYTES, "the transform of a workgroup must fit a CU's LDS");
LM_FOR_EACH_SPLIT_LOGN(LM_X)
#undef LM_X
// membership in the list (lumen_ctx_create; a context's degree is asked lm_is_split)
static inline bool lm_logn_split_supported(uint32_t logN) {
#define LM_X(n) if (logN == n) return true;
    LM_FOR_EACH_SPLIT_LOGN(LM_X)
#undef LM_X
    return false;
}
// lm_for_logn plus the split degrees: for the launches whose kernels are instantiated for both lists
template <class F>
static inline int lm_for_any_logn(lumen_ctx *ctx, uint32_t logN, F &&f) {
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
    LM_CHECK(ctx, !lm_is_split((ctx)->logN), "%s: ring degree 2^%u has no kernel instantiation (split degree: "         \
             "transforms, rescale, products and the key switch only)", what, (ctx)->logN)
// grid of a forward-bearing kernel with `blocks` logical workgroups (a split degree: two per block, lm_half_of_block)
template <int LOGN>
static inline uint32_t lm_fwd_grid(uint32_t blocks) { return lm_is_split(LOGN) ? 2 * blocks : blocks; }

// workgroup size of the register-resident forward transform at N = 2^14 (lm_ntt_forward_w14, lm_ntt_w14.h)
#define LM_W14_THREADS 512
// Geometry of the forward kernels that run lm_ntt_forward_w14 at N = 2^14 (k_limb_ntt<14, false>, k_modup_ntt<14>,
// k_moddown_ntt<14>)
// and lm_ntt_forward below it (a split degree: the LDS-resident half transform, lm_tlog).  4 waves per SIMD caps the
// N = 2^14 kernels at 128 VGPRs, so that two workgroups of 8 waves fit on a CU.
__host__ __device__ constexpr lm_geom lm_geom_fwd(int logN) {
    return logN == 14 ? lm_geom{LM_W14_THREADS, 4, lm_lds_for(1u << 13)} : lm_geom_lds(lm_tlog(logN));
}

// Launches a kernel with dynamic LDS on the context's stream: raises the kernel's dynamic-LDS limit once per
// context (hipFuncSetAttribute is not free on the launch path), fails through lm_fail.
template <class... P, class... A>
static inline int lm_launch(lumen_ctx *ctx, void (*kernel)(P...), const lm_geom &g, dim3 grid, A &&...args) {
    const void *fp = reinterpret_cast<const void *>(kernel);
    if (!ctx->lds_attr_done.count(fp)) {
        LM_HIP(ctx, hipFuncSetAttribute(fp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LM_CU_LDS_BYTES));
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
    if (!lm_is_split((int)logN)) return;
    for (size_t at = 0; at + ((size_t)1 << logN) <= tw.size(); at += (size_t)1 << logN) lm_split_tw(tw.data() + at, logN);
}

// ---- the modulus bound.  A context's moduli satisfy lm_q_bound_factor(log_n) * q < 2^64 (lumen_ctx_create).  The lazy
// forward transform takes inputs below 7q (fused basis extension) and lets values grow by 3q per stage before its one
// reduction, so its storer sees values below (3 log_n + 7) q; a split degree's outer butterfly in the loader is one of the
// log_n stages -- the half transform starts below 10q and its storer sees (3 (log_n - 1) + 10) q = (3 log_n + 7) q (lm_ntt_split.h).
// The InnerSum accumulator is lazy in [0, 2q) across the rotations (lm_keyswitch.hip, k_moddown_ntt): acc < 2q plus d < 6q
// must not wrap, 8q < 2^64 -- the factor at log_n = 0, so implied for every degree.
__host__ __device__ constexpr uint64_t lm_q_bound_factor(uint32_t log_n) { return 3ull * log_n + 8; }
static_assert(lm_q_bound_factor(0) >= 8, "the modulus bound (3 log_n + 8) q < 2^64 must imply 8 q < 2^64");
// The inverse transform's passes (lm_inv_stages, lm_ntt_bfly.h) let values reach 6q * 2^(R-1) in a pass of R stages: 48q
// in a four-stage pass, which the bound covers from log_n = 14 up.  Below that the four-stage pass runs NARROW (its two
// sums of eight brought under 12q before the fourth stage) and peaks at 36q.  Every degree's pass list is held to it.
__host__ __device__ constexpr bool lm_inv_narrow(int log_n) { return lm_q_bound_factor((uint32_t)log_n) < 48; }
__host__ __device__ constexpr uint64_t lm_inv_pass_peak(int R, bool narrow) { return R == 4 && narrow ? 36 : 3ull << R; }
// log_n: the context's degree (its bound); tlog: the degree of the transform a workgroup runs (its pass list)
__host__ __device__ constexpr bool lm_inv_fits(int log_n, int tlog) {
    for (int i = 0; i < lm_npasses(tlog); i++)
        if (lm_inv_pass_peak(lm_pass_r(tlog, i), lm_inv_narrow(tlog)) > lm_q_bound_factor((uint32_t)log_n)) return false;
    return true;
}
#define LM_X(n) static_assert(lm_inv_fits(n, lm_tlog(n)), "an inverse pass's peak (48q, or 36q narrowed) must stay under the modulus bound");
LM_FOR_EACH_LOGN(LM_X)
LM_FOR_EACH_SPLIT_LOGN(LM_X)
#undef LM_X
#define LM_X(n) static_assert(3ull * n + 7 < lm_q_bound_factor(n), "the split transform's storer bound (3 log_n + 7) q must stay under the modulus bound");
LM_FOR_EACH_SPLIT_LOGN(LM_X)
#undef LM_X
