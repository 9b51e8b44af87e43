// The LDS-resident forward limb transform (structure: lm_ntt_dev.h), the coalesced output of its runs, and the stock run
// loader and storer.
#pragma once
#include "lm_ntt_bfly.h"

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
