// The LDS-resident inverse limb transform (structure: lm_ntt_dev.h).
#pragma once
#include "lm_ntt_bfly.h"

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
        lm_inv_stages<R, false, false, true, lm_inv_narrow(LOGN)>(e, T, c);
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
        lm_inv_stages<R, UW, false, false, lm_inv_narrow(LOGN)>(e, T[LM_INV_TW_PREFETCH ? (m & 1) : 0], c);
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
        lm_inv_stages<R, true, true, false, lm_inv_narrow(LOGN)>(e, T, c);
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
