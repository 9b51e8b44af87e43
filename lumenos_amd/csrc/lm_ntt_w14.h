// The register-resident forward limb transform at N = 2^14, two workgroups per CU (structure: lm_ntt_dev.h; its launch
// geometry, lm_geom_fwd, and LM_W14_THREADS: lm_ntt_plan.h).
#pragma once
#include "lm_ntt_bfly.h"

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
