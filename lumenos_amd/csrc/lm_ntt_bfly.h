// What every limb transform is made of (structure: lm_ntt_dev.h): padded LDS addressing, twiddle sets, the lazy butterfly
// stages of a pass, the dealing of work items to lanes, and the storer protocol's optional members.
#pragma once
#include "lm_ntt_plan.h"
#include "lm_shoup.h"

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

// Butterflies (written out stage by stage in lm_fwd_stages / lm_inv_stages):
//   forward (Cooley-Tukey), fully lazy:   s = x + w*y (x rides in the multiplication's addend slot),
//       y' = (2x + 3q) - s, x' = s: both outputs grow by at most 3q per stage (x' by less; y' = x + 3q - (w*y lazily)
//       by exactly 3q when the lazy product is 0, i.e. when y or w is), so R stages on inputs below B leave values below
//       B + 3Rq;
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
// and is below 3q * 2^k <= 48q (NARROW, below: e[0] of four stages below 24q).  Unless this is the transform's last pass (whose storer multiplies by
// N^-1 and takes any value below 2^64) the outputs are brought back under 3q: k conditional
// subtractions, or one multiplication-free Shoup reduction when k >= 3.
// NO WRAP: the sums of stage st stay below 6q * 2^st and so do its differences x + C - y, so R stages need
// 3q * 2^R <= 2^64.  For R <= 3 every context's modulus bound gives that (32q < 2^64 at the least, lm_q_bound_factor).
// A four-stage pass needs 48q <= 2^64, which the bound gives from log_n = 14 up only (3 * 14 + 8 = 50), while every
// degree from 2^10 up has such a pass -- and what a pass is fed lies ANYWHERE below 3q (sums brought home by lm_csub),
// so at q = 2^64 / 38 the sum of sixteen inputs does pass 2^64 on ordinary data.  NARROW (lm_inv_narrow(log_n): the
// degrees whose bound is under 48q) therefore brings the two sums of eight, e[0] and e[8], under 12q before the fourth
// stage -- two conditional subtractions per sixteen coefficients: that stage's sums then stay below 24q, its
// differences below 12q + 24q = 36q <= 38q, and e[0] leaves below 24q like e[1].  lm_ntt_plan.h holds every degree's
// pass list to these figures (lm_inv_fits); tests/test_arith_probe.py runs both forms at the largest modulus of every
// degree that has a four-stage pass.
template <int R, bool UW, bool LAST, bool FIRST, bool NARROW = false>
__device__ __forceinline__ void lm_inv_stages(u64 *e, const lm_inv_twset<R, UW, FIRST> &T, const lm_qc &c) {
    static_assert(R <= 4, "3q * 2^R must stay below 2^64");
#pragma unroll
    for (int st = 0; st < R; st++) {
        const int half = 1 << st, span = half << 1;
        const u64 C = c.q3 << st;
        if constexpr (NARROW && R == 4)
            if (st == 3) e[0] = lm_csub(e[0], c.q3 << 2), e[8] = lm_csub(e[8], c.q3 << 2);
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

// A storer may have a member `void pre(uint32_t i0)`: it is called with the first coefficient of a run
// BEFORE the run's butterflies are computed, so that whatever the store phase reads from global memory
// (the gadget product and the accumulator in the ModDown kernel) is requested a whole pass body early.
template <class S, class = void>
struct lm_has_pre : std::false_type {};
template <class S>
struct lm_has_pre<S, std::void_t<decltype(std::declval<S &>().pre(0u))>> : std::true_type {};

// the `after` of a forward transform that has nothing to do once the storer has seen its coefficients
struct lm_no_after {
    __device__ __forceinline__ void operator()(uint32_t, uint32_t) const {}
};
