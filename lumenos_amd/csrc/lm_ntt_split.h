// The split limb transform of the degrees above 2^14 (LM_FOR_EACH_SPLIT_LOGN, lm_ntt_plan.h): which half a workgroup owns,
// the three split transforms, and the one spelling of "one piece below the split, halves above" the fused kernels call.
#pragma once
#include "lm_ntt_fwd.h"
#include "lm_ntt_inv.h"

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

// ---- one piece below the split, halves above: what a fused kernel calls at every degree it is instantiated for
// the forward transform of the half (or, below the split, the limb) that the workgroup owns: hf = lm_half_of_block
template <int LOGN, class Loader, class Storer, class After = lm_no_after>
__device__ __forceinline__ void lm_ntt_forward_half(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid, const lm_half<LOGN> &hf,
                                                    Loader &ld, Storer &st, After after = After()) {
    if constexpr (lm_is_split(LOGN))
        lm_ntt_forward_split<LOGN>(sm, tw, c, tid, hf, ld, st, after);
    else
        lm_ntt_forward<LOGN>(sm, tw, c, tid, ld, st, after);
}
// the inverse transform of a whole limb in one workgroup; `park` (N/2 words, lm_ntt_inverse_split) is only touched at a
// split degree
template <int LOGN, class Loader, class Storer>
__device__ __forceinline__ void lm_ntt_inverse_whole(u64 *sm, const tw_t *tw, const lm_qc &c, uint32_t tid, Loader &ld, u64 *park,
                                                     Storer &st) {
    if constexpr (lm_is_split(LOGN))
        lm_ntt_inverse_split<LOGN>(sm, tw, c, tid, ld, park, st);
    else
        lm_ntt_inverse<LOGN>(sm, tw, c, tid, ld, st);
}
