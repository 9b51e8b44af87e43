// matrixInnerSumEval (fhe/ligero.go:299-370): per input column
//     MulNew(ct, pt) -> InnerSum(., 1, rows) -> Rescale to level 1
// batched over columns.  InnerSum is log2(rows) rounds of
//     acc += Rot(acc)       (hoisted key-switch + NTT-domain automorphism)
// with Lattigo's hybrid (RNS-digit, alpha = #P) key switching
// [LATTIGO-RECALL]:
//   1. c1 -> coefficient domain (INTT on the L limbs)
//   2. per digit d (alpha consecutive Q limbs): extend the digit to every
//      other Q limb and to the P limbs with the float64-corrected RNS
//      reconstruction, NTT each extended limb (own limbs reuse the NTT values)
//   3. (u0,u1) = sum_d digit_d (.) evk_d  over all L+K limbs
//   4. ModDown: INTT the P limbs, extend P -> Q, NTT, (u_Q - lift) * P^-1  (P^-1 pre-folded into the key)
//   5. add c0, permute both polynomials by the automorphism table, accumulate.
// Everything but the correction term v is exact modular arithmetic; v is
// decided in 128-bit integers and falls back to the literal IEEE double
// expression of the reference near a tie (this file is compiled with
// -ffp-contract=off).
//
// Kernel shapes: the NTT-bearing steps reuse the LDS-resident limb transform
// with the basis extension fused into its load phase (k_modup_ntt,
// k_moddown_ntt: the extended limb never exists in HBM in coefficient form;
// k_pack_v first turns a digit's two source words into the two words of its exact
// integer reconstruction, so that the extension is one multiplication per target);
// both kernels are dealt by XCD-aware work lists so that the targets of one digit
// share an L2; the gadget product keeps key material in Montgomery form and
// accumulates the beta products of a coefficient in 128 bits, one reduction per output.
//
// This file is one rotation of a batch of columns: its six transform and product kernels, the per-context tables and
// work lists, and the steps a caller composes:
//   rotate_decompose                  steps 1-2, on the ciphertext alone
//   rotate_product                    steps 3-4a under one key, = rotate_mac (3) then rotate_p_to_coef (4a)
//   rotate_add, rotate_store,         the three ways a decomposed rotation ends: ModDown into an accumulator, ModDown into
//   rotate_close                      a plain gather, the closing inverse transform before a rescale (lm_ks_close.hip)
//   rotate_accumulate                 rotate_decompose + rotate_add
//   rotate_add_fold, rotate_close_fold the same two endings under the c0 fold (LUMEN_KS_C0_FOLD, lm_ks_host.h): ModDown for
//                                     polynomial 1 alone, polynomial 0 rotated by the gadget product itself (k_ks_mac_fold: the
//                                     kernel's text, lm_ks_mac_kernel.h, is included twice) and its lifts folded per coefficient
// with lumen_ks_mac_probe, which times the gadget product alone.  The other subjects of the key switch live beside it:
// the batching of its callers (batches, lanes, groups, pairs of batches: lm_ks_pair.h) in lm_ks_batch.hip; the callers in lm_innersum.hip (InnerSum with
// its lazy accumulator, matrixInnerSumEval), lm_rotate.hip (lumen_automorphism, lumen_rotate_columns / _rows / _hoisted)
// and lm_mulrelin.hip (the relinearisation); where the scratch buffers sit in HBM in lm_ks_scratch.hip (mechanism) and
// lm_placement.h (policy); Galois- and relinearisation-key loading and lookup in lm_ks_key.hip; the ciphertext x
// plaintext product (step 0, MulNew) in lm_mulplain.hip; the stream layouts and mul128 in lm_ks_dev.h; and what these
// units share on the host in lm_ks_host.h.
#include <cstdlib>
#include <cstring>

#include "lm_ks_host.h"

// v = uint64(float64(y0)/float64(m0) + float64(y1)/float64(m1))  ([LATTIGO-RECALL] reconstructRNS).
// The double expression is within 2^-49 of S = A / M, A = y0*m1 + y1*m0, M = m0*m1, and S < 2: unless
// S is that close to 1 or to 2 its truncation equals [S >= 1], which is decided exactly in 128-bit
// integers; only the (probability ~2^-46) near-ties fall back to the literal double computation.
__device__ __forceinline__ u32 bx_v(u128 A, u128 M, u64 y0, u64 y1, u64 m0, u64 m1) {
    const u128 D1 = A >= M ? A - M : M - A, D2 = 2 * M - A;
    if ((u64)(D1 >> 64) >= 8 && (u64)(D2 >> 64) >= 8) return A >= M ? 1u : 0u;
    double vf = 0.0;
    vf += (double)y0 / (double)m0;
    vf += (double)y1 / (double)m1;
    return (u32)(u64)vf;
}

// (y0, y1) -> (hi, lo) of W = y0*m1 + y1*m0 + (2 - v)*M  (lm_ks_dev.h); M = m0*m1
__device__ __forceinline__ void pack_pair(u64 a, u64 b, u64 m0, u64 m1, u128 M, u64 &hi, u64 &lo) {
    u64 l1, h1, l2, h2;
    mul128(a, m1, l1, h1);
    mul128(b, m0, l2, h2);
    const u128 A = (((u128)h1 << 64) | l1) + (((u128)h2 << 64) | l2);
    const u32 v = bx_v(A, M, a, b, m0, m1);
    const u128 W = A + (v == 0 ? 2 * M : (v == 1 ? M : (u128)0)); // + (2 - v) * M, v <= 2
    hi = (u64)(W >> LM_W_SPLIT), lo = (u64)W & ((1ull << LM_W_SPLIT) - 1);
}

// (y0, y1)[b][i] -> (hi, lo) of W = y0*m1 + y1*m0 + (2 - v)*M for every two-limb source group
// (lm_ks_dev.h).  y: [npoly][stride] with the group's two limbs at limb offsets lo, lo+1.
// One thread per PAIR of coefficients (16-byte accesses); the group is uniform per workgroup row.
__global__ __launch_bounds__(256) void k_pack_v(u64 *__restrict__ y, size_t poly_stride, uint32_t npoly,
                                                uint32_t ngroups, uint32_t group_limbs, uint32_t first_mod,
                                                uint32_t nlimbs_total, uint32_t logN, lm_mods mods) {
    const uint32_t N = 1u << logN;
    const size_t total = (size_t)npoly * ngroups * (N / 2), stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint32_t i = (uint32_t)(g & (N / 2 - 1)) * 2;
        const uint32_t grp = (uint32_t)((g >> (logN - 1)) % ngroups), p = (uint32_t)((g >> (logN - 1)) / ngroups);
        const uint32_t l0 = grp * group_limbs;
        if (l0 + 1 >= nlimbs_total) continue; // single-limb group: nothing to reconstruct
        u64 *y0 = y + (size_t)p * poly_stride + (size_t)l0 * N + i;
        const ulonglong2 av = *reinterpret_cast<const ulonglong2 *>(y0);
        const ulonglong2 bv = *reinterpret_cast<const ulonglong2 *>(y0 + N);
        const u64 m0 = mods.m[first_mod + l0].q, m1 = mods.m[first_mod + l0 + 1].q;
        u64 Ml, Mh;
        mul128(m0, m1, Ml, Mh);
        const u128 M = ((u128)Mh << 64) | Ml;
        ulonglong2 hv, lv;
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const u64 a = e ? av.y : av.x, b = e ? bv.y : bv.x;
            u64 hi, lo;
            pack_pair(a, b, m0, m1, M, hi, lo);
            if (e) hv.y = hi, lv.y = lo;
            else hv.x = hi, lv.x = lo;
        }
        *reinterpret_cast<ulonglong2 *>(y0) = hv;
        *reinterpret_cast<ulonglong2 *>(y0 + N) = lv;
    }
}

// ---- step 1, partly fused: c1 to the coefficient domain, and for the first `nf` two-limb digits the
// (hi, lo) packing as well.  Workgroups [0, B * nf): one per (column, digit), both limbs' inverse
// transforms back to back; the lane that wrote y0[i] reads it back (from L2) when y1[i] leaves its
// registers -- in the cross-wave last pass every lane sees the same coefficient indices whatever the limb --
// and the pair skips k_pack_v's round trip through HBM.  Workgroups behind them: one inverse transform
// each, for the limbs of the remaining digits (packed by k_pack_v as before).
// Why not fuse all digits: B * beta pairs are 1.5 rounds of the 256 CUs at B = 64 (measured: 246 ms per
// step against 152 + 60).  With nf = 4 the fused pairs are exactly one round and the 256 single
// transforms fill in behind them as the pairs finish -- the launch is as long as three rounds of single
// transforms, and two thirds of the packing pass are gone.
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_lds(LOGN)) void k_intt_pack(const u64 *__restrict__ acc, u64 *coef, uint32_t B,
                                                                  uint32_t L, uint32_t nf, lm_mods mods,
                                                                  lm_ninv_t yscale, const tw_t *__restrict__ tw_all) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x >= B * nf) { // a limb of an unfused digit: limb-major, as k_limb_ntt
        const uint32_t k = blockIdx.x - B * nf, l = 2 * nf + k / B, b = k % B;
        const u64 *p = acc + (((size_t)b * 2 + 1) * L + l) * N;
        u64 *o = coef + ((size_t)b * L + l) * N;
        const lm_qc q = lm_make_qc(mods.m[l]);
        const tw_t sc = yscale.t[l];
        auto ld = [&](uint32_t i0, u64 *v, int count) { lm_load_run(p, i0, v, count); };
        auto st = [&](uint32_t i, u64 v) { o[i] = lm_shoup_cs(v, sc, q.q, q.nq); };
        lm_ntt_inverse<LOGN>(sm, tw_all + (size_t)l * N, q, tid, ld, st);
        return;
    }
    const uint32_t d = blockIdx.x / B, b = blockIdx.x % B; // digit-major: two twiddle tables hot per XCD
    const uint32_t l0 = 2 * d, l1 = l0 + 1;
    const u64 *c1 = acc + ((size_t)b * 2 + 1) * L * N; // c1 of column b
    u64 *o0 = coef + ((size_t)b * L + l0) * N;
    const lm_qc q0 = lm_make_qc(mods.m[l0]);
    const tw_t s0 = yscale.t[l0];
    { // first limb: y0 to its place in coef
        const u64 *p = c1 + (size_t)l0 * N;
        auto ld = [&](uint32_t i0, u64 *v, int count) { lm_load_run(p, i0, v, count); };
        auto st = [&](uint32_t i, u64 v) { o0[i] = lm_shoup_cs(v, s0, q0.q, q0.nq); };
        lm_ntt_inverse<LOGN>(sm, tw_all + (size_t)l0 * N, q0, tid, ld, st);
    }
    __syncthreads(); // the second transform reuses the LDS
    {
        const lm_qc q1 = lm_make_qc(mods.m[l1]);
        const tw_t s1 = yscale.t[l1];
        const u64 *p = c1 + (size_t)l1 * N;
        u64 Ml, Mh;
        mul128(q0.q, q1.q, Ml, Mh);
        // the product is uniform but comes out of the vector multiplier: back to SGPRs, or it sits in
        // eight VGPRs through the whole transform
        auto uni = [](u64 x) {
            return (u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x) |
                   (u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32;
        };
        const u128 M = ((u128)uni(Mh) << 64) | uni(Ml);
        auto ld = [&](uint32_t i0, u64 *v, int count) { lm_load_run(p, i0, v, count); };
        // the y0 words of a work item of the last pass are read back before its butterflies (pre) and are
        // there when the y1 words come out of them
        constexpr int R_LAST = lm_pass_r(LOGN, 0), LOG_T0 = LOGN - R_LAST;
        constexpr int PF = (1 << R_LAST) * 5 / 8; // words requested ahead: 16 of 16 spill 14 VGPRs, 12 of 16 two
        struct pack_t {
            u64 *o0;
            const lm_qc &q0, &q1;
            tw_t s1;
            u128 M;
            u64 y0[PF];
            __device__ __forceinline__ void pre(uint32_t w) {
#pragma unroll
                for (int k = 0; k < PF; k++) y0[k] = o0[w + ((uint32_t)k << LOG_T0)];
            }
            __device__ __forceinline__ void operator()(uint32_t i, u64 v, int k) {
                const u64 y1 = lm_shoup_cs(v, s1, q1.q, q1.nq);
                // the index is made opaque so that the addresses of the pass are formed one pair at a time
                // (computed ahead, beside the y0 words, they spill)
                uint32_t j = i;
                asm volatile("" : "+v"(j));
                const u64 a = k < PF ? y0[k < PF ? k : 0] : o0[j];
                u64 hi, lo;
                pack_pair(a, y1, q0.q, q1.q, M, hi, lo);
                o0[j] = hi, o0[j + N] = lo;
                if (k >= PF && (k & 1)) asm volatile("" ::: "memory"); // two late read-backs in flight
            }
        } st{o0, q0, q1, s1, M, {}};
        uint32_t tid1 = tid; // nothing derived from the lane index is carried over from the first limb
        asm volatile("" : "+v"(tid1));
        lm_ntt_inverse<LOGN>(sm, tw_all + (size_t)l1 * N, q1, tid1, ld, st);
    }
}

// ---- step 2: digit extension + NTT.  One workgroup per (column b, digit d, target t).
// coef: [B][L][N] coefficient-domain c1; acc: [B][2][L][N] (c1 NTT values for own limbs); ext: [L+K][B][beta][N] (ks_ext_at)
// L is the level the rotation runs at (KsTables::nl) and a target t a POSITION in [0, L + K): the Q limbs of the level,
// then the limbs modulo P, whose moduli and twiddle tables sit `pshift` = (the context's L) - L entries further on
// (ks_mod_at; 0 at the top level).
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_fwd(LOGN)) void k_modup_ntt(const u64 *__restrict__ coef, const u64 *__restrict__ acc,
                                                    u64 *__restrict__ ext, const bx_t *__restrict__ bx,
                                                    uint32_t B, uint32_t L, uint32_t K, uint32_t beta, uint32_t pshift,
                                                    const uint32_t *__restrict__ work, lm_mods mods,
                                                    const tw_t *__restrict__ tw_all) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x, LK = L + K;
    // The grid only holds the (column, digit, target) triples that need an extension (a digit's own
    // limbs reuse the NTT-domain c1), in the order of a host-built work list (modup_work_list): XCD-
    // aware, so that the targets of one digit run back to back on one XCD and share its L2.
    // (a split degree: two workgroups per work-list entry, one per half of the target limb -- the packed words have no
    // spare bit, the half comes from the grid: lm_half_of_block)
    const lm_half<LOGN> hf = lm_half_of_block<LOGN>();
    const uint32_t wk = work[hf.block];
    const uint32_t b = wk & 0xFFFF, d = (wk >> 16) & 0xFF, t = wk >> 24; // t: target position (Q limbs then P limbs)
    const uint32_t mt = ks_mod_at(t, L, pshift);                         // its modulus: wave-uniform, as t is
    const bx_t c = bx[d * LK + t];
    u64 *o = ext + ks_ext_at(b, d, t, B, beta) * N + hf.off;
    const lm_qc qc = lm_make_qc(mods.m[mt]);
    const u64 *s0 = coef + ((size_t)b * L + d * K) * N;
    const u64 *s1 = c.ns == 2 ? s0 + N : s0; // second limb of the digit
    auto ld = [&](uint32_t i) { return bx_apply(c, s0[i], s1[i], qc); };
    // the extended digit is stored as it leaves the last butterfly (any value below 2^64): the gadget
    // product accumulates beta products x * k, k < q, in 128 bits (beta * 2^64 * q < 2^127: at most
    // 12 digits of moduli below 2^58.4) and its reduction takes any such sum
    // coalesced stores through the wave's own LDS block (lm_linear_out): -3.5 % on this kernel at N = 2^14 against one 64-byte run per
    // lane straight from the registers (tools/exp_modup_run_store.patch, profiles/r05_exp_linear_store.txt)
    auto out = [&](uint32_t j, u64 v0, u64 v1) {
        ulonglong2 y;
        y.x = v0, y.y = v1;
        *reinterpret_cast<ulonglong2 *>(o + j) = y;
    };
    if constexpr (LOGN == 14) { // limb in registers, two workgroups per CU: the runs go through the wave's slot, half by half
        lm_w14_runs st{sm};
        auto after = [&](uint32_t i0, uint32_t) { lm_w14_linear_out(sm, tid, i0, out); };
        lm_ntt_forward_w14(sm, tw_all + (size_t)mt * N, qc, tid, ld, st, after);
    } else { // (a split degree: the half transform, the extension fused into both loads of the outer butterfly)
        lm_lds_runs st{sm};
        auto after = [&](uint32_t, uint32_t) { lm_linear_out<lm_tlog(LOGN)>(sm, tid, out); };
        lm_ntt_forward_half<LOGN>(sm, tw_all + (size_t)mt * N, qc, tid, hf, ld, st, after);
    }
}

// ---- step 3: gadget product.  u[b][w][t][i] = sum_d ext[b][d][t][i] * key[d][w][t][i]  (storage: ks_u_at, ks_ext_at, ks_key_at)
// key in Montgomery form (k * 2^64 mod q): 128-bit accumulation, one Montgomery reduction.
// L, beta: of the level the rotation runs at; the key is the stored one, [ctx L + K][key_beta][2] with the top level's
// digit count, of which a lower level reads digits d < beta at the moduli of its positions (ks_mod_at).
// COLS columns share one read of the key limb (the key is re-read B/COLS times per launch, out of
// L2 / Infinity Cache); VEC consecutive coefficients per thread move as one VEC*8-byte access.
#ifndef LM_MAC_COLS
#define LM_MAC_COLS 4
#endif
#ifndef LM_MAC_VEC
#define LM_MAC_VEC 1
#endif
#ifndef LM_MAC_PREFETCH
#define LM_MAC_PREFETCH 1
#endif
template <int VEC>
struct mac_vec;
template <>
struct mac_vec<1> {
    u64 v[1];
    static __device__ __forceinline__ mac_vec load(const u64 *p) { return mac_vec{{*p}}; }
    // read-once streams (the extended digits): do not displace what later kernels will re-read
    static __device__ __forceinline__ mac_vec load_once(const u64 *p) { return mac_vec{{__builtin_nontemporal_load(p)}}; }
    __device__ __forceinline__ void store(u64 *p) const { *p = v[0]; }
};
template <>
struct mac_vec<2> {
    u64 v[2];
    static __device__ __forceinline__ mac_vec load(const u64 *p) {
        const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(p);
        return mac_vec{{a.x, a.y}};
    }
    static __device__ __forceinline__ mac_vec load_once(const u64 *p) {
        return mac_vec{{__builtin_nontemporal_load(p), __builtin_nontemporal_load(p + 1)}};
    }
    __device__ __forceinline__ void store(u64 *p) const {
        ulonglong2 a;
        a.x = v[0], a.y = v[1];
        *reinterpret_cast<ulonglong2 *>(p) = a;
    }
};
// One accumulator of the gadget product: sum of 64x64-bit products kept as three 64-bit columns
// (weights 1, 2^32, 2^64) plus counters of the carries out of the first two, so that a product costs
// four multiply-adds and three add-with-carry -- the compiler's 128-bit accumulate costs ~29
// instructions, and this kernel is co-limited by VALU issue and HBM.
// The third column only takes x1 * k1 with k < q < 2^58.4: no carry for up to 32 terms.
struct mac_acc {
    u64 a0, a1, a3;
    u32 c0, c1;
    __device__ __forceinline__ void clear() { a0 = a1 = a3 = 0, c0 = c1 = 0; }
    __device__ __forceinline__ void value(u64 &lo, u64 &hi) const {
        lo = a0 + (a1 << 32);
        hi = a3 + c0 + (a1 >> 32) + ((u64)c1 << 32) + (lo < a0 ? 1 : 0);
    }
};
// p += x * k0, q += x * k1 (the two polynomials of the key share the digit x).  gfx950 needs two
// wait states between a VALU write of an SGPR pair (a carry) and the VALU read of it.
__device__ __forceinline__ void mac2(mac_acc &p, mac_acc &q, u64 x, u64 k0, u64 k1) {
    const u32 x0 = (u32)x, x1 = (u32)(x >> 32);
#if LM_ASM_SHOUP
    asm("v_mad_u64_u32 %[pa0], s[98:99], %[x0], %[k00], %[pa0]\n\t"
        "v_mad_u64_u32 %[qa0], s[90:91], %[x0], %[k10], %[qa0]\n\t"
        "v_mad_u64_u32 %[pa1], s[94:95], %[x0], %[k01], %[pa1]\n\t"
        "v_addc_co_u32_e64 %[pc0], s[96:97], %[pc0], 0, s[98:99]\n\t"
        "v_mad_u64_u32 %[qa1], s[92:93], %[x0], %[k11], %[qa1]\n\t"
        "v_addc_co_u32_e64 %[qc0], s[96:97], %[qc0], 0, s[90:91]\n\t"
        "v_mad_u64_u32 %[pa3], s[96:97], %[x1], %[k01], %[pa3]\n\t"
        "v_addc_co_u32_e64 %[pc1], s[96:97], %[pc1], 0, s[94:95]\n\t"
        "v_mad_u64_u32 %[pa1], s[98:99], %[x1], %[k00], %[pa1]\n\t"
        "v_addc_co_u32_e64 %[qc1], s[96:97], %[qc1], 0, s[92:93]\n\t"
        "v_mad_u64_u32 %[qa1], s[90:91], %[x1], %[k10], %[qa1]\n\t"
        "v_mad_u64_u32 %[qa3], s[96:97], %[x1], %[k11], %[qa3]\n\t"
        "v_addc_co_u32_e64 %[pc1], s[96:97], %[pc1], 0, s[98:99]\n\t"
        "v_addc_co_u32_e64 %[qc1], s[96:97], %[qc1], 0, s[90:91]"
        : [pa0] "+v"(p.a0), [pa1] "+v"(p.a1), [pa3] "+v"(p.a3), [pc0] "+v"(p.c0), [pc1] "+v"(p.c1),
          [qa0] "+v"(q.a0), [qa1] "+v"(q.a1), [qa3] "+v"(q.a3), [qc0] "+v"(q.c0), [qc1] "+v"(q.c1)
        : [x0] "v"(x0), [x1] "v"(x1), [k00] "v"((u32)k0), [k01] "v"((u32)(k0 >> 32)), [k10] "v"((u32)k1),
          [k11] "v"((u32)(k1 >> 32))
        : "s92", "s93", "s94", "s95", "s96", "s97", "s98", "s99", "s90", "s91");
#else
    auto one = [&](mac_acc &r, u64 k) {
        const u32 k0w = (u32)k, k1w = (u32)(k >> 32);
        u64 t = r.a0 + (u64)x0 * k0w;
        r.c0 += t < r.a0, r.a0 = t;
        t = r.a1 + (u64)x0 * k1w;
        r.c1 += t < r.a1, r.a1 = t;
        t = r.a1 + (u64)x1 * k0w;
        r.c1 += t < r.a1, r.a1 = t;
        r.a3 += (u64)x1 * k1w;
    };
    one(p, k0);
    one(q, k1);
#endif
}

// the kernel twice, out of one text (lm_ks_mac_kernel.h): k_ks_mac, and k_ks_mac_fold with the c0 fold in its epilogue
#define LM_KS_MAC_FOLD 0
#include "lm_ks_mac_kernel.h"
#undef LM_KS_MAC_FOLD
#define LM_KS_MAC_FOLD 1
#include "lm_ks_mac_kernel.h"
#undef LM_KS_MAC_FOLD

// ---- steps 4+5: ModDown, add c0, automorphism, accumulate.  One workgroup per (column b,
// poly w, Q limb t): the lift of the (coefficient-domain) P limbs into q_t is fused into the load,
// the NTT runs in LDS, d = (u_t - lift) * P^-1 (+ c0 for w == 0) is formed in the last pass and
// parked in LDS; then every wave writes one block of the new accumulator limb linearly,
// acc_out[j] = acc_in[j] + d[index[j]], the automorphism being a gather out of the wave's own LDS block.  (acc is
// ping-ponged: an output needs the old accumulator at two positions, j and index[j].)
// N = 2^14: the limb stays in registers (lm_ntt_forward_w14, 512 threads, two workgroups per CU); the last pass only
// parks its raw outputs in the wave's slot, and d is formed there, half a wave's block at a time, right before that
// half is gathered (see the LOGN == 14 branch).
// The two kernels below share this body.  ACCUMULATE (k_moddown_ntt): as described, acc_out = acc_in + d o index, lazy.
// Without it (k_rotdown_ntt, the rotation alone: lumen_automorphism) acc_in is the ciphertext itself, read once, linearly,
// for the c0 that goes into d, and the gather store is acc_out[j] = d[index[j]] in canonical form: d < 6q comes under q
// with three conditional subtractions (4q, 2q, q), and no second read of acc_in at the output positions stands beside it.
template <int LOGN, bool ACCUMULATE>
__device__ __forceinline__ void moddown_body(const u64 *__restrict__ u, const u64 *__restrict__ acc_in,
                                             u64 *__restrict__ acc_out, const bx_t *__restrict__ bxp,
                                             const tw_t *__restrict__ pinv,
                                             const uint32_t *__restrict__ index,
                                             const uint32_t *__restrict__ inv_index,
                                             const uint32_t *__restrict__ work, uint32_t B,
                                             uint32_t L, uint32_t K, const lm_mods &mods,
                                             const tw_t *__restrict__ tw_all) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x;
    // host-built, XCD-aware order (moddown_work_list): the Q limbs of one polynomial, which all lift the
    // same two P-limb words, run back to back on one XCD
    const lm_half<LOGN> hf = lm_half_of_block<LOGN>(); // a split degree: two workgroups per entry, one per half
    const uint32_t wk = work[hf.block];
    const uint32_t pw = wk & 0xFFFF; // b*2 + w
    const uint32_t t = wk >> 16;
    const uint32_t w = pw & 1;
    const bx_t c = bxp[t];
    const lm_qc qc = lm_make_qc(mods.m[t]);
    const u64 *up0 = u + ks_u_at(pw, L, B, L, K) * N; // P limbs of u, coefficient domain
    const u64 *up1 = c.ns == 2 ? up0 + N : up0;
    const u64 *uq = u + ks_u_at(pw, t, B, L, K) * N;
    const u64 *ain = acc_in + ((size_t)pw * L + t) * N; // c0 (w == 0) / c1 (w == 1) limb of the accumulator
    u64 *aout = acc_out + ((size_t)pw * L + t) * N;
    // -P^-1 as a Shoup constant: (q - w, ~w') -- floor((q - w) * 2^64 / q) = 2^64 - 1 - floor(w * 2^64 / q) for
    // w * 2^64 not a multiple of q -- so that u' - lift * P^-1 is ONE multiply-add with u' in the addend slot
    tw_t pi = pinv[t];
    pi.w = qc.q - pi.w, pi.wp = ~pi.wp;
    auto ld = [&](uint32_t i) { return bx_apply(c, up0[i], up1[i], qc); };
    if constexpr (LOGN == 14) {
        // Limb in registers, two workgroups per CU.  The storer is the extension kernel's (lm_w14_runs: the raw outputs
        // of the last butterflies, any u64, go to the wave's slot; no pre(), no arithmetic), which is what leaves the
        // last pass its registers.  `after` runs once per half h = i0h >> 10 of the wave's block, on the wave's own slot:
        //  (a) combine, in place.  Lane pairs on consecutive words (the addressing of lm_w14_linear_out): coefficients
        //      i, i + 1 with i = wave << 11 | i0h | 2 lane + 128 k get slot = slot * (-P^-1) + u' (+ c0 for w == 0) -- the
        //      multiply-add of the LDS form's storer below on the same operands, so d < 6q as there; u' and c0 arrive as
        //      16-byte words, one contiguous kilobyte per load instruction;
        //  (b) gather.  In the bit-reversed order of the NTT domain an automorphism X -> X^g permutes BLOCKS onto blocks:
        //      position i evaluates at psi^e, e = 2 bitrev(i) + 1; the low b + 1 bits of g e mod 2N only depend on the
        //      low b + 1 bits of e, i.e. on the TOP b bits of i -- so the top b bits of index[i] are a function (a
        //      bijection) of the top b bits of i, for every b.  With b = 4 the unit is 1024 coefficients, and in the w14
        //      layout half h of wave `wave` is exactly the aligned block sb = 2 wave + h (bits 13..11 = wave, bit 10 = h):
        //      the output block jb = inv_index[sb * 1024] >> 10 gathers from this half and from nothing else,
        //      acc_out[j] = acc_in[j] + slot[index[j] & 1023] for the 1024 j of block jb.
        // Both block numbers are fetched before the transform, so that no dependent load sits in `after`.  (The half's
        // index words requested before its combine instead of after it: measured, no difference -- EXPERIMENTS R10.)
        const uint32_t wave = tid >> 6, lane = tid & 63;
        const uint32_t jb0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(inv_index[(2 * wave) << 10] >> 10));
        const uint32_t jb1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(inv_index[(2 * wave + 1) << 10] >> 10));
        lm_w14_runs st{sm};
        auto after = [&](uint32_t i0h, uint32_t) {
            const uint32_t pb = LM_PAD((wave << 10) | (2 * lane));
            // (in chunks of CH pairs, fenced: the 16 words of a whole half's u' and c0 beside e[16..31], still live for
            // h = 0, and the scheduler's hoisting of phase (b)'s loads over them spill 9 VGPRs)
            constexpr uint32_t CH = 4;
            const uint32_t i = (wave << 11) | i0h | (2 * lane);
            const uint32_t jb = i0h ? jb1 : jb0, sbase = wave << 10;
#pragma unroll
            for (uint32_t k0 = 0; k0 < 8; k0 += CH) {
                ulonglong2 uv[CH], cv[CH];
#pragma unroll
                for (uint32_t k = 0; k < CH; k++) {
                    uv[k] = *reinterpret_cast<const ulonglong2 *>(uq + i + 128 * (k0 + k));
                    if (w == 0) cv[k] = *reinterpret_cast<const ulonglong2 *>(ain + i + 128 * (k0 + k));
                }
#pragma unroll
                for (uint32_t k = 0; k < CH; k++) {
                    // u' - lift * P^-1 = u' + lift * (-P^-1), nothing reduced: see the storer of the LDS form
                    const uint32_t p = lm_w14_at(pb, 128 * (k0 + k));
                    const u64 a0 = w == 0 ? uv[k].x + cv[k].x : uv[k].x, a1 = w == 0 ? uv[k].y + cv[k].y : uv[k].y;
                    sm[p] = lm_shoup3<true>(sm[p], pi.w, pi.wp, qc.nq, a0);
                    sm[p + 1] = lm_shoup3<true>(sm[p + 1], pi.w, pi.wp, qc.nq, a1);
                }
                LM_W14_FENCE();
            }
            lm_wave_sync();
            uint2 p[8];
            ulonglong2 x[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                const uint32_t j = (jb << 10) + 2 * lane + k * 128;
                p[k] = *reinterpret_cast<const uint2 *>(index + j);
                if constexpr (ACCUMULATE) x[k] = *reinterpret_cast<const ulonglong2 *>(ain + j);
            }
#pragma unroll
            for (uint32_t k = 0; k < 8; k++) {
                const uint32_t j = (jb << 10) + 2 * lane + k * 128;
                ulonglong2 y;
                if constexpr (ACCUMULATE) {
                    // lazy accumulator: acc (< 2q) + d (< 6q) < 8q back under 2q, as in the LDS form below
                    y.x = lm_csub(lm_csub(x[k].x + sm[LM_PAD(sbase | (p[k].x & 1023u))], 4 * qc.q), 2 * qc.q);
                    y.y = lm_csub(lm_csub(x[k].y + sm[LM_PAD(sbase | (p[k].y & 1023u))], 4 * qc.q), 2 * qc.q);
                } else { // d < 6q alone, canonical
                    y.x = lm_csub(lm_csub(lm_csub(sm[LM_PAD(sbase | (p[k].x & 1023u))], 4 * qc.q), 2 * qc.q), qc.q);
                    y.y = lm_csub(lm_csub(lm_csub(sm[LM_PAD(sbase | (p[k].y & 1023u))], 4 * qc.q), 2 * qc.q), qc.q);
                }
                *reinterpret_cast<ulonglong2 *>(aout + j) = y;
            }
        };
        lm_ntt_forward_w14(sm, tw_all + (size_t)t * N, qc, tid, ld, st, after);
    } else {
        // the store phase combines every finished run of 8 with the gadget product u (and c0 for w == 0): both
        // are requested by pre() before the run's butterflies, not after them
        // A split degree: this workgroup owns half hf.h of the limb, NTT-domain positions [hf.off, hf.off + N/2), as the
        // output of a transform of TLOG = LOGN - 1 stages.  The storer's pointers start at the half; the gather below
        // works on blocks of the WHOLE limb (wave `wave` has left block hf.off / BLK + wave in LDS, at local positions).
        constexpr int TLOG = lm_tlog(LOGN);
        constexpr int RUN = lm_fwd_run<TLOG>();
        static_assert(RUN <= 8, "lm_load_run moves at most 8 coefficients");
        struct storer_t {
            const u64 *uq, *ain;
            u64 *sm;
            const lm_qc &qc;
            tw_t pi;
            uint32_t w;
            u64 uv[RUN], cv[RUN];
            __device__ __forceinline__ void pre(uint32_t i0) {
                lm_load_run(uq, i0, uv, RUN);
                if (w == 0) lm_load_run(ain, i0, cv, RUN);
            }
            __device__ __forceinline__ void operator()(uint32_t i0, const u64 *v, int count) {
#pragma unroll
                for (int k = 0; k < RUN; k++)
                    if (k < count) {
                        // u' - lift * P^-1 = u' + lift * (-P^-1) (u' = u * P^-1 < q comes out of the gadget product, see
                        // lumen_load_galois_key); the multiplication takes the unreduced lift and leaves [0, 3q) on top
                        // of its addend: u' (+ c0 < 2q for w == 0).  NOTHING is reduced here -- d < 6q goes to LDS as it
                        // is, and the one reduction of a rotation happens where the accumulator word is formed (below).
                        const u64 add = w == 0 ? uv[k] + cv[k] : uv[k];
                        sm[LM_PAD(i0 + k)] = lm_shoup3<true>(v[k], pi.w, pi.wp, qc.nq, add); // the slots this work item just consumed
                    }
            }
        } st{uq + hf.off, ain + hf.off, sm, qc, pi, w, {}, {}};
        // acc_out[j] = acc_in[j] + d[index[j]]: the automorphism is applied as a gather out of LDS, so the
        // accumulator itself streams through HBM linearly in 16-byte vectors.
        // NO workgroup barrier (round 5).  In the bit-reversed order of the NTT domain an automorphism X -> X^g permutes
        // BLOCKS onto blocks: position i evaluates at psi^e, e = 2 bitrev(i) + 1; the low b + 1 bits of g e mod 2N only
        // depend on the low b + 1 bits of e, i.e. on the TOP b bits of i -- so the top b bits of index[i] are a function
        // (a bijection) of the top b bits of i, for every b.  With b = log2(waves): every output block of N / waves
        // coefficients gathers from exactly ONE source block, the one a single wave has just left in LDS.  Wave w
        // therefore serves output block jb = inv_index[w * BLK] / BLK as soon as ITS OWN last pass is done (a wave's LDS
        // operations execute in order) and goes home; the waves of a workgroup finish up to 12 us apart
        // (profiles/r02_ubench_phases.txt), and the barrier this replaces made the early ones wait for the last.
        // Every lane handles 8 pairs; only the block number jb is fetched early -- the pairs' index and accumulator words are
        // requested in `after`, once the wave's last pass is done (ahead of it they cost 48 VGPRs the last pass needs).
        // (a split degree: with the whole half as the block the same argument says that output half inv_index[h N/2] / (N/2)
        // gathers from input half h alone -- in place for g = 1 mod 4, swapped for g = 3 mod 4, the row swap 2N - 1 among them)
        constexpr uint32_t NW = lm_nthreads(TLOG) / 64, BLK = (1u << TLOG) / NW, IT = BLK / 128;
        const uint32_t wave = tid >> 6, lane = tid & 63;
        const uint32_t jb = NW > 1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(inv_index[hf.off + wave * BLK] / BLK)) : 0u;
        auto after = [&](uint32_t, uint32_t) {
            uint2 p[IT];
            ulonglong2 x[IT];
#pragma unroll
            for (uint32_t k = 0; k < IT; k++) {
                const uint32_t j = jb * BLK + 2 * lane + k * 128;
                p[k] = *reinterpret_cast<const uint2 *>(index + j);
                if constexpr (ACCUMULATE) x[k] = *reinterpret_cast<const ulonglong2 *>(ain + j);
            }
            lm_wave_sync();
#pragma unroll
            for (uint32_t k = 0; k < IT; k++) {
                const uint32_t j = jb * BLK + 2 * lane + k * 128;
                // the accumulator is LAZY across the rotations of an InnerSum: words in [0, 2q).  acc (< 2q) + d (< 6q)
                // < 8q comes back under 2q with two conditional subtractions -- the only ones of the kernel (the
                // canonical form cost four per coefficient of c0 and three of c1: d to [0, q), + c0, + acc).  Its
                // readers take [0, 2q): the inverse transform's loader (< 3q), the gadget product's own-digit operand
                // (any u64), this kernel, and the rescale that ends matrixInnerSumEval (lm_rescale.hip).
                ulonglong2 y;
                if constexpr (ACCUMULATE) {
                    y.x = lm_csub(lm_csub(x[k].x + sm[LM_PAD(lm_half_local<LOGN>(p[k].x))], 4 * qc.q), 2 * qc.q);
                    y.y = lm_csub(lm_csub(x[k].y + sm[LM_PAD(lm_half_local<LOGN>(p[k].y))], 4 * qc.q), 2 * qc.q);
                } else { // the rotation alone: d < 6q, canonical -- no k_acc_canon pass follows
                    y.x = lm_csub(lm_csub(lm_csub(sm[LM_PAD(lm_half_local<LOGN>(p[k].x))], 4 * qc.q), 2 * qc.q), qc.q);
                    y.y = lm_csub(lm_csub(lm_csub(sm[LM_PAD(lm_half_local<LOGN>(p[k].y))], 4 * qc.q), 2 * qc.q), qc.q);
                }
                *reinterpret_cast<ulonglong2 *>(aout + j) = y;
            }
        };
        lm_ntt_forward_half<LOGN>(sm, tw_all + (size_t)t * N, qc, tid, hf, ld, st, after);
    }
}

#define LM_MODDOWN_PARAMS                                                                                                      \
    const u64 *__restrict__ u, const u64 *__restrict__ acc_in, u64 *__restrict__ acc_out, const bx_t *__restrict__ bxp,        \
        const tw_t *__restrict__ pinv, const uint32_t *__restrict__ index, const uint32_t *__restrict__ inv_index,             \
        const uint32_t *__restrict__ work, uint32_t B, uint32_t L, uint32_t K, lm_mods mods, const tw_t *__restrict__ tw_all
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_fwd(LOGN)) void k_moddown_ntt(LM_MODDOWN_PARAMS) {
    moddown_body<LOGN, true>(u, acc_in, acc_out, bxp, pinv, index, inv_index, work, B, L, K, mods, tw_all);
}
// ModDown that ends in a plain gather: out = sigma_g(c0 + k0, k1), canonical; acc_in = the input ciphertexts, acc_out = the
// output set (another block: a workgroup's output block is another workgroup's c0)
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_fwd(LOGN)) void k_rotdown_ntt(LM_MODDOWN_PARAMS) {
    moddown_body<LOGN, false>(u, acc_in, acc_out, bxp, pinv, index, inv_index, work, B, L, K, mods, tw_all);
}

// -------------------------------------------------------------------- host side
namespace {

bx_t make_bx(const uint64_t *src, uint32_t ns, uint64_t t) {
    bx_t c;
    memset(&c, 0, sizeof(c));
    c.ns = ns;
    uint64_t m_mod_t = 1;
    for (uint32_t a = 0; a < ns; a++) m_mod_t = h_mulmod(m_mod_t, src[a] % t, t);
    c.b57 = h_tw((1ull << LM_W_SPLIT) % t, t);
    c.c_t = (t - h_mulmod(2 % t, m_mod_t, t)) % t;
    return c;
}

// (M/m_a)^-1 mod m_a for source a of the group src[0..ns)
uint64_t hat_inv(const uint64_t *src, uint32_t ns, uint32_t a) {
    uint64_t h = 1;
    for (uint32_t b = 0; b < ns; b++)
        if (b != a) h = h_mulmod(h, src[b] % src[a], src[a]);
    return h_invmod(h, src[a]);
}

} // namespace

int get_tables(lumen_ctx *ctx, KsTables **out) { return get_tables_at(ctx, ctx->L, out); }

// Level nl of the chain: digits d = limbs [dK, min(dK + K, nl)) -- for K = 2 and odd nl the last one is the single
// limb nl - 1, which a higher level pairs with limb nl, so its constants are the level's own -- extended to the
// positions [0, nl + K) of ks_mod_at.  The tables of the top level stay under the name (and with the contents) they
// always had; a lower level's are "ks_tables:<nl>".
int get_tables_at(lumen_ctx *ctx, uint32_t nl, KsTables **out) {
    LM_SHARED_LOCK(ctx);
    LM_CHECK(ctx, nl >= 1 && nl <= ctx->L, "key switch at %u limbs: the chain has %u", nl, ctx->L);
    const std::string name = nl == ctx->L ? std::string("ks_tables") : "ks_tables:" + std::to_string(nl);
    auto it = ctx->ext.find(name);
    if (it != ctx->ext.end()) {
        *out = static_cast<KsTables *>(it->second.get());
        return 0;
    }
    const uint32_t L = nl, K = ctx->K, LK = L + K, pshift = ctx->L - nl, ctxLK = ctx->L + K;
    LM_CHECK(ctx, K >= 1 && K <= 2, "key switching supports 1 or 2 special primes (have %u)", K);
    auto sp = std::make_shared<KsTables>();
    KsTables &tb = *sp;
    tb.nl = L;
    tb.beta = (L + K - 1) / K;
    std::vector<bx_t> bx((size_t)tb.beta * LK);
    for (uint32_t d = 0; d < tb.beta; d++) {
        const uint32_t lo = d * K, hi = std::min(lo + K, L), ns = hi - lo;
        for (uint32_t t = 0; t < LK; t++) {
            bx_t c = make_bx(ctx->mod + lo, ns, ctx->mod[ks_mod_at(t, L, pshift)]);
            c.own = (t >= lo && t < hi) ? 1 : 0;
            bx[(size_t)d * LK + t] = c;
        }
    }
    // (by modulus index, as the inverse transforms read it: the limbs modulo P at the context's L + a)
    for (uint32_t i = 0; i < LM_MAX_LIMBS; i++) tb.yscale.t[i] = ctx->ninv[i < ctxLK ? i : 0];
    for (uint32_t d = 0; d < tb.beta; d++) {
        const uint32_t lo = d * K, hi = std::min(lo + K, L), ns = hi - lo;
        for (uint32_t a = 0; a < ns; a++) {
            const uint64_t m = ctx->mod[lo + a];
            tb.yscale.t[lo + a] = h_tw(h_mulmod(ctx->ninv[lo + a].w, hat_inv(ctx->mod + lo, ns, a), m), m);
        }
    }
    for (uint32_t a = 0; a < K; a++) {
        const uint64_t m = ctx->mod[ctx->L + a];
        tb.yscale.t[ctx->L + a] = h_tw(h_mulmod(ctx->ninv[ctx->L + a].w, hat_inv(ctx->mod + ctx->L, K, a), m), m);
    }
    std::vector<bx_t> bxp(L);
    std::vector<tw_t> pinv(L);
    for (uint32_t t = 0; t < L; t++) {
        bxp[t] = make_bx(ctx->mod + ctx->L, K, ctx->mod[t]);
        const uint64_t q = ctx->mod[t];
        pinv[t] = h_tw(h_invmod(h_p_mod(ctx, q), q), q);
    }
    // the c0 fold: 2M and the bound of a lift, |W - 2M| < 2M (K == 2) or the residue itself, < p (K == 1); S modulo q_t
    {
        unsigned __int128 M = 1;
        for (uint32_t a = 0; a < K; a++) M *= ctx->mod[ctx->L + a]; // two moduli below 2^61
        const unsigned __int128 bound = K == 2 ? 2 * M : M;
        tb.m2_lo = K == 2 ? (u64)(2 * M) : 0, tb.m2_hi = K == 2 ? (u64)((2 * M) >> 64) : 0;
        for (tb.lift_bits = 0; tb.lift_bits < 128 && (bound >> tb.lift_bits); tb.lift_bits++) {}
    }
    std::vector<sfold_t> sfold(L);
    for (uint32_t t = 0; t < L; t++) {
        const uint64_t q = ctx->mod[t];
        const uint64_t r63 = (1ull << 63) % q, r64 = h_mulmod(r63, 2 % q, q), r128 = h_mulmod(r64, r64, q);
        sfold[t].r64 = h_tw(r64, q), sfold[t].r128 = h_tw(r128, q);
        sfold[t].off = q - h_mulmod(r63, r128, q), sfold[t].pad = 0;
    }
    std::vector<uint16_t> pairs;
    for (uint32_t t = 0; t < LK; t++)
        for (uint32_t d = 0; d < tb.beta; d++)
            if (!bx[(size_t)d * LK + t].own) pairs.push_back((uint16_t)(d | (t << 8)));
    tb.pairs = pairs;
    if (tb.d_bx.upload(ctx, bx, "the key switch's extension constants") || tb.d_bxp.upload(ctx, bxp, "the key switch's lift constants") ||
        tb.d_pinv.upload(ctx, pinv, "the key switch's P^-1 table") || tb.d_sfold.upload(ctx, sfold, "the c0 fold's reduction constants"))
        return 1;
    ctx->ext[name] = sp;
    *out = sp.get();
    return 0;
}

int lm_ks_tables_view(lumen_ctx *ctx, lm_ks_view *out) {
    KsTables *tb = nullptr;
    if (int rc = get_tables(ctx, &tb)) return rc;
    out->d_bxp = tb->d_bxp.get();
    out->d_pinv = tb->d_pinv.get();
    out->yscale = &tb->yscale;
    return 0;
}

int lm_launch_pack_v(lumen_ctx *ctx, u64 *y, size_t poly_stride, uint32_t npoly, uint32_t ngroups,
                     uint32_t group_limbs, uint32_t first_mod, uint32_t nlimbs_total) {
    hipLaunchKernelGGL(k_pack_v, dim3(2048), dim3(256), 0, ctx->stream, y, poly_stride, npoly, ngroups, group_limbs,
                       first_mod, nlimbs_total, ctx->logN, ctx->mods);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

namespace {

// Tail of both work-list builders below.  Workgroup k of a launch runs on XCD k % 8, so the eight per-XCD lists are
// interleaved (lists of unequal length -- B not a multiple of 8 -- are drained in turn); the device copy is cached.
static int interleave_work_lists(lumen_ctx *ctx, const std::vector<std::vector<uint32_t>> &lists, size_t expect,
                                 const char *what, std::map<uint32_t, lm_dev<uint32_t>> &cache, uint32_t cache_key,
                                 const uint32_t **out) {
    std::vector<uint32_t> order;
    order.reserve(expect);
    std::vector<size_t> pos(8, 0);
    for (bool any = true; any;) {
        any = false;
        for (uint32_t x = 0; x < 8; x++)
            if (pos[x] < lists[x].size()) {
                order.push_back(lists[x][pos[x]++]);
                any = true;
            }
    }
    LM_CHECK(ctx, order.size() == expect, "%s work list is inconsistent", what);
    lm_dev<uint32_t> d;
    if (int rc = d.upload(ctx, order, "a key-switch work list")) return rc;
    *out = (cache[cache_key] = std::move(d)).get();
    return 0;
}

// Workgroup order of the extension kernel for a batch of B columns.  Workgroup k runs on XCD k % 8
// (round-robin dispatch), each XCD has its own 4 MB L2, and a digit is read once per target limb:
// XCD x takes the columns b == x (mod 8); inside it the targets come in groups of LM_MODUP_TGROUP, and
// for each group the (column, digit) pairs are walked with the group's targets innermost -- the
// workgroups that read the same digit are adjacent on one XCD (one fabric read, the rest L2 hits)
// while only LM_MODUP_TGROUP twiddle tables (256 KB each at N = 2^14) are live in that L2.
// (LM_MODUP_TGROUP = ctx->tune.modup_tgroup: a run-time switch since round 5 so that an A/B can alternate orders
// inside one process; the lists are cached per (batch size, group size).)
static int modup_work_list(lumen_ctx *ctx, KsTables *tb, uint32_t B, const uint32_t **out) {
    const uint32_t LM_MODUP_TGROUP = ctx->tune.modup_tgroup;
    LM_SHARED_LOCK(ctx); // the cached lists are shared with the context's clones
    // packed as column (16 bits) | digit (8) | target position (8): refuse what does not fit
    LM_CHECK(ctx, B >= 1 && B <= 65535 && tb->beta <= 255 && tb->nl + ctx->K <= 255,
             "key-switch batch of %u columns (beta %u) does not fit the packed work list", B, tb->beta);
    const uint32_t cache_key = B | (LM_MODUP_TGROUP << 16);
    auto it = tb->d_work.find(cache_key);
    if (it != tb->d_work.end()) {
        *out = it->second.get();
        return 0;
    }
    const uint32_t LK = tb->nl + ctx->K, beta = tb->beta;
    std::vector<std::vector<uint8_t>> need(beta); // digit -> targets that need an extension
    for (uint16_t pr : tb->pairs) need[pr & 0xFF].push_back((uint8_t)(pr >> 8));
    std::vector<std::vector<uint32_t>> lists(8);
    for (uint32_t x = 0; x < 8; x++)
        for (uint32_t t0 = 0; t0 < LK; t0 += LM_MODUP_TGROUP)
            for (uint32_t b = x; b < B; b += 8)
                for (uint32_t d = 0; d < beta; d++)
                    for (uint8_t t : need[d])
                        if (t >= t0 && t < t0 + LM_MODUP_TGROUP) lists[x].push_back(b | (d << 16) | ((uint32_t)t << 24));
    return interleave_work_lists(ctx, lists, (size_t)B * tb->pairs.size(), "extension", tb->d_work, cache_key, out);
}

// The same for ModDown: (polynomial pw = 2b + w, Q limb t); XCD x takes the polynomials pw == x (mod 8),
// targets in groups of LM_MODDOWN_TGROUP, the group's targets innermost.
// c1_only (the c0 fold: polynomial 0 needs no ModDown): the entries of polynomial 1 alone, B L of them, under a key of
// their own; XCD x then takes the COLUMNS b == x (mod 8) -- by pw the odd polynomials would sit on four of the eight.
static int moddown_work_list(lumen_ctx *ctx, KsTables *tb, uint32_t B, const uint32_t **out, bool c1_only = false) {
    const uint32_t LM_MODDOWN_TGROUP = ctx->tune.moddown_tgroup;
    LM_SHARED_LOCK(ctx);
    // packed as polynomial 2b + w (16 bits) | target limb (16)
    LM_CHECK(ctx, B >= 1 && 2 * (uint64_t)B <= 65535, "key-switch batch of %u columns does not fit the packed work list", B);
    const uint32_t cache_key = B | (LM_MODDOWN_TGROUP << 17) | (c1_only ? 1u << 31 : 0u);
    auto it = tb->d_work_down.find(cache_key);
    if (it != tb->d_work_down.end()) {
        *out = it->second.get();
        return 0;
    }
    const uint32_t L = tb->nl;
    std::vector<std::vector<uint32_t>> lists(8);
    for (uint32_t x = 0; x < 8; x++)
        for (uint32_t t0 = 0; t0 < L; t0 += LM_MODDOWN_TGROUP)
            for (uint32_t pw = c1_only ? 2 * x + 1 : x; pw < 2 * B; pw += c1_only ? 16 : 8)
                for (uint32_t t = t0; t < std::min<uint32_t>(t0 + LM_MODDOWN_TGROUP, L); t++) lists[x].push_back(pw | (t << 16));
    return interleave_work_lists(ctx, lists, (size_t)(c1_only ? 1 : 2) * B * L, "ModDown", tb->d_work_down, cache_key, out);
}

// digits whose packing is fused into the c1 inverse transform (k_intt_pack): the largest count whose
// B * nf two-transform workgroups are whole rounds of the device's workgroup slots (CUs x resident
// workgroups per CU: 256 x 1 at N = 2^14, so 4 of 6 digits at B = 64), so that no slot waits for a
// straggling pair; none when a launch does not even fill the slots once (small rings: every workgroup
// runs at once and a two-transform workgroup would just make the launch twice as long).
// LUMEN_KS_FUSED_DIGITS overrides (0 = k_pack_v for all).
template <int LOGN>
static uint32_t intt_pack_slots(lumen_ctx *ctx) {
    static const uint32_t v = [&] {
        hipDeviceProp_t prop;
        int per_cu = 0;
        if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return 256u;
        // (the query answers 0 for more than 64 KB of dynamic LDS until the kernel is allowed that much)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_intt_pack<LOGN>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)LM_CU_LDS_BYTES);
        constexpr lm_geom g = lm_geom_lds(LOGN);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_intt_pack<LOGN>, g.threads, g.lds) != hipSuccess || per_cu < 1) {
            // by hand: LDS (160 KB per CU) and the 2048 lanes of a CU
            per_cu = (int)std::max<size_t>(1, std::min<size_t>(LM_CU_LDS_BYTES / g.lds, 2048 / g.threads));
        }
        (void)hipGetLastError();
        if (ctx->tune.debug)
            fprintf(stderr, "[lumenos_hip] k_intt_pack<%d>: %d workgroup(s) per CU, %d CUs\n", LOGN, per_cu,
                    prop.multiProcessorCount);
        return (uint32_t)prop.multiProcessorCount * (uint32_t)per_cu;
    }();
    return v;
}
static uint32_t ks_fused_digits(lumen_ctx *ctx, uint32_t B, uint32_t L) {
    // a split degree: k_intt_pack's read-back is tied to the pass plan of a one-piece inverse and is not built there --
    // the switch is ignored (every digit goes through k_pack_v, same residues)
    if (lm_is_split(ctx->logN)) return 0;
    const long forced = ctx->tune.ks_fused_digits; // LUMEN_KS_FUSED_DIGITS at context creation / lumen_ctx_set_tuning
    const uint32_t pairs = L / 2; // digits with two limbs
    if (forced >= 0) return std::min<uint32_t>((uint32_t)forced, pairs);
    uint32_t slots = 0;
    if (lm_for_logn(ctx, ctx->logN, [&](auto n) { return slots = intt_pack_slots<n>(ctx), 0; })) return 0;
    for (uint32_t nf = pairs; nf >= 1; nf--)
        if (((uint64_t)B * nf) % slots == 0) return nf;
    return 0;
}

// 3. the gadget product of a batch of B columns at the level of `tb` under `key`, [ctx L + K][key_beta][2] whatever the
// level (the RNS gadget does not depend on it): the limbs modulo P sit behind the context's L Q limbs, in the moduli
// and in the stored key
// `ext`: block 0 of the extended digits, in the layout of Bh columns; ext1: the block of the columns from Bh on (a pair,
// lm_ks_pair.h; a single batch has Bh == B and no second block)
static int launch_ks_mac(lumen_ctx *ctx, const u64 *ext, const u64 *ext1, uint32_t Bh, const u64 *acc, const u64 *key, u64 *u, uint32_t B,
                         KsTables *tb) {
    const uint32_t L = tb->nl, K = ctx->K, pshift = ctx->L - L, key_beta = (ctx->L + K - 1) / K;
    LM_CHECK(ctx, Bh >= 1 && Bh <= B && (Bh == B || (ext1 && B <= 2 * Bh)), "gadget product: %u columns do not fit blocks of %u", B, Bh);
    const dim3 grid(((ctx->N / LM_MAC_VEC + 255) / 256) * (L + K) * ((B + LM_MAC_COLS - 1) / LM_MAC_COLS));
    hipLaunchKernelGGL(k_ks_mac, grid, dim3(256), 0, ctx->stream, ext, ext1 ? ext1 : ext, Bh, acc, key, u, B, L, K, tb->beta, pshift, key_beta,
                       ctx->logN, ctx->mods);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}
// ... of a doubling whose c0 is folded (k_ks_mac_fold): polynomial 0 of acc_out is written here, under gk's tables
static int launch_ks_mac_fold(lumen_ctx *ctx, const u64 *ext, const u64 *ext1, uint32_t Bh, const u64 *acc, const lm_galois_key &gk, u64 *u,
                              u64 *acc_out, uint32_t B, KsTables *tb) {
    const uint32_t L = tb->nl, K = ctx->K, pshift = ctx->L - L, key_beta = (ctx->L + K - 1) / K;
    LM_CHECK(ctx, ctx->N >= 256 && LM_MAC_VEC == 1, "the folded gadget product works on blocks of 256 coefficients");
    LM_CHECK(ctx, Bh >= 1 && Bh <= B && (Bh == B || (ext1 && B <= 2 * Bh)), "gadget product: %u columns do not fit blocks of %u", B, Bh);
    const dim3 grid((ctx->N / 256) * (L + K) * ((B + LM_MAC_COLS - 1) / LM_MAC_COLS));
    hipLaunchKernelGGL(k_ks_mac_fold, grid, dim3(256), 0, ctx->stream, ext, ext1 ? ext1 : ext, Bh, acc, gk.d_key.get(), u, B, L, K, tb->beta, pshift,
                       key_beta, ctx->logN, ctx->mods, acc_out, gk.d_index.get(), gk.d_inv_index.get());
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// 4b + 5. lift to Q, NTT, combine, automorphism: accumulated into out = in + ... (ACCUMULATE, k_moddown_ntt) or stored as a
// plain gather (k_rotdown_ntt)
template <bool ACCUMULATE>
static int launch_moddown(lumen_ctx *ctx, const u64 *in, u64 *out, uint32_t B, const lm_galois_key &gk, KsTables *tb,
                          const KsScratch &s, bool c1_only = false) {
    const uint32_t L = tb->nl, K = ctx->K;
    const uint32_t *work_down = nullptr;
    if (int rc = moddown_work_list(ctx, tb, B, &work_down, c1_only)) return rc;
    const uint32_t items = (c1_only ? 1 : 2) * B * L; // one forward transform each
    lm_prof_scope ps(ctx, ACCUMULATE ? "ks_moddown_ntt" : "ks_rotdown_ntt", (uint64_t)items);
    return lm_for_any_logn(ctx, ctx->logN, [&](auto n) {
        constexpr int LN = decltype(n)::value;
        return lm_launch(ctx, ACCUMULATE ? k_moddown_ntt<LN> : k_rotdown_ntt<LN>, lm_geom_fwd(LN), lm_fwd_grid<LN>(items), s.u, in, out, tb->d_bxp.get(), tb->d_pinv.get(),
                         gk.d_index.get(), gk.d_inv_index.get(), work_down, B, L, K, ctx->mods, ctx->sh->tw_fwd.get());
    });
}

} // namespace

// Steps 1-4a of a rotation of acc, [B][2][L][N], L = the level of `tb`, in two halves.
// rotate_decompose, steps 1-2: the digits of c1 extended to every limb, in s.coef and s.ext.  It depends on the ciphertext
// alone -- not on the key, not on the Galois element -- so several rotations of one ciphertext share it
// (lumen_rotate_hoisted: [LATTIGO-RECALL] Evaluator.DecomposeNTT before AutomorphismHoisted).
int rotate_decompose(lumen_ctx *ctx, const u64 *acc, uint32_t B, KsTables *tb, const KsScratch &s) {
    const uint32_t N = ctx->N, L = tb->nl, K = ctx->K, beta = tb->beta;
    const uint32_t pshift = ctx->L - L; // the limbs modulo P sit behind the context's L Q limbs (moduli, twiddles)
    // 1. c1 -> coefficient domain, scaled for the basis extension, and the (hi, lo) packing of the two-limb
    // digits: fused into the transform for the first nf digits, k_pack_v for the others
    const uint32_t nf = K == 2 ? ks_fused_digits(ctx, B, L) : 0;
    if (nf) {
        const uint32_t grid = B * nf + B * (L - 2 * nf);
        lm_prof_scope ps(ctx, "ks_intt_c1", (uint64_t)B * L);
        if (int rc = lm_for_logn(ctx, ctx->logN, [&](auto n) {
                return lm_launch(ctx, k_intt_pack<n>, lm_geom_lds(n), grid, acc, s.coef, B, L, nf, ctx->mods, tb->yscale,
                                 ctx->sh->tw_inv.get());
            }))
            return rc;
    } else {
        if (int rc = lm_launch_ntt_strided(ctx, acc + (size_t)L * N, (size_t)2 * L * N, s.coef, (size_t)L * N, B,
                                           lm_map_q(L), true, "ks_intt_c1", &tb->yscale))
            return rc;
    }
    if (K == 2 && nf < beta) { // the digits the transform did not pack
        lm_prof_scope ps(ctx, "ks_pack_v", (uint64_t)B);
        if (int rc = lm_launch_pack_v(ctx, s.coef + (size_t)2 * nf * N, (size_t)L * N, B, beta - nf, K, 2 * nf, L - 2 * nf)) return rc;
    }
    // 2. digit extension + NTT: one launch for a single batch; for a pair (lm_ks_pair.h) one per half, each with the work list
    // and the `ext` layout of a batch of s.half columns, on the half's own columns of coef and acc (column-major both: the
    // column base is an offset) and into the half's own block
    {
        const lm_ks_ext_plan plan = lm_ks_ext_launches(B, s.half, s.second_first);
        for (uint32_t k = 0; k < plan.n; k++) {
            const lm_ks_ext_launch &h = plan.at[k];
            const uint64_t nb = (uint64_t)h.count * tb->pairs.size();
            const uint32_t *work = nullptr;
            if (int rc = modup_work_list(ctx, tb, h.count, &work)) return rc;
            const u64 *coef_h = s.coef + (size_t)h.first * L * N, *acc_h = acc + (size_t)h.first * 2 * L * N;
            u64 *ext_h = h.block ? s.ext1 : s.ext;
            lm_prof_scope ps(ctx, "ks_modup_ntt", nb);
            if (int rc = lm_for_any_logn(ctx, ctx->logN, [&](auto n) {
                    return lm_launch(ctx, k_modup_ntt<n>, lm_geom_fwd(n), lm_fwd_grid<n>((uint32_t)nb), coef_h, acc_h, ext_h, tb->d_bx.get(), plan.layout, L, K,
                                     beta, pshift, work, ctx->mods, ctx->sh->tw_fwd.get());
                }))
                return rc;
        }
    }
    return 0;
}

// rotate_product, steps 3-4a, under one key: reads s.ext and acc, leaves the gadget product u in s.u, its limbs modulo P
// in the coefficient domain and packed.  What follows is the seam between the ways a rotation ends: ModDown into an
// accumulator (rotate_accumulate), ModDown into a plain gather (rotate_store) or, for the last rotation before a rescale,
// the closing inverse transform (rotate_close).
int rotate_product(lumen_ctx *ctx, const u64 *acc, uint32_t B, const lm_galois_key &gk, KsTables *tb, const KsScratch &s) {
    if (int rc = rotate_mac(ctx, acc, B, gk, tb, s)) return rc;
    return rotate_p_to_coef(ctx, s.u, B, tb);
}

// 3. gadget product: s.u, all nl + K limbs in the NTT domain
int rotate_mac(lumen_ctx *ctx, const u64 *acc, uint32_t B, const lm_galois_key &gk, KsTables *tb, const KsScratch &s) {
    lm_prof_scope ps(ctx, "ks_mac", (uint64_t)B);
    return launch_ks_mac(ctx, s.ext, s.ext1, lm_ks_ext_launches(B, s.half).layout, acc, gk.d_key.get(), s.u, B, tb);
}

// 4a. P limbs of u -> coefficient domain (in place) and packed; u: any block of s.u's layout (ks_u_at).  c1_only: those
// of polynomial 1 of every column alone -- every other pair of K limbs; polynomial 0's stay in the NTT domain
int rotate_p_to_coef(lumen_ctx *ctx, u64 *u, uint32_t B, KsTables *tb, bool c1_only) {
    const uint32_t N = ctx->N, L = tb->nl, K = ctx->K;
    u64 *up = u + ks_u_at(c1_only ? 1 : 0, L, B, L, K) * N; // the limbs modulo P: [2B][K]
    const size_t pstride = (size_t)(c1_only ? 2 : 1) * K * N;
    const uint32_t npoly = c1_only ? B : B * 2;
    if (int rc = lm_launch_ntt_strided(ctx, up, pstride, up, pstride, npoly, lm_map_p(ctx), true, "ks_intt_p",
                                       &tb->yscale))
        return rc;
    if (K == 2) {
        lm_prof_scope ps(ctx, "ks_pack_v", (uint64_t)B);
        if (int rc = lm_launch_pack_v(ctx, up, pstride, npoly, 1u, K, ctx->L, K)) return rc;
    }
    return 0;
}

// acc, acc_out: [B][2][L][N], L = the level of `tb`; acc_out = acc + Rot_galEl(acc) for every column
int rotate_accumulate(lumen_ctx *ctx, const u64 *acc, u64 *acc_out, uint32_t B, const lm_galois_key &gk,
                      KsTables *tb, const KsScratch &s) {
    if (int rc = rotate_decompose(ctx, acc, B, tb, s)) return rc;
    return rotate_add(ctx, acc, acc_out, B, gk, tb, s);
}

// After rotate_decompose: acc_out = acc + Rot_galEl(acc) for every column, lazy; `acc_out` is another block than `acc`.
int rotate_add(lumen_ctx *ctx, const u64 *acc, u64 *acc_out, uint32_t B, const lm_galois_key &gk, KsTables *tb, const KsScratch &s) {
    if (int rc = rotate_product(ctx, acc, B, gk, tb, s)) return rc;
    return launch_moddown<true>(ctx, acc, acc_out, B, gk, tb, s);
}

// After rotate_product: out = Rot_galEl(in) for every column, canonical, [B][2][L][N] both; `out` is another block than `in`.
int rotate_store(lumen_ctx *ctx, const u64 *in, u64 *out, uint32_t B, const lm_galois_key &gk, KsTables *tb, const KsScratch &s) {
    return launch_moddown<false>(ctx, in, out, B, gk, tb, s);
}

// The same for polynomial 1 of every column alone (ModDown's c1_only work list): polynomial 1 of `out` = the ModDown of
// polynomial 1 of s.u under gk's tables, canonical; `in` is not read (c0 rides on polynomial 0) and polynomial 0 of `out` is
// not written.  s.u went through rotate_p_to_coef, c1_only or not.
int rotate_store_c1(lumen_ctx *ctx, const u64 *in, u64 *out, uint32_t B, const lm_galois_key &gk, KsTables *tb, const KsScratch &s) {
    return launch_moddown<false>(ctx, in, out, B, gk, tb, s, true);
}

// After rotate_decompose: coef_out = the coefficient form of acc + Rot_galEl(acc), [B][2][L][N]: the last rotation before a
// rescale (lm_ks_close.hip)
int rotate_close(lumen_ctx *ctx, const u64 *acc, u64 *coef_out, uint32_t B, const lm_galois_key &gk, uint64_t gal_el,
                 KsTables *tb, const KsScratch &s) {
    if (int rc = rotate_product(ctx, acc, B, gk, tb, s)) return rc;
    const uint32_t *work_down = nullptr;
    if (int rc = moddown_work_list(ctx, tb, B, &work_down)) return rc;
    return ks_close_launch(ctx, acc, coef_out, B, gk, gal_el, tb, s, work_down);
}

// ---- the c0 fold (lm_ks_host.h).  Three words of two's complement hold |S| < 2^191, and S is a signed sum of
// 2^rotations - 1 lifts, each below 2^lift_bits in magnitude; k_ks_mac_fold works on aligned blocks of 256 coefficients
// and k_ks_close is not built for a split degree.
// The fold also needs doublings to save on: per 64-column batch at N = 2^14 a folded doubling saves 86 us of ModDown and
// costs 29 us in the gadget product and a lift fold (8 us the first, 26 us after it), and the close costs 16 us more and
// a lift fold of its own.  A plan of two rotations has ONE doubling: -86 + 29 + 8 + 26 + 16 = -7 us of a call of about
// 2.2 ms -- measured, tools/c0_fold_rows.py: not distinguishable from noise, under the project's 1 % bar (EXPERIMENTS R19) --
// so it keeps the plain route; from three rotations on
// every further doubling saves 31 us.  -DLM_KS_FOLD_MIN_ROTATIONS=2 builds the variant that measurement used.
#ifndef LM_KS_FOLD_MIN_ROTATIONS
#define LM_KS_FOLD_MIN_ROTATIONS 3
#endif
bool ks_fold_serves(const lumen_ctx *ctx, const KsTables *tb, uint32_t rotations) {
    return ctx->N >= 256 && !lm_is_split(ctx->logN) && ctx->K >= 1 && ctx->K <= 2 && rotations >= LM_KS_FOLD_MIN_ROTATIONS &&
           rotations + tb->lift_bits <= 191;
}

int rotate_add_fold(lumen_ctx *ctx, const u64 *acc, u64 *acc_out, uint32_t B, const lm_galois_key &gk, uint64_t gal_el, KsTables *tb,
                    const KsScratch &s, const u64 *s_in, u64 *s_out) {
    {
        lm_prof_scope ps(ctx, "ks_mac", (uint64_t)B);
        if (int rc = launch_ks_mac_fold(ctx, s.ext, s.ext1, lm_ks_ext_launches(B, s.half).layout, acc, gk, s.u, acc_out, B, tb)) return rc;
    }
    if (int rc = rotate_p_to_coef(ctx, s.u, B, tb)) return rc;
    if (int rc = lift_fold_launch(ctx, s.u, s_in, s_out, B, gal_el, tb)) return rc;
    return launch_moddown<true>(ctx, acc, acc_out, B, gk, tb, s, true);
}

int rotate_close_fold(lumen_ctx *ctx, const u64 *acc, u64 *coef_out, uint32_t B, const lm_galois_key &gk, uint64_t gal_el,
                      KsTables *tb, const KsScratch &s, const u64 *s_in, u64 *s_out) {
    if (int rc = rotate_product(ctx, acc, B, gk, tb, s)) return rc;
    if (int rc = lift_fold_launch(ctx, s.u, s_in, s_out, B, gal_el, tb)) return rc;
    const uint32_t *work_down = nullptr;
    if (int rc = moddown_work_list(ctx, tb, B, &work_down)) return rc;
    return ks_close_launch(ctx, acc, coef_out, B, gk, gal_el, tb, s, work_down, s_out);
}

// Times the gadget product alone on caller-chosen device blocks: how its speed depends on WHERE in HBM its
// three streams sit (tools/ks_mac_placement.py).  A NULL block = the one the product itself uses (the key
// switch's scratch, the first Galois key loaded).  The blocks' contents are whatever they hold: the kernel's
// control flow does not depend on data.  HIP-event time of `reps` launches on the context's stream.
extern "C" int lumen_ks_mac_probe(lumen_ctx *ctx, uint32_t batch, const void *ext, const void *acc, const void *key,
                                  void *u, uint32_t reps, float *ms_per_launch) {
    LM_CHECK(nullptr, ctx && ms_per_launch, "lumen_ks_mac_probe: NULL argument");
    LM_ENTER(ctx);
    KsTables *tb = nullptr;
    if (int rc = get_tables(ctx, &tb)) return rc;
    const uint32_t N = ctx->N, L = ctx->L, B = batch ? batch : ks_batch(ctx);
    LM_CHECK(ctx, B <= 65535 && reps >= 1 && reps <= 100000, "lumen_ks_mac_probe: batch %u / reps %u out of range", B, reps);
    KsScratch s;
    if (int rc = get_scratch(ctx, B, tb, &s)) return rc;
    if (!acc) acc = lm_scratch(ctx, "ks_acc", (size_t)B * 2 * L * N * 8);
    if (!acc) return 1;
    if (!key) {
        LM_SHARED_LOCK(ctx);
        LM_CHECK(ctx, !ctx->gkeys.empty(), "lumen_ks_mac_probe: no Galois key loaded");
        key = ctx->gkeys.begin()->second.d_key.get();
    }
    const u64 *pe = ext ? (const u64 *)ext : s.ext;
    u64 *pu = u ? (u64 *)u : s.u;
    auto launch = [&] { return launch_ks_mac(ctx, pe, nullptr, B, (const u64 *)acc, (const u64 *)key, pu, B, tb); }; // the top level's
    for (int i = 0; i < 3; i++)
        if (int rc = launch()) return rc;
    LM_HIP(ctx, hipEventRecord(ctx->tm0, ctx->stream));
    for (uint32_t i = 0; i < reps; i++)
        if (int rc = launch()) return rc;
    LM_HIP(ctx, hipEventRecord(ctx->tm1, ctx->stream));
    LM_HIP(ctx, hipEventSynchronize(ctx->tm1));
    float ms = 0;
    LM_HIP(ctx, hipEventElapsedTime(&ms, ctx->tm0, ctx->tm1));
    *ms_per_launch = ms / (float)reps;
    return 0;
}
