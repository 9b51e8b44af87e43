// The closing rotation of an InnerSum that a rescale follows (matrixInnerSumEval, lm_innersum.hip).
//
// A rotation ends in k_moddown_ntt: per (column, polynomial, Q limb t) it lifts the P limbs of the gadget product into
// q_t, runs a FORWARD transform of that lift and forms
//     acc_out_t = acc_in_t + sigma_ntt(u'_t - NTT_t(lift_t) * P^-1 (+ c0_t for polynomial 0)).
// After the last rotation the next reader of the accumulator is the rescale, whose first pass is an INVERSE transform of
// every one of those limbs.  NTT_t is a ring isomorphism and the automorphism commutes with it, so modulo q_t, exactly,
//     INTT_t(acc_out_t) = INTT_t(acc_in_t + sigma_ntt(u'_t (+ c0_t))) - sigma_coef(lift_t * P^-1):
// the lift is in the coefficient domain already (the packed (hi, lo) words of u's P limbs) and needs no transform.
//   sigma_ntt : the gather the key carries, out[j] = in[index[j]];
//   sigma_coef: X^k -> X^(g k mod 2N) with X^N = -1, i.e. output coefficient i takes source coefficient
//               i' = g^-1 i mod 2N, negated when i' >= N (then from i' - N): g (i' - N) = i - g N = i + N (mod 2N), g odd.
// k_ks_close is that right-hand side: the rescale's inverse transform (it reports under that name, rescale_intt) with
// the last ModDown's operands in its loader and the lift in its storer.  The last of a batch's ModDown launches, its
// forward transforms, and one write and one read of the accumulator are gone; the result is the coefficient-form limb
// k_rescale_coef reads (lm_rescale.hip, lm_rescale_polys_from_coef).
// Also here, because it shares sigma_coef: k_lift_fold, the coefficient half of the c0 fold (LUMEN_KS_C0_FOLD, lm_ks_host.h), and
// the FOLD form of k_ks_close that takes polynomial 0's lift from it.
#include "lm_ks_host.h"

#ifndef LM_KS_CLOSE_PF
#define LM_KS_CLOSE_PF 4 // lift words requested ahead of the coefficient that consumes them (pairs of (hi, lo))
#endif

// One workgroup per (column b, polynomial w, Q limb t), dealt by ModDown's work list (moddown_work_list).
// u: the gadget product (ks_u_at), its P limbs in the coefficient domain and packed (steps 1-4a of rotate_accumulate);
// acc_in: [B][2][L][N], lazy; out: [B][2][L][N] coefficient form, canonical; ginv: g^-1 mod 2N.
// FOLD (the c0 fold, LUMEN_KS_C0_FOLD): polynomial 0 arrives as c0 = A - P^-1 NTT(S), A in acc_in and S, the folded lifts
// of every rotation INCLUDING this one (k_lift_fold below), in fold_s, [B][3][N]: the loader is the same on A, and the
// storer of a w == 0 workgroup subtracts P^-1 (S[i] mod q_t), S read linearly at the output coefficient itself -- no
// gather and no sign, both are in S.  Polynomial 1 is as without.
template <int LOGN, bool FOLD>
__global__ LM_GEOM_BOUNDS(lm_geom_lds(LOGN)) void k_ks_close(const u64 *__restrict__ u, const u64 *__restrict__ acc_in,
                                                              u64 *__restrict__ out, const bx_t *__restrict__ bxp,
                                                              const tw_t *__restrict__ pinv,
                                                              const uint32_t *__restrict__ index,
                                                              const uint32_t *__restrict__ inv_index, uint32_t ginv,
                                                              const uint32_t *__restrict__ work, uint32_t B, uint32_t L,
                                                              uint32_t K, lm_mods mods, lm_ninv_t ninv,
                                                              const tw_t *__restrict__ tw_all,
                                                              const u64 *__restrict__ fold_s,
                                                              const sfold_t *__restrict__ sfc) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x;
    const uint32_t wk = work[blockIdx.x];
    const uint32_t pw = wk & 0xFFFF; // b*2 + w
    const uint32_t t = wk >> 16;
    const uint32_t w = pw & 1;
    const bx_t c = bxp[t];
    const lm_qc qc = lm_make_qc(mods.m[t]);
    const u64 *up0 = u + ks_u_at(pw, L, B, L, K) * N; // P limbs of u, coefficient domain
    const u64 *up1 = c.ns == 2 ? up0 + N : up0;
    const u64 *uq = u + ks_u_at(pw, t, B, L, K) * N;
    const u64 *ain = acc_in + ((size_t)pw * L + t) * N;
    u64 *o = out + ((size_t)pw * L + t) * N;
    // The loader's operand is acc_in[j] + x[index[j]], x = u' (+ c0 for w == 0): what k_moddown_ntt forms before its gather.
    // The gather goes through LDS, as there.  The wave-local passes of the inverse give wave `wave` the aligned block of
    // BLK = N / waves positions j (lm_deal), and index permutes such blocks onto blocks (k_moddown_ntt: the top bits of
    // index[j] are a function of the top bits of j): the block's x all comes from ONE source block sb.  The wave reads
    // that block of u' (and c0) linearly, 16-byte words, lanes on consecutive addresses, and SCATTERS it into its own
    // LDS block, x[s] to slot inv_index[s]; the loader then reads slot j beside acc_in[j], both linearly, and the first
    // pass writes its outputs to the slots its lane has just read.  No wave touches another one's block before the
    // cross-wave pass.  (Gathered straight from global memory every load instruction of the loader asks for 64 separate
    // words of an 8 KB block.)
    constexpr uint32_t NW = lm_nthreads(LOGN) / 64, BLK = N / NW, IT = BLK / 128, CH = IT < 4 ? IT : 4;
    static_assert(IT >= 1 && IT % CH == 0, "a wave stages its block as pairs of words, 128 per instruction");
    {
        const uint32_t wave = tid >> 6, lane = tid & 63;
        const uint32_t sb = NW > 1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(index[wave * BLK] / BLK)) : 0u;
#pragma unroll
        for (uint32_t k0 = 0; k0 < IT; k0 += CH) {
            uint2 p[CH];
            ulonglong2 x[CH], c0[CH];
#pragma unroll
            for (uint32_t k = 0; k < CH; k++) {
                const uint32_t s = sb * BLK + 2 * lane + (k0 + k) * 128;
                p[k] = *reinterpret_cast<const uint2 *>(inv_index + s);
                x[k] = *reinterpret_cast<const ulonglong2 *>(uq + s);
                if (w == 0) c0[k] = *reinterpret_cast<const ulonglong2 *>(ain + s);
            }
#pragma unroll
            for (uint32_t k = 0; k < CH; k++) { // u' < q, c0 < 2q: x < 3q
                sm[LM_PAD(wave * BLK + (p[k].x & (BLK - 1)))] = w == 0 ? x[k].x + c0[k].x : x[k].x;
                sm[LM_PAD(wave * BLK + (p[k].y & (BLK - 1)))] = w == 0 ? x[k].y + c0[k].y : x[k].y;
            }
        }
        lm_wave_sync();
    }
    // Ranges: u' < q (the gadget product's lm_mont_reduce_wide is canonical), the accumulator and with it c0 lazy in
    // [0, 2q).  w == 1: acc + u' < 3q as it is.  w == 0: acc + u' + c0 < 5q, one conditional subtraction of 2q brings it
    // under 3q, the inverse stages' input bound.
    auto ld = [&](uint32_t j0, u64 *v, int count) {
        lm_load_run(ain, j0, v, count);
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < count) {
                const u64 x = sm[LM_PAD(j0 + k)];
                v[k] = w == 0 ? lm_csub(v[k] + x, 2 * qc.q) : v[k] + x;
            }
    };
    // Storer: out[i] = e * N^-1 - (+-) lift[i'] * P^-1, canonical.  -P^-1 as a Shoup constant, as in k_moddown_ntt.
    // Both products come out of the multiplication lazily, in [0, 3q): r = e * N^-1 and m = lift * (-P^-1); where the
    // source coefficient wrapped the term is 3q - m in (0, 3q] instead.  r + term < 6q: three conditional subtractions.
    // The lift words of a work item's coefficient k + PF are requested when coefficient k is formed, the first PF of
    // them before the item's butterflies (pre): for g = 2N - 1, the row swap that ends InnerSum(N), i' = N - i and a
    // wave reads 512 contiguous bytes backwards; for a general g its lanes read words g^-1 apart.
    constexpr int R_LAST = lm_pass_r(LOGN, 0), LOG_T0 = LOGN - R_LAST, CNT = 1 << R_LAST;
    constexpr int PF = LM_KS_CLOSE_PF < CNT ? LM_KS_CLOSE_PF : CNT;
    tw_t npi = pinv[t];
    npi.w = qc.q - npi.w, npi.wp = ~npi.wp;
    struct close_t {
        u64 *o;
        const u64 *up0, *up1;
        const bx_t &c;
        const lm_qc &qc;
        tw_t ni, npi;
        uint32_t ginv;
        const u64 *sp; // FOLD: the three planes of the column's S for a w == 0 workgroup, NULL for w == 1
        sfold_t sf;
        u64 hi[PF], lo[PF], top[FOLD ? PF : 1];
        __device__ __forceinline__ uint32_t src(uint32_t i) const { return (ginv * i) & (2 * N - 1); }
        __device__ __forceinline__ void fetch(uint32_t i, u64 &h, u64 &l, u64 &x) const {
            if (FOLD && sp) {
                h = sp[i], l = sp[N + i], x = sp[2 * N + i];
                return;
            }
            const uint32_t s = src(i) & (N - 1);
            h = up0[s], l = up1[s];
        }
        __device__ __forceinline__ void pre(uint32_t w0) {
#pragma unroll
            for (int k = 0; k < PF; k++) fetch(w0 + ((uint32_t)k << LOG_T0), hi[k], lo[k], top[FOLD ? k : 0]);
        }
        __device__ __forceinline__ void operator()(uint32_t i, u64 v, int k) {
            const u64 h = hi[k % PF], l = lo[k % PF], x = top[FOLD ? k % PF : 0];
            if (k + PF < CNT) fetch(i + ((uint32_t)PF << LOG_T0), hi[k % PF], lo[k % PF], top[FOLD ? k % PF : 0]);
            const u64 r = lm_shoup3<true>(v, ni.w, ni.wp, qc.nq);
            u64 y;
            if (FOLD && sp) { // S mod q_t below 10q, times -P^-1: [0, 3q)
                y = r + lm_shoup3<true>(lm_s192_mod(sf, h, l, x, qc), npi.w, npi.wp, qc.nq);
            } else {
                const u64 m = lm_shoup3<true>(bx_apply(c, h, l, qc), npi.w, npi.wp, qc.nq);
                y = r + (src(i) >= N ? qc.q3 - m : m);
            }
            y = lm_csub(lm_csub(y, 4 * qc.q), 2 * qc.q);
            o[i] = lm_csub(y, qc.q);
        }
    } st{o, up0, up1, c, qc, ninv.t[t], npi, ginv, FOLD && w == 0 ? fold_s + (size_t)(pw >> 1) * 3 * N : nullptr, FOLD ? sfc[t] : sfold_t{}, {}, {}, {}};
    lm_ntt_inverse<LOGN>(sm, tw_all + (size_t)t * N, qc, tid, ld, st);
}

// g^-1 mod 2N for an odd g (Newton: every step doubles the correct low bits, 3 to start with)
static uint32_t inv_mod_2n(uint64_t g, uint32_t N) {
    uint64_t x = g;
    for (int i = 0; i < 5; i++) x *= 2 - g * x;
    return (uint32_t)(x & (2ull * N - 1));
}

int ks_close_launch(lumen_ctx *ctx, const u64 *acc, u64 *out, uint32_t B, const lm_galois_key &gk, uint64_t gal_el,
                    KsTables *tb, const KsScratch &s, const uint32_t *work_down, const u64 *fold_s) {
    const uint32_t L = tb->nl, K = ctx->K;
    const uint32_t ginv = inv_mod_2n(gal_el, ctx->N);
    // one inverse transform per workgroup, counted with the rescale's (bench_lib/report.py's transform census)
    lm_prof_scope ps(ctx, "rescale_intt", (uint64_t)B * 2 * L);
    return lm_for_logn(ctx, ctx->logN, [&](auto n) {
        constexpr int LN = decltype(n)::value;
        auto go = [&](auto kernel) {
            return lm_launch(ctx, kernel, lm_geom_lds(LN), B * 2 * L, s.u, acc, out, tb->d_bxp.get(), tb->d_pinv.get(), gk.d_index.get(),
                             gk.d_inv_index.get(), ginv, work_down, B, L, K, ctx->mods, lm_ninv_of(ctx), ctx->sh->tw_inv.get(), fold_s,
                             tb->d_sfold.get());
        };
        return fold_s ? go(k_ks_close<LN, true>) : go(k_ks_close<LN, false>);
    });
}

// ---- the coefficient half of the c0 fold: S_out[i] = S_in[i] +- (S_in[i'] + W[i'] - 2M), i' = g^-1 i mod 2N, the sign taken
// when i' >= N (sigma_coef above).  W = hi 2^57 + lo: the packed limbs modulo P of polynomial 0 (k_pack_v), 0 <= W < 4M;
// K == 1: the residue itself and no offset (m2 = 0).  Three-word signed adds on planes [B][3][N]; s_in == NULL is S = 0,
// the first rotation, which stores.  One thread per coefficient, one workgroup per 256 of them: the output and S_in[i]
// move linearly, the three words of S_in[i'] and the two of W[i'] are gathered g^-1 words apart -- every 64-byte sector
// of a column's five source planes (640 KB at N = 2^14) is asked for eight times, by different workgroups.  Workgroup k
// runs on XCD k % 8 and each XCD has its own L2, so the workgroups of ONE column are dealt to one XCD (columns b == x
// mod 8 on XCD x, as k_ks_mac deals its key slices): the planes come into that L2 once instead of into all eight.
__global__ __launch_bounds__(256) void k_lift_fold(const u64 *__restrict__ up, const u64 *__restrict__ s_in, u64 *__restrict__ s_out,
                                                   uint32_t ginv, uint32_t B, uint32_t K, uint32_t logN, u64 m2_lo, u64 m2_hi) {
    const uint32_t N = 1u << logN, C = N >> 8; // workgroups per column
    uint32_t b, chunk;
    if (B % 8 == 0) {
        const uint32_t xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        b = (j / C) * 8 + xcd, chunk = j % C;
    } else {
        b = blockIdx.x / C, chunk = blockIdx.x % C;
    }
    {
        const uint32_t i = chunk * 256 + threadIdx.x;
        const uint32_t e = (ginv * i) & (2 * N - 1), s = e & (N - 1);
        const u64 *w = up + ((size_t)2 * b * K << logN); // the limbs modulo P of polynomial 2b: [2B][K]
        lm_s192 d;
        if (K == 2) {
            const u64 hi = w[s], lo = w[N + s]; // lo < 2^57, hi < 2^61
            d = lm_s192_add(lm_s192{lo | (hi << LM_W_SPLIT), hi >> (64 - LM_W_SPLIT), 0}, lm_s192_neg(lm_s192{m2_lo, m2_hi, 0}));
        } else {
            d = lm_s192{w[s], 0, 0};
        }
        const u64 *pi = s_in ? s_in + (size_t)b * 3 * N : nullptr;
        u64 *po = s_out + (size_t)b * 3 * N;
        if (s_in) d = lm_s192_add(d, lm_s192{pi[s], pi[N + s], pi[2 * N + s]});
        if (e >= N) d = lm_s192_neg(d);
        if (s_in) d = lm_s192_add(d, lm_s192{pi[i], pi[N + i], pi[2 * N + i]});
        po[i] = d.a, po[N + i] = d.b, po[2 * N + i] = d.c;
    }
}

int lift_fold_launch(lumen_ctx *ctx, const u64 *u, const u64 *s_in, u64 *s_out, uint32_t B, uint64_t gal_el, KsTables *tb) {
    const uint32_t L = tb->nl, K = ctx->K;
    LM_CHECK(ctx, s_out && s_out != s_in, "the folded lifts need a block of their own");
    LM_CHECK(ctx, ctx->N >= 256, "the lift fold works on blocks of 256 coefficients");
    lm_prof_scope ps(ctx, "ks_lift_fold", (uint64_t)B);
    hipLaunchKernelGGL(k_lift_fold, dim3(B * (ctx->N / 256)), dim3(256), 0, ctx->stream,
                       u + ks_u_at(0, L, B, L, K) * ctx->N, s_in, s_out, inv_mod_2n(gal_el, ctx->N), B, K, ctx->logN, tb->m2_lo, tb->m2_hi);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}
