// Ciphertext x ciphertext product with relinearisation, Evaluator.MulRelinNew(ct, ct) (fhe/bfv.go:34-42 with a
// ciphertext operand): lumen_mul_relin, and the degree-2 triple before the key switch, lumen_mul_tensor.
//     d0 = T a0 b0      d1 = T (a0 b1 + a1 b0)      d2 = T a1 b1          ([LATTIGO-RECALL] bgv tensorStandard)
//     out = (d0 + k0, d1 + k1),  (k0, k1) = the hybrid key switch of d2 under the relinearisation key (s^2 -> s)
// Ciphertexts encrypt m * T^-1 + e, so the product of two carries T^-2 and one factor T brings it back: the factor
// lo_mul_plain gives its plaintext.
// The key switch is the rotation's (lm_keyswitch.hip), not a second one: rotate_accumulate computes
// acc_out = acc + sigma(c0 + k0(c1), k1(c1)) with the source taken from the accumulator's own c1.  With the
// relinearisation key, whose gather tables are the identity (lm_ks_key.hip), and the accumulator (0, d2) it leaves
// (k0, d2 + k1) in the lazy range [0, 2q); the tensor kernel therefore writes (0, d2) as the batch's accumulator and
// (d0, d1 - d2) into the output set, and one closing elementwise pass adds the two and canonicalises (it stands where
// k_acc_canon stands after an InnerSum).  Batching, lanes, per-level tables and the scratch sized and placed for the top
// level are the batch driver's (lm_ks_batch.hip), grouped as matrixInnerSumEval's.
#include "lm_ks_host.h"

// Block order of the two elementwise kernels: LIMB-MAJOR, blockIdx.x = (limb * count + ciphertext) * nblk + k, a block
// on LM_MR_PAIRS consecutive coefficient pairs of one limb of one ciphertext (all of them below N = 2^11).  The limb is
// uniform per block: its modulus and constants are scalar loads out of the kernel arguments and stay in SGPRs.
#define LM_MR_PAIRS 512u // two 16-byte words per thread and stream
__host__ __device__ __forceinline__ uint32_t mr_blocks_per_limb(uint32_t logN) {
    return (1u << (logN - 1)) > LM_MR_PAIRS ? (1u << (logN - 1)) / LM_MR_PAIRS : 1u;
}

// a: [count][2][nl][N]; b: [count][2][nl][N] (bstride = 1) or ONE ciphertext (bstride = 0); canonical words.
// tfac[l] = T * 2^64 mod q_l as a Shoup constant: a0, a1 enter Montgomery form WITH the factor T in one lazy
// multiplication by a constant ([0, 3q)), and every output is one Montgomery reduction of a 128-bit sum of at most two
// 64 x 64 products (< 6 q^2 < 2^122).  Four products per coefficient, not Karatsuba's three: measured, the three-product
// form (tools/exp_mul_tensor_karatsuba.patch) runs in the same time, 9.86 against 9.42 / 9.72 ms for 51.5 GB at the top
// level of the headline shape, 66-68 % of the HBM peak (profiles/EXPERIMENTS.md R12) -- the multiplier does not bound
// the kernel, which moves 7 (RELIN: 8) words per coefficient.
// RELIN = false: out = (d0, d1, d2), [count][3][nl][N].
// RELIN = true:  out = (d0, d1 - d2), [count][2][nl][N], and acc = (0, d2), [count][2][nl][N].
template <bool RELIN>
__global__ __launch_bounds__(256) void k_mul_tensor(const u64 *__restrict__ a, const u64 *__restrict__ b, u64 *__restrict__ out,
                                                    u64 *__restrict__ acc, uint32_t count, uint32_t bstride, uint32_t nl,
                                                    uint32_t logN, lm_mods mods, lm_ninv_t tfac) {
    const size_t N = (size_t)1 << logN;
    const uint32_t npairs = 1u << (logN - 1), nblk = mr_blocks_per_limb(logN);
    const uint32_t k = blockIdx.x % nblk, lc = blockIdx.x / nblk, c = lc % count, limb = lc / count;
    const mod_t md = mods.m[limb];
    const tw_t W = tfac.t[limb];
    const u64 q = md.q, nq = 0 - md.q;
    const u64 *a0p = a + ((size_t)c * 2 * nl + limb) * N, *a1p = a0p + (size_t)nl * N;
    const u64 *b0p = b + ((size_t)c * bstride * 2 * nl + limb) * N, *b1p = b0p + (size_t)nl * N;
    constexpr uint32_t NP = RELIN ? 2 : 3;
    u64 *o0 = out + ((size_t)c * NP * nl + limb) * N;
    ulonglong2 av0[2], av1[2], bv0[2], bv1[2];
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t p = k * LM_MR_PAIRS + threadIdx.x + 256 * u;
        if (p < npairs) {
            av0[u] = *reinterpret_cast<const ulonglong2 *>(a0p + 2 * p);
            av1[u] = *reinterpret_cast<const ulonglong2 *>(a1p + 2 * p);
            bv0[u] = *reinterpret_cast<const ulonglong2 *>(b0p + 2 * p);
            bv1[u] = *reinterpret_cast<const ulonglong2 *>(b1p + 2 * p);
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t p = k * LM_MR_PAIRS + threadIdx.x + 256 * u;
        if (p >= npairs) continue;
        ulonglong2 r0, r1, r2;
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const u64 a0 = lm_shoup3<true>(e ? av0[u].y : av0[u].x, W.w, W.wp, nq); // a0 * T * 2^64, [0, 3q)
            const u64 a1 = lm_shoup3<true>(e ? av1[u].y : av1[u].x, W.w, W.wp, nq);
            const u64 b0 = e ? bv0[u].y : bv0[u].x, b1 = e ? bv1[u].y : bv1[u].x;
            u64 lo, hi, lo2, hi2;
            mul128(a0, b0, lo, hi);
            const u64 d0 = lm_mont_reduce_wide(lo, hi, q, md.qneg, md.qinv64, 3);
            mul128(a1, b1, lo, hi);
            const u64 d2 = lm_mont_reduce_wide(lo, hi, q, md.qneg, md.qinv64, 3);
            mul128(a0, b1, lo, hi);
            mul128(a1, b0, lo2, hi2);
            lo += lo2;
            hi += hi2 + (lo < lo2 ? 1 : 0);
            u64 d1 = lm_mont_reduce_wide(lo, hi, q, md.qneg, md.qinv64, 6);
            if constexpr (RELIN) d1 = lm_submod(d1, d2, q);
            if (e) r0.y = d0, r1.y = d1, r2.y = d2;
            else r0.x = d0, r1.x = d1, r2.x = d2;
        }
        *reinterpret_cast<ulonglong2 *>(o0 + 2 * p) = r0;
        *reinterpret_cast<ulonglong2 *>(o0 + (size_t)nl * N + 2 * p) = r1;
        if constexpr (RELIN) {
            u64 *c0 = acc + ((size_t)c * 2 * nl + limb) * N;
            ulonglong2 z;
            z.x = z.y = 0;
            *reinterpret_cast<ulonglong2 *>(c0 + 2 * p) = z;
            *reinterpret_cast<ulonglong2 *>(c0 + (size_t)nl * N + 2 * p) = r2;
        } else {
            *reinterpret_cast<ulonglong2 *>(o0 + (size_t)2 * nl * N + 2 * p) = r2;
        }
    }
}

// out (canonical: (d0, d1 - d2)) += ks (the rotation's lazy accumulator, [0, 2q): (k0, d2 + k1)), canonical.
// Both [count][2][nl][N]; the tensor kernel's block order.
__global__ __launch_bounds__(256) void k_relin_close(u64 *__restrict__ out, const u64 *__restrict__ ks, uint32_t count, uint32_t nl,
                                                     uint32_t logN, lm_mods mods) {
    const size_t N = (size_t)1 << logN;
    const uint32_t npairs = 1u << (logN - 1), nblk = mr_blocks_per_limb(logN);
    const uint32_t k = blockIdx.x % nblk, lc = blockIdx.x / nblk, c = lc % count, limb = lc / count;
    const u64 q = mods.m[limb].q;
    const size_t base = ((size_t)c * 2 * nl + limb) * N;
    ulonglong2 x[2][2], y[2][2];
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t p = k * LM_MR_PAIRS + threadIdx.x + 256 * u;
        if (p < npairs)
#pragma unroll
            for (uint32_t w = 0; w < 2; w++) {
                x[u][w] = *reinterpret_cast<const ulonglong2 *>(out + base + (size_t)w * nl * N + 2 * p);
                y[u][w] = *reinterpret_cast<const ulonglong2 *>(ks + base + (size_t)w * nl * N + 2 * p);
            }
    }
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t p = k * LM_MR_PAIRS + threadIdx.x + 256 * u;
        if (p < npairs)
#pragma unroll
            for (uint32_t w = 0; w < 2; w++) {
                ulonglong2 r; // < q + 2q
                r.x = lm_csub(lm_csub(x[u][w].x + y[u][w].x, 2 * q), q);
                r.y = lm_csub(lm_csub(x[u][w].y + y[u][w].y, 2 * q), q);
                *reinterpret_cast<ulonglong2 *>(out + base + (size_t)w * nl * N + 2 * p) = r;
            }
    }
}

// -------------------------------------------------------------------- host side
namespace {

lm_ninv_t tensor_consts(const lumen_ctx *ctx) {
    lm_ninv_t f;
    for (uint32_t l = 0; l < LM_MAX_LIMBS; l++) {
        const uint64_t q = ctx->mod[l < ctx->L ? l : 0];
        f.t[l] = h_tw(h_mulmod(ctx->T % q, h_r64_mod(q), q), q);
    }
    return f;
}

uint32_t mr_grid(const lumen_ctx *ctx, uint32_t count, uint32_t nl) { return nl * count * mr_blocks_per_limb(ctx->logN); }

// a, b: `count` ciphertexts of nl limbs from these pointers on (b: one, with bcast); out / acc as k_mul_tensor takes them
template <bool RELIN>
int launch_tensor(lumen_ctx *ctx, const u64 *a, const u64 *b, bool bcast, u64 *out, u64 *acc, uint32_t count, uint32_t nl) {
    lm_prof_scope ps(ctx, "mul_tensor", count);
    hipLaunchKernelGGL(k_mul_tensor<RELIN>, dim3(mr_grid(ctx, count, nl)), dim3(256), 0, ctx->stream, a, b, out, acc, count,
                       bcast ? 0u : 1u, nl, ctx->logN, ctx->mods, tensor_consts(ctx));
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// what both entry points ask of their operands
int check_operands(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, const char *what) {
    if (int rc = check_level_of_chain(ctx, a, what)) return rc;
    LM_FULL_WIDTH(ctx, b, what);
    LM_CHECK(ctx, a->nl == b->nl, "%s: the operands have different levels (%u and %u limbs)", what, a->nl, b->nl);
    LM_CHECK(ctx, a->count == b->count || b->count == 1,
             "%s: count mismatch: %u ciphertexts times %u (the second operand has as many, or one)", what, a->count, b->count);
    LM_CHECK(ctx, (uint64_t)a->count * a->nl * mr_blocks_per_limb(ctx->logN) < (1ull << 31), "%s: %u ciphertexts are more than one launch takes",
             what, a->count);
    return 0;
}

} // namespace

extern "C" int lumen_mul_tensor(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, uint64_t *host_out) {
    LM_CHECK(nullptr, ctx && a && b && host_out, "lumen_mul_tensor: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_operands(ctx, a, b, "lumen_mul_tensor")) return rc;
    if (!a->count) return 0;
    const size_t words = (size_t)a->count * 3 * a->nl * ctx->N;
    lm_dev<u64> d;
    if (int rc = d.alloc(ctx, words, "the degree-2 ciphertexts of lumen_mul_tensor")) return rc;
    d.release_on(ctx->stream, false);
    if (int rc = launch_tensor<false>(ctx, a->d, b->d, b->count != a->count, d.get(), nullptr, a->count, a->nl)) return rc;
    return lm_d2h(ctx, host_out, d.get(), words * 8, true);
}

extern "C" int lumen_mul_relin(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, lumen_set **out) {
    LM_CHECK(nullptr, ctx && a && b && out, "lumen_mul_relin: NULL argument");
    LM_ENTER(ctx);
    LM_CHECK(ctx, ctx->K >= 1, "parameters have no special primes: key switching unavailable");
    if (int rc = check_operands(ctx, a, b, "lumen_mul_relin")) return rc;
    KsRun run;
    if (int rc = ks_run_open(ctx, a->count, a->nl, 2, true, &run)) return rc; // (refuses K > 2, as InnerSum does)
    const std::shared_ptr<lm_galois_key> rlk = lm_relin_key(ctx); // kept alive for the call
    LM_CHECK(ctx, rlk && rlk->d_key, "lumen_mul_relin: no relinearisation key loaded (lumen_load_relin_key)");
    const uint32_t nl = a->nl, count = a->count;
    const bool bcast = b->count != count;
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, count, nl, &o)) return rc;
    lm_set_guard og(ctx, o);
    const size_t ctw = (size_t)2 * nl * ctx->N;
    if (int rc = ks_run_scratch(ctx, &run)) return rc;
    // batches of a group alternate between the lanes, each in its own slice of the group's accumulators, as in
    // matrixInnerSumEval; everything of a batch -- tensor, key switch, closing pass -- stays on its lane
    auto batch = [&](uint32_t g0, uint32_t first, uint32_t B, const KsScratch &s, u64 *d2) {
        const size_t at = (size_t)(g0 + first) * ctw;
        if (int rc = launch_tensor<true>(ctx, a->d + at, bcast ? b->d : b->d + at, bcast, o->d + at, d2, B, nl)) return rc;
        if (int rc = rotate_accumulate(ctx, d2, s.acc2, B, *rlk, run.tb, s)) return rc;
        lm_prof_scope ps(ctx, "relin_close", B);
        hipLaunchKernelGGL(k_relin_close, dim3(mr_grid(ctx, B, nl)), dim3(256), 0, ctx->stream, o->d + at, s.acc2, B, nl, ctx->logN,
                           ctx->mods);
        LM_HIP(ctx, hipGetLastError());
        return 0;
    };
    if (int rc = ks_run(ctx, run, count, ctw, batch)) return rc;
    ctx->mul_counter += count; // as lumen_mul_plain counts its products; lumen_mul_tensor, a parity hook, does not
    *out = og.release();
    return 0;
}
