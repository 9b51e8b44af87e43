// Ciphertext x plaintext product, MulNew(ct, pt) (fhe/ligero.go:319): lumen_mul_plain, and step 0 of
// matrixInnerSumEval (lm_innersum.hip, through lm_ks_host.h).
#include <cstring>

#include "lm_ks_host.h"

// ---- step 0: MulNew(ct, pt): out = ct (.) (pt * T)
// The plaintext arrives once per call as raw residues; k_pt_prepare turns it into the multiplier in
// Montgomery form, ptM = pt * T * 2^64 mod q_l (one Montgomery product with c_l = T * 2^128 mod q_l),
// so that the product over the matrix is one 64x64 multiplication and one Montgomery reduction per
// residue, canonical result.
// A plaintext over Q and P (a diagonal of lumen_lintrans_load) has np = nl + K limbs BY POSITION: limb t >= nl is the
// modulus pshift = L - nl further on (ks_mod_at); a plaintext over Q alone has np = nl.
struct pt_consts_t {
    u64 c[LM_MAX_LIMBS]; // T * 2^128 mod the modulus of position l
};
__global__ void k_pt_prepare(const u64 *__restrict__ pt, u64 *__restrict__ ptM, uint32_t logN, uint32_t nl, uint32_t np,
                             uint32_t pshift, lm_mods mods, pt_consts_t pc) {
    const size_t total = (size_t)np << logN;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t limb = (uint32_t)(i >> logN), mi = ks_mod_at(limb, nl, pshift);
        u64 lo, hi;
        mul128(pt[i], pc.c[limb], lo, hi);
        ptM[i] = lm_mont_reduce(lo, hi, mods.m[mi].q, mods.m[mi].qneg);
    }
}
__global__ void k_mul_plain(const u64 *__restrict__ ct, u64 *__restrict__ out, const u64 *__restrict__ ptM,
                            size_t words, uint32_t logN, uint32_t nl, lm_mods mods) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t N = (size_t)1 << logN;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += stride) {
        const uint32_t limb = (uint32_t)((i >> logN) % nl);
        const size_t k = i & (N - 1);
        u64 lo, hi;
        mul128(ct[i], ptM[(size_t)limb * N + k], lo, hi);
        out[i] = lm_mont_reduce(lo, hi, mods.m[limb].q, mods.m[limb].qneg);
    }
}

int upload_ptT(lumen_ctx *ctx, const uint64_t *pt, uint32_t nl, u64 **out) {
    // pt * T in Montgomery form: the multiplier MulNew(ct, pt) applies
    // ([LATTIGO-RECALL] bgv tensorStandard, ciphertext x plaintext branch).  The host only checks the
    // range and stages the residues in pinned memory; the products are formed on the device, and the
    // call does not wait for the copy.
    const uint32_t N = ctx->N;
    const size_t words = (size_t)nl * N;
    u64 *h = (u64 *)lm_stage(ctx, words * sizeof(u64));
    u64 *draw = (u64 *)lm_scratch(ctx, "pt_raw", words * sizeof(u64));
    u64 *d = (u64 *)lm_scratch(ctx, "ptT", words * sizeof(u64));
    if (!h || !draw || !d) return 1;
    for (uint32_t l = 0; l < nl; l++) {
        const uint64_t q = ctx->mod[l];
        const uint64_t *src = pt + (size_t)l * N;
        uint64_t bad = 0;
        for (uint32_t k = 0; k < N; k++) bad |= (uint64_t)(src[k] >= q);
        if (bad) return lm_fail(ctx, "plaintext residue out of range at limb %u", l);
        memcpy(h + (size_t)l * N, src, (size_t)N * sizeof(u64));
    }
    LM_HIP(ctx, hipMemcpyAsync(draw, h, words * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    LM_HIP(ctx, hipEventRecord(ctx->ev_stage, ctx->stream));
    if (int rc = launch_pt_prepare(ctx, draw, d, nl, nl)) return rc;
    *out = d;
    return 0;
}

int launch_pt_prepare(lumen_ctx *ctx, const u64 *raw, u64 *ptM, uint32_t nl, uint32_t np) {
    pt_consts_t pc;
    memset(&pc, 0, sizeof(pc));
    for (uint32_t l = 0; l < np; l++) {
        const uint64_t q = ctx->mod[ks_mod_at(l, nl, ctx->L - nl)];
        const uint64_t r = h_r64_mod(q);
        pc.c[l] = h_mulmod(ctx->T % q, h_mulmod(r, r, q), q);
    }
    hipLaunchKernelGGL(k_pt_prepare, dim3(256), dim3(256), 0, ctx->stream, raw, ptM, ctx->logN, nl, np, ctx->L - nl, ctx->mods, pc);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

int launch_mul_plain(lumen_ctx *ctx, const u64 *ct, u64 *out, const u64 *ptT, size_t words, uint32_t nl,
                     uint32_t ncts) {
    lm_prof_scope ps(ctx, "mul_plain", ncts);
    hipLaunchKernelGGL(k_mul_plain, dim3(4096), dim3(256), 0, ctx->stream, ct, out, ptT, words, ctx->logN, nl,
                       ctx->mods);
    LM_HIP(ctx, hipGetLastError());
    ctx->mul_counter += ncts;
    return 0;
}

extern "C" int lumen_mul_plain(lumen_ctx *ctx, const lumen_set *in, const uint64_t *pt, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && pt && out, "lumen_mul_plain: NULL argument");
    LM_ENTER(ctx);
    LM_FULL_WIDTH(ctx, in, "lumen_mul_plain");
    u64 *ptT = nullptr;
    if (int rc = upload_ptT(ctx, pt, in->nl, &ptT)) return rc;
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, in->count, in->nl, &o)) return rc;
    lm_set_guard og(ctx, o);
    if (in->words)
        if (int rc = launch_mul_plain(ctx, in->d, o->d, ptT, in->words, in->nl, in->count)) return rc;
    *out = og.release();
    return 0;
}
