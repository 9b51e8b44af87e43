// Client-side key generation (cmd/client/main.go:74-81, fhe/ring_switch.go:16-57): KeyGenerator.GenKeyPairNew,
// GenRelinearizationKeyNew, GenGaloisKeysNew and the ring switch's GenEvaluationKeyNew [LATTIGO-RECALL], every
// key an array of gadget entries
//     (b, a) = (NTT(e) - a * s_out + fac * s_in,  a),      a uniform mod q_m, e Gaussian, over the whole basis QP
// in exactly the layouts lumen_load_public_key / lumen_load_galois_key[_ex] / lumen_load_ringswitch_key take.
//
// THE SAMPLING CONTRACT.  Everything is deterministic in (seed, key id, entry, limb, coefficient): keys generated one
// at a time, in one batched call or on another GPU are the same bytes.
//     keystream(I, s) = ChaCha20(key = seed, nonce = LE64(I) || LE32(s), counter = 0, 1, ...)   (lm_sample.hip)
//     sample index     I(key_id, e) = key_id * 4096 + e,   e = i * pw2 + j the gadget entry (RNS digit i, power-of-two
//                      digit j; pw2 = 1 everywhere but the ring-switch key with K <= 1)
//     key ids          secret 0, public 1, relinearisation 2, ring switch 3, Galois key of element g: 0x10000 + g
//     ternary secret   s = stream 0 of I(0, 0), word w -> ((w * 3) >> 32) - 1          (lo_det_small)
//     small secret     of the ring switch: the first n = 2^log_n_small coefficients of stream 0 of I(3, 0)
//     Gaussian error   of entry e: stream 1 of I(key_id, e), the CDT rule of the encryptor; ONE N-coefficient sample
//                      per entry, extended to every limb
//     uniform a        for limb m (Q limbs, then P limbs) of entry e: stream 16 + m of I(key_id, e) read as little-endian
//                      64-bit words; attempt t = 0, 1, ... for coefficient k is word number t * N + k; the first attempt
//                      with x < 2^64 - (2^64 mod q_m) is kept and a[k] = x mod q_m (unbiased; a redraw has probability
//                      below 2^-6).  a is sampled directly in the NTT domain.
// A keygen seed is key material (OS CSPRNG) and is used for nothing else: streams 0-2 of an index are the ones
// lumen_encrypt_* would draw, so a keygen seed must never be passed to lumen_encrypt_*.
//
// ADDITION: SEEDED KEYS (lumen_keygen_galois_seeded / lumen_keygen_relin_seeded; cmd/client/main.go:74-81 posts the keys
// whole, the `/keys` handler of cmd/server/main.go:66 receives them).  A seeded key takes two 32-byte seeds:
//     seed             key material, as above: the error of entry e is stream 1 of I(key_id, e) under seed; the secret is
//                      the context's generated secret
//     a_seed           PUBLIC: a for limb m of entry e is stream 16 + m of the SAME index I(key_id, e) under a_seed, by the
//                      rule above (attempt t of coefficient k is word t * N + k, the first x < 2^64 - (2^64 mod q_m) is kept
//                      as x mod q_m)
//     b                = NTT(e) - a * s_out + fac * s_in as before; only b leaves the device
// So a seeded key expanded by the server (lm_ks_key.hip: k_key_expand draws a under a_seed) is word for word the pair
// (b, a), and with a_seed == seed b would be exactly lumen_keygen_galois's -- refused, because it would publish the
// secret seed.
// ONE `a` PER KEY.  The error depends on (seed, key id, entry) alone, not on a_seed, so generating a key again under the
// same two seeds gives the same words -- harmless.  What must never happen is the SAME key (seed, key id) published under
// two different `a`: two seeded forms under two a_seeds, or the full form (whose a is drawn under seed) beside a seeded
// one.  Their b halves differ by (a2 - a1) * s_out pointwise, both a are public, and the secret follows.  So a keygen
// seed gets ONE a_seed for its whole life (drawn with it from the OS CSPRNG), and one of the two forms per key.  The
// library sees one call at a time and cannot check this; the host mirror's KeyGenerator does (fhe.hpp).
//
// The samples come from the shared sampler (lm_sample.hip: k_sample_small, k_sample_uniform).  Kernels here:
// k_keygen_secret_ntt (NTT(s) and NTT(skNew(X^(N/n))) over QP), k_keygen_gather / _square / _shoup (the secret's
// images), k_keygen_evk (one workgroup per (key, entry, limb): lift + NTT of e, the products fused into the store) and
// k_keygen_evk_seeded, the same body whose storer draws a for itself and stores b alone.
#include <cstring>

#include "lm_enc_host.h"

// NTT of small polynomials over QP: slot j of `small` ([nslots][*] int8) -> mont[j][m] = NTT(.) * 2^64 mod q_m (the form
// the storer of k_keygen_evk multiplies with) and, when given, std[j][m] = NTT(.).  loggap > 0: the polynomial is
// skNew(X^gap), coefficient i * gap = small[i].  One workgroup per (limb, slot).
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_lds(LOGN)) void k_keygen_secret_ntt(const int8_t *__restrict__ small, u64 *__restrict__ mont,
                                                                       u64 *__restrict__ stdf, uint32_t nslots, uint32_t LK,
                                                                       uint32_t loggap, lm_mods mods, lm_ninv_t rmont,
                                                                       const tw_t *__restrict__ tw_all) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x, m = blockIdx.x / nslots, j = blockIdx.x % nslots;
    const lm_qc qc = lm_make_qc(mods.m[m]);
    const int8_t *s = small + (size_t)j * N;
    u64 *om = mont + ((size_t)j * LK + m) * N, *os = stdf ? stdf + ((size_t)j * LK + m) * N : nullptr;
    const tw_t R = rmont.t[m];
    const uint32_t gmask = (1u << loggap) - 1;
    auto ld = [&](uint32_t i) -> u64 {
        if (i & gmask) return 0;
        return lm_lift_small(s[i >> loggap], &qc.q);
    };
    auto st = [&](uint32_t i0, const u64 *v, int n) {
        u64 a[8], b[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < n) {
                a[k] = lm_reduce_s(v[k], qc.q, qc.nq, qc.qinv64);
                b[k] = lm_shoup_cs(a[k], R, qc.q, qc.nq);
            }
        lm_store_run(om, i0, b, n);
        if (os) lm_store_run(os, i0, a, n);
    };
    lm_ntt_forward<LOGN>(sm, tw_all + (size_t)m * N, qc, tid, ld, st);
}

// out[key][m][k] = s[m][index[key][k]]: pi_{g^-1}(s) in the NTT domain (lo_keygen_galois: the index table of g^-1 mod 2N)
__global__ __launch_bounds__(256) void k_keygen_gather(const u64 *__restrict__ s, const uint32_t *__restrict__ index,
                                                       u64 *__restrict__ out, uint32_t LK, uint32_t logN, size_t total) {
    const size_t N = (size_t)1 << logN;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const size_t k = g & (N - 1), row = g >> logN, m = row % LK, key = row / LK;
        out[g] = s[(m << logN) + index[(key << logN) + k]];
    }
}

// out[m][k] = s[m][k]^2 (Montgomery form in, Montgomery form out): the relinearisation key's s_in
__global__ __launch_bounds__(256) void k_keygen_square(const u64 *__restrict__ s, u64 *__restrict__ out, uint32_t logN,
                                                       size_t total, lm_mods mods) {
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const mod_t md = mods.m[g >> logN];
        u64 lo, hi;
        mul128(s[g], s[g], lo, hi);
        out[g] = lm_mont_reduce(lo, hi, md.q, md.qneg);
    }
}

// the decryptor's table: tw[l][k] = (x, floor(x * 2^64 / q_l)) for x = stdf[l][k], by long division (x < q < 2^58)
__global__ __launch_bounds__(256) void k_keygen_shoup(const u64 *__restrict__ stdf, tw_t *__restrict__ tw, uint32_t logN,
                                                      size_t total, lm_mods mods) {
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const u64 q = mods.m[g >> logN].q, x = stdf[g];
        u64 r = x, wp = 0;
        for (int b = 0; b < 64; b++) {
            r <<= 1;
            const u64 ge = r >= q;
            r -= ge ? q : 0;
            wp = (wp << 1) | ge;
        }
        tw_t t;
        t.w = x, t.wp = wp;
        tw[g] = t;
    }
}

// One workgroup per (key, entry, limb), dealt limb-major like k_enc_u: one twiddle table stays hot per XCD.
//   small [nitems][N] int8 errors; out [nitems][b|a][LK][N] with the `a` halves filled by k_sample_uniform;
//   s_out + key * sout_stride and s_in: [LK][N] secrets in Montgomery form; fac [nent][LK]: P * 2^(w j) mod q_m on the
//   Q limbs of the entry's RNS digit, 0 elsewhere (NULL: 0 everywhere, the public key).
//   b = NTT(e) - a * s_out + fac * s_in, canonical; MONT: both halves leave multiplied by 2^64 mod q_m.
// The SEEDED form (lumen_keygen_*_seeded) has no `a` in memory at all: out is the packed [nitems][LK][N] block of the b
// halves and the storer draws the run's `a` itself under the public seed of `dr` -- a run of the last pass is one
// ChaCha20 block of the limb's stream (half of one at N = 2^8), k_sample_uniform's rule through lm_uniform_run.
struct kg_draw_t {
    const u64 *index; // [nitems] sample indices I(key_id, e)
    enc_seed_t seed;  // a_seed
    kg_lim_t lim;
};
template <int LOGN, bool SEEDED>
__device__ __forceinline__ void kg_evk_body(u64 *sm, const int8_t *__restrict__ small, u64 *__restrict__ out,
                                            const u64 *__restrict__ s_out, size_t sout_stride, const u64 *__restrict__ s_in,
                                            const u64 *__restrict__ fac, uint32_t nitems, uint32_t nent, uint32_t LK,
                                            uint32_t mont, const lm_mods &mods, const lm_ninv_t &rmont,
                                            const tw_t *__restrict__ tw_all, const kg_draw_t *dr) {
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x, m = blockIdx.x / nitems, it = blockIdx.x % nitems, key = it / nent, e = it % nent;
    const mod_t md = mods.m[m];
    const lm_qc qc = lm_make_qc(md);
    const int8_t *se = small + (size_t)it * N;
    u64 *ob = out + ((size_t)it * (SEEDED ? 1 : 2) * LK + m) * N, *oa = SEEDED ? nullptr : ob + (size_t)LK * N;
    const u64 *so = s_out + (size_t)key * sout_stride + (size_t)m * N, *si = s_in ? s_in + (size_t)m * N : nullptr;
    const u64 f = fac ? fac[(size_t)e * LK + m] : 0;
    const tw_t R = rmont.t[m];
    u64 I = 0, bound = 0;
    if constexpr (SEEDED) I = dr->index[it], bound = dr->lim.t[m];
    auto ld = [&](uint32_t i) -> u64 { return lm_lift_small(se[i], &qc.q); };
    auto st = [&](uint32_t i0, const u64 *v, int n) {
        u64 a[8], b[8], x[8], y[8];
        if constexpr (SEEDED)
            lm_uniform_run<lm_fwd_run<LOGN>()>(dr->seed, I, LM_UNIFORM_STREAM + m, LOGN, i0, md.q, md.qinv64, bound, a);
        else
            lm_load_run(oa, i0, a, n);
        lm_load_run(so, i0, x, n);
        if (f) lm_load_run(si, i0, y, n);
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < n) {
                u64 lo, hi;
                mul128(qc.q - a[k], x[k], lo, hi); // -a * s_out * 2^64
                if (f) {
                    u64 l2, h2;
                    mul128(f, y[k], l2, h2);
                    lo += l2;
                    hi += h2 + (lo < l2);
                }
                u64 r = lm_mont_reduce_wide(lo, hi, md.q, md.qneg, md.qinv64, 2);
                r = lm_addmod(r, lm_reduce_s(v[k], qc.q, qc.nq, qc.qinv64), qc.q);
                if (mont) {
                    r = lm_shoup_cs(r, R, qc.q, qc.nq);
                    if constexpr (!SEEDED) a[k] = lm_shoup_cs(a[k], R, qc.q, qc.nq);
                }
                b[k] = r;
            }
        lm_store_run(ob, i0, b, n);
        if constexpr (!SEEDED)
            if (mont) lm_store_run(oa, i0, a, n);
    };
    lm_ntt_forward<LOGN>(sm, tw_all + (size_t)m * N, qc, tid, ld, st);
}
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_lds(LOGN)) void k_keygen_evk(const int8_t *__restrict__ small, u64 *__restrict__ out,
                                                                const u64 *__restrict__ s_out, size_t sout_stride,
                                                                const u64 *__restrict__ s_in, const u64 *__restrict__ fac,
                                                                uint32_t nitems, uint32_t nent, uint32_t LK, uint32_t mont,
                                                                lm_mods mods, lm_ninv_t rmont,
                                                                const tw_t *__restrict__ tw_all) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    kg_evk_body<LOGN, false>(sm, small, out, s_out, sout_stride, s_in, fac, nitems, nent, LK, mont, mods, rmont, tw_all, nullptr);
}
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_lds(LOGN)) void k_keygen_evk_seeded(const int8_t *__restrict__ small, u64 *__restrict__ out,
                                                                       const u64 *__restrict__ s_out, size_t sout_stride,
                                                                       const u64 *__restrict__ s_in, const u64 *__restrict__ fac,
                                                                       uint32_t nitems, uint32_t nent, uint32_t LK,
                                                                       uint32_t mont, lm_mods mods, lm_ninv_t rmont,
                                                                       const tw_t *__restrict__ tw_all, kg_draw_t dr) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    kg_evk_body<LOGN, true>(sm, small, out, s_out, sout_stride, s_in, fac, nitems, nent, LK, mont, mods, rmont, tw_all, &dr);
}

// ------------------------------------------------------------------------------------------------- host side
// NTT(s) over QP in Montgomery form, kept by the context (and its clones) for the other keygen calls
struct KgSecret {
    lm_dev<u64> d_mont;
    KgSecret() { d_mont.release_on(nullptr, true); } // zeroed (blocking) before the block is given back
};

// a device temporary of a call: the context's stream is waited for before the block is given back, and `secret` ones
// (s, its images, the errors) are zeroed on it first
template <class T>
static int kg_alloc(lumen_ctx *ctx, lm_dev<T> &d, size_t count, bool secret) {
    return d.release_on(ctx->stream, secret).alloc(ctx, count, "key generation");
}

static lm_ninv_t kg_rmont(const lumen_ctx *ctx) { // 2^64 mod q_m
    lm_ninv_t r;
    for (uint32_t t = 0; t < LM_MAX_LIMBS; t++) {
        const uint64_t q = ctx->mod[t < ctx->L + ctx->K ? t : 0];
        r.t[t] = h_tw(h_r64_mod(q), q);
    }
    return r;
}
template <int LOGN>
static int kg_secret_ntt_t(lumen_ctx *ctx, const int8_t *small, u64 *mont, u64 *stdf, uint32_t nslots, uint32_t loggap) {
    const uint32_t LK = ctx->L + ctx->K;
    lm_prof_scope ps(ctx, "keygen_secret_ntt", (uint64_t)nslots * LK);
    return lm_launch(ctx, k_keygen_secret_ntt<LOGN>, lm_geom_lds(LOGN), nslots * LK, small, mont, stdf, nslots, LK, loggap,
                     ctx->mods, kg_rmont(ctx), ctx->sh->tw_fwd.get());
}
template <int LOGN>
static int kg_evk_t(lumen_ctx *ctx, const int8_t *small, u64 *out, const u64 *s_out, size_t sout_stride, const u64 *s_in,
                    const u64 *fac, uint32_t nitems, uint32_t nent, uint32_t mont, const kg_draw_t *dr) {
    const uint32_t LK = ctx->L + ctx->K;
    lm_prof_scope ps(ctx, dr ? "keygen_evk_seeded" : "keygen_evk_ntt", (uint64_t)nitems * LK);
    if (dr)
        return lm_launch(ctx, k_keygen_evk_seeded<LOGN>, lm_geom_lds(LOGN), nitems * LK, small, out, s_out, sout_stride, s_in,
                         fac, nitems, nent, LK, mont, ctx->mods, kg_rmont(ctx), ctx->sh->tw_fwd.get(), *dr);
    return lm_launch(ctx, k_keygen_evk<LOGN>, lm_geom_lds(LOGN), nitems * LK, small, out, s_out, sout_stride, s_in, fac, nitems,
                     nent, LK, mont, ctx->mods, kg_rmont(ctx), ctx->sh->tw_fwd.get());
}

// nkeys keys of nent entries each in ONE launch of each kernel, then one download into the caller's buffer.
// s_out: the keys' own secrets, sout_stride words apart (0: shared); fac: host [nent][LK] or NULL.
// a_seed NULL: host_out takes [nitems][b|a][LK][N], `a` drawn under `seed` by k_sample_uniform.  a_seed given (the seeded
// keys): host_out takes the b halves alone, [nitems][LK][N], and `a` under a_seed exists only in the storer's registers.
static int kg_run(lumen_ctx *ctx, const uint8_t seed[32], const std::vector<u64> &key_ids, uint32_t nent, const u64 *s_out,
                  size_t sout_stride, const u64 *s_in, const std::vector<u64> *fac, uint32_t flags, uint64_t *host_out,
                  const uint8_t *a_seed = nullptr) {
    const uint32_t N = ctx->N, LK = ctx->L + ctx->K, nkeys = (uint32_t)key_ids.size(), nitems = nkeys * nent;
    const size_t out_words = (size_t)nitems * (a_seed ? 1 : 2) * LK * N;
    LM_CHECK(ctx, nent <= LM_KG_INDEX_STRIDE && (uint64_t)nitems * LK <= 65535, "key generation: %u keys of %u entries exceed one launch",
             nkeys, nent);
    std::vector<u64> tab(nitems); // sample indices, then the gadget factors
    for (uint32_t k = 0; k < nkeys; k++)
        for (uint32_t e = 0; e < nent; e++) tab[(size_t)k * nent + e] = key_ids[k] * LM_KG_INDEX_STRIDE + e;
    if (fac) tab.insert(tab.end(), fac->begin(), fac->end());
    lm_dev<u64> d_tab, d_out;
    lm_dev<int8_t> d_e;
    if (kg_alloc(ctx, d_tab, tab.size(), false) || kg_alloc(ctx, d_out, out_words, false) || kg_alloc(ctx, d_e, (size_t)nitems * N, true)) return 1;
    if (int rc = lm_h2d_staged(ctx, d_tab.get(), tab.data(), tab.size() * 8)) return rc;
    const u64 *d_index = d_tab.get(), *d_fac = fac ? d_index + nitems : nullptr;
    {
        lm_prof_scope ps(ctx, "keygen_sample", nitems);
        if (int rc = lm_sample_small(ctx, d_e.get(), d_index, 0, nitems, 1, 1, seed)) return rc;
    }
    kg_draw_t draw{};
    if (a_seed) {
        draw.index = d_index, draw.seed = lm_sample_seed(a_seed), draw.lim = lm_sample_lim(ctx, LK);
    } else {
        lm_prof_scope ps(ctx, "keygen_uniform", (uint64_t)nitems * LK);
        if (int rc = lm_sample_uniform(ctx, d_out.get() + (size_t)LK * N, (size_t)2 * LK * N, d_index, 0, nitems, LK, seed)) return rc;
    }
    if (int rc = lm_for_logn(ctx, ctx->logN, [&](auto k) {
            return kg_evk_t<k>(ctx, d_e.get(), d_out.get(), s_out, sout_stride, s_in, d_fac, nitems, nent,
                               (flags & LUMEN_KEY_MONTGOMERY) ? 1u : 0u, a_seed ? &draw : nullptr);
        }))
        return rc;
    lm_prof_scope ps(ctx, "keygen_download", nitems);
    return lm_d2h(ctx, host_out, d_out.get(), out_words * 8, true);
}

static std::shared_ptr<KgSecret> kg_secret_of(lumen_ctx *ctx) { return lm_ext_get<KgSecret>(ctx, "keygen_secret"); }
#define LM_KG_NEED_SECRET(ctx, hold, what) \
    LM_CHECK(ctx, hold, "%s: no generated secret on the context (lumen_keygen_secret)", what)

// gadget factors [nent = rns * pw2][LK]: P * 2^(w j) mod q_m for m < L inside RNS digit i, alpha = max(K, 1)
static std::vector<u64> kg_gadget(const lumen_ctx *ctx, uint32_t rns, uint32_t pw2, uint32_t w) {
    const uint32_t L = ctx->L, LK = L + ctx->K, alpha = ctx->K ? ctx->K : 1;
    std::vector<u64> fac((size_t)rns * pw2 * LK, 0);
    for (uint32_t i = 0; i < rns; i++)
        for (uint32_t j = 0; j < pw2; j++)
            for (uint32_t m = i * alpha; m < L && m < (i + 1) * alpha; m++) {
                const uint64_t q = ctx->mod[m];
                fac[((size_t)i * pw2 + j) * LK + m] = h_mulmod(h_p_mod(ctx, q), h_powmod(2, (uint64_t)w * j, q), q);
            }
    return fac;
}

extern "C" int lumen_keygen_secret(lumen_ctx *ctx, const uint8_t seed[32], uint64_t *sk) {
    LM_CHECK(nullptr, ctx, "lumen_keygen_secret: NULL ctx");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_keygen_secret");
    LM_CHECK(ctx, seed, "lumen_keygen_secret: NULL argument");
    const uint32_t N = ctx->N, L = ctx->L, LK = L + ctx->K;
    const size_t words = (size_t)LK * N;
    auto sp = std::make_shared<KgSecret>();
    // d_sk, the decryptor's table: the first L limbs, exactly what lumen_load_secret_key would hold
    lm_dev<tw_t> d_sk;
    lm_dev<u64> d_std;
    lm_dev<int8_t> d_small;
    if (sp->d_mont.alloc(ctx, words, "the generated secret") || d_sk.alloc(ctx, (size_t)L * N, "the secret key")) return 1;
    if (kg_alloc(ctx, d_small, N, true) || kg_alloc(ctx, d_std, words, true)) return 1;
    if (int rc = lm_sample_small(ctx, d_small.get(), nullptr, LM_KG_ID_SECRET * LM_KG_INDEX_STRIDE, 1, 0, 1, seed)) return rc;
    if (int rc = lm_for_logn(ctx, ctx->logN, [&](auto k) {
            return kg_secret_ntt_t<k>(ctx, d_small.get(), sp->d_mont.get(), d_std.get(), 1, 0);
        }))
        return rc;
    hipLaunchKernelGGL(k_keygen_shoup, dim3(256), dim3(256), 0, ctx->stream, d_std.get(), d_sk.get(), ctx->logN, (size_t)L * N,
                       ctx->mods);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && sk) {
        if (lm_d2h(ctx, sk, d_std.get(), words * 8, true)) e = hipErrorUnknown;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return lm_fail(ctx, "lumen_keygen_secret failed: %s", hipGetErrorString(e));
    lm_install_secret_key_dev(ctx, std::move(d_sk));
    lm_ext_put(ctx, "keygen_secret", sp);
    return 0;
}

extern "C" int lumen_keygen_public(lumen_ctx *ctx, const uint8_t seed[32], uint64_t *pk) {
    LM_CHECK(nullptr, ctx, "lumen_keygen_public: NULL ctx");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_keygen_public");
    LM_CHECK(ctx, seed && pk, "lumen_keygen_public: NULL argument");
    const std::shared_ptr<KgSecret> s = kg_secret_of(ctx);
    LM_KG_NEED_SECRET(ctx, s, "lumen_keygen_public");
    return kg_run(ctx, seed, {LM_KG_ID_PUBLIC}, 1, s->d_mont.get(), 0, nullptr, nullptr, 0, pk);
}

// The two switching keys in either form.  a_seed NULL: the full key under `seed` alone, out [..][b|a][L+K][N].  a_seed given:
// the b halves of the seeded key, out [..][L+K][N] (THE SAMPLING CONTRACT: a under a_seed, which must differ from seed).
#define LM_KG_REFUSE_EQUAL_SEEDS(ctx, what, seed, a_seed)                                                              \
    LM_CHECK(ctx, !(a_seed) || memcmp(seed, a_seed, 32) != 0,                                                            \
             "%s: the two seeds are equal (a_seed is public: the server could regenerate e)", what)

// the seeded entry points' own refusal, ahead of the shared helper (where a NULL a_seed means the full form)
#define LM_KG_NEED_A_SEED(ctx, a_seed, what)              \
    if ((ctx) && !(a_seed)) {                             \
        LM_ENTER(ctx);                                    \
        return lm_fail(ctx, "%s: NULL argument", what);   \
    }

static int kg_relin(lumen_ctx *ctx, const char *what, const uint8_t *seed, const uint8_t *a_seed, uint64_t *out, uint32_t flags) {
    LM_CHECK(nullptr, ctx, "%s: NULL ctx", what);
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, what);
    LM_CHECK(ctx, seed && out, "%s: NULL argument", what);
    const std::shared_ptr<KgSecret> s = kg_secret_of(ctx);
    LM_KG_NEED_SECRET(ctx, s, what);
    LM_CHECK(ctx, ctx->K >= 1, "%s: parameters have no special primes: key switching unavailable", what);
    LM_CHECK(ctx, !(flags & ~(uint32_t)LUMEN_KEY_MONTGOMERY), "%s: unknown flags 0x%x", what, flags);
    LM_KG_REFUSE_EQUAL_SEEDS(ctx, what, seed, a_seed);
    const uint32_t N = ctx->N, L = ctx->L, K = ctx->K, LK = L + K, beta = (L + K - 1) / K;
    const size_t words = (size_t)LK * N;
    lm_dev<u64> d_s2;
    if (kg_alloc(ctx, d_s2, words, true)) return 1;
    hipLaunchKernelGGL(k_keygen_square, dim3(256), dim3(256), 0, ctx->stream, s->d_mont.get(), d_s2.get(), ctx->logN, words,
                       ctx->mods);
    LM_HIP(ctx, hipGetLastError());
    const std::vector<u64> fac = kg_gadget(ctx, beta, 1, 0);
    return kg_run(ctx, seed, {LM_KG_ID_RELIN}, beta, s->d_mont.get(), 0, d_s2.get(), &fac, flags, out, a_seed);
}

static int kg_galois(lumen_ctx *ctx, const char *what, const uint8_t *seed, const uint8_t *a_seed, const uint64_t *gal_els,
                     uint32_t count, uint64_t *out, uint32_t flags) {
    LM_CHECK(nullptr, ctx, "%s: NULL ctx", what);
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, what);
    LM_CHECK(ctx, seed && (count == 0 || (gal_els && out)), "%s: NULL argument", what);
    const std::shared_ptr<KgSecret> s = kg_secret_of(ctx);
    LM_KG_NEED_SECRET(ctx, s, what);
    LM_CHECK(ctx, ctx->K >= 1, "%s: parameters have no special primes: key switching unavailable", what);
    LM_CHECK(ctx, !(flags & ~(uint32_t)LUMEN_KEY_MONTGOMERY), "%s: unknown flags 0x%x", what, flags);
    LM_KG_REFUSE_EQUAL_SEEDS(ctx, what, seed, a_seed);
    const uint32_t N = ctx->N, L = ctx->L, K = ctx->K, LK = L + K, beta = (L + K - 1) / K;
    const uint64_t mask = 2ull * N - 1;
    for (uint32_t i = 0; i < count; i++)
        LM_CHECK(ctx, (gal_els[i] & 1) && gal_els[i] <= mask, "%s: Galois element %llu is not an odd residue mod 2N", what,
                 (unsigned long long)gal_els[i]);
    if (!count) return 0;
    // s_out = pi_{g^-1}(s): a gather with the automorphism's index table of g^-1 ([LATTIGO-RECALL] AutomorphismNTTIndex)
    std::vector<uint32_t> index((size_t)count * N);
    std::vector<u64> ids(count);
    for (uint32_t c = 0; c < count; c++) {
        const uint64_t g = gal_els[c];
        uint64_t inv = 1;
        for (int i = 0; i < 6; i++) inv = (inv * (2 - g * inv)) & mask;
        for (uint32_t i = 0; i < N; i++) {
            const uint64_t t1 = 2ull * h_bitrev(i, (int)ctx->logN) + 1;
            index[(size_t)c * N + i] = h_bitrev((uint32_t)((((inv * t1) & mask) - 1) >> 1), (int)ctx->logN);
        }
        ids[c] = LM_KG_ID_GALOIS + g;
    }
    const size_t words = (size_t)count * LK * N;
    lm_dev<uint32_t> d_index;
    lm_dev<u64> d_sout;
    if (kg_alloc(ctx, d_index, index.size(), false) || kg_alloc(ctx, d_sout, words, true)) return 1;
    LM_HIP(ctx, hipMemcpyAsync(d_index.get(), index.data(), index.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    LM_HIP(ctx, hipStreamSynchronize(ctx->stream)); // `index` is pageable host memory
    hipLaunchKernelGGL(k_keygen_gather, dim3(1024), dim3(256), 0, ctx->stream, s->d_mont.get(), d_index.get(), d_sout.get(),
                       LK, ctx->logN, words);
    LM_HIP(ctx, hipGetLastError());
    const std::vector<u64> fac = kg_gadget(ctx, beta, 1, 0);
    return kg_run(ctx, seed, ids, beta, d_sout.get(), (size_t)LK * N, s->d_mont.get(), &fac, flags, out, a_seed);
}

extern "C" int lumen_keygen_relin(lumen_ctx *ctx, const uint8_t seed[32], uint64_t *evk, uint32_t flags) {
    return kg_relin(ctx, "lumen_keygen_relin", seed, nullptr, evk, flags);
}
extern "C" int lumen_keygen_galois(lumen_ctx *ctx, const uint8_t seed[32], const uint64_t *gal_els, uint32_t count,
                                   uint64_t *evk, uint32_t flags) {
    return kg_galois(ctx, "lumen_keygen_galois", seed, nullptr, gal_els, count, evk, flags);
}
extern "C" int lumen_keygen_relin_seeded(lumen_ctx *ctx, const uint8_t seed[32], const uint8_t a_seed[32], uint64_t *b_out,
                                         uint32_t flags) {
    LM_KG_NEED_A_SEED(ctx, a_seed, "lumen_keygen_relin_seeded");
    return kg_relin(ctx, "lumen_keygen_relin_seeded", seed, a_seed, b_out, flags);
}
extern "C" int lumen_keygen_galois_seeded(lumen_ctx *ctx, const uint8_t seed[32], const uint8_t a_seed[32],
                                          const uint64_t *gal_els, uint32_t count, uint64_t *b_out, uint32_t flags) {
    LM_KG_NEED_A_SEED(ctx, a_seed, "lumen_keygen_galois_seeded");
    return kg_galois(ctx, "lumen_keygen_galois_seeded", seed, a_seed, gal_els, count, b_out, flags);
}

extern "C" int lumen_keygen_ringswitch(lumen_ctx *ctx, const uint8_t seed[32], uint32_t log_n_small, uint32_t base_two_w,
                                       uint64_t *key, size_t key_words, int8_t *sk_small) {
    LM_CHECK(nullptr, ctx, "lumen_keygen_ringswitch: NULL ctx");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_keygen_ringswitch");
    LM_CHECK(ctx, seed && key && sk_small, "lumen_keygen_ringswitch: NULL argument");
    const std::shared_ptr<KgSecret> s = kg_secret_of(ctx);
    LM_KG_NEED_SECRET(ctx, s, "lumen_keygen_ringswitch");
    LM_CHECK(ctx, log_n_small < ctx->logN, "lumen_keygen_ringswitch: target ring degree 2^%u is not below 2^%u", log_n_small,
             ctx->logN);
    const bool hybrid = ctx->K >= 2;
    LM_CHECK(ctx, hybrid || (base_two_w >= 1 && base_two_w <= 32), "lumen_keygen_ringswitch: BaseTwoDecomposition %u out of range",
             base_two_w);
    const uint32_t N = ctx->N, LK = ctx->L + ctx->K;
    const uint32_t rns = lumen_ringswitch_rns_digits(ctx), pw2 = lumen_ringswitch_digits(ctx, base_two_w);
    const size_t whole = (size_t)rns * pw2 * 2 * LK * N;
    LM_CHECK(ctx, key_words == whole, "lumen_keygen_ringswitch: key of %zu words: expected %zu ([rns = %u][pw2 = %u][2][L+K = %u][N = %u])",
             key_words, whole, rns, pw2, LK, N);
    const size_t n = (size_t)1 << log_n_small, words = (size_t)LK * N;
    lm_dev<u64> d_sout;
    lm_dev<int8_t> d_small;
    if (kg_alloc(ctx, d_small, N, true) || kg_alloc(ctx, d_sout, words, true)) return 1;
    if (int rc = lm_sample_small(ctx, d_small.get(), nullptr, LM_KG_ID_RINGSWITCH * LM_KG_INDEX_STRIDE, 1, 0, 1, seed)) return rc;
    // skNew(X^(N/n)) over QP
    if (int rc = lm_for_logn(ctx, ctx->logN, [&](auto k) {
            return kg_secret_ntt_t<k>(ctx, d_small.get(), d_sout.get(), nullptr, 1, ctx->logN - log_n_small);
        }))
        return rc;
    LM_HIP(ctx, hipMemcpyAsync(sk_small, d_small.get(), n, hipMemcpyDeviceToHost, ctx->stream));
    LM_HIP(ctx, hipStreamSynchronize(ctx->stream)); // caller memory
    const std::vector<u64> fac = kg_gadget(ctx, rns, pw2, hybrid ? 0 : base_two_w);
    return kg_run(ctx, seed, {LM_KG_ID_RINGSWITCH}, rns * pw2, d_sout.get(), 0, s->d_mont.get(), &fac, 0, key);
}
