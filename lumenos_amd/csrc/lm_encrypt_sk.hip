// Client-side witness encryption under the secret key (fhe/bfv.go:77: the rlwe.NewEncryptor(paramsFHE, sk) ClientBFV
// embeds; client.EncryptNew, vdec/batching_test.go:56), rlwe.Encryptor.encryptZeroSk [LATTIGO-RECALL] at the top level:
//     c1 = a,   c0 = NTT(e) + pt - a * s          a uniform mod q_l in the NTT domain, e Gaussian (sigma 3.2, |e| <= 19)
// c1 is pure randomness: it is regenerated from a PUBLIC 32-byte seed, so a ciphertext travels as c0 and the seed
// ("seeded" form) and the server expands it with no key of any kind.  L limb transforms per ciphertext against the
// (L+K) + 2K + 2L of the public-key path (lm_encrypt.hip), and the fresh noise is e itself.
//
// THE SAMPLING CONTRACT (include/lumenos_hip.h).  Deterministic in (seeds, I = first_index + i, limb, coefficient):
//     keystream(I, s) = ChaCha20(key, nonce = LE64(I) || LE32(s), counter = 0, 1, ...)           (lm_sample_dev.h)
//     e   stream 3 of keystream(I, .) under secret_seed, the encryptor's CDT rule; one N-coefficient sample per
//         ciphertext, extended to every limb (the public-key encryptor draws streams 0-2, key generation 16 + m)
//     a_l stream 16 + l of keystream(I, .) under a_seed, key generation's rejection rule (k_sample_uniform), Q limbs
//     pt  the plaintext bits of lumen_encrypt_values: slot scatter, INTT over Z_T, m * T^-1 mod q_l
//
// One kernel of its own, k_enc_sk (one workgroup per (ciphertext, Q limb): lift of e plus the scaled message in the
// load, the limb transform, - a * s in the store); e and a come from the shared sampler (lm_sample.hip), the message
// from lm_encode_coeffs (lm_encoder.hip), the key table from lm_decrypt.hip.
#include <cstring>

#include "lm_enc_host.h"

#define LM_ENCSK_ERR_STREAM 3u

// small [count][N] int8 errors; mcoef [count][N] plaintext coefficients modulo T (tinv: T^-1 mod q_l); sk [L][N] Shoup
// form; a + c * a_stride and c0 + c * c0_stride: [L][N], the `a` halves filled by k_sample_uniform.
//     c0 = NTT(e + m * T^-1) - a * s, canonical.
// Dealt limb-major like k_enc_u: one twiddle table and one limb of s stay hot per XCD.
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_lds(LOGN)) void k_enc_sk(const int8_t *__restrict__ small, const u64 *__restrict__ mcoef,
                                                            enc_tinv_t tinv, const tw_t *__restrict__ sk,
                                                            const u64 *__restrict__ a, size_t a_stride, u64 *__restrict__ c0,
                                                            size_t c0_stride, uint32_t count, lm_mods mods,
                                                            const tw_t *__restrict__ tw_all) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x;
    const uint32_t l = blockIdx.x / count, c = blockIdx.x % count;
    const lm_qc qc = lm_make_qc(mods.m[l]);
    const int8_t *se = small + (size_t)c * N;
    const u64 *mc = mcoef + (size_t)c * N;
    const u64 *al = a + (size_t)c * a_stride + (size_t)l * N;
    const tw_t *s = sk + (size_t)l * N;
    u64 *o = c0 + (size_t)c * c0_stride + (size_t)l * N;
    const tw_t ti = tinv.t[l];
    auto ld = [&](uint32_t i) {
        u64 r = lm_lift_small(se[i], &qc.q);
        lm_add_scaled_msg(r, mc[i], ti, qc); // e + m * T^-1
        return r;
    };
    auto st = [&](uint32_t i0, const u64 *v, int n) {
        u64 av[8], b[8];
        lm_load_run(al, i0, av, n);
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < n) {
                const tw_t sv = s[i0 + k];
                const u64 as = lm_shoup3<false>(av[k], sv.w, sv.wp, qc.nq); // a * s, in [0, 3q)
                const u64 x = lm_reduce_s(v[k], qc.q, qc.nq, qc.qinv64) + qc.q3 - as; // in (0, 4q)
                b[k] = lm_csub(lm_csub(x, 2 * qc.q), qc.q);
            }
        lm_store_run(o, i0, b, n);
    };
    // the generic passes also at N = 2^14: the storer's run of a and of Shoup pairs of s needs the registers the
    // second twiddle set would take (scratch otherwise, which the build refuses)
    lm_ntt_forward<LOGN, false>(sm, tw_all + (size_t)l * N, qc, tid, ld, st);
}

template <int LOGN>
static int enc_sk_t(lumen_ctx *ctx, const int8_t *small, const u64 *mcoef, const enc_tinv_t &tinv, const tw_t *sk, const u64 *a,
                    size_t a_stride, u64 *c0, size_t c0_stride, uint32_t count) {
    lm_prof_scope ps(ctx, "encrypt_sk_ntt", (uint64_t)count * ctx->L);
    return lm_launch(ctx, k_enc_sk<LOGN>, lm_geom_lds(LOGN), count * ctx->L, small, mcoef, tinv, sk, a, a_stride, c0, c0_stride,
                     count, ctx->mods, ctx->sh->tw_fwd.get());
}

// chunks bound the temporaries, as in the public-key encryptor
#define LM_ENCSK_CHUNK 256u

// what the two encrypting entry points refuse, before any device work
static int enc_sk_check(lumen_ctx *ctx, const char *what, uint32_t rows, const uint8_t secret_seed[32], const uint8_t a_seed[32]) {
    LM_CHECK(ctx, lm_ext_get<SkTable>(ctx, "secret_key"), "%s: no secret key on the context (lumen_load_secret_key, lumen_keygen_secret)",
             what);
    LM_CHECK(ctx, lm_ext_get<EncoderTables>(ctx, "encoder"), "%s: no encoder tables (lumen_encoder_set)", what);
    LM_CHECK(ctx, rows >= 1 && rows <= ctx->N, "%s: rows=%u out of range [1, N]", what, rows);
    LM_CHECK(ctx, memcmp(secret_seed, a_seed, 32) != 0, "%s: the two seeds are equal (a_seed is public: the server could regenerate e)",
             what);
    return 0;
}

// full: ciphertexts into set storage dst ([count][2][L][N]); otherwise only the c0 halves, to the host ([count][L][N])
static int enc_sk_impl(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count, const uint8_t secret_seed[32],
                       const uint8_t a_seed[32], uint64_t first_index, u64 *dst, uint64_t *c0_host) {
    const std::shared_ptr<SkTable> sk_hold = lm_ext_get<SkTable>(ctx, "secret_key");
    const std::shared_ptr<EncoderTables> enc_hold = lm_ext_get<EncoderTables>(ctx, "encoder");
    LM_CHECK(ctx, sk_hold && enc_hold, "secret-key encryption without a secret key and encoder tables");
    const uint32_t N = ctx->N, L = ctx->L;
    const size_t limbs = (size_t)L * N;
    const uint32_t chunk = std::min<uint32_t>(count, LM_ENCSK_CHUNK);
    lm_dev<int8_t> d_e; // the errors: zeroed on the stream before the block is given back
    if (d_e.release_on(ctx->stream, true).alloc(ctx, (size_t)chunk * N, "secret-key encryption")) return 1;
    u64 *dval = (u64 *)lm_scratch(ctx, "enc_val", (size_t)chunk * rows * sizeof(u64));
    u64 *dm = (u64 *)lm_scratch(ctx, "enc_m", (size_t)chunk * N * sizeof(u64));
    u64 *da = dst ? nullptr : (u64 *)lm_scratch(ctx, "encsk_a", (size_t)chunk * limbs * sizeof(u64));
    u64 *dc0 = dst ? nullptr : (u64 *)lm_scratch(ctx, "encsk_c0", (size_t)chunk * limbs * sizeof(u64));
    if (!dval || !dm || (!dst && (!da || !dc0))) return 1;
    for (uint32_t first = 0; first < count; first += chunk) {
        const uint32_t n = std::min(chunk, count - first);
        // the temporaries are reused: stream order puts these copies behind the previous chunk's kernels
        if (int rc = lm_encode_coeffs(ctx, enc_hold.get(), values + (size_t)first * rows, rows, n, dval, dm)) return rc;
        {
            lm_prof_scope ps(ctx, "encrypt_sk_sample", n);
            if (int rc = lm_sample_small(ctx, d_e.get(), nullptr, first_index + first, n, LM_ENCSK_ERR_STREAM, 1, secret_seed)) return rc;
        }
        // full form: a is the c1 half of [ct][2][L][N]; seeded form: a scratch block, and only c0 is kept
        u64 *c0 = dst ? dst + (size_t)first * 2 * limbs : dc0, *a = dst ? c0 + limbs : da;
        const size_t stride = dst ? 2 * limbs : limbs;
        {
            lm_prof_scope ps(ctx, "encrypt_sk_uniform", (uint64_t)n * L);
            if (int rc = lm_sample_uniform(ctx, a, stride, nullptr, first_index + first, n, L, a_seed)) return rc;
        }
        if (int rc = lm_for_logn(ctx, ctx->logN, [&](auto k) {
                return enc_sk_t<k>(ctx, d_e.get(), dm, enc_hold->tinv, sk_hold->d_sk.get(), a, stride, c0, stride, n);
            }))
            return rc;
        if (!dst) {
            lm_prof_scope ps(ctx, "encrypt_sk_download", n);
            if (int rc = lm_d2h(ctx, c0_host + (size_t)first * limbs, dc0, (size_t)n * limbs * sizeof(u64), true)) return rc;
        }
    }
    LM_HIP(ctx, hipStreamSynchronize(ctx->stream)); // caller memory (`values`)
    return 0;
}

extern "C" int lumen_encrypt_sk_values(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count,
                                       const uint8_t secret_seed[32], const uint8_t a_seed[32], uint64_t first_index,
                                       lumen_set **out) {
    LM_CHECK(nullptr, ctx, "lumen_encrypt_sk_values: NULL ctx");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_encrypt_sk_values");
    LM_CHECK(ctx, secret_seed && a_seed && out && (values || !count), "lumen_encrypt_sk_values: NULL argument");
    if (int rc = enc_sk_check(ctx, "lumen_encrypt_sk_values", rows, secret_seed, a_seed)) return rc;
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, count, ctx->L, &o)) return rc;
    lm_set_guard og(ctx, o); // given back on every early return below
    if (count)
        if (int rc = enc_sk_impl(ctx, values, rows, count, secret_seed, a_seed, first_index, o->d, nullptr)) return rc;
    *out = og.release();
    return 0;
}

extern "C" int lumen_encrypt_sk_seeded(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count,
                                       const uint8_t secret_seed[32], const uint8_t a_seed[32], uint64_t first_index,
                                       uint64_t *c0) {
    LM_CHECK(nullptr, ctx, "lumen_encrypt_sk_seeded: NULL ctx");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_encrypt_sk_seeded");
    LM_CHECK(ctx, secret_seed && a_seed && ((values && c0) || !count), "lumen_encrypt_sk_seeded: NULL argument");
    if (int rc = enc_sk_check(ctx, "lumen_encrypt_sk_seeded", rows, secret_seed, a_seed)) return rc;
    if (!count) return 0;
    return enc_sk_impl(ctx, values, rows, count, secret_seed, a_seed, first_index, nullptr, c0);
}

extern "C" int lumen_ct_expand_seeded(lumen_ctx *ctx, const uint64_t *c0, uint32_t count, const uint8_t a_seed[32],
                                      uint64_t first_index, lumen_set **out) {
    LM_CHECK(nullptr, ctx, "lumen_ct_expand_seeded: NULL ctx");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_ct_expand_seeded");
    LM_CHECK(ctx, a_seed && out && (c0 || !count), "lumen_ct_expand_seeded: NULL argument");
    const uint32_t N = ctx->N, L = ctx->L;
    const size_t limbs = (size_t)L * N;
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, count, L, &o)) return rc;
    lm_set_guard og(ctx, o);
    if (count) {
        const uint32_t chunk = std::min<uint32_t>(count, LM_ENCSK_CHUNK);
        for (uint32_t first = 0; first < count; first += chunk) {
            const uint32_t n = std::min(chunk, count - first);
            lm_prof_scope ps(ctx, "encrypt_sk_uniform", (uint64_t)n * L);
            if (int rc = lm_sample_uniform(ctx, o->d + (size_t)first * 2 * limbs + limbs, 2 * limbs, nullptr, first_index + first, n, L, a_seed))
                return rc;
        }
        lm_prof_scope ps(ctx, "expand_seeded_upload", count);
        if (int rc = lm_h2d_rows(ctx, o->d, 2 * limbs * sizeof(u64), c0, limbs * sizeof(u64), limbs * sizeof(u64), count)) return rc;
    }
    *out = og.release();
    return 0;
}
