// Client-side decryption of level-<=1 ciphertexts: EncryptedProof.Decrypt /
// decryptBatchedParallel (fhe/ligero.go:381-502, 577-636) = Decryptor.DecryptNew + Encoder.Decode
// [LATTIGO-RECALL]: phase = c0 + c1*s, to the coefficient domain, times T; CRT over the (<= 2) limbs,
// centred, reduced modulo T; NTT over Z_T; slot i read at the encoder's index; divided by the scale
// the rescales left behind.  The secret key lives with the client: this entry point is for a client
// that owns a GPU and for end-to-end tests, not for the proving server.
#include <cstring>

#include "lm_enc_host.h"

void lm_install_secret_key_dev(lumen_ctx *ctx, lm_dev<tw_t> &&d_sk) {
    auto sp = std::make_shared<SkTable>();
    sp->d_sk = std::move(d_sk);
    lm_ext_put(ctx, "secret_key", sp);
}

extern "C" int lumen_load_secret_key(lumen_ctx *ctx, const uint64_t *sk) {
    LM_CHECK(nullptr, ctx && sk, "lumen_load_secret_key: NULL argument");
    LM_ENTER(ctx);
    const uint32_t N = ctx->N, L = ctx->L;
    std::vector<tw_t> tab((size_t)L * N);
    for (uint32_t l = 0; l < L; l++) {
        const uint64_t q = ctx->mod[l];
        for (uint32_t k = 0; k < N; k++) {
            const uint64_t x = sk[(size_t)l * N + k];
            if (x >= q) return lm_fail(ctx, "secret key residue out of range (limb %u)", l);
            tab[(size_t)l * N + k] = h_tw(x, q);
        }
    }
    lm_dev<tw_t> d_sk;
    if (int rc = d_sk.upload(ctx, tab, "the secret key")) return rc;
    lm_install_secret_key_dev(ctx, std::move(d_sk));
    return 0;
}

// phase[c][l] = INTT(c0 + c1 * s) * T   (one workgroup per (ciphertext, limb); T * N^-1 folded)
struct dec_scale_t {
    tw_t t[LM_MAX_LIMBS];
};
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_lds(LOGN)) void k_decrypt_phase(const u64 *__restrict__ ct, const tw_t *__restrict__ sk,
                                                                       u64 *__restrict__ phase, uint32_t count, uint32_t nl,
                                                                       dec_scale_t scale, lm_mods mods,
                                                                       const tw_t *__restrict__ tw_all) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x;
    const uint32_t l = blockIdx.x / count, c = blockIdx.x % count;
    const lm_qc qc = lm_make_qc(mods.m[l]);
    const u64 *c0 = ct + ((size_t)c * 2 * nl + l) * N, *c1 = c0 + (size_t)nl * N;
    const tw_t *s = sk + (size_t)l * N;
    u64 *o = phase + ((size_t)c * nl + l) * N;
    const tw_t sc = scale.t[l];
    auto ld = [&](uint32_t i0, u64 *v, int n) {
        u64 a[8], b[8];
        lm_load_run(c0, i0, a, n);
        lm_load_run(c1, i0, b, n);
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < n) {
                const tw_t sv = s[i0 + k];
                const u64 x = lm_shoup3<false>(b[k], sv.w, sv.wp, qc.nq, a[k]); // c0 + c1*s, lazily: < 4q
                v[k] = lm_csub(lm_csub(x, 2 * qc.q), qc.q);
            }
    };
    auto st = [&](uint32_t i, u64 v) { o[i] = lm_shoup_cs(v, sc, qc.q, qc.nq); };
    lm_ntt_inverse<LOGN>(sm, tw_all + (size_t)l * N, qc, tid, ld, st);
}

// m[c][k] = centre_Q(CRT(phase limbs)) mod T
__global__ void k_decrypt_crt(const u64 *__restrict__ phase, u64 *__restrict__ m, uint32_t nl, uint32_t logN, size_t total,
                              mod_t m0, mod_t m1, tw_t q0inv_mod_q1, mod_t modT) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const size_t c = g >> logN, k = g & (((size_t)1 << logN) - 1);
    const u64 *p = phase + ((c * nl) << logN) + k;
    const u64 T = modT.q, y0 = p[0];
    if (nl == 1) {
        const u64 q0 = m0.q;
        m[g] = y0 > (q0 >> 1) ? (T - lm_reduce(q0 - y0, T, modT.qinv64)) % T : lm_reduce(y0, T, modT.qinv64);
        return;
    }
    const u64 q0 = m0.q, q1 = m1.q, y1 = p[(size_t)1 << logN];
    // Garner: y = y0 + q0 * ((y1 - y0) * q0^-1 mod q1)
    const u64 h = lm_shoup(lm_submod(y1, lm_reduce(y0, q1, m1.qinv64), q1), q0inv_mod_q1, q1);
    const u128 Q = (u128)q0 * q1, y = (u128)y0 + (u128)q0 * h;
    m[g] = y > (Q >> 1) ? (T - (u64)((Q - y) % T)) % T : (u64)(y % T);
}

// The same at any depth (Decryptor.DecryptNew of a ciphertext that was never rescaled: TestEncode,
// fhe/code_test.go:87-96), exact in word arithmetic: Garner's mixed-radix digits
//     x = d_0 + d_1 q_0 + d_2 q_0 q_1 + ...,   d_i = (y_i - d_0 - d_1 q_0 - ...) / (q_0 ... q_{i-1}) mod q_i
// x > Q/2 decided digit by digit against the digits of floor(Q/2), x mod T = sum d_i (q_0..q_{i-1} mod T).
struct garner_t {
    tw_t inv[LM_MAX_LIMBS][LM_MAX_LIMBS]; // inv[i][j] = q_j^-1 mod q_i (j < i), Shoup form
    tw_t radix_T[LM_MAX_LIMBS];          // q_0 ... q_{i-1} mod T
    u64 half[LM_MAX_LIMBS];              // mixed-radix digits of floor(Q / 2)
    u64 q_mod_T;
};
__global__ __launch_bounds__(256) void k_decrypt_garner(const u64 *__restrict__ phase, u64 *__restrict__ m, uint32_t nl,
                                                        uint32_t logN, size_t total, lm_mods mods,
                                                        const garner_t *__restrict__ G, mod_t modT) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const size_t c = g >> logN, k = g & (((size_t)1 << logN) - 1);
    const u64 *p = phase + ((c * nl) << logN) + k;
    const u64 T = modT.q;
    // every loop is unrolled over LM_MAX_LIMBS with wave-uniform guards: the digits stay in registers
    // (a dynamically indexed d[] would live in scratch memory, which the build refuses)
    u64 d[LM_MAX_LIMBS];
#pragma unroll
    for (int i = 0; i < LM_MAX_LIMBS; i++) {
        d[i] = 0;
        if ((uint32_t)i < nl) {
            const mod_t mi = mods.m[i];
            u64 v = p[(size_t)i << logN];
#pragma unroll
            for (int j = 0; j < i; j++)
                v = lm_shoup(lm_submod(v, lm_reduce(d[j], mi.q, mi.qinv64), mi.q), G->inv[i][j], mi.q);
            d[i] = v;
        }
    }
    bool above = false, decided = false; // x > floor(Q/2)?  the first differing digit from the top decides
#pragma unroll
    for (int i = LM_MAX_LIMBS - 1; i >= 0; i--)
        if ((uint32_t)i < nl && !decided && d[i] != G->half[i]) above = d[i] > G->half[i], decided = true;
    u64 acc = 0;
#pragma unroll
    for (int i = 0; i < LM_MAX_LIMBS; i++)
        if ((uint32_t)i < nl) acc = lm_addmod(acc, lm_shoup(lm_reduce(d[i], T, modT.qinv64), G->radix_T[i], T), T);
    m[g] = above ? lm_submod(acc, G->q_mod_T, T) : acc;
}

// values[c][i] = t[c][slot[i]] * scale^-1 mod T
__global__ void k_decrypt_slots(const u64 *__restrict__ t, const uint32_t *__restrict__ slot, u64 *__restrict__ values,
                                uint32_t nvalues, uint32_t logN, size_t total, tw_t sinv, u64 T) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const size_t c = g / nvalues;
    const uint32_t i = (uint32_t)(g % nvalues);
    values[g] = lm_shoup(t[(c << logN) + slot[i]], sinv, T);
}

template <int LOGN>
static int decrypt_phase_t(lumen_ctx *ctx, const u64 *ct, const tw_t *sk, u64 *phase, uint32_t count, uint32_t nl,
                           const dec_scale_t &sc) {
    lm_prof_scope ps(ctx, "decrypt_phase_intt", (uint64_t)count * nl);
    return lm_launch(ctx, k_decrypt_phase<LOGN>, lm_geom_lds(LOGN), count * nl, ct, sk, phase, count, nl, sc, ctx->mods,
                     ctx->sh->tw_inv.get());
}

int lm_decrypt_phase(lumen_ctx *ctx, const u64 *ct, uint32_t count, uint32_t nl, const SkTable *sk, u64 *phase, bool times_T) {
    dec_scale_t sc;
    for (uint32_t l = 0; l < LM_MAX_LIMBS; l++) {
        const uint64_t q = ctx->mod[l < nl ? l : 0];
        sc.t[l] = h_tw(h_mulmod(ctx->ninv[l < nl ? l : 0].w, times_T ? ctx->T % q : 1, q), q);
    }
    return lm_for_logn(ctx, ctx->logN, [&](auto k) { return decrypt_phase_t<k>(ctx, ct, sk->d_sk.get(), phase, count, nl, sc); });
}

int lm_decrypt_check(lumen_ctx *ctx, const lumen_set *set, uint64_t scale, const char *what) {
    LM_FULL_WIDTH(ctx, set, what);
    LM_CHECK(ctx, set->nl >= 1 && set->nl <= ctx->L, "%s: %u limbs out of range [1, %u]", what, set->nl, ctx->L);
    LM_CHECK(ctx, lm_ext_get<SkTable>(ctx, "secret_key"), "no secret key loaded (lumen_load_secret_key)");
    LM_CHECK(ctx, lm_ext_get<EncoderTables>(ctx, "encoder"), "no encoder tables (lumen_encoder_set)");
    LM_CHECK(ctx, scale % ctx->T != 0, "scale is 0 modulo T");
    return 0;
}

int lm_decrypt_decode(lumen_ctx *ctx, const lumen_set *set, lm_decoded *out) {
    const std::shared_ptr<SkTable> sk_hold = lm_ext_get<SkTable>(ctx, "secret_key");
    const std::shared_ptr<EncoderTables> enc_hold = lm_ext_get<EncoderTables>(ctx, "encoder");
    LM_CHECK(ctx, sk_hold && enc_hold, "lm_decrypt_decode without a secret key and encoder tables");
    const SkTable *sk = sk_hold.get();
    const EncoderTables *enc = enc_hold.get();
    const uint32_t N = ctx->N, nl = set->nl, count = set->count;
    const uint64_t T = ctx->T;
    u64 *phase = (u64 *)lm_scratch(ctx, "dec_phase", (size_t)count * nl * N * sizeof(u64));
    u64 *m = (u64 *)lm_scratch(ctx, "dec_m", (size_t)count * N * sizeof(u64));
    if (!phase || !m) return 1;
    if (int rc = lm_decrypt_phase(ctx, set->d, count, nl, sk, phase, true)) return rc;
    if (nl > 2) { // deeper than what Prove returns: exact CRT by mixed radix
        std::vector<garner_t> hg(1);
        garner_t &G = hg[0];
        memset(&G, 0, sizeof(G));
        uint64_t r = 1 % T;
        for (uint32_t i = 0; i < nl; i++) {
            G.radix_T[i] = h_tw(r, T);
            r = h_mulmod(r, ctx->mod[i] % T, T);
            for (uint32_t j = 0; j < i; j++) G.inv[i][j] = h_tw(h_invmod(ctx->mod[j] % ctx->mod[i], ctx->mod[i]), ctx->mod[i]);
        }
        G.q_mod_T = r;
        uint64_t carry = 0; // floor(Q/2) = (Q-1)/2: Q-1 has digit q_i - 1 everywhere; halve from the top
        for (int i = (int)nl - 1; i >= 0; i--) {
            const u128 v = (u128)carry * ctx->mod[i] + (ctx->mod[i] - 1);
            G.half[i] = (uint64_t)(v >> 1);
            carry = (uint64_t)(v & 1);
        }
        garner_t *dG = (garner_t *)lm_scratch(ctx, "dec_garner", sizeof(garner_t));
        if (!dG) return 1;
        if (int rc = lm_h2d_staged(ctx, dG, &G, sizeof(G))) return rc;
        lm_prof_scope ps(ctx, "decrypt_crt", count);
        const size_t total = (size_t)count * N;
        if (int rc = lm_launch_flat(ctx, k_decrypt_garner, total, phase, m, nl, ctx->logN, total, ctx->mods, dG, enc->modT)) return rc;
    } else {
        lm_prof_scope ps(ctx, "decrypt_crt", count);
        const size_t total = (size_t)count * N;
        const uint64_t q0 = ctx->mod[0], q1 = ctx->mod[nl > 1 ? 1 : 0];
        const tw_t q0inv = nl > 1 ? h_tw(h_invmod(q0 % q1, q1), q1) : h_tw(1, q1);
        if (int rc = lm_launch_flat(ctx, k_decrypt_crt, total, phase, m, nl, ctx->logN, total, ctx->mods.m[0],
                                    ctx->mods.m[nl > 1 ? 1 : 0], q0inv, enc->modT))
            return rc;
    }
    {
        lm_prof_scope ps(ctx, "decode_ntt_T", count);
        if (int r2 = lm_launch_ntt_subring(ctx, ctx->logN, enc->d_tw_fwd.get(), enc->ninvT, m, N, m, N, count, 0, false, &enc->modT))
            return r2;
    }
    out->t = m, out->slot = enc->d_slot.get();
    out->keep[0] = sk_hold, out->keep[1] = enc_hold;
    return 0;
}

int lm_decrypt_slots(lumen_ctx *ctx, const lm_decoded &dec, uint32_t count, uint64_t scale, uint32_t nvalues,
                     uint64_t *values) {
    const uint64_t T = ctx->T;
    u64 *dv = (u64 *)lm_scratch(ctx, "dec_values", (size_t)count * nvalues * sizeof(u64));
    if (!dv) return 1;
    const size_t total = (size_t)count * nvalues;
    const tw_t sinv = h_tw(h_invmod(scale % T, T), T);
    if (int rc = lm_launch_flat(ctx, k_decrypt_slots, total, dec.t, dec.slot, dv, nvalues, ctx->logN, total, sinv, T)) return rc;
    LM_HIP(ctx, hipMemcpyAsync(values, dv, total * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

extern "C" int lumen_decrypt(lumen_ctx *ctx, const lumen_set *set, uint64_t scale, uint32_t nvalues, uint64_t *values) {
    LM_CHECK(nullptr, ctx && set && values, "lumen_decrypt: NULL argument");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_decrypt");
    if (int rc = lm_decrypt_check(ctx, set, scale, "lumen_decrypt")) return rc;
    LM_CHECK(ctx, nvalues >= 1 && nvalues <= ctx->N, "nvalues=%u out of range [1, N]", nvalues);
    if (!set->count) return 0;
    lm_decoded dec;
    if (int rc = lm_decrypt_decode(ctx, set, &dec)) return rc;
    if (int rc = lm_decrypt_slots(ctx, dec, set->count, scale, nvalues, values)) return rc;
    LM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
