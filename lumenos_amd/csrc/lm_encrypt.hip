// Server-side witness encryption: server.EncryptNew per column
// (cmd/server/main.go:199-208), i.e. rlwe.Encryptor under a public key at the top level
// [LATTIGO-RECALL: encryptZero with pk, no P-extension]:
//     c0 = u*pk0 + e0 + pt,   c1 = u*pk1 + e1
// u ternary (P(-1) = P(1) = 1/3), e0/e1 discrete Gaussians of sigma 3.2 truncated at |e| <= 19.
// The reference's encryption is RANDOMISED (PRNG keyed from crypto/rand): there are no reference
// ciphertext bits to match; the contract is decryption and the error distribution.  The sampler here
// is deterministic in (seed, ciphertext index) -- see oracle/lo_encdet.c for its definition, shared
// bit for bit with the CPU checker -- so that any sharding of the columns over GPUs yields the same
// ciphertexts:
//     keystream(c, s) = ChaCha20(key = seed, nonce = LE64(c) || LE32(s), counter = block)
//     u  coefficient k  <- word k of stream 0:  ((w * 3) >> 32) - 1
//     e0/e1 coefficient k <- words 2k, 2k+1 of stream 1/2: r = w0 | w1 << 32, m = r >> 1,
//         |e| = #{ i < 19 : m >= CDT[i] },  sign = r & 1.
//
// The small polynomials come from the shared sampler (lm_sample.hip: streams 0-2 of every ciphertext in one launch,
// 3N bytes per ciphertext), the message from the encoder (lm_encoder.hip); the kernels here lift and transform
// them through the LDS-resident limb transform, the pk products and the sums fused into the stores.
#include <cstring>

#include "lm_enc_host.h"

// rlwe.Encryptor.encryptZeroPk [LATTIGO-RECALL], for ciphertext c and polynomial w in {0, 1}:
//     t_w   = u * pk_w + e_w                      over the whole basis QP (pk lives there)
//     c_w   = ModDownQPtoQ(t_w) = (t_w,Q - [t_w]_P) * P^-1   (then + pt on c_0)
// The division by P is what keeps fresh noise at a few units (delta_0 + delta_1 * s, delta in [0,1))
// instead of |u*e_pk + e_0 + e_1*s| ~ 2^8; fhe.Encode multiplies noise by up to T/2 ten times without
// a rescale, and the reference's 2048x1024 shape only fits its own LogQ heuristic with the small
// noise (tools/noise_budget.py).
// NTT is linear, so with U = NTT(u) the Q limbs never leave the NTT domain:
//     c_w[l] = U*pk_w[l]*P^-1  -  NTT( lift_{P->q_l}([t_w]_P) - e_w ) * P^-1
// Three kernels (per ciphertext (L+K) + 2K + 2L limb transforms instead of Lattigo's 3(L+K) + 2L):
//   k_enc_u      one workgroup per (ciphertext, limb of QP): U = NTT(u); Q limbs store U*pk_w*P^-1
//                into the output (P^-1 is folded into the key table), P limbs store U*pk_w into scratch
//   (limb INTT with the y-scaling of the basis extension on the 2K scratch limbs, k_enc_add_e: + e_w,
//    k_pack_v: the exact integer reconstruction, as in the key switch)
//   k_enc_down   one workgroup per (ciphertext, w, Q limb): the lift fused into the load together with
//                -e_w and, for w = 0, the message; NTT; combine with the product of k_enc_u in the store.
// Without special primes (K = 0) there is nothing to divide by: c_w = U*pk_w + NTT(e_w).
// pk: [2][LK][N] Shoup form (Q limbs times P^-1); out: [count][2][L][N]; upk: [count][2][K][N]
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_lds(LOGN)) void k_enc_u(const int8_t *__restrict__ small,
                                                               const tw_t *__restrict__ pk, u64 *__restrict__ out,
                                                               u64 *__restrict__ upk, uint32_t count, uint32_t L,
                                                               uint32_t K, lm_mods mods,
                                                               const tw_t *__restrict__ tw_all) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x, LK = L + K;
    const uint32_t t = blockIdx.x / count, c = blockIdx.x % count; // limb-major: one twiddle table hot per XCD
    const lm_qc qc = lm_make_qc(mods.m[t]);
    const int8_t *su = small + (size_t)c * 3 * N;
    const tw_t *pk0 = pk + (size_t)t * N, *pk1 = pk + (size_t)(LK + t) * N;
    u64 *o0, *o1;
    if (t < L)
        o0 = out + ((size_t)c * 2 * L + t) * N, o1 = o0 + (size_t)L * N;
    else
        o0 = upk + ((size_t)c * 2 * K + (t - L)) * N, o1 = o0 + (size_t)K * N;
    auto ld = [&](uint32_t i) { return lm_lift_small(su[i], &qc.q); };
    auto st = [&](uint32_t i0, const u64 *v, int n) {
        u64 a[8], b[8];
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < n) {
                const tw_t k0 = pk0[i0 + k], k1 = pk1[i0 + k];
                const u64 x = lm_shoup3<false>(v[k], k0.w, k0.wp, qc.nq); // any v < 2^64 -> [0, 3q)
                const u64 y = lm_shoup3<false>(v[k], k1.w, k1.wp, qc.nq);
                a[k] = lm_csub(lm_csub(x, 2 * qc.q), qc.q);
                b[k] = lm_csub(lm_csub(y, 2 * qc.q), qc.q);
            }
        lm_store_run(o0, i0, a, n);
        lm_store_run(o1, i0, b, n);
    };
    lm_ntt_forward<LOGN>(sm, tw_all + (size_t)t * N, qc, tid, ld, st);
}

// y[c][w][j][i] += e_w[c][i] * hat_j mod p_j  (the INTT before it scaled the products by hat_j =
// (P/p_j)^-1 mod p_j, the source-side factor of the basis extension: the error has to follow)
struct enc_hat_t {
    tw_t t[4];
};
__global__ __launch_bounds__(256) void k_enc_add_e(u64 *__restrict__ upk, const int8_t *__restrict__ small,
                                                   uint32_t count, uint32_t K, uint32_t L, uint32_t logN,
                                                   lm_mods mods, enc_hat_t hat) {
    const size_t total = ((size_t)count * 2 * K) << logN, N = (size_t)1 << logN;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const size_t i = g & (N - 1), limb = g >> logN;
        const uint32_t j = (uint32_t)(limb % K), w = (uint32_t)((limb / K) & 1);
        const size_t c = limb / (2 * K);
        const u64 p = mods.m[L + j].q;
        const u64 el = lm_lift_small(small[(c * 3 + 1 + w) * N + i], &p);
        upk[g] = lm_addmod(upk[g], lm_shoup(el, hat.t[j], p), p);
    }
}

// One workgroup per (ciphertext c, polynomial w, Q limb l).  HASP: the lift of the P limbs (packed by
// k_pack_v) rides in the load with -e_w; otherwise the load is e_w itself.  mcoef: the plaintexts as
// coefficient vectors modulo T ([count][N], the encoder's INTT output): NTT is linear, so the scaled
// message rides in the load of the w = 0 transform and costs no transform of its own.  pt: the
// plaintexts in the NTT domain ([count][L][N]), added in the store.  out holds U*pk_w(*P^-1) on entry.
template <int LOGN, bool HASP>
__global__ LM_GEOM_BOUNDS(lm_geom_lds(LOGN)) void k_enc_down(const int8_t *__restrict__ small,
                                                                  const u64 *__restrict__ upk,
                                                                  const bx_t *__restrict__ bxp,
                                                                  const tw_t *__restrict__ pinv,
                                                                  const u64 *__restrict__ pt,
                                                                  const u64 *__restrict__ mcoef, enc_tinv_t tinv,
                                                                  u64 *__restrict__ out, uint32_t count, uint32_t L,
                                                                  uint32_t K, lm_mods mods,
                                                                  const tw_t *__restrict__ tw_all) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x;
    const uint32_t l = blockIdx.x / (2 * count), cw = blockIdx.x % (2 * count), c = cw >> 1, w = cw & 1;
    const lm_qc qc = lm_make_qc(mods.m[l]);
    const int8_t *se = small + ((size_t)c * 3 + 1 + w) * N;
    u64 *o = out + (((size_t)c * 2 + w) * L + l) * N;
    const u64 *p = (pt && w == 0) ? pt + ((size_t)c * L + l) * N : nullptr;
    const u64 *mc = (mcoef && w == 0) ? mcoef + (size_t)c * N : nullptr;
    const tw_t ti = tinv.t[l];
    bx_t bc;
    const u64 *up0 = nullptr, *up1 = nullptr;
    tw_t pi = ti;
    if (HASP) {
        bc = bxp[l];
        up0 = upk + ((size_t)c * 2 + w) * K * N;
        up1 = bc.ns == 2 ? up0 + N : up0;
        pi = pinv[l];
    }
    auto ld = [&](uint32_t i) {
        const int8_t e = se[i];
        // HASP: -e - P*m*T^-1 (the store multiplies by -P^-1); else +e + m*T^-1.  Canonical: the lift
        // below is already < 6q and the transform takes inputs below 7q.
        // (the lift of -e stays written out: through lm_lift_small the kernel's machine code changes)
        u64 r = HASP ? (e > 0 ? qc.q - (u64)e : (u64)(-(int)e)) : lm_lift_small(e, &qc.q);
        if (mc) lm_add_scaled_msg(r, mc[i], ti, qc);
        return HASP ? bx_apply(bc, up0[i], up1[i], qc) + r : r;
    };
    auto st = [&](uint32_t i0, const u64 *v, int n) {
        u64 a[8], pv[8];
        lm_load_run(o, i0, a, n);
        if (p) lm_load_run(p, i0, pv, n);
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (k < n) {
                u64 x;
                if (HASP) { // U*pk*P^-1 - NTT(lift - e) * P^-1
                    x = a[k] + qc.q3 - lm_shoup3<true>(v[k], pi.w, pi.wp, qc.nq);
                    x = lm_csub(lm_csub(x, 2 * qc.q), qc.q);
                } else { // U*pk + NTT(e)
                    x = lm_addmod(a[k], lm_reduce_s(v[k], qc.q, qc.nq, qc.qinv64), qc.q);
                }
                if (p) x = lm_addmod(x, pv[k], qc.q);
                a[k] = x;
            }
        lm_store_run(o, i0, a, n);
    };
    lm_ntt_forward<LOGN, false>(sm, tw_all + (size_t)l * N, qc, tid, ld, st); // 111 VGPRs as it is
}

struct PkTable {
    lm_dev<tw_t> d_pk; // [2][L+K][N] Shoup form; Q limbs carry P^-1
};

extern "C" int lumen_load_public_key(lumen_ctx *ctx, const uint64_t *pk) {
    LM_CHECK(nullptr, ctx && pk, "lumen_load_public_key: NULL argument");
    LM_ENTER(ctx);
    const uint32_t N = ctx->N, L = ctx->L, K = ctx->K, LK = L + K;
    std::vector<tw_t> tab((size_t)2 * LK * N);
    for (uint32_t w = 0; w < 2; w++)
        for (uint32_t l = 0; l < LK; l++) {
            const uint64_t q = ctx->mod[l];
            // P^-1 mod q_l on the Q limbs: the products then leave k_enc_u already divided
            const uint64_t f = l < L && K ? h_invmod(h_p_mod(ctx, q), q) : 1;
            for (uint32_t k = 0; k < N; k++) {
                const uint64_t x = pk[((size_t)w * LK + l) * N + k];
                if (x >= q) return lm_fail(ctx, "public key residue out of range (poly %u limb %u)", w, l);
                tab[((size_t)w * LK + l) * N + k] = h_tw(h_mulmod(x, f, q), q);
            }
        }
    auto sp = std::make_shared<PkTable>();
    if (int rc = sp->d_pk.upload(ctx, tab, "the public key")) return rc;
    lm_ext_put(ctx, "public_key", sp);
    return 0;
}

template <int LOGN>
static int encrypt_t(lumen_ctx *ctx, const int8_t *small, const tw_t *pk, const u64 *pt, const u64 *mcoef,
                     const enc_tinv_t &tinv, u64 *out, u64 *upk, uint32_t count) {
    const uint32_t N = ctx->N, L = ctx->L, K = ctx->K, LK = L + K;
    constexpr lm_geom geom = lm_geom_lds(LOGN);
    {
        lm_prof_scope ps(ctx, "encrypt_u_ntt", (uint64_t)count * LK);
        if (int rc = lm_launch(ctx, k_enc_u<LOGN>, geom, count * LK, small, pk, out, upk, count, L, K, ctx->mods,
                               ctx->sh->tw_fwd.get()))
            return rc;
    }
    if (!K) {
        lm_prof_scope ps(ctx, "encrypt_down_ntt", (uint64_t)count * 2 * L);
        return lm_launch(ctx, k_enc_down<LOGN, false>, geom, count * 2 * L, small, upk, nullptr, nullptr, pt, mcoef, tinv,
                         out, count, L, K, ctx->mods, ctx->sh->tw_fwd.get());
    }
    lm_ks_view kv;
    if (int rc = lm_ks_tables_view(ctx, &kv)) return rc;
    // the P limbs of u*pk_w to the coefficient domain, scaled for the basis extension
    if (int rc = lm_launch_ntt_strided(ctx, upk, (size_t)K * N, upk, (size_t)K * N, count * 2, lm_map_p(ctx), true,
                                       "encrypt_intt_p", kv.yscale))
        return rc;
    {
        enc_hat_t hat;
        memset(&hat, 0, sizeof(hat));
        for (uint32_t j = 0; j < K; j++) { // yscale = N^-1 * hat_j: strip the N^-1
            const uint64_t p = ctx->mod[L + j];
            hat.t[j] = h_tw(h_mulmod(kv.yscale->t[L + j].w, N % p, p), p);
        }
        lm_prof_scope ps(ctx, "encrypt_add_e", count);
        hipLaunchKernelGGL(k_enc_add_e, dim3(1024), dim3(256), 0, ctx->stream, upk, small, count, K, L, ctx->logN,
                           ctx->mods, hat);
        LM_HIP(ctx, hipGetLastError());
    }
    if (K == 2)
        if (int rc = lm_launch_pack_v(ctx, upk, (size_t)K * N, count * 2, 1u, K, L, K)) return rc;
    lm_prof_scope ps(ctx, "encrypt_down_ntt", (uint64_t)count * 2 * L);
    return lm_launch(ctx, k_enc_down<LOGN, true>, geom, count * 2 * L, small, upk, kv.d_bxp, kv.d_pinv, pt, mcoef, tinv, out,
                     count, L, K, ctx->mods, ctx->sh->tw_fwd.get());
}

// plaintexts (NTT-domain RNS, [count][L][N]) or values ([count][rows] slot values) or neither (zeros)
static int encrypt_impl(lumen_ctx *ctx, const uint64_t *plaintexts, const uint64_t *values, uint32_t rows,
                        uint32_t count, const uint8_t seed[32], uint64_t first_index, lumen_set **out) {
    const std::shared_ptr<PkTable> pk_hold = lm_ext_get<PkTable>(ctx, "public_key");
    LM_CHECK(ctx, pk_hold, "no public key loaded (lumen_load_public_key)");
    const PkTable *pkt = pk_hold.get();
    std::shared_ptr<EncoderTables> enc_hold;
    const EncoderTables *enc = nullptr;
    if (values) {
        enc_hold = lm_ext_get<EncoderTables>(ctx, "encoder");
        LM_CHECK(ctx, enc_hold, "no encoder tables (lumen_encoder_set)");
        enc = enc_hold.get();
        LM_CHECK(ctx, rows >= 1 && rows <= ctx->N, "rows=%u out of range [1, N]", rows);
    }
    const uint32_t N = ctx->N, L = ctx->L;
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, count, L, &o)) return rc;
    lm_set_guard og(ctx, o); // given back on every early return below
    if (!count) {
        *out = og.release();
        return 0;
    }
    enc_tinv_t tinv;
    memset(&tinv, 0, sizeof(tinv));
    if (enc) { // message scale riding in k_enc_down's load: T^-1, times -P when the store divides by -P
        for (uint32_t l = 0; l < L; l++) {
            const uint64_t q = ctx->mod[l];
            uint64_t f = enc->tinv.t[l].w;
            if (ctx->K) f = (q - h_mulmod(f, h_p_mod(ctx, q), q)) % q;
            tinv.t[l] = h_tw(f, q);
        }
    }
    // chunks bound the staging buffers (plaintexts: 8*L*N bytes per ciphertext)
    const uint32_t chunk = std::min<uint32_t>(count, 256);
    int8_t *small = (int8_t *)lm_scratch(ctx, "enc_small", (size_t)chunk * 3 * N);
    u64 *dpt = plaintexts ? (u64 *)lm_scratch(ctx, "enc_pt", (size_t)chunk * L * N * sizeof(u64)) : nullptr;
    u64 *dval = values ? (u64 *)lm_scratch(ctx, "enc_val", (size_t)chunk * rows * sizeof(u64)) : nullptr;
    u64 *dm = values ? (u64 *)lm_scratch(ctx, "enc_m", (size_t)chunk * N * sizeof(u64)) : nullptr;
    u64 *upk = ctx->K ? (u64 *)lm_scratch(ctx, "enc_upk", (size_t)chunk * 2 * ctx->K * N * sizeof(u64)) : nullptr;
    if (!small || (plaintexts && !dpt) || (values && (!dval || !dm)) || (ctx->K && !upk)) return 1;
    int rc = 0;
    for (uint32_t first = 0; first < count && !rc; first += chunk) {
        const uint32_t n = std::min(chunk, count - first);
        // the staging buffers are reused: stream order puts these copies behind the previous chunk's kernels
        if (plaintexts)
            LM_HIP(ctx, hipMemcpyAsync(dpt, plaintexts + (size_t)first * L * N, (size_t)n * L * N * sizeof(u64),
                                       hipMemcpyHostToDevice, ctx->stream));
        if (values)
            if ((rc = lm_encode_coeffs(ctx, enc, values + (size_t)first * rows, rows, n, dval, dm))) break;
        {
            lm_prof_scope ps(ctx, "encrypt_pk_sample", n);
            if ((rc = lm_sample_small(ctx, small, nullptr, first_index + first, n, 0, 3, seed))) break;
        }
        u64 *dst = o->d + (size_t)first * 2 * L * N;
        rc = lm_for_logn(ctx, ctx->logN, [&](auto k) { return encrypt_t<k>(ctx, small, pkt->d_pk.get(), dpt, dm, tinv, dst, upk, n); });
    }
    if (rc) return rc;
    if (plaintexts || values) LM_HIP(ctx, hipStreamSynchronize(ctx->stream)); // caller memory
    *out = og.release();
    return 0;
}

extern "C" int lumen_encrypt_pk(lumen_ctx *ctx, const uint64_t *plaintexts, uint32_t count, const uint8_t seed[32],
                                uint64_t first_index, lumen_set **out) {
    LM_CHECK(nullptr, ctx && seed && out, "lumen_encrypt_pk: NULL argument");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_encrypt_pk");
    return encrypt_impl(ctx, plaintexts, nullptr, 0, count, seed, first_index, out);
}

extern "C" int lumen_encrypt_values(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count,
                                    const uint8_t seed[32], uint64_t first_index, lumen_set **out) {
    LM_CHECK(nullptr, ctx && values && seed && out, "lumen_encrypt_values: NULL argument");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_encrypt_values");
    return encrypt_impl(ctx, nullptr, values, rows, count, seed, first_index, out);
}
