// Encoder.Encode on the device (EncoderTables, lm_enc_host.h): the tables of the transform over Z_T and the slot
// scatter in front of it.  Used by lumen_encrypt_values, the secret-key encryptor, the decryptor and Verify.
#include "lm_enc_host.h"

extern "C" int lumen_encoder_set(lumen_ctx *ctx, uint64_t psi_t) {
    LM_CHECK(nullptr, ctx, "lumen_encoder_set: NULL ctx");
    LM_ENTER(ctx);
    const uint64_t T = ctx->T;
    const uint32_t N = ctx->N, logN = ctx->logN;
    LM_CHECK(ctx, T > 2 && (T & (2ull * N - 1)) == 1, "plaintext modulus %llu is not 1 mod 2N", (unsigned long long)T);
    LM_CHECK(ctx, T <= UINT64_MAX / (3ull * logN + 8), "plaintext modulus too large for the lazy transform");
    LM_CHECK(ctx, h_powmod(psi_t, N, T) == T - 1, "psi_t is not a primitive 2N-th root of unity modulo T");
    auto sp = std::make_shared<EncoderTables>();
    sp->modT = lm_make_mod(T);
    sp->ninvT = h_tw(h_invmod(N % T, T), T);
    for (uint32_t l = 0; l < LM_MAX_LIMBS; l++) {
        const uint64_t q = ctx->mod[l < ctx->L ? l : 0];
        sp->tinv.t[l] = h_tw(h_invmod(T % q, q), q);
    }
    std::vector<tw_t> f, b;
    lm_build_tw(T, psi_t, logN, f, b);
    lm_layout_tw(f, logN); // a split degree: the sub-tables of the half transforms, as the context's own tables
    lm_layout_tw(b, logN);
    std::vector<uint32_t> slot(N);
    const uint64_t m = 2ull * N;
    uint64_t pos = 1;
    for (uint32_t i = 0; i < N / 2; i++) {
        slot[i] = h_bitrev((uint32_t)((pos - 1) >> 1), (int)logN);
        slot[i | (N / 2)] = h_bitrev((uint32_t)((m - pos - 1) >> 1), (int)logN);
        pos = (pos * 5) & (m - 1);
    }
    if (sp->d_slot.upload(ctx, slot, "the encoder's slot table") || sp->d_tw_inv.upload(ctx, b, "the encoder's inverse twiddles") ||
        sp->d_tw_fwd.upload(ctx, f, "the encoder's forward twiddles"))
        return 1;
    lm_ext_put(ctx, "encoder", sp);
    return 0;
}

// m[c][slot[i]] = values[c][i] mod T for i < rows, 0 elsewhere (m pre-zeroed)
__global__ void k_scatter_slots(const u64 *__restrict__ values, u64 *__restrict__ m, const uint32_t *__restrict__ slot,
                                uint32_t rows, uint32_t logN, size_t total, mod_t modT) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const size_t c = g / rows;
    const uint32_t i = (uint32_t)(g % rows);
    m[(c << logN) + slot[i]] = lm_reduce(values[g], modT.q, modT.qinv64);
}

// the same with the plaintext's scale: m[c][slot[i]] = values[c][i] * scale mod T.  Encoder.Encode multiplies the VALUES
// by pt.Scale modulo T, ahead of the transform over Z_T [LATTIGO-RECALL] -- modulo T, not modulo q_l.
__global__ void k_scatter_slots_scaled(const u64 *__restrict__ values, u64 *__restrict__ m, const uint32_t *__restrict__ slot,
                                       uint32_t rows, uint32_t logN, size_t total, mod_t modT, tw_t scale) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const size_t c = g / rows;
    const uint32_t i = (uint32_t)(g % rows);
    m[(c << logN) + slot[i]] = lm_shoup(lm_reduce(values[g], modT.q, modT.qinv64), scale, modT.q);
}

int lm_encode_coeffs(lumen_ctx *ctx, const EncoderTables *enc, const uint64_t *values, uint32_t rows, uint32_t n, u64 *dval,
                     u64 *dm, uint64_t scale) {
    const uint32_t N = ctx->N;
    LM_HIP(ctx, hipMemcpyAsync(dval, values, (size_t)n * rows * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    LM_HIP(ctx, hipMemsetAsync(dm, 0, (size_t)n * N * sizeof(u64), ctx->stream));
    const size_t total = (size_t)n * rows;
    {
        lm_prof_scope ps(ctx, "encode_scatter", n);
        const uint64_t T = enc->modT.q;
        if (int rc = scale % T == 1 % T
                         ? lm_launch_flat(ctx, k_scatter_slots, total, dval, dm, enc->d_slot.get(), rows, ctx->logN, total, enc->modT)
                         : lm_launch_flat(ctx, k_scatter_slots_scaled, total, dval, dm, enc->d_slot.get(), rows, ctx->logN, total,
                                          enc->modT, h_tw(scale % T, T)))
            return rc;
    }
    lm_prof_scope ps(ctx, "encode_intt_T", n);
    return lm_launch_ntt_subring(ctx, ctx->logN, enc->d_tw_inv.get(), enc->ninvT, dm, N, dm, N, n, 0, true, &enc->modT);
}
