// Declarations shared by the client-side translation units: the samplers (lm_sample.hip), the encoder (lm_encoder.hip),
// the decryptor (lm_decrypt.hip), the two encryptors (lm_encrypt.hip, lm_encrypt_sk.hip), key generation
// (lm_keygen.hip) and Verify (lm_verify.hip).
#pragma once
#include "lm_ks_dev.h"
#include "lm_sample_dev.h"

struct enc_tinv_t {
    tw_t t[LM_MAX_LIMBS]; // message scale per Q limb: -P * T^-1 mod q_l (K > 0), T^-1 mod q_l (K = 0)
};

// A small coefficient (|v| <= 19) as a residue modulo *q.  q by address: it is read on the negative side only, as the
// loaders of the transform kernels always did; read ahead of the comparison, the compiler turns the branch into a
// select and those kernels' machine code changes (tools/kernel_asm_diff.py).
__device__ __forceinline__ u64 lm_lift_small(int8_t v, const u64 *q) { return v >= 0 ? (u64)v : *q - (u64)(-(int)v); }
// r += m * ti mod q in place, canonical: the lifted error r (canonical) takes the message coefficient m times the
// limb's message scale ti.  In place for the same reason: by value the secret-key encryptor's kernel changes.
__device__ __forceinline__ void lm_add_scaled_msg(u64 &r, u64 m, const tw_t &ti, const lm_qc &qc) {
    r = lm_shoup3<true>(m, ti.w, ti.wp, qc.nq, r); // < 4q
    r = lm_csub(lm_csub(r, 2 * qc.q), qc.q);
    r = lm_csub(r, qc.q);
}

// ---- Encoder.Encode on the device (lm_encoder.hip; [LATTIGO-RECALL] bgv.Encoder: slot i of row 0 sits at the
// evaluation point 5^i, row 1 at -5^i; slots -> INTT over Z_T -> scale by T^-1 mod q_l -> NTT)
struct EncoderTables {
    lm_dev<uint32_t> d_slot; // [N] slot -> coefficient position of the Z_T transform
    lm_dev<tw_t> d_tw_inv;   // [N] inverse twiddles modulo T
    lm_dev<tw_t> d_tw_fwd;   // [N] forward twiddles modulo T (Encoder.Decode)
    mod_t modT;
    tw_t ninvT;
    enc_tinv_t tinv; // T^-1 mod q_l
};
// Encoder.Encode up to the coefficient vector modulo T, enqueued on the context's stream: n columns of `rows` host
// values -> dm [n][N] (dval: device staging of n * rows words).  The caller waits for the stream before `values` changes.
// scale: the plaintext's scale, applied to the values modulo T ahead of the transform (1: Encode of a fresh plaintext).
int lm_encode_coeffs(lumen_ctx *ctx, const EncoderTables *enc, const uint64_t *values, uint32_t rows, uint32_t n, u64 *dval,
                     u64 *dm, uint64_t scale = 1);

// ---- the secret-key table and client-side decryption in stages (lm_decrypt.hip), shared by lumen_decrypt and
// lumen_verify_columns
struct SkTable {
    lm_dev<tw_t> d_sk; // [L][N] Shoup form
};
// a secret generated on the device (lm_keygen.hip): [L][N] Shoup form
void lm_install_secret_key_dev(lumen_ctx *ctx, lm_dev<tw_t> &&d_sk);
// what lumen_decrypt refuses about its set, scale and context (no device work)
int lm_decrypt_check(lumen_ctx *ctx, const lumen_set *set, uint64_t scale, const char *what);
// Decryptor.DecryptNew + the decoder's transform over Z_T, enqueued on the context's stream: t = [count][N] words
// below T in the transform's output order, slot[i] = the position of slot value i in it.  `keep` holds the key and
// encoder tables for as long as the caller's kernels read them.
struct lm_decoded {
    const u64 *t = nullptr;
    const uint32_t *slot = nullptr;
    std::shared_ptr<void> keep[2];
};
int lm_decrypt_decode(lumen_ctx *ctx, const lumen_set *set, lm_decoded *out);
// The decryptor's first kernel alone (k_decrypt_phase: c0 + c1 * s formed in the load of the inverse transform):
// phase [count][nl][N] = INTT(c0 + c1 * s), times T when times_T (what Decode goes on from), canonical.
int lm_decrypt_phase(lumen_ctx *ctx, const u64 *ct, uint32_t count, uint32_t nl, const SkTable *sk, u64 *phase, bool times_T);
// values[c][i] = t[c][slot[i]] * scale^-1 mod T for i < nvalues, copied to the host buffer on the context's stream
// (not waited for)
int lm_decrypt_slots(lumen_ctx *ctx, const lm_decoded &dec, uint32_t count, uint64_t scale, uint32_t nvalues,
                     uint64_t *values);

// ---- the deterministic samplers (lm_sample.hip).  Item i draws sample index d_index[i], or base + i when d_index is
// NULL, under `seed`.
// out [nitems][ns][N] int8: streams s0 .. s0 + ns - 1 of every item (stream 0: ternary, every other: Gaussian)
int lm_sample_small(lumen_ctx *ctx, int8_t *out, const u64 *d_index, u64 base, uint32_t nitems, uint32_t s0, uint32_t ns,
                    const uint8_t seed[32]);
// a + i * item_stride: [LK][N] words uniform mod q_m from stream 16 + m, NTT domain
int lm_sample_uniform(lumen_ctx *ctx, u64 *a, size_t item_stride, const u64 *d_index, u64 base, uint32_t nitems, uint32_t LK,
                      const uint8_t seed[32]);
// the kernel arguments of a launch that draws for itself (k_keygen_evk_seeded, k_key_expand): the seed as the cipher's
// key words, and the rejection bounds 2^64 - (2^64 mod q_m) of the first LK moduli
enc_seed_t lm_sample_seed(const uint8_t seed[32]);
kg_lim_t lm_sample_lim(const lumen_ctx *ctx, uint32_t LK);

// ---- the sample indices of key generation (lm_keygen.hip, THE SAMPLING CONTRACT): I(key_id, e) = key_id * 4096 + e.
// The loaders of seeded keys (lm_ks_key.hip) draw `a` under the same indices.
#define LM_KG_INDEX_STRIDE 4096ull
#define LM_KG_ID_SECRET 0ull
#define LM_KG_ID_PUBLIC 1ull
#define LM_KG_ID_RELIN 2ull
#define LM_KG_ID_RINGSWITCH 3ull
#define LM_KG_ID_GALOIS 0x10000ull
