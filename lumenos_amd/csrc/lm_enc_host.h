// Host-side declarations shared by the encryptors and the key generator: the public-key encryptor, the encoder and the
// decryptor (lm_encrypt.hip), the secret-key encryptor (lm_encrypt_sk.hip) and key generation (lm_keygen.hip).
#pragma once
#include "lm_ks_dev.h"

struct enc_tinv_t {
    tw_t t[LM_MAX_LIMBS]; // message scale per Q limb: -P * T^-1 mod q_l (K > 0), T^-1 mod q_l (K = 0)
};

// ---- Encoder.Encode on the device ([LATTIGO-RECALL] bgv.Encoder: slot i of row 0 sits at the
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
int lm_encode_coeffs(lumen_ctx *ctx, const EncoderTables *enc, const uint64_t *values, uint32_t rows, uint32_t n, u64 *dval,
                     u64 *dm);

struct SkTable {
    lm_dev<tw_t> d_sk; // [L][N] Shoup form
};
// a secret generated on the device (lm_keygen.hip): [L][N] Shoup form
void lm_install_secret_key_dev(lumen_ctx *ctx, lm_dev<tw_t> &&d_sk);

// ---- the deterministic samplers of key generation (lm_keygen.hip), shared with the secret-key encryptor
// out [nitems][N] int8: item i draws `stream` (0: ternary, else Gaussian) of sample index d_index[i] under `seed`
int lm_kg_small(lumen_ctx *ctx, int8_t *out, const u64 *d_index, uint32_t nitems, uint32_t stream, const uint8_t seed[32]);
// a + i * item_stride: [LK][N] words uniform mod q_m from stream 16 + m of sample index d_index[i], NTT domain
int lm_kg_uniform(lumen_ctx *ctx, u64 *a, size_t item_stride, const u64 *d_index, uint32_t nitems, uint32_t LK,
                  const uint8_t seed[32]);
// host words -> a device temporary, through the pinned staging buffer
int lm_kg_upload(lumen_ctx *ctx, void *dev, const void *host, size_t bytes);

// lm_ctx.hip
int lm_d2h(lumen_ctx *ctx, void *host, const void *dev, size_t bytes, bool wait);
// `height` rows of `width` bytes, spitch apart on the host, to rows dpitch apart on the device; returns when `host` may
// be reused.  Page-locked memory: one DMA; pageable memory goes through the bounce buffers in whole rows.
int lm_h2d_rows(lumen_ctx *ctx, void *dev, size_t dpitch, const void *host, size_t spitch, size_t width, size_t height);
