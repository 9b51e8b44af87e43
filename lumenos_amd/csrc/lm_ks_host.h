// Host-side declarations shared by the units of the Galois key switch: the rotation (lm_keyswitch.hip), the placement of
// its scratch buffers (lm_ks_scratch.hip), the ciphertext x plaintext product that precedes it (lm_mulplain.hip) and the
// ciphertext x ciphertext product that ends in one (lm_mulrelin.hip).
#pragma once
#include "lm_ks_dev.h"

// per-context constants of the key switch at one level of the modulus chain (nl of the context's L limbs; below, L
// stands for nl) and its cached work lists (lm_keyswitch.hip)
struct KsTables {
    lm_dev<bx_t> d_bx;   // [beta][L+K], targets by position (ks_mod_at)
    lm_dev<bx_t> d_bxp;  // [L]  (P -> q_t)
    lm_dev<tw_t> d_pinv; // [L]  P^-1 mod q_t
    uint32_t nl = 0;     // the level: Q limbs of the ciphertexts it switches
    uint32_t beta = 0;   // ceil(nl / K) digits
    lm_ninv_t yscale; // per modulus: N^-1 * (M/m)^-1 mod m of the source group the modulus sits in
    std::vector<uint16_t> pairs; // (digit | target << 8) of every extension the key switch needs, target-major
    std::map<uint32_t, lm_dev<uint32_t>> d_work; // per batch size: the workgroup order of the extension kernel
    std::map<uint32_t, lm_dev<uint32_t>> d_work_down; // ... and of the ModDown kernel
};
int get_tables(lumen_ctx *ctx, KsTables **out); // the top level's
// the tables of the level with nl limbs, 1 <= nl <= L, built at its first use and cached (nl == L: get_tables)
int get_tables_at(lumen_ctx *ctx, uint32_t nl, KsTables **out);

// the scratch buffers of one lane
struct KsScratch {
    u64 *coef, *ext, *u, *acc2;
};

// acc, acc_out: [B][2][nl][N] at the level of `tb`; acc_out = acc + Rot_galEl(acc) for every column (lm_keyswitch.hip).
// s: scratch of a batch of B columns at the TOP level, of which a lower level uses a prefix of every block.
int rotate_accumulate(lumen_ctx *ctx, const u64 *acc, u64 *acc_out, uint32_t B, const lm_galois_key &gk,
                      KsTables *tb, const KsScratch &s);
// the last rotation of an InnerSum that a rescale follows, after its steps 1-4a (lm_ks_close.hip): out, [B][2][nl][N], gets
// the COEFFICIENT form of acc + Rot_galEl(acc), canonical -- what the rescale's inverse transform would have made of it.
// work_down: ModDown's work list for B columns at the level of `tb`.
int ks_close_launch(lumen_ctx *ctx, const u64 *acc, u64 *out, uint32_t B, const lm_galois_key &gk, uint64_t gal_el,
                    KsTables *tb, const KsScratch &s, const uint32_t *work_down);
// the scratch of a batch of B columns on `lane`, placed by measurement at a context's first key switch (lm_ks_scratch.hip).
// tb: always the TOP level's tables, whatever level asks -- the blocks are sized, and the candidates timed, once.
int get_scratch(lumen_ctx *ctx, uint32_t B, KsTables *tb, KsScratch *s, int lane = 0, u64 **group_acc = nullptr,
                size_t group_acc_bytes = 0);

// step 0, MulNew(ct, pt) (lm_mulplain.hip): the plaintext as the device multiplier pt * T, and out = ct (.) it
int upload_ptT(lumen_ctx *ctx, const uint64_t *pt, uint32_t nl, u64 **out);
int launch_mul_plain(lumen_ctx *ctx, const u64 *ct, u64 *out, const u64 *ptT, size_t words, uint32_t nl,
                     uint32_t ncts);

// the relinearisation key as a switching key with identity gather tables (lm_ks_key.hip); empty before lumen_load_relin_key
std::shared_ptr<lm_galois_key> lm_relin_key(lumen_ctx *ctx);
// a set at a level of the chain: full width, 1 <= nl <= L (lm_keyswitch.hip)
int check_level_of_chain(lumen_ctx *ctx, const lumen_set *in, const char *what);
// the batching of a key switch, shared by InnerSum and the relinearisation (lm_keyswitch.hip)
uint32_t ks_batch(const lumen_ctx *ctx);
uint32_t ks_lanes(const lumen_ctx *ctx);
// enqueue on the context's second stream for the lifetime of the guard
struct LaneGuard {
    lumen_ctx *ctx;
    hipStream_t saved;
    LaneGuard(lumen_ctx *c, int lane) : ctx(c), saved(c->stream) {
        if (lane) ctx->stream = ctx->stream2;
    }
    ~LaneGuard() { ctx->stream = saved; }
};
