// The rotation alone (host only): Evaluator.Automorphism / RotateColumnsNew / RotateRowsNew / RotateHoistedNew (the
// evaluator that ServerBFV embeds, fhe/bfv.go:13-21).  out = sigma_g(c0 + k0(c1), k1(c1)): decompose, product, and a
// ModDown that ends in a plain gather (k_rotdown_ntt, lm_keyswitch.hip).  The input set is read in place and the output
// set is the destination: no accumulator, no ping-pong, no copy, no canonicalising pass.  Batches, lanes and scratch are
// the batch driver's (lm_ks_batch.hip).
#include "lm_ks_host.h"

extern "C" uint64_t lumen_galois_element(const lumen_ctx *ctx, int64_t k) {
    if (!ctx || ctx->N < 2) return 0;
    // [LATTIGO-RECALL] rlwe.Parameters.GaloisElement: 5 generates the column rotations, its order mod 2N is N / 2
    const int64_t order = (int64_t)(ctx->N >> 1);
    int64_t e = k % order;
    if (e < 0) e += order;
    const uint64_t mask = 2ull * ctx->N - 1;
    uint64_t g = 1, b = 5;
    for (; e; e >>= 1, b = (b * b) & mask)
        if (e & 1) g = (g * b) & mask;
    return g;
}

namespace {

#define LM_MAX_HOISTED 64u

// outs[i] = Automorphism(in, gal_els[i]) for the n_els elements; the decomposition of a batch runs once, whatever n_els
int rotate_sets(lumen_ctx *ctx, const lumen_set *in, const uint64_t *gal_els, uint32_t n_els, lumen_set **outs, const char *what) {
    for (uint32_t i = 0; i < n_els; i++) outs[i] = nullptr;
    if (int rc = check_level_of_chain(ctx, in, what)) return rc;
    LM_CHECK(ctx, n_els <= LM_MAX_HOISTED, "%s: %u Galois elements, at most %u in one call", what, n_els, LM_MAX_HOISTED);
    bool keyed = false;
    for (uint32_t i = 0; i < n_els; i++) {
        LM_CHECK(ctx, (gal_els[i] & 1) && gal_els[i] < 2ull * ctx->N, "%s: Galois element %llu is not an odd residue mod 2N", what,
                 (unsigned long long)gal_els[i]);
        keyed = keyed || gal_els[i] != 1;
    }
    // the identity is a copy and needs no key ([LATTIGO-RECALL] Evaluator.Automorphism returns the input for galEl == 1)
    const uint32_t count = in->count, nl = in->nl;
    KsRun run;
    std::vector<const lm_galois_key *> keys(n_els, nullptr);
    if (keyed) {
        LM_CHECK(ctx, ctx->K >= 1, "parameters have no special primes: key switching unavailable");
        if (int rc = ks_run_open(ctx, count, nl, 2, false, &run)) return rc; // (refuses K > 2, as InnerSum does)
        for (uint32_t i = 0; i < n_els; i++)
            if (gal_els[i] != 1)
                if (int rc = ks_find_key(ctx, gal_els[i], &keys[i])) return rc;
    }
    std::vector<lm_set_guard> made; // the new sets go back unless the call succeeds
    made.reserve(n_els);
    for (uint32_t i = 0; i < n_els; i++) {
        lumen_set *o = nullptr;
        if (int rc = lumen_set_create(ctx, count, nl, &o)) return rc;
        made.emplace_back(ctx, o);
    }
    if (count) {
        for (uint32_t i = 0; i < n_els; i++)
            if (gal_els[i] == 1)
                LM_HIP(ctx, hipMemcpyAsync(made[i].s->d, in->d, in->words * 8, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (count && keyed) {
        const size_t ctw = (size_t)2 * nl * ctx->N;
        if (int rc = ks_run_scratch(ctx, &run)) return rc;
        auto batch = [&](uint32_t, uint32_t first, uint32_t B, const KsScratch &s, u64 *) {
            const u64 *src = in->d + (size_t)first * ctw;
            if (int rc = rotate_decompose(ctx, src, B, run.tb, s)) return rc; // once per batch: s.ext survives the loop
            for (uint32_t i = 0; i < n_els; i++) {
                if (!keys[i]) continue;
                if (int rc = rotate_product(ctx, src, B, *keys[i], run.tb, s)) return rc; // s.u, rewritten per element
                if (int rc = rotate_store(ctx, src, made[i].s->d + (size_t)first * ctw, B, *keys[i], run.tb, s)) return rc;
            }
            return 0;
        };
        if (int rc = ks_run(ctx, run, count, ctw, batch)) return rc; // (joined: the caller reads the sets on the main stream)
    }
    for (uint32_t i = 0; i < n_els; i++) outs[i] = made[i].release();
    return 0;
}

} // namespace

extern "C" int lumen_automorphism(lumen_ctx *ctx, const lumen_set *in, uint64_t gal_el, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && out, "lumen_automorphism: NULL argument");
    LM_ENTER(ctx);
    return rotate_sets(ctx, in, &gal_el, 1, out, "lumen_automorphism");
}

extern "C" int lumen_rotate_columns(lumen_ctx *ctx, const lumen_set *in, int64_t k, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && out, "lumen_rotate_columns: NULL argument");
    LM_ENTER(ctx);
    const uint64_t g = lumen_galois_element(ctx, k);
    return rotate_sets(ctx, in, &g, 1, out, "lumen_rotate_columns");
}

extern "C" int lumen_rotate_rows(lumen_ctx *ctx, const lumen_set *in, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && out, "lumen_rotate_rows: NULL argument");
    LM_ENTER(ctx);
    const uint64_t g = 2ull * ctx->N - 1; // [LATTIGO-RECALL] GaloisElementForRowRotation
    return rotate_sets(ctx, in, &g, 1, out, "lumen_rotate_rows");
}

extern "C" int lumen_rotate_hoisted(lumen_ctx *ctx, const lumen_set *in, const uint64_t *gal_els, uint32_t n_els, lumen_set **outs) {
    LM_CHECK(nullptr, ctx && in && gal_els && outs, "lumen_rotate_hoisted: NULL argument");
    LM_ENTER(ctx);
    return rotate_sets(ctx, in, gal_els, n_els, outs, "lumen_rotate_hoisted");
}
