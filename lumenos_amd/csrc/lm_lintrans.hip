// The diagonal linear transform, single-hoisted ([LATTIGO-RECALL] Evaluator.MultiplyByDiagMatrix, the non-BSGS branch of
// LinearTransformation, on the *bgv.Evaluator that ServerBFV embeds, fhe/bfv.go:13-21):
//     out = sum_k diag_k (.) Rot_k(ct)
// with ONE decomposition of c1 per batch, per non-zero diagonal one gadget product and one multiply-accumulate over Q and P
// (k_diag_gather), and ONE ModDown for the whole sum.  The lazy accumulator, its identity tables and its close are
// InnerSum's (lm_innersum.hip): ModDown(x + P y) = ModDown(x) + y exactly, so diagonal 0's product m_0 (.) ct -- or a
// zeroed block -- goes through lazy_close as `cur` and the sum comes out canonical.  Batches, lanes and scratch are the
// batch driver's (lm_ks_batch.hip).  The double-hoisted (baby-step / giant-step) form is not built.
#include <algorithm>

#include "lm_ks_host.h"

// A resident transform: the diagonals as the kernel's multipliers, m_k = pt_k * T in Montgomery form, by POSITION (the
// level's nl limbs of Q, then the K limbs modulo P: ks_mod_at), converted once at load.
struct lumen_lintrans {
    const lm_shared *home = nullptr; // the tables of the context that loaded it: it serves that context and its clones
    uint32_t nl = 0, K = 0, N = 0;
    std::vector<uint64_t> gal; // per diagonal: its Galois element, 1 for diagonal 0
    int zero = -1;             // which diagonal is diagonal 0, or none
    lm_dev<u64> d_m;           // [n][nl + K][N]
    const u64 *m(size_t d) const { return d_m.get() + d * (nl + K) * N; }
    bool keyed() const { return gal.size() > (zero >= 0 ? 1u : 0u); }
};

// ---- the term of a diagonal: k_lazy_gather's term step (lm_innersum.hip) with the product in front of the sum.
// Elementwise over the 2B (L + K) limbs of u's layout ([L][2B] Q limbs, behind them [2B][K]; ks_u_at on both sides), right
// after k_ks_mac, every limb in the NTT domain:
//     lazy[pw][t][j] = (first ? 0 : lazy[pw][t][j]) + mont(m[t][j] * (u[pw][t][index[j]] (+ c0[t][index[j]] for w == 0, t < L)))
// The Q limbs of u carry P^-1 (folded into the key), so Lattigo's P * c0 is plain c0 there; on the limbs modulo P it is 0.
// m: the diagonal's multiplier, [L + K][N] by position, not permuted -- sigma applies to the ciphertext alone.  One
// thread per PAIR of outputs: the index words, the multiplier and the accumulator move as 8 / 16-byte accesses, linearly;
// the gathered words come from the aligned source block the output block maps to, out of L2, as in k_lazy_gather.
// RANGES, for every modulus q of a context.  u < q (lm_mont_reduce_wide) and c0 < q (a canonical input set), so the factor
// is below 2q, and with m < q the Montgomery input is below 2q * q < q * 2^64 (2q < 2^64): lm_mont_reduce takes it and its
// reduced product is below q.  Added to a CANONICAL accumulator word it gives a value below 2q, and one conditional
// subtraction restores canonical form: every accumulator word is canonical whatever the number of diagonals, and the
// inverse transform of the limbs modulo P and the ModDown of lazy_close take the block as they take a gadget product.
__global__ __launch_bounds__(256) void k_diag_gather(const u64 *__restrict__ u, const u64 *__restrict__ ct, const u64 *__restrict__ m,
                                                     u64 *__restrict__ lazy, const uint32_t *__restrict__ index, uint32_t B, uint32_t L,
                                                     uint32_t K, uint32_t pshift, uint32_t logN, uint32_t first, lm_mods mods) {
    const uint32_t N = 1u << logN, nq = L * 2 * B; // limbs [0, nq) of the layout are Q limbs: [L][2B]; behind them [2B][K]
    const size_t total = (size_t)2 * B * (L + K) * (N / 2), stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint32_t j = (uint32_t)(g & (N / 2 - 1)) * 2, limb = (uint32_t)(g >> (logN - 1));
        const uint32_t t = limb < nq ? limb / (2 * B) : L + (limb - nq) % K;
        const uint32_t pw = limb < nq ? limb % (2 * B) : (limb - nq) / K;
        const mod_t md = mods.m[ks_mod_at(t, L, pshift)];
        const size_t o = ((size_t)limb << logN) + j;
        const uint2 p = *reinterpret_cast<const uint2 *>(index + j);
        const ulonglong2 mm = *reinterpret_cast<const ulonglong2 *>(m + ((size_t)t << logN) + j);
        u64 x = u[((size_t)limb << logN) + p.x], y = u[((size_t)limb << logN) + p.y];
        if (t < L && !(pw & 1)) {
            const u64 *c = ct + (((size_t)pw * L + t) << logN); // [B][2][L][N]: polynomial pw = 2b + w, limb t
            x += c[p.x], y += c[p.y];
        }
        ulonglong2 v;
        v.x = v.y = 0;
        if (!first) v = *reinterpret_cast<const ulonglong2 *>(lazy + o);
        u64 lo, hi;
        mul128(mm.x, x, lo, hi);
        v.x = lm_csub(v.x + lm_mont_reduce(lo, hi, md.q, md.qneg), md.q);
        mul128(mm.y, y, lo, hi);
        v.y = lm_csub(v.y + lm_mont_reduce(lo, hi, md.q, md.qneg), md.q);
        *reinterpret_cast<ulonglong2 *>(lazy + o) = v;
    }
}

// -------------------------------------------------------------------- host side
namespace {

// after rotate_mac under the diagonal's key (u = s.u, index = the key's gather table)
int diag_gather(lumen_ctx *ctx, const u64 *u, const u64 *ct, const u64 *m, u64 *lazy, const uint32_t *index, bool first, uint32_t B,
                KsTables *tb) {
    lm_prof_scope ps(ctx, "ks_diag_gather", (uint64_t)B);
    hipLaunchKernelGGL(k_diag_gather, dim3(2048), dim3(256), 0, ctx->stream, u, ct, m, lazy, index, B, tb->nl, ctx->K, ctx->L - tb->nl,
                       ctx->logN, first ? 1u : 0u, ctx->mods);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// outs[i] = lts[i](in) for the n_lts transforms; the decomposition of a batch runs once, whatever n_lts, and the lane's
// lazy block goes from one transform to the next.  A set of no ciphertexts looks no key up.
int transforms_run(lumen_ctx *ctx, const lumen_set *in, const lumen_lintrans *const *lts, uint32_t n_lts, lumen_set **outs, const char *what) {
    for (uint32_t i = 0; i < n_lts; i++) outs[i] = nullptr;
    if (int rc = check_level_of_chain(ctx, in, what)) return rc;
    bool keyed = false;
    for (uint32_t i = 0; i < n_lts; i++) {
        LM_CHECK(ctx, lts[i], "%s: transform %u is NULL", what, i);
        LM_CHECK(ctx, lts[i]->home == ctx->sh.get(), "%s: transform %u was loaded on another context", what, i);
        LM_CHECK(ctx, in->nl == lts[i]->nl, "%s: the set has %u limbs, transform %u was loaded at the level of %u", what, in->nl, i,
                 lts[i]->nl);
        keyed = keyed || lts[i]->keyed();
    }
    const uint32_t count = in->count, nl = in->nl, N = ctx->N;
    KsRun run;
    std::vector<std::vector<const lm_galois_key *>> keys(n_lts);
    if (keyed && count) { // every key resolved first: the refusal for a missing one comes before any work
        if (int rc = ks_run_open(ctx, count, nl, 2, false, &run)) return rc;
        for (uint32_t i = 0; i < n_lts; i++) {
            keys[i].assign(lts[i]->gal.size(), nullptr);
            for (size_t d = 0; d < lts[i]->gal.size(); d++)
                if ((int)d != lts[i]->zero)
                    if (int rc = ks_find_key(ctx, lts[i]->gal[d], &keys[i][d])) return rc;
        }
    }
    std::vector<lm_set_guard> made; // the new sets go back unless the call succeeds
    made.reserve(n_lts);
    for (uint32_t i = 0; i < n_lts; i++) {
        lumen_set *o = nullptr;
        if (int rc = lumen_set_create(ctx, count, nl, &o)) return rc;
        made.emplace_back(ctx, o);
    }
    const size_t ctw = (size_t)2 * nl * N;
    const uint64_t counted = ctx->mul_counter; // the counter is the Mul / MulNew wrappers' (bfv.go:34-42), as for the rotations
    if (count && !keyed) { // diagonal 0 alone: no key, no key switch
        for (uint32_t i = 0; i < n_lts; i++)
            if (int rc = launch_mul_plain(ctx, in->d, made[i].s->d, lts[i]->m(lts[i]->zero), in->words, nl, count)) return rc;
    }
    if (count && keyed) {
        if (int rc = ks_run_scratch(ctx, &run)) return rc;
        u64 *lazy[2] = {nullptr, nullptr};
        if (int rc = lazy_blocks(ctx, run, lazy)) return rc;
        auto batch = [&](uint32_t, uint32_t first, uint32_t B, const KsScratch &s, u64 *) {
            const u64 *src = in->d + (size_t)first * ctw;
            u64 *lz = lazy[&s == &run.s[1]];
            if (int rc = rotate_decompose(ctx, src, B, run.tb, s)) return rc; // once per batch: s.ext survives the loops
            for (uint32_t i = 0; i < n_lts; i++) {
                const lumen_lintrans &lt = *lts[i];
                u64 *dst = made[i].s->d + (size_t)first * ctw;
                if (!lt.keyed()) {
                    if (int rc = launch_mul_plain(ctx, src, dst, lt.m(lt.zero), (size_t)B * ctw, nl, B)) return rc;
                    continue;
                }
                bool fst = true;
                for (size_t d = 0; d < lt.gal.size(); d++) {
                    if (!keys[i][d]) continue;
                    if (int rc = rotate_mac(ctx, src, B, *keys[i][d], run.tb, s)) return rc; // s.u, rewritten per diagonal
                    if (int rc = diag_gather(ctx, s.u, src, lt.m(d), lz, keys[i][d]->d_index.get(), fst, B, run.tb)) return rc;
                    fst = false;
                }
                // cur = m_0 (.) ct, or nothing: lazy_close adds it behind the ModDown
                if (lt.zero >= 0) {
                    if (int rc = launch_mul_plain(ctx, src, s.acc2, lt.m(lt.zero), (size_t)B * ctw, nl, B)) return rc;
                } else {
                    LM_HIP(ctx, hipMemsetAsync(s.acc2, 0, (size_t)B * ctw * 8, ctx->stream));
                }
                if (int rc = lazy_close(ctx, s.acc2, dst, lz, B, run.tb, s)) return rc;
            }
            return 0;
        };
        if (int rc = ks_run(ctx, run, count, ctw, batch)) return rc; // (joined: the caller reads the sets on the main stream)
    }
    ctx->mul_counter = counted;
    for (uint32_t i = 0; i < n_lts; i++) outs[i] = made[i].release();
    return 0;
}

} // namespace

extern "C" int lumen_lintrans_load(lumen_ctx *ctx, const int64_t *k, const uint64_t *pts, uint32_t n, uint32_t nl, lumen_lintrans **out) {
    LM_CHECK(nullptr, ctx && k && pts && out, "lumen_lintrans_load: NULL argument");
    LM_ENTER(ctx);
    *out = nullptr;
    const uint32_t N = ctx->N, K = ctx->K, np = nl + K;
    LM_CHECK(ctx, n >= 1, "lumen_lintrans_load: a transform has at least one diagonal");
    LM_CHECK(ctx, nl >= 1 && nl <= ctx->L, "lumen_lintrans_load: level of %u limbs, the chain has %u", nl, ctx->L);
    LM_CHECK(ctx, K >= 1, "parameters have no special primes: key switching unavailable");
    LM_CHECK(ctx, K <= 2, "key switching supports 1 or 2 special primes (have %u)", K);
    auto lt = std::make_unique<lumen_lintrans>();
    lt->home = ctx->sh.get(), lt->nl = nl, lt->K = K, lt->N = N;
    const int64_t half = (int64_t)(N / 2);
    std::vector<int64_t> seen;
    for (uint32_t d = 0; d < n; d++) {
        LM_CHECK(ctx, k[d] > -half && k[d] < half, "lumen_lintrans_load: diagonal %lld is outside (-N/2, N/2) = (-%lld, %lld)",
                 (long long)k[d], (long long)half, (long long)half);
        const int64_t e = k[d] < 0 ? k[d] + half : k[d];
        LM_CHECK(ctx, std::find(seen.begin(), seen.end(), e) == seen.end(), "lumen_lintrans_load: diagonal %lld is given twice (modulo N/2)",
                 (long long)k[d]);
        seen.push_back(e);
        if (!e) lt->zero = (int)d;
        lt->gal.push_back(lumen_galois_element(ctx, e));
    }
    for (uint32_t d = 0; d < n; d++)
        for (uint32_t t = 0; t < np; t++) {
            const uint64_t q = ctx->mod[ks_mod_at(t, nl, ctx->L - nl)];
            const uint64_t *src = pts + ((size_t)d * np + t) * N;
            uint64_t bad = 0;
            for (uint32_t i = 0; i < N; i++) bad |= (uint64_t)(src[i] >= q);
            LM_CHECK(ctx, !bad, "lumen_lintrans_load: plaintext residue out of range at diagonal %lld, limb %u", (long long)k[d], t);
        }
    const size_t words = (size_t)n * np * N;
    lm_dev<u64> raw;
    if (raw.upload(ctx, reinterpret_cast<const u64 *>(pts), words, "a transform's diagonals") || lt->d_m.alloc(ctx, words, "a transform's multipliers")) return 1;
    raw.release_on(ctx->stream, false); // the conversion reads it
    for (uint32_t d = 0; d < n; d++)
        if (int rc = launch_pt_prepare(ctx, raw.get() + (size_t)d * np * N, lt->d_m.get() + (size_t)d * np * N, nl, np)) return rc;
    *out = lt.release();
    return 0;
}

extern "C" void lumen_lintrans_destroy(lumen_ctx *ctx, lumen_lintrans *lt) {
    if (!lt) return;
    if (ctx) {
        LM_ENTER(ctx);
        lt->d_m.release_on(ctx->stream, false); // a transform still enqueued reads it (the lanes are joined on the main stream)
        delete lt;
        return;
    }
    delete lt;
}

extern "C" uint32_t lumen_lintrans_galois_elements(const lumen_lintrans *lt, uint64_t *gal_els) {
    if (!lt || !gal_els) return 0;
    uint32_t cnt = 0;
    for (size_t d = 0; d < lt->gal.size(); d++)
        if ((int)d != lt->zero) gal_els[cnt++] = lt->gal[d];
    return cnt;
}

extern "C" int lumen_linear_transform(lumen_ctx *ctx, const lumen_set *in, const lumen_lintrans *lt, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && lt && out, "lumen_linear_transform: NULL argument");
    LM_ENTER(ctx);
    return transforms_run(ctx, in, &lt, 1, out, "lumen_linear_transform");
}

extern "C" int lumen_linear_transforms(lumen_ctx *ctx, const lumen_set *in, const lumen_lintrans *const *lts, uint32_t n_lts,
                                       lumen_set **outs) {
    LM_CHECK(nullptr, ctx && in && lts && outs, "lumen_linear_transforms: NULL argument");
    LM_ENTER(ctx);
    return transforms_run(ctx, in, lts, n_lts, outs, "lumen_linear_transforms");
}
