// The diagonal linear transform, single-hoisted ([LATTIGO-RECALL] Evaluator.MultiplyByDiagMatrix, the non-BSGS branch of
// LinearTransformation, on the *bgv.Evaluator that ServerBFV embeds, fhe/bfv.go:13-21):
//     out = sum_k diag_k (.) Rot_k(ct)
// with ONE decomposition of c1 per batch, per non-zero diagonal one gadget product and one multiply-accumulate over Q and P
// (k_diag_gather), and ONE ModDown for the whole sum.  The lazy accumulator, its identity tables and its close are
// InnerSum's (lm_innersum.hip): ModDown(x + P y) = ModDown(x) + y exactly, so diagonal 0's product m_0 (.) ct -- or a
// zeroed block -- goes through lazy_close as `cur` and the sum comes out canonical.  Batches, lanes and scratch are the
// batch driver's (lm_ks_batch.hip).
// The double-hoisted (baby-step / giant-step) form ([LATTIGO-RECALL] MultiplyByDiagMatrixBSGS) sits on the same object and
// the same kernel: with n1 baby steps a diagonal e = j + i, i = e mod n1 the baby, j = e - i the giant, and
//     out = ModDown( sum_j sigma_{g_j}( KS_j( sum_i m'_{j+i} (.) baby_i ) ) ),   m'_e = sigma_{g_j}^-1(m_e),
// baby_i = sigma_{g_i}(gadget(c1) + (P c0, 0)) over Q and P.  The inner sum is the single-hoisted loop above, into one
// lazy block per giant; a giant step ModDowns polynomial 1 of its block alone, key-switches it under g_j and adds it,
// with polynomial 0 still in QP, to the block the closing ModDown takes (bsgs_batch).  About n1 + D / n1 gadget products
// and keys for D diagonals instead of D.
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
    // double-hoisted (lumen_lintrans_load_bsgs): n1 baby steps, 0 for a single-hoisted transform.  Diagonal d is
    // e = giant[d] + baby[d], baby[d] = e mod n1, and m(d) is pre-rotated by -giant[d]; babies / giants: the distinct
    // non-zero ones, ascending -- the keys the transform needs, in lumen_lintrans_galois_elements' order
    uint32_t n1 = 0;
    std::vector<uint32_t> baby, giant, babies, giants;
    bool keyed() const { return n1 ? !babies.empty() || !giants.empty() : gal.size() > (zero >= 0 ? 1u : 0u); }
    uint32_t blocks() const { return n1 ? (uint32_t)giants.size() + 1 : 0; } // lazy blocks of a batch beyond the lane's own
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

// ---- the double-hoisted form's own passes, elementwise in k_lazy_gather's style: one thread per PAIR of outputs over the
// 2B (L + K) limbs of u's layout, 8 / 16-byte linear accesses, gathered words from the aligned source block.

// A giant step's accumulate, after rotate_mac under the giant's key on ModDown(tmp)[1] (u = s.u, index = the key's table):
//     acc[pw][t][x] = (first ? 0 : acc[pw][t][x]) + u[pw][t][index[x]] + (pw even ? tmp[pw][t][index[x]] : 0)
// over ALL L + K limbs: polynomial 0 of tmp never left QP, so no c0 of the input rides here (it is inside tmp already) and
// the limbs modulo P take part like the others.  Polynomial 1 of tmp is not read (its limbs modulo P are in the
// coefficient domain by now).  RANGE: u < q (lm_mont_reduce_wide), tmp < q and acc < q (canonical lazy blocks), so the sum
// is below 3q < 2^64 and two conditional subtractions (2q, q) bring it back under q.
__global__ __launch_bounds__(256) void k_bsgs_giant(const u64 *__restrict__ u, const u64 *__restrict__ tmp, u64 *__restrict__ acc,
                                                    const uint32_t *__restrict__ index, uint32_t B, uint32_t L, uint32_t K,
                                                    uint32_t pshift, uint32_t logN, uint32_t first, lm_mods mods) {
    const uint32_t N = 1u << logN, nq = L * 2 * B;
    const size_t total = (size_t)2 * B * (L + K) * (N / 2), stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint32_t j = (uint32_t)(g & (N / 2 - 1)) * 2, limb = (uint32_t)(g >> (logN - 1));
        const uint32_t t = limb < nq ? limb / (2 * B) : L + (limb - nq) % K;
        const uint32_t pw = limb < nq ? limb % (2 * B) : (limb - nq) / K;
        const u64 q = mods.m[ks_mod_at(t, L, pshift)].q;
        const size_t base = (size_t)limb << logN, o = base + j;
        const uint2 p = *reinterpret_cast<const uint2 *>(index + j);
        u64 x = u[base + p.x], y = u[base + p.y];
        if (!(pw & 1)) x += tmp[base + p.x], y += tmp[base + p.y];
        ulonglong2 v;
        v.x = v.y = 0;
        if (!first) v = *reinterpret_cast<const ulonglong2 *>(acc + o);
        v.x = lm_csub(lm_csub(v.x + x, 2 * q), q), v.y = lm_csub(lm_csub(v.y + y, 2 * q), q);
        *reinterpret_cast<ulonglong2 *>(acc + o) = v;
    }
}

// The term of baby 0, baby_0 = (P c0, P c1) on Q and 0 on P -- no key, no permutation:
//     lazy[pw][t][x] = (first ? 0 : lazy[pw][t][x]) + mont(m[t][x] * ct[pw][t][x])     on the Q limbs of BOTH polynomials
// and on the limbs modulo P zero when `first`, nothing otherwise.  (The Q limbs of a lazy block carry P^-1, so P * c is
// plain c: k_diag_gather.)  RANGE: ct < q (a canonical input set) and m < q, so the Montgomery input is below
// q^2 < q * 2^64 and the product below q; added to a canonical word, one conditional subtraction.
__global__ __launch_bounds__(256) void k_bsgs_plain(const u64 *__restrict__ ct, const u64 *__restrict__ m, u64 *__restrict__ lazy, uint32_t B,
                                                    uint32_t L, uint32_t K, uint32_t pshift, uint32_t logN, uint32_t first, lm_mods mods) {
    const uint32_t N = 1u << logN, nq = L * 2 * B;
    const size_t total = (size_t)2 * B * (L + K) * (N / 2), stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint32_t j = (uint32_t)(g & (N / 2 - 1)) * 2, limb = (uint32_t)(g >> (logN - 1));
        const size_t o = ((size_t)limb << logN) + j;
        ulonglong2 v;
        v.x = v.y = 0;
        if (limb >= nq) { // a limb modulo P
            if (first) *reinterpret_cast<ulonglong2 *>(lazy + o) = v;
            continue;
        }
        const uint32_t t = limb / (2 * B), pw = limb % (2 * B);
        const mod_t md = mods.m[ks_mod_at(t, L, pshift)];
        const ulonglong2 mm = *reinterpret_cast<const ulonglong2 *>(m + ((size_t)t << logN) + j);
        const ulonglong2 c = *reinterpret_cast<const ulonglong2 *>(ct + (((size_t)pw * L + t) << logN) + j); // [B][2][L][N]
        if (!first) v = *reinterpret_cast<const ulonglong2 *>(lazy + o);
        u64 lo, hi;
        mul128(mm.x, c.x, lo, hi);
        v.x = lm_csub(v.x + lm_mont_reduce(lo, hi, md.q, md.qneg), md.q);
        mul128(mm.y, c.y, lo, hi);
        v.y = lm_csub(v.y + lm_mont_reduce(lo, hi, md.q, md.qneg), md.q);
        *reinterpret_cast<ulonglong2 *>(lazy + o) = v;
    }
}

// The load's pre-rotation of a multiplier: dst[t][x] = src[t][index[x]] for the np limbs of a diagonal, NTT domain; index:
// the gather table of the inverse of the giant's automorphism.  Another block than src.
__global__ __launch_bounds__(256) void k_bsgs_pt_gather(const u64 *__restrict__ src, u64 *__restrict__ dst, const uint32_t *__restrict__ index,
                                                        uint32_t np, uint32_t logN) {
    const uint32_t N = 1u << logN;
    const size_t total = (size_t)np * (N / 2), stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint32_t j = (uint32_t)(g & (N / 2 - 1)) * 2;
        const size_t base = (g >> (logN - 1)) << logN;
        const uint2 p = *reinterpret_cast<const uint2 *>(index + j);
        ulonglong2 v;
        v.x = src[base + p.x], v.y = src[base + p.y];
        *reinterpret_cast<ulonglong2 *>(dst + base + j) = v;
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

int bsgs_plain(lumen_ctx *ctx, const u64 *ct, const u64 *m, u64 *lazy, bool first, uint32_t B, KsTables *tb) {
    lm_prof_scope ps(ctx, "ks_bsgs_plain", (uint64_t)B);
    hipLaunchKernelGGL(k_bsgs_plain, dim3(2048), dim3(256), 0, ctx->stream, ct, m, lazy, B, tb->nl, ctx->K, ctx->L - tb->nl, ctx->logN,
                       first ? 1u : 0u, ctx->mods);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// after rotate_mac under the giant's key (u = s.u, index = the key's gather table)
int bsgs_giant(lumen_ctx *ctx, const u64 *u, const u64 *tmp, u64 *acc, const uint32_t *index, bool first, uint32_t B, KsTables *tb) {
    lm_prof_scope ps(ctx, "ks_bsgs_giant", (uint64_t)B);
    hipLaunchKernelGGL(k_bsgs_giant, dim3(2048), dim3(256), 0, ctx->stream, u, tmp, acc, index, B, tb->nl, ctx->K, ctx->L - tb->nl, ctx->logN,
                       first ? 1u : 0u, ctx->mods);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// the keys of one transform of a call, resolved before anything is enqueued: per diagonal (single-hoisted), or per baby
// and per giant in the order of lumen_lintrans::babies / giants (double-hoisted)
struct LtKeys {
    std::vector<const lm_galois_key *> diag, baby, giant;
};

int find_keys(lumen_ctx *ctx, const lumen_lintrans &lt, LtKeys *k) {
    if (!lt.n1) {
        k->diag.assign(lt.gal.size(), nullptr);
        for (size_t d = 0; d < lt.gal.size(); d++)
            if ((int)d != lt.zero)
                if (int rc = ks_find_key(ctx, lt.gal[d], &k->diag[d])) return rc;
        return 0;
    }
    k->baby.assign(lt.babies.size(), nullptr), k->giant.assign(lt.giants.size(), nullptr);
    for (size_t a = 0; a < lt.babies.size(); a++)
        if (int rc = ks_find_key(ctx, lumen_galois_element(ctx, (int64_t)lt.babies[a]), &k->baby[a])) return rc;
    for (size_t a = 0; a < lt.giants.size(); a++)
        if (int rc = ks_find_key(ctx, lumen_galois_element(ctx, (int64_t)lt.giants[a]), &k->giant[a])) return rc;
    return 0;
}

// The double-hoisted transform of a batch: dst = lt(src), canonical.  blocks: lt.blocks() lazy blocks of `bw` words each,
// of s.u's layout -- block 0 is the sum the closing ModDown takes, and giant 0's inner sum with it (tmp_0 is added as it
// is); block 1 + a is tmp of giants[a].  *ext_ok: s.ext holds the decomposition of src's c1; the giants overwrite it.
//   babies:  the single-hoisted loop, every term into the block of its diagonal's giant, m pre-rotated at load;
//   giant j: step 4a and the storing ModDown (identity tables) for polynomial 1 of tmp_j alone, into polynomial 1 of
//            s.acc2; its decomposition and gadget product under g_j; k_bsgs_giant adds sigma_{g_j}(v + (tmp_j[0], 0));
//   close:   lazy_close with a zeroed `cur` -- diagonal 0 went into block 0 over Q like every other baby-0 term.
int bsgs_batch(lumen_ctx *ctx, const lumen_lintrans &lt, const LtKeys &keys, const u64 *src, u64 *dst, uint32_t B, KsTables *tb,
               const KsScratch &s, u64 *blocks, size_t bw, bool *ext_ok) {
    const uint32_t nb = lt.blocks();
    const size_t ctw = (size_t)2 * tb->nl * ctx->N;
    std::vector<char> first(nb, 1);
    auto block_of = [&](uint32_t j) -> uint32_t {
        return j ? 1 + (uint32_t)(std::lower_bound(lt.giants.begin(), lt.giants.end(), j) - lt.giants.begin()) : 0;
    };
    for (size_t d = 0; d < lt.baby.size(); d++)
        if (!lt.baby[d]) {
            const uint32_t blk = block_of(lt.giant[d]);
            if (int rc = bsgs_plain(ctx, src, lt.m(d), blocks + blk * bw, first[blk], B, tb)) return rc;
            first[blk] = 0;
        }
    for (size_t a = 0; a < lt.babies.size(); a++) {
        if (!*ext_ok) {
            if (int rc = rotate_decompose(ctx, src, B, tb, s)) return rc;
            *ext_ok = true;
        }
        if (int rc = rotate_mac(ctx, src, B, *keys.baby[a], tb, s)) return rc; // s.u = the gadget product under g_i
        for (size_t d = 0; d < lt.baby.size(); d++)
            if (lt.baby[d] == lt.babies[a]) {
                const uint32_t blk = block_of(lt.giant[d]);
                if (int rc = diag_gather(ctx, s.u, src, lt.m(d), blocks + blk * bw, keys.baby[a]->d_index.get(), first[blk], B, tb)) return rc;
                first[blk] = 0;
            }
    }
    std::shared_ptr<lm_galois_key> id;
    if (!lt.giants.empty())
        if (int rc = identity_tables(ctx, &id)) return rc;
    for (size_t a = 0; a < lt.giants.size(); a++) {
        u64 *tmp = blocks + (1 + a) * bw;
        if (int rc = rotate_p_to_coef(ctx, tmp, B, tb, true)) return rc;
        KsScratch st = s;
        st.u = tmp;
        if (int rc = rotate_store_c1(ctx, src, s.acc2, B, *id, tb, st)) return rc; // d1, polynomial 1 of s.acc2
        *ext_ok = false;
        if (int rc = rotate_decompose(ctx, s.acc2, B, tb, s)) return rc; // (the steps read polynomial 1 alone)
        if (int rc = rotate_mac(ctx, s.acc2, B, *keys.giant[a], tb, s)) return rc;
        if (int rc = bsgs_giant(ctx, s.u, tmp, blocks, keys.giant[a]->d_index.get(), first[0], B, tb)) return rc;
        first[0] = 0;
    }
    LM_HIP(ctx, hipMemsetAsync(s.acc2, 0, (size_t)B * ctw * 8, ctx->stream));
    return lazy_close(ctx, s.acc2, dst, blocks, B, tb, s);
}

// outs[i] = lts[i](in) for the n_lts transforms; the decomposition of a batch runs once for the single-hoisted transforms,
// whatever n_lts (a double-hoisted one with giants overwrites it: what follows decomposes again), and the lane's
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
    std::vector<LtKeys> keys(n_lts);
    uint32_t nblocks = 0; // the lazy blocks of the double-hoisted transforms, per lane
    if (keyed && count) { // every key resolved first: the refusal for a missing one comes before any work
        if (int rc = ks_run_open(ctx, count, nl, 2, false, &run)) return rc;
        for (uint32_t i = 0; i < n_lts; i++) {
            if (int rc = find_keys(ctx, *lts[i], &keys[i])) return rc;
            if (lts[i]->keyed()) nblocks = std::max(nblocks, lts[i]->blocks());
        }
    }
    // a block is 2 (L + K) N words per column (235 MB at the headline shape and 64 columns): the batch is halved until the
    // lanes' blocks take at most a quarter of the device's memory
    const size_t colw = (size_t)2 * (ctx->L + ctx->K) * N;
    if (nblocks) {
        size_t free_b = 0, total_b = 0;
        LM_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        while (run.Bmax > 1 && (size_t)run.lanes * nblocks * run.Bmax * colw * 8 > total_b / 4) run.Bmax = (run.Bmax + 1) / 2;
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
        // the double-hoisted transforms' blocks, drawn only when one runs: per lane `nblocks` of the lazy block's size
        const size_t bw = (size_t)run.Bmax * colw;
        u64 *bsgs[2] = {nullptr, nullptr};
        if (nblocks) {
            bsgs[0] = (u64 *)lm_scratch(ctx, "ks_bsgs", nblocks * bw * 8);
            bsgs[1] = run.lanes > 1 ? (u64 *)lm_scratch(ctx, "ks_bsgs_b", nblocks * bw * 8) : bsgs[0];
            if (!bsgs[0] || !bsgs[1]) return 1;
        }
        auto batch = [&](uint32_t, uint32_t first, uint32_t B, const KsScratch &s, u64 *) {
            const u64 *src = in->d + (size_t)first * ctw;
            const int lane = &s == &run.s[1];
            u64 *lz = lazy[lane];
            bool ext_ok = false; // s.ext holds the decomposition of this batch: once, unless a giant step overwrote it
            for (uint32_t i = 0; i < n_lts; i++) {
                const lumen_lintrans &lt = *lts[i];
                u64 *dst = made[i].s->d + (size_t)first * ctw;
                if (!lt.keyed()) {
                    if (int rc = launch_mul_plain(ctx, src, dst, lt.m(lt.zero), (size_t)B * ctw, nl, B)) return rc;
                    continue;
                }
                if (lt.n1) {
                    if (int rc = bsgs_batch(ctx, lt, keys[i], src, dst, B, run.tb, s, bsgs[lane], bw, &ext_ok)) return rc;
                    continue;
                }
                if (!ext_ok) {
                    if (int rc = rotate_decompose(ctx, src, B, run.tb, s)) return rc; // s.ext survives the loops
                    ext_ok = true;
                }
                bool fst = true;
                for (size_t d = 0; d < lt.gal.size(); d++) {
                    if (!keys[i].diag[d]) continue;
                    if (int rc = rotate_mac(ctx, src, B, *keys[i].diag[d], run.tb, s)) return rc; // s.u, rewritten per diagonal
                    if (int rc = diag_gather(ctx, s.u, src, lt.m(d), lz, keys[i].diag[d]->d_index.get(), fst, B, run.tb)) return rc;
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

// Both loads; fn names the entry point in a refusal.  bsgs: n1 baby steps, and every multiplier pre-rotated by minus its
// giant step on the device -- k_pt_prepare into a staging block, then one gather under the table of g_{N/2 - j}.
int load(lumen_ctx *ctx, const char *fn, const int64_t *k, const uint64_t *pts, uint32_t n, uint32_t nl, bool bsgs, uint32_t n1,
         lumen_lintrans **out) {
    *out = nullptr;
    const uint32_t N = ctx->N, K = ctx->K, np = nl + K;
    LM_CHECK(ctx, n >= 1, "%s: a transform has at least one diagonal", fn);
    LM_CHECK(ctx, !bsgs || n1 >= 1, "%s: n1 = 0 baby steps; a double-hoisted transform has at least one", fn);
    LM_CHECK(ctx, nl >= 1 && nl <= ctx->L, "%s: level of %u limbs, the chain has %u", fn, nl, ctx->L);
    LM_CHECK(ctx, K >= 1, "parameters have no special primes: key switching unavailable");
    LM_CHECK(ctx, K <= 2, "key switching supports 1 or 2 special primes (have %u)", K);
    auto lt = std::make_unique<lumen_lintrans>();
    lt->home = ctx->sh.get(), lt->nl = nl, lt->K = K, lt->N = N;
    const int64_t half = (int64_t)(N / 2);
    std::vector<int64_t> seen;
    for (uint32_t d = 0; d < n; d++) {
        LM_CHECK(ctx, k[d] > -half && k[d] < half, "%s: diagonal %lld is outside (-N/2, N/2) = (-%lld, %lld)", fn, (long long)k[d],
                 (long long)half, (long long)half);
        const int64_t e = k[d] < 0 ? k[d] + half : k[d];
        LM_CHECK(ctx, std::find(seen.begin(), seen.end(), e) == seen.end(), "%s: diagonal %lld is given twice (modulo N/2)", fn,
                 (long long)k[d]);
        seen.push_back(e);
        if (!e) lt->zero = (int)d;
        lt->gal.push_back(lumen_galois_element(ctx, e));
        if (bsgs) {
            const uint32_t i = (uint32_t)(e % n1), j = (uint32_t)e - i;
            lt->baby.push_back(i), lt->giant.push_back(j);
            if (i) lt->babies.push_back(i);
            if (j) lt->giants.push_back(j);
        }
    }
    if (bsgs) {
        lt->n1 = n1;
        for (auto *v : {&lt->babies, &lt->giants}) {
            std::sort(v->begin(), v->end());
            v->erase(std::unique(v->begin(), v->end()), v->end());
        }
    }
    for (uint32_t d = 0; d < n; d++)
        for (uint32_t t = 0; t < np; t++) {
            const uint64_t q = ctx->mod[ks_mod_at(t, nl, ctx->L - nl)];
            const uint64_t *src = pts + ((size_t)d * np + t) * N;
            uint64_t bad = 0;
            for (uint32_t i = 0; i < N; i++) bad |= (uint64_t)(src[i] >= q);
            LM_CHECK(ctx, !bad, "%s: plaintext residue out of range at diagonal %lld, limb %u", fn, (long long)k[d], t);
        }
    const size_t words = (size_t)n * np * N;
    lm_dev<u64> raw;
    if (raw.upload(ctx, reinterpret_cast<const u64 *>(pts), words, "a transform's diagonals") || lt->d_m.alloc(ctx, words, "a transform's multipliers")) return 1;
    raw.release_on(ctx->stream, false); // the conversion reads it
    // the giants' inverse gather tables, one behind the other, and the block the conversion of a rotated diagonal goes through
    lm_dev<uint32_t> back;
    lm_dev<u64> stage;
    if (!lt->giants.empty()) {
        std::vector<uint32_t> index(lt->giants.size() * (size_t)N);
        const uint64_t mask = 2ull * N - 1;
        for (size_t a = 0; a < lt->giants.size(); a++) {
            const uint64_t g = lumen_galois_element(ctx, half - (int64_t)lt->giants[a]);
            for (uint32_t i = 0; i < N; i++) { // [LATTIGO-RECALL] ring.AutomorphismNTTIndex, as a Galois key's table
                const uint64_t t1 = 2ull * h_bitrev(i, (int)ctx->logN) + 1;
                index[a * N + i] = h_bitrev((uint32_t)(((g * t1 & mask) - 1) >> 1), (int)ctx->logN);
            }
        }
        if (back.upload(ctx, index, "a transform's pre-rotation tables") || stage.alloc(ctx, (size_t)np * N, "a transform's staging block")) return 1;
        back.release_on(ctx->stream, false), stage.release_on(ctx->stream, false);
    }
    for (uint32_t d = 0; d < n; d++) {
        const u64 *src = raw.get() + (size_t)d * np * N;
        u64 *dst = lt->d_m.get() + (size_t)d * np * N;
        const uint32_t j = bsgs ? lt->giant[d] : 0;
        if (int rc = launch_pt_prepare(ctx, src, j ? stage.get() : dst, nl, np)) return rc;
        if (j) {
            const size_t a = (size_t)(std::lower_bound(lt->giants.begin(), lt->giants.end(), j) - lt->giants.begin());
            hipLaunchKernelGGL(k_bsgs_pt_gather, dim3(std::min<uint32_t>(2048, (np * (N / 2) + 255) / 256)), dim3(256), 0, ctx->stream, stage.get(), dst,
                               back.get() + a * N, np, ctx->logN);
            LM_HIP(ctx, hipGetLastError());
        }
    }
    *out = lt.release();
    return 0;
}

} // namespace

extern "C" int lumen_lintrans_load(lumen_ctx *ctx, const int64_t *k, const uint64_t *pts, uint32_t n, uint32_t nl, lumen_lintrans **out) {
    LM_CHECK(nullptr, ctx && k && pts && out, "lumen_lintrans_load: NULL argument");
    LM_ENTER(ctx);
    return load(ctx, "lumen_lintrans_load", k, pts, n, nl, false, 0, out);
}

extern "C" int lumen_lintrans_load_bsgs(lumen_ctx *ctx, const int64_t *k, const uint64_t *pts, uint32_t n, uint32_t nl, uint32_t n1,
                                        lumen_lintrans **out) {
    LM_CHECK(nullptr, ctx && k && pts && out, "lumen_lintrans_load_bsgs: NULL argument");
    LM_ENTER(ctx);
    return load(ctx, "lumen_lintrans_load_bsgs", k, pts, n, nl, true, n1, out);
}

// the power of two n1 in [1, N/2] with the fewest keys -- distinct babies != 0 plus distinct giants != 0 --, the smaller
// on a tie; 0 for an argument the load would refuse
extern "C" uint32_t lumen_lintrans_best_baby_steps(uint32_t log_n, const int64_t *k, uint32_t n) {
    if (!k || !n || log_n < 1 || log_n > 31) return 0;
    const int64_t half = (int64_t)1 << (log_n - 1);
    std::vector<uint64_t> es(n);
    for (uint32_t d = 0; d < n; d++) {
        if (!(k[d] > -half && k[d] < half)) return 0;
        es[d] = (uint64_t)(k[d] < 0 ? k[d] + half : k[d]);
    }
    uint32_t best = 0;
    size_t best_cost = 0;
    for (uint64_t n1 = 1; n1 <= (uint64_t)half; n1 *= 2) {
        std::vector<uint64_t> bs, gs;
        for (uint64_t e : es) {
            if (e % n1) bs.push_back(e % n1);
            if (e - e % n1) gs.push_back(e - e % n1);
        }
        size_t cost = 0;
        for (auto *v : {&bs, &gs}) {
            std::sort(v->begin(), v->end());
            cost += (size_t)(std::unique(v->begin(), v->end()) - v->begin());
        }
        if (!best || cost < best_cost) best = (uint32_t)n1, best_cost = cost;
    }
    return best;
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
    if (lt->n1) { // double-hoisted: the babies' keys, then the giants', ascending; at most one of each per diagonal
        const uint64_t mask = 2ull * lt->N - 1;
        for (auto *v : {&lt->babies, &lt->giants})
            for (uint32_t x : *v) {
                uint64_t g = 1, b = 5; // 5^x mod 2N: lumen_galois_element without a context
                for (uint32_t e = x; e; e >>= 1, b = (b * b) & mask)
                    if (e & 1) g = (g * b) & mask;
                gal_els[cnt++] = g;
            }
        return cnt;
    }
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
