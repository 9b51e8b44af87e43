// InnerSum and matrixInnerSumEval (fhe/ligero.go:299-370): per input column
//     MulNew(ct, pt) -> InnerSum(., 1, rows) -> Rescale to level 1
// batched over columns.  InnerSum(ct, batch, n) is ONE algorithm, the double-and-add of [LATTIGO-RECALL]
// Evaluator.InnerSum (rlwe/inner_sum.go): cur = ct, and for i = 0, 1, ..., j = n >> i while j > 1:
//     j odd:  lazy (+)= sigma_{5^k}(gadget(cur.c1) + (P cur.c0, 0)),  k = (n - (n & (2^(i+1) - 1))) batch      -- over Q and P
//     cur = cur + Rot_{2^i batch}(cur)                                                  -- a rotation (lm_keyswitch.hip)
// The term and the doubling of an iteration share one decomposition of cur.c1.  A SumPlan lists the iterations of a call
// with their keys, before anything is enqueued; inner_sum_batch walks it on a batch of columns.  Two endings:
//   * no lazy term (n a power of two): cur is the sum, in [0, 2q).  The driver canonicalises it (k_acc_canon) -- or the
//     rescale that follows absorbs the range, and then the last doubling may write the rescale's coefficient-form input
//     itself (rotate_close, lm_ks_close.hip);
//   * lazy terms: the lazy accumulator takes ONE ModDown, over the sum of popcount(n) - 1 terms, and out = ModDown(lazy) +
//     cur, canonical (lazy_close).
// For batch 1 and n a power of two <= N the doublings are the rotations of lumen_inner_sum_galois_elements, which fold the
// two slot rows with the row swap at n == N.  Batches, lanes, groups and scratch are the batch driver's (lm_ks_batch.hip).
#include <algorithm>

#include "lm_ks_host.h"

// words of a lazy accumulator ([0, 2q), see k_moddown_ntt) to canonical form: for the callers that hand the
// accumulator out as it is (lumen_inner_sum; matrixInnerSumEval when there is no limb to drop).  Elementwise,
// [count][2][L][N], 16-byte accesses.
__global__ __launch_bounds__(256) void k_acc_canon(u64 *__restrict__ acc, size_t pairs, uint32_t logN, uint32_t L, lm_mods mods) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < pairs; g += stride) {
        const u64 q = mods.m[(uint32_t)((g >> (logN - 1)) % L)].q;
        ulonglong2 v = *reinterpret_cast<ulonglong2 *>(acc + 2 * g);
        v.x = lm_csub(v.x, q), v.y = lm_csub(v.y, q);
        *reinterpret_cast<ulonglong2 *>(acc + 2 * g) = v;
    }
}

// ---- the lazy gather-accumulate of an InnerSum of general length (lazy_gather: a term, the close).  Elementwise over
// the 2B (L + K) limbs of u's layout (ks_u_at on both sides), right after k_ks_mac, every limb in the NTT domain:
//     lazy[pw][t][j] = (first ? 0 : lazy[pw][t][j]) + u[pw][t][index[j]] (+ c0[t][index[j]] for w == 0, t < L)
// The Q limbs of u carry P^-1 (folded into the key, see moddown_body's storer), so Lattigo's P * c0 is plain c0 there;
// on the limbs modulo P it is 0.  The same index table serves every limb.  One thread per PAIR of outputs: the index
// words and the accumulator move as 8 / 16-byte accesses, linearly; the two gathered words come from the aligned source
// block the output block maps to (moddown_body: the top bits of index[j] are a function of the top bits of j), at most
// N words apart, out of L2.
// The close (u == NULL, index == NULL: no product, the identity): lazy[pw][t][j] += c1[t][j] for w == 1, t < L alone.
// RANGES.  u < q (lm_mont_reduce_wide), cur in [0, 2q) (the lazy accumulator of the doublings), the stored word < q:
// the sum is below 4q < 2^64 for every modulus of a context ((3 logN + 8) q < 2^64) and comes back under q with two
// conditional subtractions.  Every accumulator word is CANONICAL whatever the number of terms: the inverse transform
// of the limbs modulo P and the ModDown that close the sum take it as they take a gadget product.
__global__ __launch_bounds__(256) void k_lazy_gather(const u64 *__restrict__ u, const u64 *__restrict__ cur, u64 *__restrict__ lazy,
                                                     const uint32_t *__restrict__ index, uint32_t B, uint32_t L, uint32_t K,
                                                     uint32_t pshift, uint32_t logN, uint32_t first, lm_mods mods) {
    const uint32_t N = 1u << logN, nq = L * 2 * B; // limbs [0, nq) of the layout are Q limbs: [L][2B]; behind them [2B][K]
    const size_t total = (size_t)2 * B * (L + K) * (N / 2), stride = (size_t)gridDim.x * blockDim.x;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint32_t j = (uint32_t)(g & (N / 2 - 1)) * 2, limb = (uint32_t)(g >> (logN - 1));
        const uint32_t t = limb < nq ? limb / (2 * B) : L + (limb - nq) % K;
        const uint32_t pw = limb < nq ? limb % (2 * B) : (limb - nq) / K;
        const bool with_c = t < L && (pw & 1) == (u ? 0u : 1u); // c0 rides on a term's polynomial 0, c1 on the close's polynomial 1
        if (!u && !with_c) continue;
        const u64 q = mods.m[ks_mod_at(t, L, pshift)].q;
        const size_t o = ((size_t)limb << logN) + j;
        uint2 p;
        p.x = j, p.y = j + 1;
        if (index) p = *reinterpret_cast<const uint2 *>(index + j);
        ulonglong2 v;
        v.x = v.y = 0;
        if (!first) v = *reinterpret_cast<const ulonglong2 *>(lazy + o);
        if (u) v.x += u[((size_t)limb << logN) + p.x], v.y += u[((size_t)limb << logN) + p.y];
        if (with_c) {
            const u64 *c = cur + (((size_t)pw * L + t) << logN); // [B][2][L][N]: polynomial pw = 2b + w, limb t
            v.x += c[p.x], v.y += c[p.y];
        }
        v.x = lm_csub(lm_csub(v.x, 2 * q), q), v.y = lm_csub(lm_csub(v.y, 2 * q), q);
        *reinterpret_cast<ulonglong2 *>(lazy + o) = v;
    }
}

// -------------------------------------------------------------------- host side
namespace {

int acc_canon(lumen_ctx *ctx, u64 *acc, size_t words, uint32_t L) {
    if (!words) return 0;
    hipLaunchKernelGGL(k_acc_canon, dim3(2048), dim3(256), 0, ctx->stream, acc, words / 2, ctx->logN, L, ctx->mods);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// ---- the plan of an InnerSum(., batch, n)

// batch 1 and a power of two <= N: the rotations of lumen_inner_sum_galois_elements, no lazy term
bool is_plain(const lumen_ctx *ctx, uint32_t batch, uint32_t n) { return batch == 1 && n && !(n & (n - 1)) && n <= ctx->N; }

// The walk: fn(term, doubling) per iteration, in order, with the Galois elements of the lazy term (0: none) and of the
// doubling; the first non-zero status ends it.  (batch, n) is plain or passes general_check.
template <class Fn>
int sum_walk(const lumen_ctx *ctx, uint32_t batch, uint32_t n, Fn &&fn) {
    if (is_plain(ctx, batch, n)) {
        uint64_t gal[64];
        const uint32_t cnt = lumen_inner_sum_galois_elements(ctx, n, gal);
        for (uint32_t r = 0; r < cnt; r++)
            if (int rc = fn((uint64_t)0, gal[r])) return rc;
        return 0;
    }
    for (uint32_t i = 0, j = n; j > 1; i++, j >>= 1) {
        const uint64_t term = (j & 1) ? lumen_galois_element(ctx, (int64_t)((uint64_t)(n - (n & ((2u << i) - 1))) * batch)) : 0;
        if (int rc = fn(term, lumen_galois_element(ctx, (int64_t)((uint64_t)batch << i)))) return rc;
    }
    return 0;
}

struct SumPlan {
    struct Step {
        const lm_galois_key *dbl = nullptr, *term = nullptr; // the doubling's key; the lazy term's, or none
        uint64_t dbl_el = 0;                                  // the doubling's Galois element (the c0 fold's sigma_coef)
    } it[32];                                                // n < 2^32: at most 31 iterations
    uint32_t cnt = 0;
    uint64_t last_el = 0; // the Galois element of the last doubling (rotate_close)
    bool lazy = false;    // some iteration has a lazy term
};

// every key resolved, in order of first use: the refusal for a missing one comes before any work
int sum_plan(lumen_ctx *ctx, uint32_t batch, uint32_t n, SumPlan *p) {
    return sum_walk(ctx, batch, n, [&](uint64_t term, uint64_t dbl) {
        SumPlan::Step &st = p->it[p->cnt++];
        if (term) {
            if (int rc = ks_find_key(ctx, term, &st.term)) return rc;
            p->lazy = true;
        }
        p->last_el = st.dbl_el = dbl;
        return ks_find_key(ctx, dbl, &st.dbl);
    });
}

int general_check(lumen_ctx *ctx, uint32_t batch, uint32_t n, const char *what) {
    LM_CHECK(ctx, batch >= 1 && n >= 1, "%s: batch size %u and length %u must both be at least 1", what, batch, n);
    LM_CHECK(ctx, ctx->K >= 1, "parameters have no special primes: key switching unavailable");
    LM_CHECK(ctx, ctx->K <= 2, "key switching supports 1 or 2 special primes (have %u)", ctx->K);
    if (is_plain(ctx, batch, n)) return 0;
    LM_CHECK(ctx, (uint64_t)batch * n <= ctx->N / 2, "%s: batch size %u x length %u spans beyond the slot row of %u slots", what, batch, n,
             ctx->N / 2);
    return 0;
}

} // namespace

// ---- the lazy accumulator: a block of s.u's size and layout per lane, words canonical.  lazy_blocks, identity_tables and
// lazy_close are the diagonal linear transform's too (lm_ks_host.h)

// one more block per lane, of the gadget product's size at the top level
int lazy_blocks(lumen_ctx *ctx, const KsRun &run, u64 **lazy) {
    const size_t bytes = (size_t)run.Bcap() * 2 * (ctx->L + ctx->K) * ctx->N * 8;
    lazy[0] = (u64 *)lm_scratch(ctx, "ks_lazy", bytes);
    lazy[1] = run.lanes > 1 ? (u64 *)lm_scratch(ctx, "ks_lazy_b", bytes) : lazy[0];
    return lazy[0] && lazy[1] ? 0 : 1;
}

// A term, after rotate_mac under its key (u = s.u, index = the key's gather table): lazy = (first ? 0 : lazy) +
// sigma(u + (c0, 0)) over Q and P, no ModDown; `first` stores where later terms add.  The close's first step (u and index
// NULL, the identity): lazy_1 += cur.c1 on the Q limbs.  cur in [0, 2q).
static int lazy_gather(lumen_ctx *ctx, const u64 *u, const u64 *cur, u64 *lazy, const uint32_t *index, bool first, uint32_t B, KsTables *tb) {
    lm_prof_scope ps(ctx, "ks_lazy_gather", (uint64_t)B);
    hipLaunchKernelGGL(k_lazy_gather, dim3(2048), dim3(256), 0, ctx->stream, u, cur, lazy, index, B, tb->nl, ctx->K, ctx->L - tb->nl,
                       ctx->logN, first ? 1u : 0u, ctx->mods);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// the identity's gather tables, owned by the context and built at first use: the ModDown of the lazy accumulator
// permutes nothing (the relinearisation key has such a pair too, but it may not be loaded)
int identity_tables(lumen_ctx *ctx, std::shared_ptr<lm_galois_key> *out) {
    static const char *const NAME = "ks_identity";
    LM_SHARED_LOCK(ctx);
    auto gk = lm_ext_get<lm_galois_key>(ctx, NAME);
    if (!gk) {
        gk = std::make_shared<lm_galois_key>();
        std::vector<uint32_t> index(ctx->N);
        for (uint32_t i = 0; i < ctx->N; i++) index[i] = i;
        if (gk->d_index.upload(ctx, index, "the identity's index table") || gk->d_inv_index.upload(ctx, index, "the identity's index table"))
            return 1;
        lm_ext_put(ctx, NAME, gk);
    }
    *out = std::move(gk);
    return 0;
}

// out = ModDown(lazy) + cur for every column, canonical; `out` is another block than `cur`, lazy is consumed.
// lazy_1 += c1 on the Q limbs, step 4a on the lazy block, then the rotation's storing ModDown under the identity with the
// lazy block for its gadget product: it adds `cur`'s c0 to polynomial 0 itself and nothing to polynomial 1.
int lazy_close(lumen_ctx *ctx, const u64 *cur, u64 *out, u64 *lazy, uint32_t B, KsTables *tb, const KsScratch &s) {
    std::shared_ptr<lm_galois_key> id;
    if (int rc = identity_tables(ctx, &id)) return rc;
    if (int rc = lazy_gather(ctx, nullptr, cur, lazy, nullptr, false, B, tb)) return rc;
    if (int rc = rotate_p_to_coef(ctx, lazy, B, tb)) return rc;
    KsScratch sl = s;
    sl.u = lazy;
    return rotate_store(ctx, cur, out, B, *id, tb, sl);
}

namespace {

// ---- InnerSum(., batch, n) of the B columns of acc, in place: canonical when the plan has lazy terms, in [0, 2q) when
// it has none.  `lazy`: the lane's lazy accumulator (a plan with lazy terms).  With close_out (a rescale follows a plan
// that has a doubling and no lazy term) the last doubling leaves the sum there in coefficient form instead, and acc
// holds nothing the caller may use.  fold_s (with close_out alone): two blocks of ks_fold_words for the c0 fold
// (LUMEN_KS_C0_FOLD, lm_ks_host.h) -- polynomial 0 then goes through the doublings as (A, S) and is whole again only in
// close_out.
int inner_sum_batch(lumen_ctx *ctx, u64 *acc, uint32_t B, const SumPlan &plan, KsTables *tb, const KsScratch &s, u64 *lazy,
                    u64 *close_out, u64 *fold_s = nullptr) {
    LM_CHECK(ctx, !close_out || (plan.cnt && !plan.lazy), "InnerSum has no rotation to close");
    // |S| < (2^cnt - 1) 2^lift_bits must fit three words of two's complement
    LM_CHECK(ctx, !fold_s || (close_out && ks_fold_serves(ctx, tb, plan.cnt)),
             "the c0 fold cannot hold the lifts of %u rotations of %u bits in 192", plan.cnt, tb->lift_bits);
    u64 *cur = acc, *other = s.acc2; // ping-pong: the automorphism reads two positions of the old accumulator per output
    bool first = true;
    for (uint32_t r = 0; r < plan.cnt; r++) {
        const SumPlan::Step &st = plan.it[r];
        if (int rc = rotate_decompose(ctx, cur, B, tb, s)) return rc; // once per iteration: s.ext survives the lazy term
        if (fold_s) { // S ping-pongs as the accumulator does; the first rotation has none to read
            const u64 *s_in = r ? fold_s + ((r - 1) & 1) * ks_fold_words(ctx, B) : nullptr;
            u64 *s_out = fold_s + (r & 1) * ks_fold_words(ctx, B);
            if (r + 1 == plan.cnt) return rotate_close_fold(ctx, cur, close_out, B, *st.dbl, st.dbl_el, tb, s, s_in, s_out);
            if (int rc = rotate_add_fold(ctx, cur, other, B, *st.dbl, st.dbl_el, tb, s, s_in, s_out)) return rc;
            std::swap(cur, other);
            continue;
        }
        if (st.term) {
            if (int rc = rotate_mac(ctx, cur, B, *st.term, tb, s)) return rc;
            if (int rc = lazy_gather(ctx, s.u, cur, lazy, st.term->d_index.get(), first, B, tb)) return rc;
            first = false;
        }
        if (close_out && r + 1 == plan.cnt) // from whichever of the two blocks the doublings so far have left the sum in
            return rotate_close(ctx, cur, close_out, B, *st.dbl, plan.last_el, tb, s);
        if (int rc = rotate_add(ctx, cur, other, B, *st.dbl, tb, s)) return rc;
        std::swap(cur, other);
    }
    if (plan.lazy) {
        if (int rc = lazy_close(ctx, cur, other, lazy, B, tb, s)) return rc;
        std::swap(cur, other);
    }
    if (cur != acc)
        LM_HIP(ctx, hipMemcpyAsync(acc, cur, (size_t)B * 2 * tb->nl * ctx->N * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

int check_inner_sum_level(lumen_ctx *ctx, const lumen_set *in, const char *what) {
    LM_FULL_WIDTH(ctx, in, what);
    // lumen_inner_sum and lumen_matrix_inner_sum serve the top level, where the path calls InnerSum
    // (fhe/ligero.go:319-325 -- MulNew and InnerSum precede the rescale), and refuse anything else: their callers
    // rely on that.  The *_at_level entry points take a set at any level of the chain.
    LM_CHECK(ctx, in->nl == ctx->L, "%s is implemented at the top level only (set has %u of %u limbs)", what,
             in->nl, ctx->L);
    return 0;
}

// InnerSum(ct, batch, n) at the level of `in` (checked by the caller).  `general`: the name of a general entry point,
// which takes what general_check does; NULL for the others, which take batch 1 and a power of two <= N.  A plain sum
// stays on one lane.  A set of no ciphertexts looks no key up.
int inner_sum_run(lumen_ctx *ctx, const lumen_set *in, uint32_t batch, uint32_t n, const char *general, lumen_set **out) {
    if (general) {
        if (int rc = general_check(ctx, batch, n, general)) return rc;
    } else {
        LM_CHECK(ctx, is_plain(ctx, batch, n), "InnerSum length %u is not a power of two <= N", n);
    }
    KsRun run;
    if (int rc = ks_run_open(ctx, in->count, in->nl, is_plain(ctx, batch, n) ? 1 : 2, false, &run, true)) return rc;
    SumPlan plan;
    if (in->count)
        if (int rc = sum_plan(ctx, batch, n, &plan)) return rc;
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, in->count, in->nl, &o)) return rc;
    lm_set_guard og(ctx, o);
    if (in->words)
        LM_HIP(ctx, hipMemcpyAsync(o->d, in->d, in->words * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (int rc = ks_run_scratch(ctx, &run)) return rc;
    u64 *lazy[2] = {nullptr, nullptr};
    if (plan.lazy)
        if (int rc = lazy_blocks(ctx, run, lazy)) return rc;
    const size_t ctw = (size_t)2 * in->nl * ctx->N;
    auto batch_fn = [&](uint32_t, uint32_t first, uint32_t B, const KsScratch &s, u64 *) {
        return inner_sum_batch(ctx, o->d + (size_t)first * ctw, B, plan, run.tb, s, lazy[&s == &run.s[1]], nullptr);
    };
    if (int rc = ks_run(ctx, run, in->count, ctw, batch_fn)) return rc;
    if (!plan.lazy) // the doublings leave [0, 2q)
        if (int rc = acc_canon(ctx, o->d, o->words, in->nl)) return rc;
    *out = og.release();
    return 0;
}

// matrixInnerSumEval at the level of `matrix` (checked by the caller), nl limbs in, min(nl, 2) out: MulNew, the batch
// above in the group's accumulator, the group's rescale.  `general` as for inner_sum_run.
int matrix_inner_sum_run(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt, uint32_t rows, const char *general,
                         lumen_set **out) {
    if (general) {
        if (int rc = general_check(ctx, 1, rows, general)) return rc;
    } else {
        LM_CHECK(ctx, is_plain(ctx, 1, rows), "rows=%u is not a power of two <= N", rows);
    }
    KsRun run;
    if (int rc = ks_run_open(ctx, matrix->count, matrix->nl, 2, true, &run, true)) return rc;
    SumPlan plan;
    if (matrix->count)
        if (int rc = sum_plan(ctx, 1, rows, &plan)) return rc;
    u64 *ptT = nullptr;
    if (int rc = upload_ptT(ctx, pt, matrix->nl, &ptT)) return rc;
    const uint32_t N = ctx->N, L = matrix->nl, target = std::min<uint32_t>(2, L);
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, matrix->count, target, &o)) return rc;
    lm_set_guard og(ctx, o);
    const size_t ctw = (size_t)2 * L * N, octw = (size_t)2 * target * N;
    if (int rc = ks_run_scratch(ctx, &run)) return rc; // run.acc: the group's accumulators
    u64 *lazy[2] = {nullptr, nullptr};
    if (plan.lazy)
        if (int rc = lazy_blocks(ctx, run, lazy)) return rc;
    u64 *work = (u64 *)lm_scratch(ctx, "rescale_work", run.group_bytes);
    u64 *tbuf = (u64 *)lm_scratch(ctx, "rescale_t", (size_t)run.group * 2 * N * 8);
    if (!work || !tbuf) return 1;
    // The last doubling of a batch writes the rescale's coefficient-form input itself, at the batch's place in `work`
    // (LUMEN_KS_CLOSE_FUSED, lm_ks_close.hip): when a rescale follows, there is a rotation (rows > 1), the chain has the
    // coefficient form's tables and the sum ends in a doubling -- with lazy terms it ends in lazy_close, whose canonical
    // words the unfused rescale takes.
    bool close = false;
    // (a split degree has no k_ks_close -- its storer is tied to the pass plan of a one-piece inverse: the switch is ignored
    // there, ModDown and the whole rescale run, same residues)
    if (L > target && rows > 1 && ctx->tune.ks_close_fused && !plan.lazy && !lm_is_split(ctx->logN)) {
        const int rc = lm_rescale_coef_ready(ctx);
        if (rc && rc != 2) return rc;
        close = rc == 0;
    }
    // The c0 fold (LUMEN_KS_C0_FOLD): on this route polynomial 0's first reader after MulNew is the closing inverse
    // transform, so the doublings keep it as (A, S) and run ModDown for polynomial 1 alone (lm_ks_host.h).  Per lane two
    // blocks of S, one signed three-word integer per coefficient and column.
    u64 *fold_s[2] = {nullptr, nullptr};
    if (close && ctx->tune.ks_c0_fold && ks_fold_serves(ctx, run.tb, plan.cnt)) {
        const size_t bytes = 2 * ks_fold_words(ctx, run.Bcap()) * 8; // (a pair folds in blocks of its own size: S blocks of 2 Bmax columns)
        fold_s[0] = (u64 *)lm_scratch(ctx, "ks_fold_s", bytes);
        fold_s[1] = run.lanes > 1 ? (u64 *)lm_scratch(ctx, "ks_fold_s_b", bytes) : fold_s[0];
        if (!fold_s[0] || !fold_s[1]) return 1;
    }
    auto batch_fn = [&](uint32_t g0, uint32_t first, uint32_t B, const KsScratch &s, u64 *a) {
        if (int rc = launch_mul_plain(ctx, matrix->d + (size_t)(g0 + first) * ctw, a, ptT, (size_t)B * ctw, L, B)) // ligero.go:319
            return rc;
        const int lane = &s == &run.s[1];
        return inner_sum_batch(ctx, a, B, plan, run.tb, s, lazy[lane], close ? work + (size_t)first * ctw : nullptr, fold_s[lane]); // ligero.go:325
    };
    // the rescale of the group needs both lanes.  ligero.go:331-333
    auto end_of_group = [&](uint32_t g0, uint32_t gn) {
        if (close) // the inverse transforms are done
            return lm_rescale_polys_from_coef(ctx, work, L, o->d + (size_t)g0 * octw, target, gn * 2);
        if (L > target) return lm_rescale_polys(ctx, run.acc, L, o->d + (size_t)g0 * octw, target, gn * 2, work, tbuf);
        if (!plan.lazy) // no rescale to absorb the range the doublings leave
            if (int rc = acc_canon(ctx, run.acc, (size_t)gn * ctw, L)) return rc;
        LM_HIP(ctx, hipMemcpyAsync(o->d + (size_t)g0 * octw, run.acc, (size_t)gn * ctw * 8, hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    };
    if (int rc = ks_run(ctx, run, matrix->count, ctw, batch_fn, end_of_group)) return rc;
    *out = og.release();
    return 0;
}

} // namespace

extern "C" int lumen_inner_sum_general(lumen_ctx *ctx, const lumen_set *in, uint32_t batch_size, uint32_t n, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && out, "lumen_inner_sum_general: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_level_of_chain(ctx, in, "InnerSum")) return rc;
    return inner_sum_run(ctx, in, batch_size, n, "lumen_inner_sum_general", out);
}

extern "C" int lumen_matrix_inner_sum_general(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt, uint32_t rows,
                                              lumen_set **out) {
    LM_CHECK(nullptr, ctx && matrix && pt && out, "lumen_matrix_inner_sum_general: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_level_of_chain(ctx, matrix, "matrixInnerSumEval")) return rc;
    return matrix_inner_sum_run(ctx, matrix, pt, rows, "lumen_matrix_inner_sum_general", out);
}

// the elements of the walk in order of first use, without duplicates or the identity; 0 for what general_check refuses
extern "C" uint32_t lumen_inner_sum_general_elements(const lumen_ctx *ctx, uint32_t batch_size, uint32_t n, uint64_t *gal_els) {
    if (!ctx || !gal_els) return 0;
    if (!is_plain(ctx, batch_size, n) && (!batch_size || !n || (uint64_t)batch_size * n > ctx->N / 2)) return 0;
    uint32_t cnt = 0;
    sum_walk(ctx, batch_size, n, [&](uint64_t term, uint64_t dbl) { // at most 2 log2(n) <= 62 elements
        for (uint64_t g : {term, dbl})
            if (g > 1 && std::find(gal_els, gal_els + cnt, g) == gal_els + cnt) gal_els[cnt++] = g;
        return 0;
    });
    return cnt;
}

extern "C" int lumen_inner_sum(lumen_ctx *ctx, const lumen_set *in, uint32_t n, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && out, "lumen_inner_sum: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_inner_sum_level(ctx, in, "InnerSum")) return rc;
    return inner_sum_run(ctx, in, 1, n, nullptr, out);
}

extern "C" int lumen_inner_sum_at_level(lumen_ctx *ctx, const lumen_set *in, uint32_t n, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && out, "lumen_inner_sum_at_level: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_level_of_chain(ctx, in, "InnerSum")) return rc;
    return inner_sum_run(ctx, in, 1, n, nullptr, out);
}

extern "C" int lumen_matrix_inner_sum(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt,
                                      uint32_t rows, lumen_set **out) {
    LM_CHECK(nullptr, ctx && matrix && pt && out, "lumen_matrix_inner_sum: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_inner_sum_level(ctx, matrix, "matrixInnerSumEval")) return rc;
    return matrix_inner_sum_run(ctx, matrix, pt, rows, nullptr, out);
}

extern "C" int lumen_matrix_inner_sum_at_level(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt,
                                               uint32_t rows, lumen_set **out) {
    LM_CHECK(nullptr, ctx && matrix && pt && out, "lumen_matrix_inner_sum_at_level: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_level_of_chain(ctx, matrix, "matrixInnerSumEval")) return rc;
    return matrix_inner_sum_run(ctx, matrix, pt, rows, nullptr, out);
}
