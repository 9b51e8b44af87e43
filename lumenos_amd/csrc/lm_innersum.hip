// InnerSum and matrixInnerSumEval (fhe/ligero.go:299-370): per input column
//     MulNew(ct, pt) -> InnerSum(., 1, rows) -> Rescale to level 1
// batched over columns.  InnerSum is log2(rows) rounds of
//     acc += Rot(acc)       (hoisted key-switch + NTT-domain automorphism)
// each of them one rotate_accumulate (lm_keyswitch.hip) on a batch of columns; the last one before a rescale is a
// rotate_close (lm_ks_close.hip).  Batches, lanes, groups and scratch are the batch driver's (lm_ks_batch.hip).
//
// The same for a length that is no power of two, or a batch size above 1 (lumen_inner_sum_general,
// lumen_matrix_inner_sum_general): the lazy double-and-add, see inner_sum_general_batch below.
#include <algorithm>
#include <map>

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

// -------------------------------------------------------------------- host side
namespace {

int acc_canon(lumen_ctx *ctx, u64 *acc, size_t words, uint32_t L) {
    if (!words) return 0;
    hipLaunchKernelGGL(k_acc_canon, dim3(2048), dim3(256), 0, ctx->stream, acc, words / 2, ctx->logN, L, ctx->mods);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// InnerSum(., 1, n) of the B columns of acc, in place.  With close_out (a rescale follows and n > 1) the last rotation
// leaves its result there in coefficient form instead, and acc holds nothing the caller may use.
int inner_sum_batch(lumen_ctx *ctx, u64 *acc, uint32_t B, uint32_t n, KsTables *tb, const KsScratch &s,
                    u64 *close_out = nullptr) {
    uint64_t gal[64];
    const uint32_t cnt = lumen_inner_sum_galois_elements(ctx, n, gal);
    LM_CHECK(ctx, !close_out || cnt, "InnerSum(%u) has no rotation to close", n);
    for (uint32_t r = 0; r < cnt; r++) {
        const lm_galois_key *gk;
        if (int rc = ks_find_key(ctx, gal[r], &gk)) return rc;
        // ping-pong: the automorphism reads two positions of the old accumulator per output
        u64 *src = (r & 1) ? s.acc2 : acc, *dst = (r & 1) ? acc : s.acc2;
        if (close_out && r + 1 == cnt) // whichever of the two blocks the rotations so far have left the accumulator in
            return rotate_close(ctx, src, close_out, B, *gk, gal[r], tb, s);
        if (int rc = rotate_accumulate(ctx, src, dst, B, *gk, tb, s)) return rc;
    }
    if (cnt & 1)
        LM_HIP(ctx, hipMemcpyAsync(acc, s.acc2, (size_t)B * 2 * tb->nl * ctx->N * 8, hipMemcpyDeviceToDevice,
                                   ctx->stream));
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

// InnerSum(ct, 1, n) at the level of `in` (checked by the caller), on one lane
int inner_sum_at(lumen_ctx *ctx, const lumen_set *in, uint32_t n, lumen_set **out) {
    LM_CHECK(ctx, n && !(n & (n - 1)) && n <= ctx->N, "InnerSum length %u is not a power of two <= N", n);
    KsRun run;
    if (int rc = ks_run_open(ctx, in->count, in->nl, 1, false, &run)) return rc;
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, in->count, in->nl, &o)) return rc;
    lm_set_guard og(ctx, o);
    if (in->words)
        LM_HIP(ctx, hipMemcpyAsync(o->d, in->d, in->words * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (int rc = ks_run_scratch(ctx, &run)) return rc;
    const size_t ctw = (size_t)2 * in->nl * ctx->N;
    auto batch = [&](uint32_t, uint32_t first, uint32_t B, const KsScratch &s, u64 *) {
        return inner_sum_batch(ctx, o->d + (size_t)first * ctw, B, n, run.tb, s);
    };
    if (int rc = ks_run(ctx, run, in->count, ctw, batch)) return rc;
    if (int rc = acc_canon(ctx, o->d, o->words, in->nl)) return rc; // the rotations leave [0, 2q)
    *out = og.release();
    return 0;
}

// matrixInnerSumEval at the level of `matrix` (checked by the caller): nl limbs in, min(nl, 2) out
int matrix_inner_sum_at(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt, uint32_t rows, lumen_set **out) {
    LM_CHECK(ctx, rows && !(rows & (rows - 1)) && rows <= ctx->N, "rows=%u is not a power of two <= N", rows);
    KsRun run;
    if (int rc = ks_run_open(ctx, matrix->count, matrix->nl, 2, true, &run)) return rc;
    u64 *ptT = nullptr;
    if (int rc = upload_ptT(ctx, pt, matrix->nl, &ptT)) return rc;
    const uint32_t N = ctx->N, L = matrix->nl;
    const uint32_t target = std::min<uint32_t>(2, L);
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, matrix->count, target, &o)) return rc;
    lm_set_guard og(ctx, o);
    const size_t ctw = (size_t)2 * L * N, octw = (size_t)2 * target * N;
    if (int rc = ks_run_scratch(ctx, &run)) return rc; // run.acc: the group's accumulators
    u64 *work = (u64 *)lm_scratch(ctx, "rescale_work", run.group_bytes);
    u64 *tbuf = (u64 *)lm_scratch(ctx, "rescale_t", (size_t)run.group * 2 * N * 8);
    if (!work || !tbuf) return 1;
    // The last rotation of a batch writes the rescale's coefficient-form input itself, at the batch's place in `work`
    // (LUMEN_KS_CLOSE_FUSED, lm_ks_close.hip): when a rescale follows, there is a rotation (rows > 1) and the chain has
    // the coefficient form's tables.
    bool close = false;
    if (L > target && rows > 1 && ctx->tune.ks_close_fused) {
        const int rc = lm_rescale_coef_ready(ctx);
        if (rc && rc != 2) return rc;
        close = rc == 0;
    }
    auto batch = [&](uint32_t g0, uint32_t first, uint32_t B, const KsScratch &s, u64 *a) {
        if (int rc = launch_mul_plain(ctx, matrix->d + (size_t)(g0 + first) * ctw, a, ptT, (size_t)B * ctw, L, B)) // ligero.go:319
            return rc;
        return inner_sum_batch(ctx, a, B, rows, run.tb, s, close ? work + (size_t)first * ctw : nullptr); // ligero.go:325
    };
    // the rescale of the group needs both lanes.  ligero.go:331-333
    auto end_of_group = [&](uint32_t g0, uint32_t gn) {
        if (close) // the inverse transforms are done
            return lm_rescale_polys_from_coef(ctx, work, L, o->d + (size_t)g0 * octw, target, gn * 2);
        if (L > target) return lm_rescale_polys(ctx, run.acc, L, o->d + (size_t)g0 * octw, target, gn * 2, work, tbuf);
        if (int rc = acc_canon(ctx, run.acc, (size_t)gn * ctw, L)) return rc; // no rescale to absorb the lazy range
        LM_HIP(ctx, hipMemcpyAsync(o->d + (size_t)g0 * octw, run.acc, (size_t)gn * ctw * 8, hipMemcpyDeviceToDevice, ctx->stream));
        return 0;
    };
    if (int rc = ks_run(ctx, run, matrix->count, ctw, batch, end_of_group)) return rc;
    *out = og.release();
    return 0;
}

// ---- InnerSum(ct, batch, n) for any n: the lazy double-and-add of [LATTIGO-RECALL] Evaluator.InnerSum
// (rlwe/inner_sum.go).  cur = ct, and for i = 0, 1, ..., j = n >> i while j > 0:
//     j odd, j > 1:  lazy (+)= sigma_{5^k}(gadget(cur.c1) + (P cur.c0, 0)),  k = (n - (n & (2^(i+1) - 1))) batch    -- over Q and P
//     j == 1:        out = (no lazy term: n a power of two) ? cur : ModDown(lazy) + cur;  stop
//     cur = cur + Rot_{2^i batch}(cur)                                                          -- the existing rotation
// The lazy accumulator takes ONE ModDown, over the sum of popcount(n) - 1 terms; the terms and the doubling of an
// iteration share one decomposition of cur.c1.

bool is_pow2(uint32_t n) { return n && !(n & (n - 1)); }

// the elements in order of first use, without duplicates or the identity; 0 for what general_check refuses
uint32_t general_elements(const lumen_ctx *ctx, uint32_t batch, uint32_t n, uint64_t *gal) {
    if (batch == 1 && is_pow2(n) && n <= ctx->N) return lumen_inner_sum_galois_elements(ctx, n, gal);
    if (!batch || !n || (uint64_t)batch * n > ctx->N / 2) return 0;
    uint32_t cnt = 0;
    auto add = [&](uint64_t k) {
        const uint64_t g = lumen_galois_element(ctx, (int64_t)k);
        if (g == 1 || std::find(gal, gal + cnt, g) != gal + cnt) return;
        gal[cnt++] = g;
    };
    for (uint32_t i = 0, j = n; j > 1; i++, j >>= 1) { // at most 2 log2(n) <= 32 elements
        if (j & 1) add((uint64_t)(n - (n & ((2u << i) - 1))) * batch);
        add((uint64_t)batch << i);
    }
    return cnt;
}

int general_check(lumen_ctx *ctx, uint32_t batch, uint32_t n, const char *what) {
    LM_CHECK(ctx, batch >= 1 && n >= 1, "%s: batch size %u and length %u must both be at least 1", what, batch, n);
    LM_CHECK(ctx, ctx->K >= 1, "parameters have no special primes: key switching unavailable");
    LM_CHECK(ctx, ctx->K <= 2, "key switching supports 1 or 2 special primes (have %u)", ctx->K);
    if (batch == 1 && is_pow2(n) && n <= ctx->N) return 0;
    LM_CHECK(ctx, (uint64_t)batch * n <= ctx->N / 2, "%s: batch size %u x length %u spans beyond the slot row of %u slots", what, batch, n,
             ctx->N / 2);
    return 0;
}

struct GeneralKeys {
    std::map<uint64_t, const lm_galois_key *> by_el;
    int find(lumen_ctx *ctx, uint32_t batch, uint32_t n) { // every refusal for a missing key comes before any work
        uint64_t gal[64];
        const uint32_t cnt = general_elements(ctx, batch, n, gal);
        for (uint32_t r = 0; r < cnt; r++)
            if (int rc = ks_find_key(ctx, gal[r], &by_el[gal[r]])) return rc;
        return 0;
    }
    const lm_galois_key &rot(const lumen_ctx *ctx, uint64_t k) const { return *by_el.at(lumen_galois_element(ctx, (int64_t)k)); }
};

// one more block per lane, of the gadget product's size at the top level: the lazy accumulator
int general_lazy_blocks(lumen_ctx *ctx, const KsRun &run, u64 **lazy) {
    const size_t bytes = (size_t)run.Bmax * 2 * (ctx->L + ctx->K) * ctx->N * 8;
    lazy[0] = (u64 *)lm_scratch(ctx, "ks_lazy", bytes);
    lazy[1] = run.lanes > 1 ? (u64 *)lm_scratch(ctx, "ks_lazy_b", bytes) : lazy[0];
    return lazy[0] && lazy[1] ? 0 : 1;
}

// InnerSum(., batch, n) of the B columns of acc, in place and canonical; n is no power of two, or batch > 1
int inner_sum_general_batch(lumen_ctx *ctx, u64 *acc, uint32_t B, uint32_t batch, uint32_t n, const GeneralKeys &keys, KsTables *tb,
                            const KsScratch &s, u64 *lazy) {
    u64 *cur = acc, *other = s.acc2; // ping-pong, as inner_sum_batch
    bool have_lazy = false;
    for (uint32_t i = 0, j = n; j > 0; i++, j >>= 1) {
        if (j == 1) { // the last iteration decomposes nothing
            if (!have_lazy) {
                if (int rc = acc_canon(ctx, cur, (size_t)B * 2 * tb->nl * ctx->N, tb->nl)) return rc;
            } else {
                if (int rc = lazy_close(ctx, cur, other, lazy, B, tb, s)) return rc;
                std::swap(cur, other);
            }
            break;
        }
        if (int rc = rotate_decompose(ctx, cur, B, tb, s)) return rc; // once per iteration: s.ext survives the lazy term
        if (j & 1) {
            const lm_galois_key &gk = keys.rot(ctx, (uint64_t)(n - (n & ((2u << i) - 1))) * batch);
            if (int rc = rotate_mac(ctx, cur, B, gk, tb, s)) return rc;
            if (int rc = rotate_lazy_term(ctx, cur, lazy, B, gk, !have_lazy, tb, s)) return rc;
            have_lazy = true;
        }
        if (int rc = rotate_add(ctx, cur, other, B, keys.rot(ctx, (uint64_t)batch << i), tb, s)) return rc;
        std::swap(cur, other);
    }
    if (cur != acc)
        LM_HIP(ctx, hipMemcpyAsync(acc, cur, (size_t)B * 2 * tb->nl * ctx->N * 8, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

int inner_sum_general_at(lumen_ctx *ctx, const lumen_set *in, uint32_t batch, uint32_t n, lumen_set **out) {
    if (int rc = general_check(ctx, batch, n, "lumen_inner_sum_general")) return rc;
    if (batch == 1 && is_pow2(n)) return inner_sum_at(ctx, in, n, out); // its words exactly, the row swap at n == N included
    KsRun run;
    if (int rc = ks_run_open(ctx, in->count, in->nl, 2, false, &run)) return rc;
    GeneralKeys keys;
    if (int rc = keys.find(ctx, batch, n)) return rc;
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, in->count, in->nl, &o)) return rc;
    lm_set_guard og(ctx, o);
    if (in->words)
        LM_HIP(ctx, hipMemcpyAsync(o->d, in->d, in->words * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (int rc = ks_run_scratch(ctx, &run)) return rc;
    u64 *lazy[2];
    if (int rc = general_lazy_blocks(ctx, run, lazy)) return rc;
    const size_t ctw = (size_t)2 * in->nl * ctx->N;
    auto batch_fn = [&](uint32_t, uint32_t first, uint32_t B, const KsScratch &s, u64 *) {
        return inner_sum_general_batch(ctx, o->d + (size_t)first * ctw, B, batch, n, keys, run.tb, s, lazy[&s == &run.s[1]]);
    };
    if (int rc = ks_run(ctx, run, in->count, ctw, batch_fn)) return rc;
    *out = og.release();
    return 0;
}

// matrixInnerSumEval for rows of any length: MulNew, the batch above in the group's accumulator, the group's rescale.
// A length that is no power of two ends in the close, not in a rotation: the unfused rescale takes its canonical words.
int matrix_inner_sum_general_at(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt, uint32_t rows, lumen_set **out) {
    if (int rc = general_check(ctx, 1, rows, "lumen_matrix_inner_sum_general")) return rc;
    if (is_pow2(rows)) return matrix_inner_sum_at(ctx, matrix, pt, rows, out);
    KsRun run;
    if (int rc = ks_run_open(ctx, matrix->count, matrix->nl, 2, true, &run)) return rc;
    GeneralKeys keys;
    if (int rc = keys.find(ctx, 1, rows)) return rc;
    u64 *ptT = nullptr;
    if (int rc = upload_ptT(ctx, pt, matrix->nl, &ptT)) return rc;
    const uint32_t N = ctx->N, L = matrix->nl, target = std::min<uint32_t>(2, L);
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, matrix->count, target, &o)) return rc;
    lm_set_guard og(ctx, o);
    const size_t ctw = (size_t)2 * L * N, octw = (size_t)2 * target * N;
    if (int rc = ks_run_scratch(ctx, &run)) return rc;
    u64 *lazy[2];
    if (int rc = general_lazy_blocks(ctx, run, lazy)) return rc;
    u64 *work = (u64 *)lm_scratch(ctx, "rescale_work", run.group_bytes);
    u64 *tbuf = (u64 *)lm_scratch(ctx, "rescale_t", (size_t)run.group * 2 * N * 8);
    if (!work || !tbuf) return 1;
    auto batch_fn = [&](uint32_t g0, uint32_t first, uint32_t B, const KsScratch &s, u64 *a) {
        if (int rc = launch_mul_plain(ctx, matrix->d + (size_t)(g0 + first) * ctw, a, ptT, (size_t)B * ctw, L, B)) return rc;
        return inner_sum_general_batch(ctx, a, B, 1, rows, keys, run.tb, s, lazy[&s == &run.s[1]]);
    };
    auto end_of_group = [&](uint32_t g0, uint32_t gn) {
        if (L > target) return lm_rescale_polys(ctx, run.acc, L, o->d + (size_t)g0 * octw, target, gn * 2, work, tbuf);
        LM_HIP(ctx, hipMemcpyAsync(o->d + (size_t)g0 * octw, run.acc, (size_t)gn * ctw * 8, hipMemcpyDeviceToDevice, ctx->stream));
        return 0; // the close left canonical words
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
    return inner_sum_general_at(ctx, in, batch_size, n, out);
}

extern "C" int lumen_matrix_inner_sum_general(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt, uint32_t rows,
                                              lumen_set **out) {
    LM_CHECK(nullptr, ctx && matrix && pt && out, "lumen_matrix_inner_sum_general: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_level_of_chain(ctx, matrix, "matrixInnerSumEval")) return rc;
    return matrix_inner_sum_general_at(ctx, matrix, pt, rows, out);
}

extern "C" uint32_t lumen_inner_sum_general_elements(const lumen_ctx *ctx, uint32_t batch_size, uint32_t n, uint64_t *gal_els) {
    if (!ctx || !gal_els) return 0;
    return general_elements(ctx, batch_size, n, gal_els);
}

extern "C" int lumen_inner_sum(lumen_ctx *ctx, const lumen_set *in, uint32_t n, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && out, "lumen_inner_sum: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_inner_sum_level(ctx, in, "InnerSum")) return rc;
    return inner_sum_at(ctx, in, n, out);
}

extern "C" int lumen_inner_sum_at_level(lumen_ctx *ctx, const lumen_set *in, uint32_t n, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && out, "lumen_inner_sum_at_level: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_level_of_chain(ctx, in, "InnerSum")) return rc;
    return inner_sum_at(ctx, in, n, out);
}

extern "C" int lumen_matrix_inner_sum(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt,
                                      uint32_t rows, lumen_set **out) {
    LM_CHECK(nullptr, ctx && matrix && pt && out, "lumen_matrix_inner_sum: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_inner_sum_level(ctx, matrix, "matrixInnerSumEval")) return rc;
    return matrix_inner_sum_at(ctx, matrix, pt, rows, out);
}

extern "C" int lumen_matrix_inner_sum_at_level(lumen_ctx *ctx, const lumen_set *matrix, const uint64_t *pt,
                                               uint32_t rows, lumen_set **out) {
    LM_CHECK(nullptr, ctx && matrix && pt && out, "lumen_matrix_inner_sum_at_level: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_level_of_chain(ctx, matrix, "matrixInnerSumEval")) return rc;
    return matrix_inner_sum_at(ctx, matrix, pt, rows, out);
}
