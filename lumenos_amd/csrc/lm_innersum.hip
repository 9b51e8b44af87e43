// InnerSum and matrixInnerSumEval (fhe/ligero.go:299-370): per input column
//     MulNew(ct, pt) -> InnerSum(., 1, rows) -> Rescale to level 1
// batched over columns.  InnerSum is log2(rows) rounds of
//     acc += Rot(acc)       (hoisted key-switch + NTT-domain automorphism)
// each of them one rotate_accumulate (lm_keyswitch.hip) on a batch of columns; the last one before a rescale is a
// rotate_close (lm_ks_close.hip).  Batches, lanes, groups and scratch are the batch driver's (lm_ks_batch.hip).
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

} // namespace

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
