// The committed polynomial evaluated at the point the client asks for: the server answers
// GET /prove?point=z with the proof AND the claimed value P(z) (cmd/server/main.go:255-258, written to the response
// at :158-171), which the verifier checks as InnerProduct(MatZ, a) == value with a = [1, z, z^2, ...]
// (fhe/ligero.go:569).  P = core.NewDensePolyFromMatrix(matrix): the witness flattened row-major, coefficient
// i*cols + j is M[i][j]; Evaluate is Horner over those coefficients (core/poly.go:13-45).
//
// Over a block of `count` witness columns of `rows` values (host layout [count][rows], what lumen_encrypt_values
// takes) whose first column has global index c0:
//     partial = sum_j z^(c0+j) * sum_i M[i][c0+j] * w^i  (mod T),   w = z^cols
// The w^i table is Prove's vector b (fhe/ligero.go:210-216) and the z^(c0+j) table the per-column factors; both are
// built on the device in Montgomery form (x * 2^64 mod T) and read from L2.  One pass over the values:
//   k_poly_eval_cols  one workgroup per column: 16-byte loads along the column, products summed lazily in 128 bits
//                     (8 per Montgomery reduction), the column's sum times z^(c0+j) -> one word per column
//   k_poly_sum        the words of all columns -> one u64
// A value >= T enters the products as it is: x * w^i and (x mod T) * w^i are the same residue, so the result is
// that of the reduced witness lumen_encrypt_values commits to (lm_encoder.hip, k_scatter_slots).
#include <cstring>

#include "lm_common.h"
#include "lm_polyeval_dev.h"

namespace {
constexpr size_t PE_CHUNK_BYTES = (size_t)128 << 20; // columns staged on the device per launch
} // namespace

// out[i] = base^(e0 + i) * 2^64 mod q for i < n; baseM = base * 2^64 mod q, oneM = 2^64 mod q
__global__ __launch_bounds__(256) void k_poly_pow_table(u64 *__restrict__ out, uint32_t n, u64 baseM, uint64_t e0, u64 oneM,
                                                        mod_t m) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 r = oneM, b = baseM;
    for (uint64_t e = e0 + i; e; e >>= 1) {
        if (e & 1) r = pe_mont_mul(r, b, m);
        b = pe_mont_mul(b, b, m);
    }
    out[i] = r;
}

int lm_poly_pow_table(lumen_ctx *ctx, u64 *out, uint32_t n, uint64_t baseM, uint64_t e0) {
    const uint64_t T = ctx->T;
    hipLaunchKernelGGL(k_poly_pow_table, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, out, n, baseM, e0,
                       h_r64_mod(T), lm_make_mod(T));
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// part[j] = z^(c0+j) * sum_i x[j][i] * w^i mod q; wM / zM: the two tables in Montgomery form.  PAIRS: rows is even, so
// every column starts on a 16-byte boundary and is read two words per load.
template <bool PAIRS>
__global__ __launch_bounds__(PE_THREADS) void k_poly_eval_cols(const u64 *__restrict__ x, const u64 *__restrict__ wM,
                                                               const u64 *__restrict__ zM, u64 *__restrict__ part,
                                                               uint32_t rows, mod_t m) {
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const u64 *col = x + (size_t)j * rows;
    u64 acc = 0;
    if (PAIRS) {
        const uint32_t np = rows >> 1;
        const ulonglong2 *c2 = reinterpret_cast<const ulonglong2 *>(col);
        const ulonglong2 *w2 = reinterpret_cast<const ulonglong2 *>(wM);
        for (uint32_t p0 = tid; p0 < np; p0 += PE_UNROLL * PE_THREADS) {
            ulonglong2 a[PE_UNROLL], b[PE_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < PE_UNROLL; u++) {
                const uint32_t p = p0 + u * PE_THREADS;
                if (p < np) {
                    a[u] = c2[p];
                    b[u] = w2[p];
                } else {
                    a[u] = make_ulonglong2(0, 0);
                    b[u] = make_ulonglong2(0, 0);
                }
            }
            u128 t = 0;
#pragma unroll
            for (uint32_t u = 0; u < PE_UNROLL; u++) t += (u128)a[u].x * b[u].x + (u128)a[u].y * b[u].y;
            acc = lm_addmod(acc, lm_mont_reduce_wide((u64)t, (u64)(t >> 64), m.q, m.qneg, m.qinv64, 2 * PE_UNROLL), m.q);
        }
    } else {
        for (uint32_t i0 = tid; i0 < rows; i0 += 2 * PE_UNROLL * PE_THREADS) {
            u64 a[2 * PE_UNROLL], b[2 * PE_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < 2 * PE_UNROLL; u++) {
                const uint32_t i = i0 + u * PE_THREADS;
                a[u] = i < rows ? col[i] : 0;
                b[u] = i < rows ? wM[i] : 0;
            }
            u128 t = 0;
#pragma unroll
            for (uint32_t u = 0; u < 2 * PE_UNROLL; u++) t += (u128)a[u] * b[u];
            acc = lm_addmod(acc, lm_mont_reduce_wide((u64)t, (u64)(t >> 64), m.q, m.qneg, m.qinv64, 2 * PE_UNROLL), m.q);
        }
    }
    acc = pe_block_sum(acc, m);
    if (tid == 0) part[j] = pe_mont_mul(acc, zM[j], m);
}

// out[0] = sum_j part[j] mod q (one workgroup)
__global__ __launch_bounds__(PE_THREADS) void k_poly_sum(const u64 *__restrict__ part, uint32_t n, u64 *__restrict__ out, mod_t m) {
    u64 acc = 0;
    for (uint32_t i = threadIdx.x; i < n; i += PE_THREADS) acc = lm_addmod(acc, part[i], m.q);
    acc = pe_block_sum(acc, m);
    if (threadIdx.x == 0) out[0] = acc;
}

int lm_poly_eval_check(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count, uint64_t first_column,
                       uint32_t cols, const char *what) {
    LM_CHECK(ctx, values || !count, "%s: values is NULL", what);
    LM_CHECK(ctx, rows >= 1 && rows <= ctx->N, "%s: rows=%u out of range [1, N = %u]", what, rows, ctx->N);
    LM_CHECK(ctx, first_column + count <= cols && first_column <= cols,
             "%s: first_column + count = %llu + %u exceeds cols = %u", what, (unsigned long long)first_column, count, cols);
    LM_CHECK(ctx, ctx->T >= 2, "%s: the context has no plaintext modulus (T = %llu)", what, (unsigned long long)ctx->T);
    LM_CHECK(ctx, ctx->T < PE_MAX_T, "%s: plaintext modulus T = %llu out of range (below 2^60 for the lazy sums)", what,
             (unsigned long long)ctx->T);
    return 0;
}

// Enqueues the evaluation of one block on the context's stream and the copy of its partial into the context's pinned
// staging; lm_poly_eval_finish waits for it.  Page-locked `values` are only enqueued (the caller keeps them alive
// until _finish), pageable ones go through the bounce buffers and have been read when this returns.
int lm_poly_eval_enqueue(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count, uint64_t first_column,
                         uint32_t cols, uint64_t z, const char *what) {
    if (int rc = lm_poly_eval_check(ctx, values, rows, count, first_column, cols, what)) return rc;
    const uint64_t T = ctx->T;
    const mod_t m = lm_make_mod(T);
    u64 *dout = (u64 *)lm_scratch(ctx, "poly_out", 8);
    if (!dout) return 1;
    if (!count) {
        LM_HIP(ctx, hipMemsetAsync(dout, 0, 8, ctx->stream));
    } else {
        const bool pinned = lm_host_is_pinned(values);
        const uint32_t chunk = (uint32_t)std::min<size_t>(count, std::max<size_t>(1, PE_CHUNK_BYTES / ((size_t)rows * 8)));
        u64 *dval = (u64 *)lm_scratch(ctx, "poly_val", (size_t)chunk * rows * 8);
        u64 *dw = (u64 *)lm_scratch(ctx, "poly_w", (size_t)rows * 8);
        u64 *dz = (u64 *)lm_scratch(ctx, "poly_z", (size_t)count * 8);
        u64 *dpart = (u64 *)lm_scratch(ctx, "poly_part", (size_t)count * 8);
        if (!dval || !dw || !dz || !dpart) return 1;
        // Montgomery forms of z, w = z^cols and 1 (host: three scalars; the tables are built on the device)
        const uint64_t R = h_r64_mod(T), zr = z % T;
        const uint64_t zMont = h_mulmod(zr, R, T), wMont = h_mulmod(h_powmod(zr, cols, T), R, T);
        {
            lm_prof_scope ps(ctx, "poly_tables", (uint64_t)rows + count);
            if (int rc = lm_poly_pow_table(ctx, dw, rows, wMont, 0)) return rc;
            if (int rc = lm_poly_pow_table(ctx, dz, count, zMont, first_column)) return rc;
        }
        for (uint32_t c = 0; c < count; c += chunk) {
            const uint32_t n = std::min(chunk, count - c);
            const size_t bytes = (size_t)n * rows * 8;
            // stream order puts the copy into the staging block behind the previous chunk's kernel
            if (pinned) LM_HIP(ctx, hipMemcpyAsync(dval, values + (size_t)c * rows, bytes, hipMemcpyHostToDevice, ctx->stream));
            else if (int rc = lm_h2d(ctx, dval, values + (size_t)c * rows, bytes)) return rc;
            lm_prof_scope ps(ctx, "poly_eval", n);
            if (rows & 1)
                hipLaunchKernelGGL(k_poly_eval_cols<false>, dim3(n), dim3(PE_THREADS), 0, ctx->stream, dval, dw, dz + c, dpart + c,
                                   rows, m);
            else
                hipLaunchKernelGGL(k_poly_eval_cols<true>, dim3(n), dim3(PE_THREADS), 0, ctx->stream, dval, dw, dz + c, dpart + c,
                                   rows, m);
            LM_HIP(ctx, hipGetLastError());
        }
        lm_prof_scope ps(ctx, "poly_sum", count);
        hipLaunchKernelGGL(k_poly_sum, dim3(1), dim3(PE_THREADS), 0, ctx->stream, dpart, count, dout, m);
        LM_HIP(ctx, hipGetLastError());
    }
    u64 *h = (u64 *)lm_stage(ctx, 8);
    if (!h) return 1;
    LM_HIP(ctx, hipMemcpyAsync(h, dout, 8, hipMemcpyDeviceToHost, ctx->stream));
    LM_HIP(ctx, hipEventRecord(ctx->ev_stage, ctx->stream));
    return 0;
}

int lm_poly_eval_finish(lumen_ctx *ctx, uint64_t *partial) {
    LM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    LM_CHECK(ctx, ctx->stage_host, "lm_poly_eval_finish without an evaluation enqueued");
    *partial = *(const u64 *)ctx->stage_host;
    return 0;
}

extern "C" int lumen_poly_eval_columns(lumen_ctx *ctx, const uint64_t *values, uint32_t rows, uint32_t count,
                                       uint64_t first_column, uint32_t cols, uint64_t z, uint64_t *partial) {
    LM_CHECK(nullptr, ctx, "lumen_poly_eval_columns: ctx is NULL");
    LM_CHECK(ctx, partial, "lumen_poly_eval_columns: partial is NULL");
    LM_ENTER(ctx);
    if (int rc = lm_poly_eval_enqueue(ctx, values, rows, count, first_column, cols, z, "lumen_poly_eval_columns")) return rc;
    return lm_poly_eval_finish(ctx, partial);
}
