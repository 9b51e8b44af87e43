// The per-column loop of Proof.Verify (fhe/ligero.go:554-567) for a client that owns a GPU: for every opened level-1
// ciphertext of the proof, resident on the device after lumen_ct_deserialize,
//   core.VerifyMerklePath(Ct, path, root, idx)            (core/tree.go:225-268)
//   InnerProduct(Values, r) == Encode(MatR)[idx]
//   InnerProduct(Values, b) == Encode(MatZ)[idx],  b = [1, w, w^2, ...], w = z^cols
// without the decrypted values or the ciphertexts' bytes leaving the device.
//   side stream   k_leaf_sha256 over the opened ciphertexts (the lumen_leaf_digests_begin job), under the decryption
//   main stream   k_decrypt_phase, CRT, transform over Z_T (lm_decrypt_decode: lumen_decrypt's stages) -> t[count][N]
//                 k_poly_pow_table: w^i;  k_verify_prep: r and b times scale^-1, Montgomery form, scattered into the
//                 decoder's output order (zero where a position holds no slot below `rows`)
//                 k_verify_dot: one workgroup per column, one linear pass over t[c][.] with 16-byte loads, both
//                 products from the same loads, summed lazily in 128 bits (8 products per Montgomery reduction)
//                 k_verify_paths (lm_hash.hip, beside sha256_compress) once the digests are there
// Only count * 24 bytes of verdicts come back.
#include <cstring>

#include "lm_enc_host.h"
#include "lm_polyeval_dev.h"

// lm_hash.hip
int lm_verify_paths(lumen_ctx *ctx, const uint8_t *digests, const uint32_t *leaf_index, const uint8_t *paths, uint32_t depth,
                    const uint8_t *root, uint32_t count, uint32_t flag, uint32_t *bad);

// vr[slot[i]] = (r[i] mod T) * scale^-1 * 2^64, vb[slot[i]] = w^i * scale^-1 * 2^64 (mod T) for i < rows; bM[i] = w^i * 2^64,
// sinvM = scale^-1 * 2^64, sinvM2 = scale^-1 * 2^128.  vr / vb are zeroed before.
__global__ __launch_bounds__(256) void k_verify_prep(const u64 *__restrict__ r, const u64 *__restrict__ bM,
                                                     const uint32_t *__restrict__ slot, uint32_t rows, u64 sinvM, u64 sinvM2,
                                                     mod_t m, u64 *__restrict__ vr, u64 *__restrict__ vb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const uint32_t p = slot[i];
    vr[p] = pe_mont_mul(lm_reduce(r[i], m.q, m.qinv64), sinvM2, m);
    vb[p] = pe_mont_mul(bM[i], sinvM, m);
}

// got[c] = {sum_p t[c][p] * vr[p], sum_p t[c][p] * vb[p]} * 2^-64 mod T; bad[c] = flag_r where the first is not want_r[c]
// | flag_b where the second is not want_z[c].  n2 = N / 2 pairs of words per column.
__global__ __launch_bounds__(PE_THREADS) void k_verify_dot(const u64 *__restrict__ t, const u64 *__restrict__ vr,
                                                           const u64 *__restrict__ vb, uint32_t n2,
                                                           const u64 *__restrict__ want_r, const u64 *__restrict__ want_z,
                                                           uint32_t flag_r, uint32_t flag_b, u64 *__restrict__ got,
                                                           uint32_t *__restrict__ bad, mod_t m) {
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    const ulonglong2 *c2 = reinterpret_cast<const ulonglong2 *>(t) + (size_t)c * n2;
    const ulonglong2 *r2 = reinterpret_cast<const ulonglong2 *>(vr);
    const ulonglong2 *b2 = reinterpret_cast<const ulonglong2 *>(vb);
    u64 accr = 0, accb = 0;
    for (uint32_t p0 = tid; p0 < n2; p0 += PE_UNROLL * PE_THREADS) {
        ulonglong2 a[PE_UNROLL], x[PE_UNROLL], y[PE_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < PE_UNROLL; u++) {
            const uint32_t p = p0 + u * PE_THREADS;
            if (p < n2) {
                a[u] = c2[p];
                x[u] = r2[p];
                y[u] = b2[p];
            } else {
                a[u] = x[u] = y[u] = make_ulonglong2(0, 0);
            }
        }
        u128 sr = 0, sb = 0;
#pragma unroll
        for (uint32_t u = 0; u < PE_UNROLL; u++) {
            sr += (u128)a[u].x * x[u].x + (u128)a[u].y * x[u].y;
            sb += (u128)a[u].x * y[u].x + (u128)a[u].y * y[u].y;
        }
        accr = lm_addmod(accr, lm_mont_reduce_wide((u64)sr, (u64)(sr >> 64), m.q, m.qneg, m.qinv64, 2 * PE_UNROLL), m.q);
        accb = lm_addmod(accb, lm_mont_reduce_wide((u64)sb, (u64)(sb >> 64), m.q, m.qneg, m.qinv64, 2 * PE_UNROLL), m.q);
    }
    accr = pe_block_sum(accr, m);
    __syncthreads();
    accb = pe_block_sum(accb, m);
    if (tid == 0) {
        got[2 * (size_t)c] = accr, got[2 * (size_t)c + 1] = accb;
        bad[c] = (accr != want_r[c] ? flag_r : 0u) | (accb != want_z[c] ? flag_b : 0u);
    }
}

extern "C" int lumen_verify_columns(lumen_ctx *ctx, const lumen_set *opened, uint64_t scale, uint32_t rows, const uint64_t *r,
                                    uint64_t w, const uint64_t *want_r, const uint64_t *want_z, const uint32_t *leaf_index,
                                    const uint8_t *paths, uint32_t depth, const uint8_t root[32], uint32_t *status,
                                    uint64_t *got, uint64_t *values) {
    LM_CHECK(nullptr, ctx, "lumen_verify_columns: ctx is NULL");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_verify_columns");
    LM_CHECK(ctx, opened, "lumen_verify_columns: opened is NULL");
    LM_CHECK(ctx, r, "lumen_verify_columns: r is NULL");
    LM_CHECK(ctx, want_r, "lumen_verify_columns: want_r is NULL");
    LM_CHECK(ctx, want_z, "lumen_verify_columns: want_z is NULL");
    LM_CHECK(ctx, leaf_index, "lumen_verify_columns: leaf_index is NULL");
    LM_CHECK(ctx, root, "lumen_verify_columns: root is NULL");
    LM_CHECK(ctx, status, "lumen_verify_columns: status is NULL");
    LM_CHECK(ctx, paths || !depth, "lumen_verify_columns: paths is NULL with depth = %u", depth);
    LM_CHECK(ctx, rows >= 1 && rows <= ctx->N, "lumen_verify_columns: rows=%u out of range [1, N = %u]", rows, ctx->N);
    LM_CHECK(ctx, depth <= 32, "lumen_verify_columns: depth=%u out of range [0, 32]", depth);
    const uint32_t N = ctx->N, count = opened->count;
    const uint64_t T = ctx->T;
    LM_CHECK(ctx, T >= 2, "lumen_verify_columns: the context has no plaintext modulus (T = %llu)", (unsigned long long)T);
    LM_CHECK(ctx, T < PE_MAX_T, "lumen_verify_columns: plaintext modulus T = %llu out of range (below 2^60 for the lazy sums)",
             (unsigned long long)T);
    if (int rc = lm_decrypt_check(ctx, opened, scale, "lumen_verify_columns")) return rc;
    for (uint32_t i = 0; i < count; i++)
        LM_CHECK(ctx, depth == 32 || leaf_index[i] < (1u << depth), "lumen_verify_columns: leaf_index[%u] = %u is not below 2^depth = 2^%u",
                 i, leaf_index[i], depth);
    LM_CHECK(ctx, !ctx->aux_digests, "lumen_verify_columns: a lumen_leaf_digests_begin job is in flight on this context");
    if (!count) return 0;

    // the leaves on the side stream, under everything below
    if (int rc = lumen_leaf_digests_begin(ctx, opened)) return rc;
    auto drop_job = [&](int rc) { // an error below must not leave the job in flight
        void *unused = nullptr;
        const std::string msg = ctx->err;
        lumen_leaf_digests_end_device(ctx, &unused);
        ctx->err = msg;
        return rc;
    };

    // r | want_r | want_z | root | paths | leaf_index in one staged upload
    const size_t path_bytes = (size_t)count * depth * 32;
    const size_t o_wr = (size_t)rows * 8, o_wz = o_wr + (size_t)count * 8, o_root = o_wz + (size_t)count * 8,
                 o_paths = o_root + 32, o_idx = o_paths + path_bytes, in_bytes = o_idx + (size_t)count * 4;
    const size_t o_bad = (size_t)count * 16, out_bytes = o_bad + (size_t)count * 8;
    uint8_t *hin = (uint8_t *)lm_stage(ctx, in_bytes);
    uint8_t *din = (uint8_t *)lm_scratch(ctx, "verify_in", in_bytes);
    uint8_t *dout = (uint8_t *)lm_scratch(ctx, "verify_out", out_bytes);
    u64 *dvec = (u64 *)lm_scratch(ctx, "verify_vec", (size_t)2 * N * 8);
    u64 *dpow = (u64 *)lm_scratch(ctx, "verify_pow", (size_t)rows * 8);
    if (!hin || !din || !dout || !dvec || !dpow) return drop_job(1);
    memcpy(hin, r, (size_t)rows * 8);
    memcpy(hin + o_wr, want_r, (size_t)count * 8);
    memcpy(hin + o_wz, want_z, (size_t)count * 8);
    memcpy(hin + o_root, root, 32);
    if (path_bytes) memcpy(hin + o_paths, paths, path_bytes);
    memcpy(hin + o_idx, leaf_index, (size_t)count * 4);
    auto enqueue = [&]() -> int {
        LM_HIP(ctx, hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, ctx->stream));
        LM_HIP(ctx, hipEventRecord(ctx->ev_stage, ctx->stream));
        lm_decoded dec;
        if (int rc = lm_decrypt_decode(ctx, opened, &dec)) return rc;
        if (values)
            if (int rc = lm_decrypt_slots(ctx, dec, count, scale, rows, values)) return rc;
        const mod_t m = lm_make_mod(T);
        const uint64_t R = h_r64_mod(T), sinv = h_invmod(scale % T, T);
        const uint64_t sinvM = h_mulmod(sinv, R, T), sinvM2 = h_mulmod(sinvM, R, T);
        u64 *vr = dvec, *vb = dvec + N;
        {
            lm_prof_scope ps(ctx, "verify_prep", rows);
            if (int rc = lm_poly_pow_table(ctx, dpow, rows, h_mulmod(w % T, R, T), 0)) return rc;
            LM_HIP(ctx, hipMemsetAsync(dvec, 0, (size_t)2 * N * 8, ctx->stream));
            hipLaunchKernelGGL(k_verify_prep, dim3((rows + 255) / 256), dim3(256), 0, ctx->stream, (const u64 *)din, dpow, dec.slot,
                               rows, sinvM, sinvM2, m, vr, vb);
            LM_HIP(ctx, hipGetLastError());
        }
        {
            lm_prof_scope ps(ctx, "verify_dot", count);
            hipLaunchKernelGGL(k_verify_dot, dim3(count), dim3(PE_THREADS), 0, ctx->stream, dec.t, vr, vb, N / 2,
                               (const u64 *)(din + o_wr), (const u64 *)(din + o_wz), LUMEN_VERIFY_BAD_R, LUMEN_VERIFY_BAD_B,
                               (u64 *)dout, (uint32_t *)(dout + o_bad), m);
            LM_HIP(ctx, hipGetLastError());
        }
        return 0;
    };
    if (int rc = enqueue()) return drop_job(rc);
    void *ddig = nullptr; // waits for the side stream
    if (int rc = lumen_leaf_digests_end_device(ctx, &ddig)) return rc;
    if (int rc = lm_verify_paths(ctx, (const uint8_t *)ddig, (const uint32_t *)(din + o_idx), din + o_paths, depth, din + o_root,
                                 count, LUMEN_VERIFY_BAD_PATH, (uint32_t *)(dout + o_bad) + count))
        return rc;
    std::vector<uint64_t> hout(out_bytes / 8);
    LM_HIP(ctx, hipMemcpyAsync(hout.data(), dout, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    LM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t *bad = (const uint32_t *)(hout.data() + (size_t)count * 2);
    for (uint32_t i = 0; i < count; i++) status[i] = bad[i] | bad[count + i];
    if (got) memcpy(got, hout.data(), (size_t)count * 16);
    return 0;
}
