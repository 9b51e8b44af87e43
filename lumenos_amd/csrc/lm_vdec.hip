// The front end of the proof of decryption (cmd/client/main.go:203-208, Proof.ProveDecrypt -> vdec.ProveBfvDecBatched,
// vdec/prover.go:50-98): everything that function does before its cgo call into lazer is BGV arithmetic on the client's
// own ciphertexts.
//     BatchCiphertexts (vdec/batching.go:9-41)   out = sum_j ct_j * pt(alpha_j)          lumen_batch_ciphertexts
//     witness generation (prover.go:104-119)     centred coefficients of sk, ct0, ct1,   lumen_vdec_witness
//                                                the scaled message and the error
// BatchColumns (batching.go:43-64) and the transcript are host work (lumenos_amd/host/fhe.cpp); lazer itself is out of
// scope: this file ends at the arguments of ProveVdecLnpTbox.
//
// THE BATCH.  lo_mul_plain(ct, lo_encode(v)) multiplies ct by NTT_l(m * T^-1) * T = NTT_l(m mod q_l), m the coefficient
// vector modulo T of the slot values v (lm_encode_coeffs): Encode's T^-1 and MulNew's T cancel and appear nowhere.  So
//     out[w][l] = sum_j ct_j[w][l] (.) NTT_l(m_j mod q_l),     m_j = INTT_T(scatter(alpha_j * pt_scale mod T))
// One kernel, k_batch_mac: a workgroup owns a Q limb and a chunk of the columns, transforms m_j for each column of its
// chunk and multiplies both ciphertext halves into its partial sum in the store of the transform.  The loader lifts
// m mod q_l times 2^64 (one Shoup constant per limb: the transform is linear, the Montgomery factor rides through it), so
// the store forms each product with one 64 x 64 multiplication and one Montgomery reduction.  k_batch_sum adds the
// chunks' partial sums.  Modular sums are exact: the residues do not depend on the chunk count.
//
// THE BUDGET (include/lumenos_hip.h).  A full-size plaintext costs about N * T in noise: the batch only decrypts where
// T * count * N * T * (B + 1) < Q_level / 2.  The library computes what it is asked to compute; tools/noise_budget.py
// --vdec says whether a shape fits, and fhe::Proof::ProveDecrypt checks the decryption relation on the device.
//
// RECORDED DEVIATION.  prover.go:119 passes isNTT = false for a plaintext that IS in the NTT domain: it hands lazer limb
// 0's NTT-domain words of the scaled message as if they were coefficients.  That is not reproduced: m_delta here is the
// coefficient-domain polynomial m * T^-1 mod q_0, consistent with c0 and c1, so that c0 + c1 * s - m_delta = err holds.
#include <cstring>

#include "lm_enc_host.h"

struct batch_r64_t {
    tw_t t[LM_MAX_LIMBS]; // 2^64 mod q_l, Shoup form
};

// Storer of one column: v (.) c0 and v (.) c1 into the two halves of the partial sum, canonical.  pre() requests the run
// of c0 before the run's butterflies (and, being there, keeps the last pass to ONE twiddle set: lm_fwd_last); c1 and
// the partial sum follow pair by pair, so that two words of each are live per step.
template <int RUN> // coefficients per run of the last pass (lm_fwd_run)
struct batch_storer {
    const u64 *a0, *a1;
    u64 *p0, *p1;
    const lm_qc &qc;
    u64 qneg;
    bool first; // the chunk's first column writes the partial sum without reading it
    u64 x0[8];
    __device__ __forceinline__ void pre(uint32_t i0) { lm_load_run(a0, i0, x0, RUN); }
    __device__ __forceinline__ void mac(u64 w0, u64 w1, u64 y0, u64 y1, u64 *p) const {
        ulonglong2 s;
        u64 lo, hi;
        mul128(w0, y0, lo, hi);
        s.x = lm_mont_reduce(lo, hi, qc.q, qneg);
        mul128(w1, y1, lo, hi);
        s.y = lm_mont_reduce(lo, hi, qc.q, qneg);
        if (!first) {
            const ulonglong2 t = *reinterpret_cast<const ulonglong2 *>(p);
            s.x = lm_csub(s.x + t.x, qc.q), s.y = lm_csub(s.y + t.y, qc.q);
        }
        *reinterpret_cast<ulonglong2 *>(p) = s;
    }
    __device__ __forceinline__ void operator()(uint32_t i0, const u64 *v, int n) {
#pragma unroll
        for (int k = 0; k < 8; k += 2)
            if (k < n) {
                const u64 w0 = lm_reduce_s(v[k], qc.q, qc.nq, qc.qinv64), w1 = lm_reduce_s(v[k + 1], qc.q, qc.nq, qc.qinv64);
                const ulonglong2 y = *reinterpret_cast<const ulonglong2 *>(a1 + i0 + k);
                mac(w0, w1, x0[k], x0[k + 1], p0 + i0 + k);
                mac(w0, w1, y.x, y.y, p1 + i0 + k);
            }
    }
};

// mcoef [count][N] coefficients modulo T; ct [count][2][nl][N]; partial [chunks][2][nl][N].  Workgroup (l, c) -- dealt
// limb-major like k_enc_sk: one twiddle table stays hot per XCD -- owns columns [c * count / chunks, (c + 1) * count /
// chunks).  The dealing of the last pass does not depend on the column: a lane meets the same runs for every column, so
// the words of the partial sum it updates are its own and the read-modify-write needs neither barrier nor atomics.
template <int LOGN>
__global__ LM_GEOM_BOUNDS(lm_geom_lds(LOGN)) void k_batch_mac(const u64 *__restrict__ mcoef, batch_r64_t r64,
                                                               const u64 *__restrict__ ct, u64 *__restrict__ partial,
                                                               uint32_t count, uint32_t nl, uint32_t chunks, lm_mods mods,
                                                               const tw_t *__restrict__ tw_all) {
    extern __shared__ __attribute__((aligned(16))) u64 sm[];
    constexpr uint32_t N = 1u << LOGN;
    const uint32_t tid = threadIdx.x;
    const uint32_t l = blockIdx.x / chunks, c = blockIdx.x % chunks;
    const lm_qc qc = lm_make_qc(mods.m[l]);
    const u64 qneg = mods.m[l].qneg;
    const uint32_t j0 = (uint32_t)((uint64_t)c * count / chunks), j1 = (uint32_t)((uint64_t)(c + 1) * count / chunks);
    u64 *p0 = partial + (((size_t)c * 2) * nl + l) * N, *p1 = p0 + (size_t)nl * N;
    if (j0 == j1) { // an empty chunk (more chunks than columns)
        for (uint32_t i = tid; i < N; i += blockDim.x) p0[i] = 0, p1[i] = 0;
        return;
    }
    const tw_t rr = r64.t[l];
    for (uint32_t j = j0; j < j1; j++) {
        const u64 *mc = mcoef + (size_t)j * N;
        const u64 *a0 = ct + ((size_t)j * 2 * nl + l) * N, *a1 = a0 + (size_t)nl * N;
        const bool first = j == j0;
        auto ld = [&](uint32_t i) { return lm_shoup3<true>(mc[i], rr.w, rr.wp, qc.nq); }; // m * 2^64 mod q_l, in [0, 3q)
        batch_storer<lm_fwd_run<LOGN>()> st{a0, a1, p0, p1, qc, qneg, first};
        // the generic passes also at N = 2^14, as k_enc_sk: the second twiddle set of the register form does not fit
        // next to the runs of ciphertext words and of the partial sum (scratch otherwise, which the build refuses)
        lm_ntt_forward<LOGN, false>(sm, tw_all + (size_t)l * N, qc, tid, ld, st);
        __syncthreads(); // the next column's first pass overwrites what other waves' last pass is still reading
    }
}

// out[w][l][k] = sum_c partial[c][w][l][k] mod q_l, canonical; total = 2 * nl * N
__global__ void k_batch_sum(const u64 *__restrict__ partial, u64 *__restrict__ out, uint32_t chunks, uint32_t nl, uint32_t logN,
                            size_t total, lm_mods mods) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const u64 q = mods.m[(g >> logN) % nl].q;
    u64 acc = partial[g];
    for (uint32_t c = 1; c < chunks; c++) acc = lm_addmod(acc, partial[(size_t)c * total + g], q);
    out[g] = acc;
}

template <int LOGN>
static int batch_mac_t(lumen_ctx *ctx, const u64 *mcoef, const batch_r64_t &r64, const u64 *ct, u64 *partial, uint32_t count,
                       uint32_t nl, uint32_t chunks) {
    lm_prof_scope ps(ctx, "batch_mac_ntt", (uint64_t)count * nl);
    return lm_launch(ctx, k_batch_mac<LOGN>, lm_geom_lds(LOGN), nl * chunks, mcoef, r64, ct, partial, count, nl, chunks, ctx->mods,
                     ctx->sh->tw_fwd.get());
}

// LUMEN_BATCH_CHUNKS, or nl * chunks workgroups at about the CU count
static uint32_t batch_chunks(lumen_ctx *ctx, uint32_t count, uint32_t nl) {
    if (ctx->tune.batch_chunks) return ctx->tune.batch_chunks;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus < 1) cus = 256;
    (void)hipGetLastError();
    return std::min(count, std::max(1u, ((uint32_t)cus + nl / 2) / nl));
}

extern "C" int lumen_batch_ciphertexts(lumen_ctx *ctx, const lumen_set *cts, const uint64_t *alphas, uint32_t rows,
                                       uint64_t pt_scale, lumen_set **out) {
    LM_CHECK(nullptr, ctx, "lumen_batch_ciphertexts: NULL ctx");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_batch_ciphertexts");
    LM_CHECK(ctx, cts && alphas && out, "lumen_batch_ciphertexts: NULL argument");
    LM_CHECK(ctx, cts->count >= 1, "lumen_batch_ciphertexts: empty set (count == 0)");
    LM_CHECK(ctx, rows >= 1 && rows <= ctx->N, "lumen_batch_ciphertexts: rows=%u out of range [1, N]", rows);
    LM_FULL_WIDTH(ctx, cts, "lumen_batch_ciphertexts");
    LM_CHECK(ctx, cts->nl >= 1 && cts->nl <= ctx->L, "lumen_batch_ciphertexts: %u limbs out of range [1, %u]", cts->nl, ctx->L);
    LM_CHECK(ctx, ctx->T < (1ull << 60), "lumen_batch_ciphertexts: plaintext modulus of 2^60 or more");
    const std::shared_ptr<EncoderTables> enc_hold = lm_ext_get<EncoderTables>(ctx, "encoder");
    LM_CHECK(ctx, enc_hold, "lumen_batch_ciphertexts: no encoder tables (lumen_encoder_set)");
    LM_CHECK(ctx, pt_scale % ctx->T != 0, "lumen_batch_ciphertexts: pt_scale is 0 modulo T");
    const uint32_t N = ctx->N, nl = cts->nl, count = cts->count;
    const size_t ctw = (size_t)2 * nl * N;
    const uint32_t chunks = batch_chunks(ctx, count, nl);
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, 1, nl, &o)) return rc;
    lm_set_guard og(ctx, o);
    u64 *dval = (u64 *)lm_scratch(ctx, "batch_val", (size_t)count * rows * sizeof(u64));
    u64 *dm = (u64 *)lm_scratch(ctx, "batch_m", (size_t)count * N * sizeof(u64));
    // one chunk: its partial sum IS the result
    u64 *partial = chunks > 1 ? (u64 *)lm_scratch(ctx, "batch_partial", (size_t)chunks * ctw * sizeof(u64)) : o->d;
    if (!dval || !dm || !partial) return 1;
    if (int rc = lm_encode_coeffs(ctx, enc_hold.get(), alphas, rows, count, dval, dm, pt_scale)) return rc;
    batch_r64_t r64;
    for (uint32_t l = 0; l < LM_MAX_LIMBS; l++) {
        const uint64_t q = ctx->mod[l < nl ? l : 0];
        r64.t[l] = h_tw(h_r64_mod(q), q);
    }
    if (int rc = lm_for_logn(ctx, ctx->logN, [&](auto k) { return batch_mac_t<k>(ctx, dm, r64, cts->d, partial, count, nl, chunks); }))
        return rc;
    if (chunks > 1) {
        lm_prof_scope ps(ctx, "batch_sum", chunks);
        if (int rc = lm_launch_flat(ctx, k_batch_sum, ctw, partial, o->d, chunks, nl, ctx->logN, ctw, ctx->mods)) return rc;
    }
    ctx->mul_counter += count;
    LM_HIP(ctx, hipStreamSynchronize(ctx->stream)); // caller memory (`alphas`)
    *out = og.release();
    return 0;
}

// ---- witness generation on ONE ciphertext of one limb
// limb 0 of the secret as plain residues (the key table holds Shoup pairs: .w is the residue)
__global__ void k_vdec_sk_words(const tw_t *__restrict__ sk, u64 *__restrict__ out, uint32_t n) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) out[g] = sk[g].w;
}
// canonical residues modulo q -> centred: x > q / 2 -> x - q.  sub: subtracted modulo q first (NULL: nothing)
__global__ void k_vdec_centre(const u64 *__restrict__ x, const u64 *__restrict__ sub, int64_t *__restrict__ out, size_t total,
                              u64 q) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const u64 v = sub ? lm_submod(x[g], sub[g], q) : x[g];
    out[g] = v > (q >> 1) ? -(int64_t)(q - v) : (int64_t)v;
}
// the secret's coefficients into int8; *bad counts what is outside {-1, 0, 1}
__global__ void k_vdec_centre_sk(const u64 *__restrict__ x, int8_t *__restrict__ out, uint32_t n, u64 q, uint32_t *__restrict__ bad) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const u64 v = x[g];
    const bool ok = v <= 1 || v == q - 1;
    out[g] = v == q - 1 ? -1 : (int8_t)(v & 1);
    if (!ok) atomicAdd(bad, 1u);
}
// m_delta = m * T^-1 mod q_0 (m: coefficients modulo T, lifted uncentred as Encode does), canonical
__global__ void k_vdec_mdelta(const u64 *__restrict__ m, u64 *__restrict__ out, uint32_t n, tw_t tinv, u64 q) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) out[g] = lm_shoup(m[g], tinv, q);
}

extern "C" int lumen_vdec_witness(lumen_ctx *ctx, const lumen_set *ct, const uint64_t *m, uint32_t rows, uint64_t scale,
                                  int8_t *sk, int64_t *c0, int64_t *c1, int64_t *m_delta, int64_t *err) {
    LM_CHECK(nullptr, ctx, "lumen_vdec_witness: NULL ctx");
    LM_ENTER(ctx);
    LM_REFUSE_SPLIT(ctx, "lumen_vdec_witness");
    LM_CHECK(ctx, ct && m && sk && c0 && c1 && m_delta, "lumen_vdec_witness: NULL argument");
    LM_CHECK(ctx, rows >= 1 && rows <= ctx->N, "lumen_vdec_witness: rows=%u out of range [1, N]", rows);
    LM_FULL_WIDTH(ctx, ct, "lumen_vdec_witness");
    LM_CHECK(ctx, ct->count == 1, "lumen_vdec_witness: a set of %u ciphertexts (the witness is defined on ONE)", ct->count);
    LM_CHECK(ctx, ct->nl == 1, "lumen_vdec_witness: %u limbs (rescale to one limb first: lumen_rescale(., 1))", ct->nl);
    LM_CHECK(ctx, ctx->T < (1ull << 60), "lumen_vdec_witness: plaintext modulus of 2^60 or more");
    const std::shared_ptr<SkTable> sk_hold = lm_ext_get<SkTable>(ctx, "secret_key");
    const std::shared_ptr<EncoderTables> enc_hold = lm_ext_get<EncoderTables>(ctx, "encoder");
    LM_CHECK(ctx, sk_hold, "lumen_vdec_witness: no secret key on the context (lumen_load_secret_key, lumen_keygen_secret)");
    LM_CHECK(ctx, enc_hold, "lumen_vdec_witness: no encoder tables (lumen_encoder_set)");
    LM_CHECK(ctx, scale % ctx->T != 0, "lumen_vdec_witness: scale is 0 modulo T");
    const uint32_t N = ctx->N;
    const uint64_t q0 = ctx->mod[0];
    // the secret's images: zeroed on the stream before the blocks are given back
    lm_dev<u64> d_s;
    lm_dev<int8_t> d_s8;
    if (d_s.release_on(ctx->stream, true).alloc(ctx, N, "the witness's secret")) return 1;
    if (d_s8.release_on(ctx->stream, true).alloc(ctx, N, "the witness's secret")) return 1;
    // u64 [4][N]: c0 | c1 coefficients, m_delta, phase; then int64 [4][N]: c0 | c1 | m_delta | err; then the flag
    unsigned char *blk = (unsigned char *)lm_scratch(ctx, "vdec_wit", (size_t)8 * N * sizeof(u64) + sizeof(uint32_t));
    u64 *dval = (u64 *)lm_scratch(ctx, "vdec_val", (size_t)rows * sizeof(u64));
    u64 *dm = (u64 *)lm_scratch(ctx, "vdec_m", (size_t)N * sizeof(u64));
    if (!blk || !dval || !dm) return 1;
    u64 *coef = (u64 *)blk, *md = coef + 2 * (size_t)N, *phase = md + N;
    int64_t *o64 = (int64_t *)(phase + N);
    uint32_t *bad = (uint32_t *)(o64 + 4 * (size_t)N);
    LM_HIP(ctx, hipMemsetAsync(bad, 0, sizeof(uint32_t), ctx->stream));
    lm_prof_scope ps(ctx, "vdec_witness", 1);
    // c0, c1
    if (int rc = lm_launch_ntt_strided(ctx, ct->d, N, coef, N, 2, lm_map_q(1), true, "vdec_intt")) return rc;
    if (int rc = lm_launch_flat(ctx, k_vdec_centre, (size_t)2 * N, coef, (const u64 *)nullptr, o64, (size_t)2 * N, q0)) return rc;
    // sk
    if (int rc = lm_launch_flat(ctx, k_vdec_sk_words, N, sk_hold->d_sk.get(), d_s.get(), N)) return rc;
    if (int rc = lm_launch_ntt_strided(ctx, d_s.get(), N, d_s.get(), N, 1, lm_map_q(1), true, "vdec_intt")) return rc;
    if (int rc = lm_launch_flat(ctx, k_vdec_centre_sk, N, d_s.get(), d_s8.get(), N, q0, bad)) return rc;
    // m_delta
    if (int rc = lm_encode_coeffs(ctx, enc_hold.get(), m, rows, 1, dval, dm, scale)) return rc;
    if (int rc = lm_launch_flat(ctx, k_vdec_mdelta, N, dm, md, N, enc_hold->tinv.t[0], q0)) return rc;
    if (int rc = lm_launch_flat(ctx, k_vdec_centre, N, md, (const u64 *)nullptr, o64 + 2 * (size_t)N, (size_t)N, q0)) return rc;
    // err = INTT(c0 + c1 * s) - m_delta: the e whose smallness lazer proves
    if (err) {
        if (int rc = lm_decrypt_phase(ctx, ct->d, 1, 1, sk_hold.get(), phase, false)) return rc;
        if (int rc = lm_launch_flat(ctx, k_vdec_centre, N, phase, (const u64 *)md, o64 + 3 * (size_t)N, (size_t)N, q0)) return rc;
    }
    uint32_t hbad = 0;
    if (int rc = lm_d2h(ctx, &hbad, bad, sizeof(hbad), true)) return rc;
    LM_CHECK(ctx, hbad == 0, "lumen_vdec_witness: %u coefficients of the secret key are outside {-1, 0, 1}", hbad);
    if (int rc = lm_d2h(ctx, sk, d_s8.get(), N, false)) return rc;
    if (int rc = lm_d2h(ctx, c0, o64, (size_t)N * 8, false)) return rc;
    if (int rc = lm_d2h(ctx, c1, o64 + N, (size_t)N * 8, false)) return rc;
    if (int rc = lm_d2h(ctx, m_delta, o64 + 2 * (size_t)N, (size_t)N * 8, false)) return rc;
    if (err)
        if (int rc = lm_d2h(ctx, err, o64 + 3 * (size_t)N, (size_t)N * 8, false)) return rc;
    LM_HIP(ctx, hipStreamSynchronize(ctx->stream)); // caller memory (`m`) and every download above
    return 0;
}
