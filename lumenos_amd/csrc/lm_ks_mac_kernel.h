// The gadget product's kernel, TEXTUALLY included twice by lm_keyswitch.hip (no include guard): with LM_KS_MAC_FOLD 0 it
// defines k_ks_mac, with 1 k_ks_mac_fold, the same product with the c0 fold of matrixInnerSumEval's doublings in its
// epilogue.  Two kernels out of one text, and not a template over a shared body: k_ks_mac then is, to the instruction,
// the kernel it was before the fold existed (tools/kernel_asm_diff.py), whoever calls it.
#if LM_KS_MAC_FOLD
// acc_out: the other block of the accumulator's ping-pong; index, inv_index: the rotation's gather tables
__global__ __launch_bounds__(256) void k_ks_mac_fold(const u64 *__restrict__ ext, const u64 *__restrict__ ext1, uint32_t Bh,
                                                     const u64 *__restrict__ acc,
                                                     const u64 *__restrict__ key, u64 *__restrict__ u, uint32_t B,
                                                     uint32_t L, uint32_t K, uint32_t beta, uint32_t pshift,
                                                     uint32_t key_beta, uint32_t logN, lm_mods mods,
                                                     u64 *__restrict__ acc_out, const uint32_t *__restrict__ index,
                                                     const uint32_t *__restrict__ inv_index) {
#else
__global__ __launch_bounds__(256) void k_ks_mac(const u64 *__restrict__ ext, const u64 *__restrict__ ext1, uint32_t Bh,
                                                const u64 *__restrict__ acc,
                                                const u64 *__restrict__ key, u64 *__restrict__ u, uint32_t B,
                                                uint32_t L, uint32_t K, uint32_t beta, uint32_t pshift,
                                                uint32_t key_beta, uint32_t logN, lm_mods mods) {
#endif
    typedef mac_vec<LM_MAC_VEC> vec;
    const uint32_t N = 1u << logN, LK = L + K;
    // 1-D grid, XCD-aware: workgroup k runs on XCD k % 8 (round-robin dispatch) and each XCD has its own
    // L2, so the G column groups that share one slice of the key are dealt to the SAME XCD back to
    // back -- the slice is fetched into that L2 once instead of once per column group.
    const uint32_t G = (B + LM_MAC_COLS - 1) / LM_MAC_COLS, per_limb = N / (256 * LM_MAC_VEC) ? N / (256 * LM_MAC_VEC) : 1;
    const uint32_t slices = per_limb * LK;
    uint32_t slice, z;
    if (slices % 8 == 0) {
        const uint32_t xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        z = j % G;
        slice = (j / G) * 8 + xcd;
    } else {
        z = blockIdx.x % G;
        slice = blockIdx.x / G;
    }
    const uint32_t i = ((slice % per_limb) * 256 + threadIdx.x) * LM_MAC_VEC; // first coefficient
    // limbs in descending order: the extension kernel wrote the highest target group last, so those
    // digits are the likeliest to still sit in the Infinity Cache
    // (walking the Q limbs first and the limbs modulo P last, so that what the next three kernels read is what was written
    // last -- with the extension kernel writing its P-limb targets first -- was measured: this kernel -2 %, the extension
    // kernel +1.2 %, the step +0.3 %: profiles/r06_exp_ks_p_last_interleaved.txt)
    const uint32_t t = LK - 1 - slice / per_limb;                             // target position
    const uint32_t mt = ks_mod_at(t, L, pshift);                              // its modulus and key limb
    const uint32_t b0 = z * LM_MAC_COLS;
    if (i >= N) return;
    const mod_t md = mods.m[mt];
    const uint32_t own = t < L ? t / K : 0xFFFFFFFFu; // digit whose limbs include t: its "extension" is c1 itself
    mac_acc a0[LM_MAC_COLS][LM_MAC_VEC], a1[LM_MAC_COLS][LM_MAC_VEC];
#pragma unroll
    for (int c = 0; c < LM_MAC_COLS; c++)
#pragma unroll
        for (int e = 0; e < LM_MAC_VEC; e++) a0[c][e].clear(), a1[c][e].clear();
    // columns past the end of the batch re-read the last one (never stored): all loads of a digit are
    // then unconditional and issued together, one digit ahead of the multiply-adds that consume them
    struct digit_t {
        vec k0, k1, x[LM_MAC_COLS];
    };
    auto fetch = [&](uint32_t d) {
        digit_t g;
        g.k0 = vec::load(key + ks_key_at(d, 0, mt, key_beta) * N + i);
        g.k1 = vec::load(key + ks_key_at(d, 1, mt, key_beta) * N + i);
#pragma unroll
        for (int c = 0; c < LM_MAC_COLS; c++) {
            const uint32_t bc = b0 + c < B ? b0 + c : B - 1;
            // the extended digits sit in blocks of Bh columns (a pair of batches, lm_ks_pair.h: two; a single batch has Bh == B):
            // column bc is local column bc % Bh of block bc / Bh -- workgroup-uniform, as bc is
            const u64 *xb = bc < Bh ? ext : ext1;
            g.x[c] = d == own ? vec::load(acc + ((size_t)(bc * 2 + 1) * L + t) * N + i)
                              : vec::load_once(xb + ks_ext_at(bc < Bh ? bc : bc - Bh, d, t, Bh, beta) * N + i);
        }
        return g;
    };
    // software pipeline over the digits: the loads of digit d + PF are issued before the multiply-adds of digit d
    // (the ring of PF + 1 register sets is indexed statically: the loop advances by whole turns of it)
    constexpr int PF = LM_MAC_PREFETCH;
    digit_t q[PF + 1];
#pragma unroll
    for (int j = 0; j < PF; j++)
        if ((uint32_t)j < beta) q[j] = fetch(j);
    for (uint32_t d0 = 0; d0 < beta; d0 += PF + 1) {
#pragma unroll
        for (int j = 0; j <= PF; j++) {
            const uint32_t d = d0 + j;
            if (d < beta) { // wave-uniform
                if (d + PF < beta) q[(j + PF) % (PF + 1)] = fetch(d + PF);
#pragma unroll
                for (int c = 0; c < LM_MAC_COLS; c++)
#pragma unroll
                    for (int e = 0; e < LM_MAC_VEC; e++) mac2(a0[c][e], a1[c][e], q[j].x[c].v[e], q[j].k0.v[e], q[j].k1.v[e]);
            }
        }
    }
#if LM_KS_MAC_FOLD
    u64 u0[LM_MAC_COLS]; // polynomial 0's word, for the fold below
#endif
#pragma unroll
    for (int c = 0; c < LM_MAC_COLS; c++) {
        if (b0 + c < B) {
            u64 *o = u + ks_u_at((b0 + c) * 2, t, B, L, K) * N + i, *o1 = u + ks_u_at((b0 + c) * 2 + 1, t, B, L, K) * N + i;
            vec r0, r1;
#pragma unroll
            for (int e = 0; e < LM_MAC_VEC; e++) {
                u64 lo, hi;
                a0[c][e].value(lo, hi);
                r0.v[e] = lm_mont_reduce_wide(lo, hi, md.q, md.qneg, md.qinv64, beta);
                a1[c][e].value(lo, hi);
                r1.v[e] = lm_mont_reduce_wide(lo, hi, md.q, md.qneg, md.qinv64, beta);
            }
#if LM_KS_MAC_FOLD
            if (t >= L) r0.store(o); // a Q limb of polynomial 0 goes into the fold below, not to u
            u0[c] = r0.v[0];
#else
            r0.store(o);
#endif
            r1.store(o1);
        }
    }
#if LM_KS_MAC_FOLD
    // The c0 fold.  Nothing reads polynomial 0 of a doubling's sum before the closing inverse transform, so its ModDown
    // is not run per rotation: with c0 = A - P^-1 NTT(S) (S: one signed integer per coefficient, k_lift_fold) the
    // rotation is A_out = A + sigma_ntt(A + u0') on the Q limbs, and u0' is in this kernel's registers.  The workgroup
    // owns the aligned block of 256 positions [i0, i0 + 256) of limb t for its columns, and the automorphism permutes
    // aligned blocks onto blocks (moddown_body: the top bits of index[j] are a function of the top bits of j): it parks
    // x[i] = A[i] + u0'[i] (A lazy < 2q, u0' < q: < 3q) in LDS and writes the one output block that gathers from it,
    // jb = inv_index[i0] >> 8: A_out[j] = A[j] + x[index[j] & 255] < 5q, back under 2q with two conditional
    // subtractions (the lazy range of k_moddown_ntt's accumulator).  The limbs modulo P and polynomial 1 went to u above.
    {
        static_assert(LM_MAC_VEC == 1, "the fold parks one coefficient per thread");
        __shared__ u64 park[LM_MAC_COLS][256];
        if (t < L) { // workgroup-uniform
            const uint32_t i0 = i - threadIdx.x;
            const uint32_t j = (inv_index[i0] & ~255u) + threadIdx.x;
            const uint32_t src = index[j] & 255u;
            u64 aj[LM_MAC_COLS];
#pragma unroll
            for (int c = 0; c < LM_MAC_COLS; c++)
                if (b0 + c < B) {
                    const u64 *a = acc + ((size_t)(b0 + c) * 2 * L + t) * N;
                    park[c][threadIdx.x] = a[i] + u0[c];
                    aj[c] = a[j];
                }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < LM_MAC_COLS; c++)
                if (b0 + c < B)
                    acc_out[((size_t)(b0 + c) * 2 * L + t) * N + j] = lm_csub(lm_csub(aj[c] + park[c][src], 4 * md.q), 2 * md.q);
        }
    }
#endif
}
