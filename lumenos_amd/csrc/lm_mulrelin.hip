// Ciphertext x ciphertext product with relinearisation, Evaluator.MulRelinNew(ct, ct) (fhe/bfv.go:34-42 with a
// ciphertext operand): lumen_mul_relin, and the degree-2 triple before the key switch, lumen_mul_tensor.
//     d0 = T a0 b0      d1 = T (a0 b1 + a1 b0)      d2 = T a1 b1          ([LATTIGO-RECALL] bgv tensorStandard)
//     out = (d0 + k0, d1 + k1),  (k0, k1) = the hybrid key switch of d2 under the relinearisation key (s^2 -> s)
// Ciphertexts encrypt m * T^-1 + e, so the product of two carries T^-2 and one factor T brings it back: the factor
// lo_mul_plain gives its plaintext.
// The key switch is the rotation's (lm_keyswitch.hip), not a second one: rotate_accumulate computes
// acc_out = acc + sigma(c0 + k0(c1), k1(c1)) with the source taken from the accumulator's own c1.  With the
// relinearisation key, whose gather tables are the identity (lm_ks_key.hip), and the accumulator (0, d2) it leaves
// (k0, d2 + k1) in the lazy range [0, 2q); the tensor kernel therefore writes (0, d2) as the batch's accumulator and
// (d0, d1 - d2) into the output set, and one closing elementwise pass adds the two and canonicalises (it stands where
// k_acc_canon stands after an InnerSum).  Batching, lanes, per-level tables and the scratch sized and placed for the top
// level are the batch driver's (lm_ks_batch.hip), grouped as matrixInnerSumEval's.
// Sums of products with ONE relinearisation per sum -- Lattigo's MulNew(a_0, b_0), MulThenAdd(a_i, b_i, acc), Relinearize(acc)
// ([LATTIGO-RECALL]) -- are lumen_mul_relin_dot and lumen_mul_tensor_dot, further down: k_tensor_dot forms the summed triple of a
// group's terms in one pass, in the same two shapes, and the key switch and the closing pass above run once per group.
#include "lm_ks_host.h"

// Block order of the two elementwise kernels: LIMB-MAJOR, blockIdx.x = (limb * count + ciphertext) * nblk + k, a block
// on LM_MR_PAIRS consecutive coefficient pairs of one limb of one ciphertext (all of them below N = 2^11).  The limb is
// uniform per block: its modulus and constants are scalar loads out of the kernel arguments and stay in SGPRs.
#define LM_MR_PAIRS 512u // two 16-byte words per thread and stream
__host__ __device__ __forceinline__ uint32_t mr_blocks_per_limb(uint32_t logN) {
    return (1u << (logN - 1)) > LM_MR_PAIRS ? (1u << (logN - 1)) / LM_MR_PAIRS : 1u;
}

// a: [count][2][nl][N]; b: [count][2][nl][N] (bstride = 1) or ONE ciphertext (bstride = 0); canonical words.
// tfac[l] = T * 2^64 mod q_l as a Shoup constant: a0, a1 enter Montgomery form WITH the factor T in one lazy
// multiplication by a constant ([0, 3q)), and every output is one Montgomery reduction of a 128-bit sum of at most two
// 64 x 64 products (< 6 q^2 < 2^122).  Four products per coefficient, not Karatsuba's three: measured, the three-product
// form (tools/exp_mul_tensor_karatsuba.patch) runs in the same time, 9.86 against 9.42 / 9.72 ms for 51.5 GB at the top
// level of the headline shape, 66-68 % of the HBM peak (profiles/EXPERIMENTS.md R12) -- the multiplier does not bound
// the kernel, which moves 7 (RELIN: 8) words per coefficient.
// RELIN = false: out = (d0, d1, d2), [count][3][nl][N].
// RELIN = true:  out = (d0, d1 - d2), [count][2][nl][N], and acc = (0, d2), [count][2][nl][N].
template <bool RELIN>
__global__ __launch_bounds__(256) void k_mul_tensor(const u64 *__restrict__ a, const u64 *__restrict__ b, u64 *__restrict__ out,
                                                    u64 *__restrict__ acc, uint32_t count, uint32_t bstride, uint32_t nl,
                                                    uint32_t logN, lm_mods mods, lm_ninv_t tfac) {
    const size_t N = (size_t)1 << logN;
    const uint32_t npairs = 1u << (logN - 1), nblk = mr_blocks_per_limb(logN);
    const uint32_t k = blockIdx.x % nblk, lc = blockIdx.x / nblk, c = lc % count, limb = lc / count;
    const mod_t md = mods.m[limb];
    const tw_t W = tfac.t[limb];
    const u64 q = md.q, nq = 0 - md.q;
    const u64 *a0p = a + ((size_t)c * 2 * nl + limb) * N, *a1p = a0p + (size_t)nl * N;
    const u64 *b0p = b + ((size_t)c * bstride * 2 * nl + limb) * N, *b1p = b0p + (size_t)nl * N;
    constexpr uint32_t NP = RELIN ? 2 : 3;
    u64 *o0 = out + ((size_t)c * NP * nl + limb) * N;
    ulonglong2 av0[2], av1[2], bv0[2], bv1[2];
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t p = k * LM_MR_PAIRS + threadIdx.x + 256 * u;
        if (p < npairs) {
            av0[u] = *reinterpret_cast<const ulonglong2 *>(a0p + 2 * p);
            av1[u] = *reinterpret_cast<const ulonglong2 *>(a1p + 2 * p);
            bv0[u] = *reinterpret_cast<const ulonglong2 *>(b0p + 2 * p);
            bv1[u] = *reinterpret_cast<const ulonglong2 *>(b1p + 2 * p);
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t p = k * LM_MR_PAIRS + threadIdx.x + 256 * u;
        if (p >= npairs) continue;
        ulonglong2 r0, r1, r2;
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const u64 a0 = lm_shoup3<true>(e ? av0[u].y : av0[u].x, W.w, W.wp, nq); // a0 * T * 2^64, [0, 3q)
            const u64 a1 = lm_shoup3<true>(e ? av1[u].y : av1[u].x, W.w, W.wp, nq);
            const u64 b0 = e ? bv0[u].y : bv0[u].x, b1 = e ? bv1[u].y : bv1[u].x;
            u64 lo, hi, lo2, hi2;
            mul128(a0, b0, lo, hi);
            const u64 d0 = lm_mont_reduce_wide(lo, hi, q, md.qneg, md.qinv64, 3);
            mul128(a1, b1, lo, hi);
            const u64 d2 = lm_mont_reduce_wide(lo, hi, q, md.qneg, md.qinv64, 3);
            mul128(a0, b1, lo, hi);
            mul128(a1, b0, lo2, hi2);
            lo += lo2;
            hi += hi2 + (lo < lo2 ? 1 : 0);
            u64 d1 = lm_mont_reduce_wide(lo, hi, q, md.qneg, md.qinv64, 6);
            if constexpr (RELIN) d1 = lm_submod(d1, d2, q);
            if (e) r0.y = d0, r1.y = d1, r2.y = d2;
            else r0.x = d0, r1.x = d1, r2.x = d2;
        }
        *reinterpret_cast<ulonglong2 *>(o0 + 2 * p) = r0;
        *reinterpret_cast<ulonglong2 *>(o0 + (size_t)nl * N + 2 * p) = r1;
        if constexpr (RELIN) {
            u64 *c0 = acc + ((size_t)c * 2 * nl + limb) * N;
            ulonglong2 z;
            z.x = z.y = 0;
            *reinterpret_cast<ulonglong2 *>(c0 + 2 * p) = z;
            *reinterpret_cast<ulonglong2 *>(c0 + (size_t)nl * N + 2 * p) = r2;
        } else {
            *reinterpret_cast<ulonglong2 *>(o0 + (size_t)2 * nl * N + 2 * p) = r2;
        }
    }
}

// out (canonical: (d0, d1 - d2)) += ks (the rotation's lazy accumulator, [0, 2q): (k0, d2 + k1)), canonical.
// Both [count][2][nl][N]; the tensor kernel's block order.
__global__ __launch_bounds__(256) void k_relin_close(u64 *__restrict__ out, const u64 *__restrict__ ks, uint32_t count, uint32_t nl,
                                                     uint32_t logN, lm_mods mods) {
    const size_t N = (size_t)1 << logN;
    const uint32_t npairs = 1u << (logN - 1), nblk = mr_blocks_per_limb(logN);
    const uint32_t k = blockIdx.x % nblk, lc = blockIdx.x / nblk, c = lc % count, limb = lc / count;
    const u64 q = mods.m[limb].q;
    const size_t base = ((size_t)c * 2 * nl + limb) * N;
    ulonglong2 x[2][2], y[2][2];
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t p = k * LM_MR_PAIRS + threadIdx.x + 256 * u;
        if (p < npairs)
#pragma unroll
            for (uint32_t w = 0; w < 2; w++) {
                x[u][w] = *reinterpret_cast<const ulonglong2 *>(out + base + (size_t)w * nl * N + 2 * p);
                y[u][w] = *reinterpret_cast<const ulonglong2 *>(ks + base + (size_t)w * nl * N + 2 * p);
            }
    }
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t p = k * LM_MR_PAIRS + threadIdx.x + 256 * u;
        if (p < npairs)
#pragma unroll
            for (uint32_t w = 0; w < 2; w++) {
                ulonglong2 r; // < q + 2q
                r.x = lm_csub(lm_csub(x[u][w].x + y[u][w].x, 2 * q), q);
                r.y = lm_csub(lm_csub(x[u][w].y + y[u][w].y, 2 * q), q);
                *reinterpret_cast<ulonglong2 *>(out + base + (size_t)w * nl * N + 2 * p) = r;
            }
    }
}

// ---- the summed tensor of a dot product, sum_i a_e x b_e over the n terms e = g n + i of group g: one pass over the
// pairs, ONE degree-2 triple per group (lumen_mul_relin_dot, lumen_mul_tensor_dot).
// Lazy across the terms.  The operands are canonical words, so a product is below q^2, and the three sums are kept as
// 128-bit integers: per term the four 64 x 64 products and their additions, nothing else.  A chunk of at most
// LM_DOT_CHUNK terms ends in ONE Montgomery quotient step per output word, r = S 2^-64 mod q as any 64-bit word, and ONE
// multiplication by the per-limb Shoup constant tfac = T 2^64 mod q (k_mul_tensor's, applied there per operand), which
// takes any 64-bit word and leaves the canonical T S mod q; chunks of a longer sum are folded modulo q.
// THE BOUND.  Every context has F q < 2^64 with F = lm_q_bound_factor(log_n) >= lm_q_bound_factor(8) = 32
// (lumen_ctx_create).  P products sum to S < P 2^128 / F^2, so S fits 128 bits and its upper word is below P 2^64 / F^2;
// the quotient step adds mulhi(m, q) + carry <= q < 2^64 / F to it, and r stays a 64-bit word when P / F^2 + 1 / F <= 1,
// P <= F^2 - F = 992.  d1 sums two products per term: LM_DOT_CHUNK = 256 terms are P = 512 of them.  (lm_mont_reduce_wide's
// own contract, terms q < 2^63 for factors that are any 64-bit word, would allow 8 terms; these factors are below q.)
#define LM_DOT_CHUNK 256u
static_assert(2ull * LM_DOT_CHUNK <= lm_q_bound_factor(8) * lm_q_bound_factor(8) - lm_q_bound_factor(8),
              "a chunk's 2 * LM_DOT_CHUNK products of canonical words must reduce from a 64-bit upper word under the modulus bound of the smallest ring degree");

// Block order: k_mul_tensor's, with the group where it has the ciphertext: blockIdx.x = (limb * groups + group) * nblk + k,
// a block on 256 * U consecutive coefficient pairs of one limb of every term of one group; the terms are a loop inside
// the block, the next term's four 16-byte loads issued before the current term's multiplies.  U = 2 is k_mul_tensor's
// block; U = 1 doubles the blocks of a launch with few groups (profiles/EXPERIMENTS.md, "The dot product").
// PARTS.  A launch with few groups still leaves most CUs without a block, and a wave streams its terms one after the
// other: with parts > 1 the terms of a group are split over `parts` blocks, blockIdx.x = ((limb * groups + group) * parts
// + part) * nblk + k, part r on terms [r per, min(n, (r + 1) per)), per = ceil(n / parts); each writes its canonical triple
// into block r of a [parts][groups][3][nl][N] buffer (RELIN = false), and k_dot_fold adds the parts.
template <uint32_t U>
__host__ __device__ __forceinline__ uint32_t dot_blocks_per_limb(uint32_t logN) {
    return (1u << (logN - 1)) > 256u * U ? (1u << (logN - 1)) / (256u * U) : 1u;
}

// S 2^-64 mod q as a 64-bit word (the quotient step of lm_mont_reduce, not brought home), then times tfac: canonical
__device__ __forceinline__ u64 dot_close(u128 S, tw_t W, u64 q, u64 nq, u64 qneg) {
    const u64 lo = (u64)S, hi = (u64)(S >> 64);
    const u64 m = lo * qneg;
    return lm_shoup_cs(hi + lm_mulhi(m, q) + (lo != 0), W, q, nq);
}

// a: [groups * n][2][nl][N]; b: as many (bgroup = 1: b[g n + i]) or n ciphertexts (bgroup = 0: b[i], one vector against
// every group); canonical words; a and b may be the same block.
// RELIN = false: out = (D0, D1, D2), [groups][3][nl][N].
// RELIN = true:  out = (D0, D1 - D2), [groups][2][nl][N], and acc = (0, D2), [groups][2][nl][N]: k_mul_tensor<true>'s two.
template <bool RELIN, uint32_t U>
__global__ __launch_bounds__(256) void k_tensor_dot(const u64 *__restrict__ a, const u64 *__restrict__ b, u64 *__restrict__ out,
                                                    u64 *__restrict__ acc, uint32_t groups, uint32_t n, uint32_t bgroup, uint32_t parts,
                                                    uint32_t nl, uint32_t logN, lm_mods mods, lm_ninv_t tfac) {
    const size_t N = (size_t)1 << logN, ctw = (size_t)2 * nl * N;
    const uint32_t npairs = 1u << (logN - 1), nblk = dot_blocks_per_limb<U>(logN);
    const uint32_t k = blockIdx.x % nblk, lgp = blockIdx.x / nblk, part = lgp % parts, lg = lgp / parts, g = lg % groups, limb = lg / groups;
    const uint32_t per = (n + parts - 1) / parts, i0 = part * per, i1 = min(n, i0 + per);
    const mod_t md = mods.m[limb];
    const tw_t W = tfac.t[limb];
    const u64 q = md.q, nq = 0 - md.q;
    const u64 *ap = a + (size_t)g * n * ctw + limb * N;
    const u64 *bp = b + (size_t)g * bgroup * n * ctw + limb * N;
    uint32_t p[U];
    bool live[U];
#pragma unroll
    for (uint32_t u = 0; u < U; u++) p[u] = k * 256 * U + threadIdx.x + 256 * u, live[u] = p[u] < npairs;
    ulonglong2 cur[U][4] = {}, nxt[U][4] = {}; // a0, a1, b0, b1 of one term (a lane past the limb's end keeps zeros)
    auto load = [&](ulonglong2(&v)[U][4], uint32_t i) {
#pragma unroll
        for (uint32_t u = 0; u < U; u++)
            if (live[u]) {
                v[u][0] = *reinterpret_cast<const ulonglong2 *>(ap + i * ctw + 2 * p[u]);
                v[u][1] = *reinterpret_cast<const ulonglong2 *>(ap + i * ctw + (size_t)nl * N + 2 * p[u]);
                v[u][2] = *reinterpret_cast<const ulonglong2 *>(bp + i * ctw + 2 * p[u]);
                v[u][3] = *reinterpret_cast<const ulonglong2 *>(bp + i * ctw + (size_t)nl * N + 2 * p[u]);
            }
    };
    u128 s0[U][2], s1[U][2], s2[U][2]; // the chunk's wide sums
    u64 f0[U][2], f1[U][2], f2[U][2];  // the chunks before it, canonical
#pragma unroll
    for (uint32_t u = 0; u < U; u++)
#pragma unroll
        for (int e = 0; e < 2; e++) s0[u][e] = s1[u][e] = s2[u][e] = 0, f0[u][e] = f1[u][e] = f2[u][e] = 0;
    if (i0 < i1) load(cur, i0);
    for (uint32_t i = i0, in_chunk = 0; i < i1; i++) {
        if (i + 1 < i1) load(nxt, i + 1);
#pragma unroll
        for (uint32_t u = 0; u < U; u++)
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const u64 a0 = e ? cur[u][0].y : cur[u][0].x, a1 = e ? cur[u][1].y : cur[u][1].x;
                const u64 b0 = e ? cur[u][2].y : cur[u][2].x, b1 = e ? cur[u][3].y : cur[u][3].x;
                s0[u][e] += (u128)a0 * b0;
                s1[u][e] += (u128)a0 * b1;
                s1[u][e] += (u128)a1 * b0;
                s2[u][e] += (u128)a1 * b1;
            }
        if (++in_chunk == LM_DOT_CHUNK || i + 1 == i1) { // (uniform) the chunk's one reduction per output word
            in_chunk = 0;
#pragma unroll
            for (uint32_t u = 0; u < U; u++)
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    f0[u][e] = lm_addmod(f0[u][e], dot_close(s0[u][e], W, q, nq, md.qneg), q);
                    f1[u][e] = lm_addmod(f1[u][e], dot_close(s1[u][e], W, q, nq, md.qneg), q);
                    f2[u][e] = lm_addmod(f2[u][e], dot_close(s2[u][e], W, q, nq, md.qneg), q);
                    s0[u][e] = s1[u][e] = s2[u][e] = 0;
                }
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++)
#pragma unroll
            for (uint32_t w = 0; w < 4; w++) cur[u][w] = nxt[u][w];
    }
    constexpr uint32_t NP = RELIN ? 2 : 3;
    u64 *o0 = out + (((size_t)part * groups + g) * NP * nl + limb) * N;
#pragma unroll
    for (uint32_t u = 0; u < U; u++) {
        if (!live[u]) continue;
        ulonglong2 r0, r1, r2;
        r0.x = f0[u][0], r0.y = f0[u][1];
        r2.x = f2[u][0], r2.y = f2[u][1];
        r1.x = RELIN ? lm_submod(f1[u][0], f2[u][0], q) : f1[u][0];
        r1.y = RELIN ? lm_submod(f1[u][1], f2[u][1], q) : f1[u][1];
        *reinterpret_cast<ulonglong2 *>(o0 + 2 * p[u]) = r0;
        *reinterpret_cast<ulonglong2 *>(o0 + (size_t)nl * N + 2 * p[u]) = r1;
        if constexpr (RELIN) {
            u64 *c0 = acc + ((size_t)g * 2 * nl + limb) * N;
            ulonglong2 z;
            z.x = z.y = 0;
            *reinterpret_cast<ulonglong2 *>(c0 + 2 * p[u]) = z;
            *reinterpret_cast<ulonglong2 *>(c0 + (size_t)nl * N + 2 * p[u]) = r2;
        } else {
            *reinterpret_cast<ulonglong2 *>(o0 + (size_t)2 * nl * N + 2 * p[u]) = r2;
        }
    }
}

// The parts of a split sum added up: part, [parts][groups][3][nl][N] canonical, to k_tensor_dot's two output forms.
// k_relin_close's block order (the group where it has the ciphertext).
template <bool RELIN>
__global__ __launch_bounds__(256) void k_dot_fold(const u64 *__restrict__ part, u64 *__restrict__ out, u64 *__restrict__ acc, uint32_t groups,
                                                  uint32_t parts, uint32_t nl, uint32_t logN, lm_mods mods) {
    const size_t N = (size_t)1 << logN, pw = (size_t)groups * 3 * nl * N;
    const uint32_t npairs = 1u << (logN - 1), nblk = mr_blocks_per_limb(logN);
    const uint32_t k = blockIdx.x % nblk, lg = blockIdx.x / nblk, g = lg % groups, limb = lg / groups;
    const u64 q = mods.m[limb].q;
    const u64 *src = part + ((size_t)g * 3 * nl + limb) * N;
    constexpr uint32_t NP = RELIN ? 2 : 3;
    u64 *o0 = out + ((size_t)g * NP * nl + limb) * N;
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t p = k * LM_MR_PAIRS + threadIdx.x + 256 * u;
        if (p >= npairs) continue;
        ulonglong2 r[3];
#pragma unroll
        for (uint32_t w = 0; w < 3; w++) r[w] = *reinterpret_cast<const ulonglong2 *>(src + (size_t)w * nl * N + 2 * p);
        for (uint32_t t = 1; t < parts; t++)
#pragma unroll
            for (uint32_t w = 0; w < 3; w++) {
                const ulonglong2 x = *reinterpret_cast<const ulonglong2 *>(src + t * pw + (size_t)w * nl * N + 2 * p);
                r[w].x = lm_addmod(r[w].x, x.x, q), r[w].y = lm_addmod(r[w].y, x.y, q);
            }
        if constexpr (RELIN) r[1].x = lm_submod(r[1].x, r[2].x, q), r[1].y = lm_submod(r[1].y, r[2].y, q);
        *reinterpret_cast<ulonglong2 *>(o0 + 2 * p) = r[0];
        *reinterpret_cast<ulonglong2 *>(o0 + (size_t)nl * N + 2 * p) = r[1];
        if constexpr (RELIN) {
            u64 *c0 = acc + ((size_t)g * 2 * nl + limb) * N;
            ulonglong2 z;
            z.x = z.y = 0;
            *reinterpret_cast<ulonglong2 *>(c0 + 2 * p) = z;
            *reinterpret_cast<ulonglong2 *>(c0 + (size_t)nl * N + 2 * p) = r[2];
        } else {
            *reinterpret_cast<ulonglong2 *>(o0 + (size_t)2 * nl * N + 2 * p) = r[2];
        }
    }
}

// -------------------------------------------------------------------- host side
namespace {

lm_ninv_t tensor_consts(const lumen_ctx *ctx) {
    lm_ninv_t f;
    for (uint32_t l = 0; l < LM_MAX_LIMBS; l++) {
        const uint64_t q = ctx->mod[l < ctx->L ? l : 0];
        f.t[l] = h_tw(h_mulmod(ctx->T % q, h_r64_mod(q), q), q);
    }
    return f;
}

uint32_t mr_grid(const lumen_ctx *ctx, uint32_t count, uint32_t nl) { return nl * count * mr_blocks_per_limb(ctx->logN); }

// a, b: `count` ciphertexts of nl limbs from these pointers on (b: one, with bcast); out / acc as k_mul_tensor takes them
template <bool RELIN>
int launch_tensor(lumen_ctx *ctx, const u64 *a, const u64 *b, bool bcast, u64 *out, u64 *acc, uint32_t count, uint32_t nl) {
    lm_prof_scope ps(ctx, "mul_tensor", count);
    hipLaunchKernelGGL(k_mul_tensor<RELIN>, dim3(mr_grid(ctx, count, nl)), dim3(256), 0, ctx->stream, a, b, out, acc, count,
                       bcast ? 0u : 1u, nl, ctx->logN, ctx->mods, tensor_consts(ctx));
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// what both entry points ask of their operands
int check_operands(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, const char *what) {
    if (int rc = check_level_of_chain(ctx, a, what)) return rc;
    LM_FULL_WIDTH(ctx, b, what);
    LM_CHECK(ctx, a->nl == b->nl, "%s: the operands have different levels (%u and %u limbs)", what, a->nl, b->nl);
    LM_CHECK(ctx, a->count == b->count || b->count == 1,
             "%s: count mismatch: %u ciphertexts times %u (the second operand has as many, or one)", what, a->count, b->count);
    LM_CHECK(ctx, (uint64_t)a->count * a->nl * mr_blocks_per_limb(ctx->logN) < (1ull << 31), "%s: %u ciphertexts are more than one launch takes",
             what, a->count);
    return 0;
}

} // namespace

extern "C" int lumen_mul_tensor(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, uint64_t *host_out) {
    LM_CHECK(nullptr, ctx && a && b && host_out, "lumen_mul_tensor: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_operands(ctx, a, b, "lumen_mul_tensor")) return rc;
    if (!a->count) return 0;
    const size_t words = (size_t)a->count * 3 * a->nl * ctx->N;
    lm_dev<u64> d;
    if (int rc = d.alloc(ctx, words, "the degree-2 ciphertexts of lumen_mul_tensor")) return rc;
    d.release_on(ctx->stream, false);
    if (int rc = launch_tensor<false>(ctx, a->d, b->d, b->count != a->count, d.get(), nullptr, a->count, a->nl)) return rc;
    return lm_d2h(ctx, host_out, d.get(), words * 8, true);
}

extern "C" int lumen_mul_relin(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, lumen_set **out) {
    LM_CHECK(nullptr, ctx && a && b && out, "lumen_mul_relin: NULL argument");
    LM_ENTER(ctx);
    LM_CHECK(ctx, ctx->K >= 1, "parameters have no special primes: key switching unavailable");
    if (int rc = check_operands(ctx, a, b, "lumen_mul_relin")) return rc;
    KsRun run;
    if (int rc = ks_run_open(ctx, a->count, a->nl, 2, true, &run)) return rc; // (refuses K > 2, as InnerSum does)
    const std::shared_ptr<lm_galois_key> rlk = lm_relin_key(ctx); // kept alive for the call
    LM_CHECK(ctx, rlk && rlk->d_key, "lumen_mul_relin: no relinearisation key loaded (lumen_load_relin_key)");
    const uint32_t nl = a->nl, count = a->count;
    const bool bcast = b->count != count;
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, count, nl, &o)) return rc;
    lm_set_guard og(ctx, o);
    const size_t ctw = (size_t)2 * nl * ctx->N;
    if (int rc = ks_run_scratch(ctx, &run)) return rc;
    // batches of a group alternate between the lanes, each in its own slice of the group's accumulators, as in
    // matrixInnerSumEval; everything of a batch -- tensor, key switch, closing pass -- stays on its lane
    auto batch = [&](uint32_t g0, uint32_t first, uint32_t B, const KsScratch &s, u64 *d2) {
        const size_t at = (size_t)(g0 + first) * ctw;
        if (int rc = launch_tensor<true>(ctx, a->d + at, bcast ? b->d : b->d + at, bcast, o->d + at, d2, B, nl)) return rc;
        if (int rc = rotate_accumulate(ctx, d2, s.acc2, B, *rlk, run.tb, s)) return rc;
        lm_prof_scope ps(ctx, "relin_close", B);
        hipLaunchKernelGGL(k_relin_close, dim3(mr_grid(ctx, B, nl)), dim3(256), 0, ctx->stream, o->d + at, s.acc2, B, nl, ctx->logN,
                           ctx->mods);
        LM_HIP(ctx, hipGetLastError());
        return 0;
    };
    if (int rc = ks_run(ctx, run, count, ctw, batch)) return rc;
    ctx->mul_counter += count; // as lumen_mul_plain counts its products; lumen_mul_tensor, a parity hook, does not
    *out = og.release();
    return 0;
}

// -------------------------------------------------------------------- the dot product: one relinearisation per sum
namespace {

// U by the size of the launch: k_mul_tensor's block of 512 pairs from LM_DOT_WIDE_GRID blocks on, half of it below, where
// the wider block would leave CUs without one (measured: profiles/EXPERIMENTS.md, "The dot product"); LUMEN_DOT_PAIRS = 256 / 512 overrides
#define LM_DOT_WIDE_GRID 2048u
uint32_t dot_unroll(const lumen_ctx *ctx, uint32_t groups, uint32_t nl) {
    if (ctx->tune.dot_pairs) return ctx->tune.dot_pairs / 256;
    return (uint64_t)groups * nl * dot_blocks_per_limb<2>(ctx->logN) >= LM_DOT_WIDE_GRID ? 2u : 1u;
}

// The parts a group's terms are split into: one from LM_DOT_SPLIT_BELOW blocks of 256 pairs on (a block per CU), where a
// split only adds the partial sums' traffic; below that as many as bring the launch to LM_DOT_SPLIT_GRID blocks, a part
// keeping at least LM_DOT_SPLIT_TERMS terms (measured: profiles/EXPERIMENTS.md, "The dot product").  LUMEN_DOT_PARTS overrides.  No part
// is empty: parts = ceil(n / per).
#define LM_DOT_SPLIT_BELOW 256u
#define LM_DOT_SPLIT_GRID 768u
#define LM_DOT_SPLIT_TERMS 16u
uint32_t dot_parts(const lumen_ctx *ctx, uint32_t groups, uint32_t n, uint32_t nl) {
    uint32_t parts = ctx->tune.dot_parts;
    if (!parts) {
        const uint64_t blocks = (uint64_t)groups * nl * dot_blocks_per_limb<1>(ctx->logN);
        parts = blocks >= LM_DOT_SPLIT_BELOW ? 1u : (uint32_t)std::min<uint64_t>(LM_DOT_SPLIT_GRID / blocks, n / LM_DOT_SPLIT_TERMS);
    }
    parts = std::max(1u, std::min(parts, n));
    const uint32_t per = (n + parts - 1) / parts;
    return (n + per - 1) / per;
}

// a: `groups` groups of n ciphertexts of nl limbs from this pointer on; b: as many, or (bvec) n; out / acc as k_tensor_dot
// takes them.  A split sum goes through the lane's "dot_partial" scratch and k_dot_fold, in the same scope.
template <bool RELIN>
int launch_dot(lumen_ctx *ctx, const u64 *a, const u64 *b, bool bvec, u64 *out, u64 *acc, uint32_t groups, uint32_t n, uint32_t nl) {
    lm_prof_scope ps(ctx, "mul_tensor_dot", groups);
    const uint32_t bgroup = bvec ? 0u : 1u, parts = dot_parts(ctx, groups, n, nl);
    const lm_ninv_t tfac = tensor_consts(ctx);
    if (parts > 1) {
        u64 *partial = (u64 *)lm_scratch(ctx, ctx->stream == ctx->stream2 ? "dot_partial_b" : "dot_partial",
                                        (size_t)parts * groups * 3 * nl * ctx->N * sizeof(u64));
        if (!partial) return 1;
        hipLaunchKernelGGL((k_tensor_dot<false, 1>), dim3(groups * nl * parts * dot_blocks_per_limb<1>(ctx->logN)), dim3(256), 0, ctx->stream,
                           a, b, partial, nullptr, groups, n, bgroup, parts, nl, ctx->logN, ctx->mods, tfac);
        LM_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_dot_fold<RELIN>, dim3(mr_grid(ctx, groups, nl)), dim3(256), 0, ctx->stream, partial, out, acc, groups, parts, nl,
                           ctx->logN, ctx->mods);
    } else if (dot_unroll(ctx, groups, nl) == 2) {
        hipLaunchKernelGGL((k_tensor_dot<RELIN, 2>), dim3(groups * nl * dot_blocks_per_limb<2>(ctx->logN)), dim3(256), 0, ctx->stream, a, b,
                           out, acc, groups, n, bgroup, 1u, nl, ctx->logN, ctx->mods, tfac);
    } else {
        hipLaunchKernelGGL((k_tensor_dot<RELIN, 1>), dim3(groups * nl * dot_blocks_per_limb<1>(ctx->logN)), dim3(256), 0, ctx->stream, a, b,
                           out, acc, groups, n, bgroup, 1u, nl, ctx->logN, ctx->mods, tfac);
    }
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// what both entry points ask of their operands
int check_dot_operands(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, uint32_t n, const char *what) {
    LM_CHECK(ctx, n != 0, "%s: a sum of no terms (n == 0)", what);
    if (int rc = check_level_of_chain(ctx, a, what)) return rc;
    LM_FULL_WIDTH(ctx, b, what);
    LM_CHECK(ctx, a->nl == b->nl, "%s: the operands have different levels (%u and %u limbs)", what, a->nl, b->nl);
    LM_CHECK(ctx, a->count % n == 0, "%s: %u ciphertexts are no multiple of the %u terms of a sum", what, a->count, n);
    LM_CHECK(ctx, b->count == a->count || b->count == n,
             "%s: count mismatch: %u ciphertexts times %u (the second operand has as many, or the %u of one sum)", what, a->count,
             b->count, n);
    LM_CHECK(ctx, (uint64_t)(a->count / n) * a->nl * dot_blocks_per_limb<1>(ctx->logN) < (1ull << 30),
             "%s: %u sums are more than one launch takes", what, a->count / n);
    return 0;
}

} // namespace

extern "C" int lumen_mul_tensor_dot(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, uint32_t n, uint64_t *host_out) {
    LM_CHECK(nullptr, ctx && a && b && host_out, "lumen_mul_tensor_dot: NULL argument");
    LM_ENTER(ctx);
    if (int rc = check_dot_operands(ctx, a, b, n, "lumen_mul_tensor_dot")) return rc;
    const uint32_t groups = a->count / n;
    if (!groups) return 0;
    const size_t words = (size_t)groups * 3 * a->nl * ctx->N;
    lm_dev<u64> d;
    if (int rc = d.alloc(ctx, words, "the degree-2 ciphertexts of lumen_mul_tensor_dot")) return rc;
    d.release_on(ctx->stream, false);
    if (int rc = launch_dot<false>(ctx, a->d, b->d, b->count != a->count, d.get(), nullptr, groups, n, a->nl)) return rc;
    return lm_d2h(ctx, host_out, d.get(), words * 8, true);
}

extern "C" int lumen_mul_relin_dot(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, uint32_t n, lumen_set **out) {
    LM_CHECK(nullptr, ctx && a && b && out, "lumen_mul_relin_dot: NULL argument");
    LM_ENTER(ctx);
    LM_CHECK(ctx, ctx->K >= 1, "parameters have no special primes: key switching unavailable");
    if (int rc = check_dot_operands(ctx, a, b, n, "lumen_mul_relin_dot")) return rc;
    const uint32_t nl = a->nl, groups = a->count / n;
    KsRun run;
    if (int rc = ks_run_open(ctx, groups, nl, 2, true, &run)) return rc; // (refuses K > 2, as InnerSum does)
    const std::shared_ptr<lm_galois_key> rlk = lm_relin_key(ctx); // kept alive for the call
    LM_CHECK(ctx, rlk && rlk->d_key, "lumen_mul_relin_dot: no relinearisation key loaded (lumen_load_relin_key)");
    const bool bvec = b->count != a->count;
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create(ctx, groups, nl, &o)) return rc;
    lm_set_guard og(ctx, o);
    const size_t ctw = (size_t)2 * nl * ctx->N;
    if (int rc = ks_run_scratch(ctx, &run)) return rc;
    // lumen_mul_relin's batch over the `groups` outputs: a batch's summed tensor reads its groups' n terms each, and its
    // key switch and closing pass stay on its lane
    auto batch = [&](uint32_t g0, uint32_t first, uint32_t B, const KsScratch &s, u64 *d2) {
        const size_t at = (size_t)(g0 + first) * ctw;
        if (int rc = launch_dot<true>(ctx, a->d + at * n, bvec ? b->d : b->d + at * n, bvec, o->d + at, d2, B, n, nl)) return rc;
        if (int rc = rotate_accumulate(ctx, d2, s.acc2, B, *rlk, run.tb, s)) return rc;
        lm_prof_scope ps(ctx, "relin_close", B);
        hipLaunchKernelGGL(k_relin_close, dim3(mr_grid(ctx, B, nl)), dim3(256), 0, ctx->stream, o->d + at, s.acc2, B, nl, ctx->logN,
                           ctx->mods);
        LM_HIP(ctx, hipGetLastError());
        return 0;
    };
    if (int rc = ks_run(ctx, run, groups, ctw, batch)) return rc;
    ctx->mul_counter += a->count; // the products formed, as lumen_mul_relin counts them; the parity hook counts nothing
    *out = og.release();
    return 0;
}
