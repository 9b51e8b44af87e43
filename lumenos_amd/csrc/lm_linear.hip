// The evaluator's linear operations: Evaluator.Add / Sub / Mul(ct, uint64) / MulThenAdd of the *bgv.Evaluator that
// ServerBFV embeds (fhe/bfv.go:13-21), as fhe/ntt.go:27-236 and vdec/batching.go:24-34 call them one ciphertext at a
// time.  All of them are ONE kernel, k_lincomb: out = sum_t w_t * in_t over up to eight operands in a single pass, every
// input word read once and every output word written once.  The plaintext forms (Add / Sub / MulThenAdd with an
// rlwe.Plaintext operand) are the two forms of k_plain_linear.  Nothing here is a transform: every ring degree a
// context can have is served, and lane shards too.
#include <cstring>

#include "lm_ks_host.h"

#define LM_LIN_MAX_TERMS 8

// ---- the lazy sum.  A Shoup product of ANY 64-bit word lands in [0, 3q) (lm_shoup3), a unit term adds x < q or
// q - x <= q, so the sum of eight terms stays below 24q.  Every context has (3 log_n + 8) q < 2^64 with log_n >= 8
// (lumen_ctx_create, lm_q_bound_factor), i.e. 32q < 2^64: the accumulator cannot wrap, and ONE reduction of a 64-bit word
// (lm_reduce_s) brings it home.
static_assert(3ull * LM_LIN_MAX_TERMS <= lm_q_bound_factor(8), "eight lazy terms of 3q each must stay under the modulus bound of the smallest ring degree");

enum : uint32_t { LIN_MUL = 0, LIN_ADD = 1, LIN_SUB = 2 };

struct lin_mod {
    u64 q, qinv64;
};
// By value in the kernel arguments (NT = 8: 3.6 KB of the 4 KB there are): operand pointers, strides and scalars are
// indexed by compile-time constants after unrolling and live in SGPRs -- a run-time-indexed pointer array in registers is
// how a kernel gets scratch (k_decrypt_garner's note, lm_decrypt.hip).
template <int NT>
struct lincomb_args {
    const u64 *in[NT];
    u64 *out;
    uint32_t ct_stride[NT]; // words from one ciphertext of operand t to the next; 0: its one ciphertext meets every ciphertext of the result
    uint32_t nl_in[NT];     // its limb count (>= nl: a deeper operand contributes its first limbs)
    uint32_t kind[NT];      // LIN_MUL / LIN_ADD / LIN_SUB
    tw_t w[NT][LM_MAX_LIMBS]; // LIN_MUL: centre_T(w_t) mod q_l with its Shoup companion
    lin_mod m[LM_MAX_LIMBS];
    uint32_t nl, lognw; // limbs of the result; log2 of the words of one limb (N, or N >> logw of a lane shard)
    uint32_t rows;      // count * 2 * nl limb rows of the result
};
static_assert(sizeof(lincomb_args<LM_LIN_MAX_TERMS>) <= 4096, "the widest combination must fit the kernel argument segment");

// One work item = 64 consecutive 16-byte vectors of one limb row of the result (a limb has at least 64 words; one of
// fewer than 128 leaves the upper lanes idle): row, limb and with them modulus, scalars and every operand's base address
// are wave-uniform.  `it` must be wave-uniform.
struct lin_at {
    uint32_t c, p, l, k; // ciphertext, polynomial, limb, first word of this lane's vector
};
__device__ __forceinline__ bool lin_decode(uint64_t it, uint32_t lognw, uint32_t nl, uint32_t lane, lin_at &at) {
    const uint32_t logv = lognw - 1;               // vectors per limb
    const uint32_t logc = logv > 6 ? logv - 6 : 0; // items per limb
    const uint32_t row = (uint32_t)(it >> logc);
    const uint32_t v = ((uint32_t)(it & ((1u << logc) - 1)) << 6) + lane;
    const uint32_t cp = row / nl;
    at.l = row - cp * nl, at.p = cp & 1, at.c = cp >> 1, at.k = v << 1;
    return v < (1u << logv);
}
__host__ __device__ static inline uint64_t lin_items(uint32_t rows, uint32_t lognw) {
    const uint32_t logv = lognw - 1;
    return (uint64_t)rows << (logv > 6 ? logv - 6 : 0);
}
// Guideline 11: four waves per workgroup, at most 2048 workgroups, the rest by the grid-stride loop
static inline dim3 lin_grid(uint64_t items) { return dim3((uint32_t)std::min<uint64_t>((items + 3) / 4, 2048)); }

// (no __restrict__: the destination may BE one of the operands -- a thread reads its vectors, then writes the same place)
template <int NT>
__global__ __launch_bounds__(256) void k_lincomb(lincomb_args<NT> a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    const uint64_t items = lin_items(a.rows, a.lognw);
    for (uint64_t it = wave; it < items; it += nwaves) {
        lin_at at;
        if (!lin_decode(it, a.lognw, a.nl, lane, at)) continue;
        const u64 q = a.m[at.l].q, nq = 0 - q;
        ulonglong2 x[NT];
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const size_t off = (size_t)at.c * a.ct_stride[t] + (((size_t)(at.p * a.nl_in[t] + at.l)) << a.lognw) + at.k;
            x[t] = *reinterpret_cast<const ulonglong2 *>(a.in[t] + off);
        }
        u64 s0 = 0, s1 = 0;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (a.kind[t] == LIN_ADD) { // wave-uniform
                s0 += x[t].x, s1 += x[t].y;
            } else if (a.kind[t] == LIN_SUB) {
                s0 += q - x[t].x, s1 += q - x[t].y;
            } else {
                const tw_t W = a.w[t][at.l];
                s0 = lm_shoup3<true>(x[t].x, W.w, W.wp, nq, s0);
                s1 = lm_shoup3<true>(x[t].y, W.w, W.wp, nq, s1);
            }
        }
        ulonglong2 r;
        r.x = lm_reduce_s(s0, q, nq, a.m[at.l].qinv64);
        r.y = lm_reduce_s(s1, q, nq, a.m[at.l].qinv64);
        const size_t off = (((size_t)(at.c * 2 + at.p) * a.nl + at.l) << a.lognw) + at.k;
        *reinterpret_cast<ulonglong2 *>(a.out + off) = r;
    }
}

// ---- the plaintext operand.  MAC = false: out = (c0 +- pt, c1), pt the raw residues (Evaluator.Add / Sub(ct, pt): c1 is
// copied, or left alone when the call works in place).  MAC = true: acc += a (.) ptM, ptM = pt * T in Montgomery form --
// k_mul_plain's multiplier and its one Montgomery reduction, then the addition: MulNew followed by Add, word for word.
struct plain_linear_args {
    const u64 *a;
    u64 *out;      // MAC: the accumulator, read and written
    const u64 *pt; // [nl_a][N]
    uint32_t a_stride, nl_a; // as in lincomb_args
    uint32_t nl, logN, rows;
    uint32_t sub, copy_c1;
};
template <bool MAC>
__global__ __launch_bounds__(256) void k_plain_linear(plain_linear_args a, lm_mods mods) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    const uint64_t items = lin_items(a.rows, a.logN);
    for (uint64_t it = wave; it < items; it += nwaves) {
        lin_at at;
        if (!lin_decode(it, a.logN, a.nl, lane, at)) continue;
        if (!MAC && at.p == 1 && !a.copy_c1) continue;
        const u64 q = mods.m[at.l].q;
        const size_t ao = (size_t)at.c * a.a_stride + (((size_t)(at.p * a.nl_a + at.l)) << a.logN) + at.k;
        const size_t oo = (((size_t)(at.c * 2 + at.p) * a.nl + at.l) << a.logN) + at.k;
        const ulonglong2 x = *reinterpret_cast<const ulonglong2 *>(a.a + ao);
        ulonglong2 r = x;
        if (MAC) {
            const ulonglong2 m = *reinterpret_cast<const ulonglong2 *>(a.pt + ((size_t)at.l << a.logN) + at.k);
            const ulonglong2 acc = *reinterpret_cast<const ulonglong2 *>(a.out + oo);
            const u64 qneg = mods.m[at.l].qneg;
            u64 lo, hi;
            mul128(x.x, m.x, lo, hi);
            r.x = lm_addmod(acc.x, lm_mont_reduce(lo, hi, q, qneg), q);
            mul128(x.y, m.y, lo, hi);
            r.y = lm_addmod(acc.y, lm_mont_reduce(lo, hi, q, qneg), q);
        } else if (at.p == 0) {
            const ulonglong2 m = *reinterpret_cast<const ulonglong2 *>(a.pt + ((size_t)at.l << a.logN) + at.k);
            r.x = a.sub ? lm_submod(x.x, m.x, q) : lm_addmod(x.x, m.x, q);
            r.y = a.sub ? lm_submod(x.y, m.y, q) : lm_addmod(x.y, m.y, q);
        }
        *reinterpret_cast<ulonglong2 *>(a.out + oo) = r;
    }
}

// ------------------------------------------------------------------ host side
namespace {

// Evaluator.Mul(ct, uint64) on limb q: w mod T, centred to (-T/2, T/2], its non-negative residue mod q.  The raw
// Montgomery-form words of RootForwardUint64 that fhe/ntt.go passes go through as they are; with q == T (a plain
// context) this is w mod T.
uint64_t centred_scalar(uint64_t w, uint64_t T, uint64_t q) {
    w %= T;
    if (w > (T >> 1)) {
        const uint64_t r = (T - w) % q;
        return r ? q - r : 0;
    }
    return w % q;
}

bool ranges_meet(const u64 *a, size_t aw, const u64 *b, size_t bw) { return aw && bw && a < b + bw && b < a + aw; }

// The destination of a call: *out as it is (checked against the result's shape), or a new set.  An operand may BE the
// destination (same storage, same shape: the kernels read a vector and write the same place); any other meeting of an
// operand's device range with the destination's is refused.
int lin_destination(lumen_ctx *ctx, const char *what, const lumen_set *const *in, uint32_t n, uint32_t count, uint32_t nl,
                    uint32_t logw, lumen_set **out, lm_set_guard &fresh, lumen_set **dst) {
    if (*out) {
        lumen_set *o = *out;
        LM_CHECK(ctx, o->count == count && o->nl == nl && o->logw == logw,
                 "%s: the destination holds %u ciphertexts of %u limbs (lane width 1/%u), the result has %u of %u (1/%u)", what,
                 o->count, o->nl, 1u << o->logw, count, nl, 1u << logw);
        for (uint32_t t = 0; t < n; t++) {
            if (!ranges_meet(in[t]->d, in[t]->words, o->d, o->words)) continue;
            LM_CHECK(ctx, in[t]->d == o->d && in[t]->count == count && in[t]->nl == nl,
                     "%s: operand %u overlaps the destination without being it (in place means the same ciphertexts, limbs and "
                     "storage)", what, t);
        }
        *dst = o;
        return 0;
    }
    lumen_set *o = nullptr;
    if (int rc = lumen_set_create_lanes(ctx, count, nl, logw, &o)) return rc;
    fresh.s = o;
    *dst = o;
    return 0;
}

template <int NT>
int launch_lincomb(lumen_ctx *ctx, const lumen_set *const *in, const uint64_t *w, lumen_set *dst) {
    lincomb_args<NT> a;
    memset(&a, 0, sizeof(a));
    for (int t = 0; t < NT; t++) {
        a.in[t] = in[t]->d;
        a.ct_stride[t] = in[t]->count == 1 && dst->count != 1 ? 0 : (uint32_t)lm_ctw(ctx, in[t]);
        a.nl_in[t] = in[t]->nl;
        const uint64_t wT = w[t] % ctx->T;
        a.kind[t] = wT == 1 ? LIN_ADD : wT == ctx->T - 1 ? LIN_SUB : LIN_MUL; // the centred scalar is +1 / -1 on every limb
        if (a.kind[t] == LIN_MUL)
            for (uint32_t l = 0; l < dst->nl; l++) a.w[t][l] = h_tw(centred_scalar(w[t], ctx->T, ctx->mod[l]), ctx->mod[l]);
    }
    for (uint32_t l = 0; l < dst->nl; l++) a.m[l].q = ctx->mod[l], a.m[l].qinv64 = ctx->mods.m[l].qinv64;
    a.out = dst->d;
    a.nl = dst->nl, a.lognw = ctx->logN - dst->logw, a.rows = dst->count * 2 * dst->nl;
    lm_prof_scope ps(ctx, "lincomb", dst->count);
    hipLaunchKernelGGL(k_lincomb<NT>, lin_grid(lin_items(a.rows, a.lognw)), dim3(256), 0, ctx->stream, a);
    LM_HIP(ctx, hipGetLastError());
    return 0;
}

// out = sum_{t<n} w[t] * in[t]: the one implementation behind the five scalar entry points
int lincomb(lumen_ctx *ctx, const char *what, const lumen_set *const *in, const uint64_t *w, uint32_t n, lumen_set **out) {
    LM_CHECK(ctx, n >= 1 && n <= LM_LIN_MAX_TERMS, "%s: %u operands, the combination takes 1 to %u", what, n, LM_LIN_MAX_TERMS);
    for (uint32_t t = 0; t < n; t++) LM_CHECK(ctx, in[t], "%s: operand %u is NULL", what, t);
    LM_CHECK(ctx, ctx->T >= 2, "%s: the context has no plaintext modulus", what);
    uint32_t count = 1, nl = in[0]->nl; // count 1: every operand is one ciphertext
    bool many = false;
    const uint32_t logw = in[0]->logw;
    for (uint32_t t = 0; t < n; t++) {
        LM_CHECK(ctx, in[t]->logw == logw, "%s: mixed lane widths: operand 0 holds 1/%u of every limb, operand %u holds 1/%u", what,
                 1u << logw, t, 1u << in[t]->logw);
        if (in[t]->count != 1) {
            LM_CHECK(ctx, !many || in[t]->count == count,
                     "%s: operand %u has %u ciphertexts where another has %u: counts must be equal, or 1", what, t, in[t]->count, count);
            count = in[t]->count, many = true;
        }
        nl = std::min(nl, in[t]->nl); // Lattigo's min-level rule: a deeper operand gives its first limbs
    }
    if (*out)
        LM_CHECK(ctx, (*out)->logw == logw, "%s: mixed lane widths: the operands hold 1/%u of every limb, the destination 1/%u", what,
                 1u << logw, 1u << (*out)->logw);
    lm_set_guard fresh(ctx, nullptr);
    lumen_set *dst = nullptr;
    if (int rc = lin_destination(ctx, what, in, n, count, nl, logw, out, fresh, &dst)) return rc;
    if (dst->words) {
        int rc = 1;
        switch (n) {
#define LM_X(NT) \
    case NT: rc = launch_lincomb<NT>(ctx, in, w, dst); break;
            LM_X(1) LM_X(2) LM_X(3) LM_X(4) LM_X(5) LM_X(6) LM_X(7) LM_X(8)
#undef LM_X
        }
        if (rc) return rc;
    }
    fresh.release();
    *out = dst;
    return 0;
}

// MAC: acc += a (.) pt * T; otherwise out = (c0 +- pt, c1)
int plain_linear(lumen_ctx *ctx, const char *what, const lumen_set *a, const uint64_t *pt, lumen_set **out, bool mac, bool sub) {
    LM_FULL_WIDTH(ctx, a, what);
    if (*out) LM_FULL_WIDTH(ctx, *out, what);
    uint32_t count = a->count, nl = a->nl;
    if (mac) {
        const lumen_set *acc = *out;
        LM_CHECK(ctx, !ranges_meet(a->d, a->words, acc->d, acc->words), "%s: the accumulator overlaps the ciphertext operand", what);
        LM_CHECK(ctx, a->count == acc->count || a->count == 1,
                 "%s: the operand has %u ciphertexts where the accumulator has %u: counts must be equal, or 1", what, a->count, acc->count);
        count = acc->count, nl = std::min(a->nl, acc->nl);
    }
    lm_set_guard fresh(ctx, nullptr);
    lumen_set *dst = nullptr;
    if (int rc = lin_destination(ctx, what, &a, mac ? 0 : 1, count, nl, 0, out, fresh, &dst)) return rc;
    // the range check, the staged copy and (MAC) the multiplier of lumen_mul_plain, as they are: upload_ptT leaves the raw
    // residues in "pt_raw" and pt * T in Montgomery form in "ptT"
    u64 *ptT = nullptr;
    if (int rc = upload_ptT(ctx, pt, a->nl, &ptT)) return rc;
    const u64 *raw = (const u64 *)lm_scratch(ctx, "pt_raw", (size_t)a->nl * ctx->N * sizeof(u64));
    if (!raw) return 1;
    if (dst->words) {
        plain_linear_args p;
        p.a = a->d, p.out = dst->d, p.pt = mac ? ptT : raw;
        p.a_stride = a->count == 1 && dst->count != 1 ? 0 : (uint32_t)lm_ctw(ctx, a);
        p.nl_a = a->nl, p.nl = nl, p.logN = ctx->logN, p.rows = dst->count * 2 * nl;
        p.sub = sub, p.copy_c1 = dst->d != a->d;
        lm_prof_scope ps(ctx, "plain_linear", dst->count);
        const dim3 grid = lin_grid(lin_items(p.rows, p.logN));
        if (mac)
            hipLaunchKernelGGL(k_plain_linear<true>, grid, dim3(256), 0, ctx->stream, p, ctx->mods);
        else
            hipLaunchKernelGGL(k_plain_linear<false>, grid, dim3(256), 0, ctx->stream, p, ctx->mods);
        LM_HIP(ctx, hipGetLastError());
    }
    fresh.release();
    *out = dst;
    return 0;
}

} // namespace

extern "C" int lumen_linear_combination(lumen_ctx *ctx, const lumen_set *const *in, const uint64_t *w, uint32_t n, lumen_set **out) {
    LM_CHECK(nullptr, ctx && in && w && out, "lumen_linear_combination: NULL argument");
    LM_ENTER(ctx);
    return lincomb(ctx, "lumen_linear_combination", in, w, n, out);
}

extern "C" int lumen_add(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, lumen_set **out) {
    LM_CHECK(nullptr, ctx && a && b && out, "lumen_add: NULL argument");
    LM_ENTER(ctx);
    const lumen_set *in[2] = {a, b};
    const uint64_t w[2] = {1, 1};
    return lincomb(ctx, "lumen_add", in, w, 2, out);
}

extern "C" int lumen_sub(lumen_ctx *ctx, const lumen_set *a, const lumen_set *b, lumen_set **out) {
    LM_CHECK(nullptr, ctx && a && b && out, "lumen_sub: NULL argument");
    LM_ENTER(ctx);
    LM_CHECK(ctx, ctx->T >= 2, "lumen_sub: the context has no plaintext modulus");
    const lumen_set *in[2] = {a, b};
    const uint64_t w[2] = {1, ctx->T - 1};
    return lincomb(ctx, "lumen_sub", in, w, 2, out);
}

extern "C" int lumen_mul_scalar(lumen_ctx *ctx, const lumen_set *a, uint64_t w, lumen_set **out) {
    LM_CHECK(nullptr, ctx && a && out, "lumen_mul_scalar: NULL argument");
    LM_ENTER(ctx);
    if (int rc = lincomb(ctx, "lumen_mul_scalar", &a, &w, 1, out)) return rc;
    ctx->mul_counter += (*out)->count; // the counter of the ServerBFV.Mul / MulNew wrappers, bfv.go:34-42
    return 0;
}

extern "C" int lumen_mul_scalar_then_add(lumen_ctx *ctx, const lumen_set *a, uint64_t w, lumen_set *acc) {
    LM_CHECK(nullptr, ctx && a && acc, "lumen_mul_scalar_then_add: NULL argument");
    LM_ENTER(ctx);
    LM_CHECK(ctx, !ranges_meet(a->d, a->words, acc->d, acc->words), "lumen_mul_scalar_then_add: the accumulator overlaps the ciphertext operand");
    const lumen_set *in[2] = {acc, a};
    const uint64_t ws[2] = {1, w};
    lumen_set *dst = acc;
    return lincomb(ctx, "lumen_mul_scalar_then_add", in, ws, 2, &dst);
}

extern "C" int lumen_add_plain(lumen_ctx *ctx, const lumen_set *a, const uint64_t *pt, lumen_set **out) {
    LM_CHECK(nullptr, ctx && a && pt && out, "lumen_add_plain: NULL argument");
    LM_ENTER(ctx);
    return plain_linear(ctx, "lumen_add_plain", a, pt, out, false, false);
}

extern "C" int lumen_sub_plain(lumen_ctx *ctx, const lumen_set *a, const uint64_t *pt, lumen_set **out) {
    LM_CHECK(nullptr, ctx && a && pt && out, "lumen_sub_plain: NULL argument");
    LM_ENTER(ctx);
    return plain_linear(ctx, "lumen_sub_plain", a, pt, out, false, true);
}

extern "C" int lumen_mul_plain_then_add(lumen_ctx *ctx, const lumen_set *a, const uint64_t *pt, lumen_set *acc) {
    LM_CHECK(nullptr, ctx && a && pt && acc, "lumen_mul_plain_then_add: NULL argument");
    LM_ENTER(ctx);
    lumen_set *dst = acc;
    return plain_linear(ctx, "lumen_mul_plain_then_add", a, pt, &dst, true, false);
}
