// TEST INFRASTRUCTURE ONLY: runs the device arithmetic primitives of lumenos_amd/csrc/ one call per row and hands the raw
// 64-bit results back (tests/test_arith_probe.py compares them with the integer definitions of tests/arith_model.py).
// Nothing is copied from the headers: every kernel below only calls them.  Needs the HIP runtime alone, no lumen_ctx.
//
// Every entry point is  int probe_<family>(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out):
// upload, ONE kernel launch, download, the HIP status.  consts[0 .. 3] = modulus, floor(2^64 / modulus), a count, one
// family-specific word; the family's tables follow from consts[4].  Results are not normalised.
//
// lm_shoup3<true> takes its multiplier through "s" constraints, so wherever a multiplier, a twiddle set or a table of
// constants reaches a <true> form it is indexed by blockIdx alone (one per workgroup) and the lanes walk the rows: per
// lane it would be squashed to lane 0's by the compiler's readfirstlane and the test would check nothing.
// Build: hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -I lumenos_amd/csrc -shared
//        tests/cpp/arith_probe.hip -o tests/cpp/libarith_probe.so      (tests/helpers.py, build_arith_probe)
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "lm_enc_host.h"
#include "lm_ks_dev.h"
#include "lm_ntt_bfly.h"
#include "lm_polyeval_dev.h"
#include "lm_sample_dev.h"
#include "lm_shoup.h"

#define PROBE_THREADS 256
#define PROBE_HDR 4 // consts[0 .. 3]

static __device__ __forceinline__ lm_qc probe_qc(const u64 *consts) {
    lm_qc c;
    c.q = consts[0], c.nq = 0 - consts[0], c.q3 = 3 * consts[0], c.qinv64 = consts[1];
    return c;
}

// ---- lm_shoup3 in its five forms.  in [n][2] = (a, x); consts: count multipliers (w, wp); out [count][5][n]
#define PROBE_SHOUP3_FORMS 5
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_shoup3(const u64 *in, size_t n, const u64 *consts, u64 *out) {
    const u64 nq = 0 - consts[0];
    const u64 w = consts[PROBE_HDR + 2 * blockIdx.x], wp = consts[PROBE_HDR + 2 * blockIdx.x + 1];
    u64 *o = out + (size_t)blockIdx.x * PROBE_SHOUP3_FORMS * n;
    for (size_t i = threadIdx.x; i < n; i += PROBE_THREADS) {
        const u64 a = in[2 * i], x = in[2 * i + 1];
        o[0 * n + i] = lm_shoup3<true>(a, w, wp, nq, x);
        o[1 * n + i] = lm_shoup3<false>(a, w, wp, nq, x);
        o[2 * n + i] = lm_shoup3<true>(a, w, wp, nq);
        o[3 * n + i] = lm_shoup3<false>(a, w, wp, nq);
        o[4 * n + i] = lm_shoup3_c(a, w, wp, nq, x);
    }
}

// ---- lm_arith.h, what lm_shoup.h builds on the chain, and lm_add_scaled_msg (lm_enc_host.h; its r is x when x is
// canonical, else 0).  Same operands; out [count][12][n]
#define PROBE_ARITH_FORMS 12
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_arith(const u64 *in, size_t n, const u64 *consts, u64 *out) {
    const lm_qc c = probe_qc(consts);
    tw_t W;
    W.w = consts[PROBE_HDR + 2 * blockIdx.x], W.wp = consts[PROBE_HDR + 2 * blockIdx.x + 1];
    u64 *o = out + (size_t)blockIdx.x * PROBE_ARITH_FORMS * n;
    for (size_t i = threadIdx.x; i < n; i += PROBE_THREADS) {
        const u64 a = in[2 * i], x = in[2 * i + 1];
        o[0 * n + i] = lm_shoup_lazy(a, W, c.q);
        o[1 * n + i] = lm_shoup(a, W, c.q);
        o[2 * n + i] = lm_shoup_cs(a, W, c.q, c.nq);
        o[3 * n + i] = lm_reduce(a, c.q, c.qinv64);
        o[4 * n + i] = lm_reduce_s(a, c.q, c.nq, c.qinv64);
        o[5 * n + i] = lm_csub(a, x);
        o[6 * n + i] = lm_csub(a, c.q);
        o[7 * n + i] = lm_addmod(a, x, c.q);
        o[8 * n + i] = lm_submod(a, x, c.q);
        o[9 * n + i] = lm_bfly_diff(a, c.q3, x);
        o[10 * n + i] = lm_bfly_diff(a, W.w, x); // any wave-uniform word in q3's place
        u64 r = x < c.q ? x : 0;
        lm_add_scaled_msg(r, a, W, c);
        o[11 * n + i] = r;
    }
}

// ---- lm_mont_reduce, lm_mont_reduce_wide.  in [n][3] = (lo, hi, terms); consts[3] = qneg; out [2][n]
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_mont(const u64 *in, size_t n, const u64 *consts, u64 *out) {
    const size_t i = (size_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
    if (i >= n) return;
    const u64 q = consts[0], qinv64 = consts[1], qneg = consts[3];
    out[i] = lm_mont_reduce(in[3 * i], in[3 * i + 1], q, qneg);
    out[n + i] = lm_mont_reduce_wide(in[3 * i], in[3 * i + 1], q, qneg, qinv64, (uint32_t)in[3 * i + 2]);
}

// ---- the butterfly stages.  in [n][16] (a case of R stages takes the first 2^R words of a row); consts: count twiddle
// sets of 15 (w, wp), a case takes the first 2^R - 1 in ITS OWN layout (lm_twset / lm_inv_twset).  blockIdx.x = set,
// blockIdx.y = case; out [cases][count][n][16], words a case does not write stay ~0.
#define PROBE_E 16
#define PROBE_TWSET 15
template <int R, bool UW>
static __device__ __forceinline__ void probe_fwd(const u64 *in, size_t n, const u64 *tws, const lm_qc &c, u64 *o) {
    lm_twset<R, UW> T;
#pragma unroll
    for (int k = 0; k < (1 << R) - 1; k++) T.w[k].w = tws[2 * k], T.w[k].wp = tws[2 * k + 1];
    for (size_t i = threadIdx.x; i < n; i += PROBE_THREADS) {
        u64 e[1 << R];
#pragma unroll
        for (int k = 0; k < (1 << R); k++) e[k] = in[PROBE_E * i + k];
        lm_fwd_stages<R, UW>(e, T, c);
#pragma unroll
        for (int k = 0; k < (1 << R); k++) o[PROBE_E * i + k] = e[k];
    }
}
#define PROBE_FWD_CASES 8 // case = (R - 1) * 2 + UW
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_fwd(const u64 *in, size_t n, const u64 *consts, u64 *out) {
    const lm_qc c = probe_qc(consts);
    const u64 *tws = consts + PROBE_HDR + (size_t)blockIdx.x * 2 * PROBE_TWSET;
    u64 *o = out + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * n * PROBE_E;
    switch (blockIdx.y) {
#define PROBE_CASE(R, UW) \
    case (R - 1) * 2 + UW: probe_fwd<R, UW>(in, n, tws, c, o); break;
        PROBE_CASE(1, 0) PROBE_CASE(1, 1) PROBE_CASE(2, 0) PROBE_CASE(2, 1)
        PROBE_CASE(3, 0) PROBE_CASE(3, 1) PROBE_CASE(4, 0) PROBE_CASE(4, 1)
#undef PROBE_CASE
    default: break;
    }
}

template <int R, bool UW, bool LAST, bool FIRST, bool NARROW = false>
static __device__ __forceinline__ void probe_inv(const u64 *in, size_t n, const u64 *tws, const lm_qc &c, u64 *o) {
    lm_inv_twset<R, UW, FIRST> T;
#pragma unroll
    for (int k = 0; k < (1 << R) - 1; k++) T.w[k].w = tws[2 * k], T.w[k].wp = tws[2 * k + 1];
    for (size_t i = threadIdx.x; i < n; i += PROBE_THREADS) {
        u64 e[1 << R];
#pragma unroll
        for (int k = 0; k < (1 << R); k++) e[k] = in[PROBE_E * i + k];
        lm_inv_stages<R, UW, LAST, FIRST, NARROW>(e, T, c);
#pragma unroll
        for (int k = 0; k < (1 << R); k++) o[PROBE_E * i + k] = e[k];
    }
}
// case = (R - 1) * 8 + FIRST * 4 + LAST * 2 + UW; cases 32 .. 39: R = 4 again, NARROW (the degrees under 48q < 2^64)
#define PROBE_INV_CASES 40
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_inv(const u64 *in, size_t n, const u64 *consts, u64 *out) {
    const lm_qc c = probe_qc(consts);
    const u64 *tws = consts + PROBE_HDR + (size_t)blockIdx.x * 2 * PROBE_TWSET;
    u64 *o = out + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * n * PROBE_E;
    switch (blockIdx.y) {
#define PROBE_CASE(R, F, L, UW) \
    case (R - 1) * 8 + F * 4 + L * 2 + UW: probe_inv<R, UW, L, F>(in, n, tws, c, o); break;
#define PROBE_CASES(R)                                                                                          \
    PROBE_CASE(R, 0, 0, 0) PROBE_CASE(R, 0, 0, 1) PROBE_CASE(R, 0, 1, 0) PROBE_CASE(R, 0, 1, 1) PROBE_CASE(R, 1, 0, 0) \
        PROBE_CASE(R, 1, 0, 1) PROBE_CASE(R, 1, 1, 0) PROBE_CASE(R, 1, 1, 1)
        PROBE_CASES(1) PROBE_CASES(2) PROBE_CASES(3) PROBE_CASES(4)
#undef PROBE_CASES
#undef PROBE_CASE
#define PROBE_CASE(F, L, UW) \
    case 32 + F * 4 + L * 2 + UW: probe_inv<4, UW, L, F, true>(in, n, tws, c, o); break;
        PROBE_CASE(0, 0, 0) PROBE_CASE(0, 0, 1) PROBE_CASE(0, 1, 0) PROBE_CASE(0, 1, 1)
        PROBE_CASE(1, 0, 0) PROBE_CASE(1, 0, 1) PROBE_CASE(1, 1, 0) PROBE_CASE(1, 1, 1)
#undef PROBE_CASE
    default: break;
    }
}

// ---- bx_apply.  in [n][2] = (a, b); consts: count extensions (b57.w, b57.wp, c_t, ns); out [count][n]
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_bx(const u64 *in, size_t n, const u64 *consts, u64 *out) {
    const lm_qc qc = probe_qc(consts);
    const u64 *k = consts + PROBE_HDR + (size_t)blockIdx.x * 4;
    bx_t c;
    c.b57.w = k[0], c.b57.wp = k[1], c.c_t = k[2], c.ns = (uint32_t)k[3], c.own = 0;
    for (size_t i = threadIdx.x; i < n; i += PROBE_THREADS) out[(size_t)blockIdx.x * n + i] = bx_apply(c, in[2 * i], in[2 * i + 1], qc);
}

// ---- lm_s192_add / _neg / _mod.  in [n][6] = (x, y); consts[4 .. 8] = r64.w, r64.wp, r128.w, r128.wp, off;
// out [n][7] = x + y, -x, x mod q
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_s192(const u64 *in, size_t n, const u64 *consts, u64 *out) {
    const size_t i = (size_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
    if (i >= n) return;
    const lm_qc qc = probe_qc(consts);
    sfold_t f;
    f.r64.w = consts[4], f.r64.wp = consts[5], f.r128.w = consts[6], f.r128.wp = consts[7], f.off = consts[8], f.pad = 0;
    const lm_s192 x{in[6 * i], in[6 * i + 1], in[6 * i + 2]}, y{in[6 * i + 3], in[6 * i + 4], in[6 * i + 5]};
    const lm_s192 s = lm_s192_add(x, y), m = lm_s192_neg(x);
    u64 *o = out + 7 * i;
    o[0] = s.a, o[1] = s.b, o[2] = s.c, o[3] = m.a, o[4] = m.b, o[5] = m.c;
    o[6] = lm_s192_mod(f, x.a, x.b, x.c, qc);
}

// ---- pe_mont_mul, pe_block_sum.  in [n][3] = (a, b, v); consts[3] = qneg; out [n] products, then one sum of v per
// block of PE_THREADS rows (rows past n count as 0)
__global__ __launch_bounds__(PE_THREADS) void k_probe_pe(const u64 *in, size_t n, const u64 *consts, u64 *out) {
    const size_t i = (size_t)blockIdx.x * PE_THREADS + threadIdx.x;
    mod_t m;
    m.q = consts[0], m.qinv64 = consts[1], m.qneg = consts[3], m.r2 = 0;
    if (i < n) out[i] = pe_mont_mul(in[3 * i], in[3 * i + 1], m);
    const u64 s = pe_block_sum(i < n ? in[3 * i + 2] : 0, m);
    if (threadIdx.x == 0) out[n + blockIdx.x] = s;
}

// ---- the small-coefficient rules.  in [n][8]: the 16 keystream words of a block, two per 64-bit word, low first;
// out [n][27] = lm_ternary16 (2 words), lm_gauss8 (1 word), lm_lift_small of the 16 + 8 coefficients
#define PROBE_SAMPLE_OUT 27
__global__ __launch_bounds__(PROBE_THREADS) void k_probe_sample(const u64 *in, size_t n, const u64 *consts, u64 *out, enc_cdt_t cdt) {
    const size_t i = (size_t)blockIdx.x * PROBE_THREADS + threadIdx.x;
    if (i >= n) return;
    u32 w[16];
#pragma unroll
    for (int k = 0; k < 8; k++) w[2 * k] = (u32)in[8 * i + k], w[2 * k + 1] = (u32)(in[8 * i + k] >> 32);
    union {
        uint4 v;
        int8_t b[16];
        u64 d[2];
    } t;
    union {
        uint2 v;
        int8_t b[8];
        u64 d;
    } g;
    t.v = lm_ternary16(w);
    g.v = lm_gauss8(w, cdt);
    u64 *o = out + PROBE_SAMPLE_OUT * i;
    o[0] = t.d[0], o[1] = t.d[1], o[2] = g.d;
#pragma unroll
    for (int k = 0; k < 16; k++) o[3 + k] = lm_lift_small(t.b[k], consts);
#pragma unroll
    for (int k = 0; k < 8; k++) o[19 + k] = lm_lift_small(g.b[k], consts);
}

namespace {
struct probe_buf {
    u64 *p = nullptr;
    ~probe_buf() {
        if (p) (void)hipFree(p);
    }
};
// upload `in` and `consts`, fill `out`'s device image with ~0, launch, download
template <class Launch>
int probe_run(const uint64_t *in, size_t in_words, const uint64_t *consts, size_t const_words, uint64_t *out, size_t out_words,
              Launch launch) {
    probe_buf din, dc, dout;
    hipError_t e;
    if ((e = hipMalloc((void **)&din.p, (in_words ? in_words : 1) * 8)) != hipSuccess) return (int)e;
    if ((e = hipMalloc((void **)&dc.p, const_words * 8)) != hipSuccess) return (int)e;
    if ((e = hipMalloc((void **)&dout.p, (out_words ? out_words : 1) * 8)) != hipSuccess) return (int)e;
    if (in_words && (e = hipMemcpy(din.p, in, in_words * 8, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
    if ((e = hipMemcpy(dc.p, consts, const_words * 8, hipMemcpyHostToDevice)) != hipSuccess) return (int)e;
    if (out_words && (e = hipMemset(dout.p, 0xff, out_words * 8)) != hipSuccess) return (int)e;
    if (out_words) launch((const u64 *)din.p, (const u64 *)dc.p, dout.p);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return (int)e;
    if (out_words && (e = hipMemcpy(out, dout.p, out_words * 8, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
    return 0;
}
inline unsigned probe_blocks(size_t n) { return (unsigned)((n + PROBE_THREADS - 1) / PROBE_THREADS); }
constexpr size_t PROBE_MAX_ROWS = (size_t)1 << 24, PROBE_MAX_COUNT = 1 << 12; // grids and buffers stay small
inline bool probe_ok(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out, bool counted) {
    return in && consts && out && n <= PROBE_MAX_ROWS && (!counted || (consts[2] >= 1 && consts[2] <= PROBE_MAX_COUNT));
}
} // namespace

#define PROBE_BAD_ARGS (-1)

extern "C" {
int probe_shoup3(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out) {
    if (!probe_ok(in, n, consts, out, true)) return PROBE_BAD_ARGS;
    const size_t cnt = consts[2];
    return probe_run(in, 2 * n, consts, PROBE_HDR + 2 * cnt, out, cnt * PROBE_SHOUP3_FORMS * n, [&](const u64 *i, const u64 *c, u64 *o) {
        k_probe_shoup3<<<dim3((unsigned)cnt), dim3(PROBE_THREADS)>>>(i, n, c, o);
    });
}
int probe_arith(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out) {
    if (!probe_ok(in, n, consts, out, true)) return PROBE_BAD_ARGS;
    const size_t cnt = consts[2];
    return probe_run(in, 2 * n, consts, PROBE_HDR + 2 * cnt, out, cnt * PROBE_ARITH_FORMS * n, [&](const u64 *i, const u64 *c, u64 *o) {
        k_probe_arith<<<dim3((unsigned)cnt), dim3(PROBE_THREADS)>>>(i, n, c, o);
    });
}
int probe_mont(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out) {
    if (!probe_ok(in, n, consts, out, false)) return PROBE_BAD_ARGS;
    return probe_run(in, 3 * n, consts, PROBE_HDR, out, 2 * n, [&](const u64 *i, const u64 *c, u64 *o) {
        k_probe_mont<<<dim3(probe_blocks(n)), dim3(PROBE_THREADS)>>>(i, n, c, o);
    });
}
int probe_fwd_stages(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out) {
    if (!probe_ok(in, n, consts, out, true)) return PROBE_BAD_ARGS;
    const size_t cnt = consts[2];
    return probe_run(in, PROBE_E * n, consts, PROBE_HDR + 2 * PROBE_TWSET * cnt, out, PROBE_FWD_CASES * cnt * n * PROBE_E,
                     [&](const u64 *i, const u64 *c, u64 *o) {
                         k_probe_fwd<<<dim3((unsigned)cnt, PROBE_FWD_CASES), dim3(PROBE_THREADS)>>>(i, n, c, o);
                     });
}
int probe_inv_stages(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out) {
    if (!probe_ok(in, n, consts, out, true)) return PROBE_BAD_ARGS;
    const size_t cnt = consts[2];
    return probe_run(in, PROBE_E * n, consts, PROBE_HDR + 2 * PROBE_TWSET * cnt, out, PROBE_INV_CASES * cnt * n * PROBE_E,
                     [&](const u64 *i, const u64 *c, u64 *o) {
                         k_probe_inv<<<dim3((unsigned)cnt, PROBE_INV_CASES), dim3(PROBE_THREADS)>>>(i, n, c, o);
                     });
}
int probe_bx(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out) {
    if (!probe_ok(in, n, consts, out, true)) return PROBE_BAD_ARGS;
    const size_t cnt = consts[2];
    return probe_run(in, 2 * n, consts, PROBE_HDR + 4 * cnt, out, cnt * n, [&](const u64 *i, const u64 *c, u64 *o) {
        k_probe_bx<<<dim3((unsigned)cnt), dim3(PROBE_THREADS)>>>(i, n, c, o);
    });
}
int probe_s192(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out) {
    if (!probe_ok(in, n, consts, out, false)) return PROBE_BAD_ARGS;
    return probe_run(in, 6 * n, consts, PROBE_HDR + 5, out, 7 * n, [&](const u64 *i, const u64 *c, u64 *o) {
        k_probe_s192<<<dim3(probe_blocks(n)), dim3(PROBE_THREADS)>>>(i, n, c, o);
    });
}
int probe_pe(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out) {
    if (!probe_ok(in, n, consts, out, false)) return PROBE_BAD_ARGS;
    const size_t blocks = (n + PE_THREADS - 1) / PE_THREADS;
    return probe_run(in, 3 * n, consts, PROBE_HDR, out, n + blocks, [&](const u64 *i, const u64 *c, u64 *o) {
        k_probe_pe<<<dim3((unsigned)blocks), dim3(PE_THREADS)>>>(i, n, c, o);
    });
}
int probe_sample(const uint64_t *in, size_t n, const uint64_t *consts, uint64_t *out) {
    if (!probe_ok(in, n, consts, out, false)) return PROBE_BAD_ARGS;
    enc_cdt_t cdt;
    for (int k = 0; k < 19; k++) cdt.t[k] = H_GAUSS_CDT[k];
    return probe_run(in, 8 * n, consts, PROBE_HDR, out, PROBE_SAMPLE_OUT * n, [&](const u64 *i, const u64 *c, u64 *o) {
        k_probe_sample<<<dim3(probe_blocks(n)), dim3(PROBE_THREADS)>>>(i, n, c, o, cdt);
    });
}
// 1: the hand-scheduled chain, 0: the compiler's (which build this library is)
int probe_asm_shoup(void) { return LM_ASM_SHOUP; }
}
