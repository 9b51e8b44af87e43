// The switching keys of the hybrid key switch (lm_keyswitch.hip), Galois keys and the relinearisation key: which
// elements an InnerSum needs, and a key's way to the device -- range check, Montgomery form with P^-1 folded in, the
// gadget product's limb-major layout (ks_key_at) -- with the gather tables of its automorphism (the identity for the
// relinearisation key).  key_to_device and key_install are shared by the loaders.  A SEEDED key (lumen_keygen_*_seeded)
// arrives as its b halves and the public seed of its `a` halves: b takes the same conversion, `a` is drawn here, by the
// sampling contract of lm_keygen.hip, straight into the gadget product's layout (k_key_expand).
#include "lm_enc_host.h"
#include "lm_ks_host.h"

extern "C" uint32_t lumen_inner_sum_galois_elements(const lumen_ctx *ctx, uint32_t n, uint64_t *gal_els) {
    // InnerSum(ct, 1, n), n a power of two: rotations by 2^i; when n == N the
    // column rotations span one slot row (N/2) and the rows are folded with the
    // row-swap element 2N-1.  5 generates the column group.
    if (!ctx || !gal_els || n == 0 || (n & (n - 1))) return 0;
    const uint64_t two_n = 2ull * ctx->N;
    const uint32_t span = n == ctx->N ? n >> 1 : n;
    uint32_t cnt = 0;
    uint64_t g = 5; // 5^(2^i)
    for (uint32_t r = 1; r < span; r <<= 1) {
        gal_els[cnt++] = g;
        g = (g * g) & (two_n - 1);
    }
    if (n == ctx->N) gal_els[cnt++] = two_n - 1;
    return cnt;
}

// key words -> the form the gadget product multiplies with, on the device: dst = src * fac[limb] mod q (canonical).
// A residue >= q is reported through `bad` (the smallest offending row [digit][b|a][limb]).
// HALVES = 2: the caller's rows are [digit][b|a][limb]; HALVES = 1: [digit][limb], the b halves of a seeded key.
template <int HALVES>
__global__ __launch_bounds__(256) void k_key_prepare(const u64 *__restrict__ src, u64 *__restrict__ dst, uint32_t logN, uint32_t LK,
                                                     size_t words, lm_mods mods, lm_ninv_t fac, uint32_t *__restrict__ bad) {
    const uint32_t beta = (uint32_t)((words >> logN) / (HALVES * LK));
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(i >> logN), t = row % LK; // row = (d * HALVES + w) * LK + t: the caller's order
        const u64 q = mods.m[t].q, x = src[i];
        if (x >= q) atomicMin(bad, row);
        const size_t o = (ks_key_at(row / (HALVES * LK), HALVES == 2 ? (row / LK) & 1 : 0, t, beta) << logN) + (i & (((size_t)1 << logN) - 1));
        dst[o] = lm_shoup_cs(x, fac.t[t], q, 0 - q);
    }
}

// The `a` halves of a seeded key: blockIdx.y = d * LK + t (digit = gadget entry, limb), one thread per block of 8
// coefficients, as k_sample_uniform deals them.  a = stream 16 + t of sample index base + d under `seed`, times the
// limb's factor, written where the gadget product reads polynomial 1 of (d, t): never in the caller's order.
__global__ __launch_bounds__(256) void k_key_expand(u64 *__restrict__ dst, u64 base, uint32_t beta, uint32_t LK, uint32_t logN,
                                                    lm_mods mods, kg_lim_t lim, lm_ninv_t fac, enc_seed_t seed) {
    const uint32_t blk = blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= (1u << (logN - 3))) return;
    const uint32_t d = blockIdx.y / LK, t = blockIdx.y % LK;
    const u64 q = mods.m[t].q;
    u64 r[8];
    lm_uniform_run<8>(seed, base + d, LM_UNIFORM_STREAM + t, logN, blk * 8, q, mods.m[t].qinv64, lim.t[t], r);
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = lm_shoup_cs(r[k], fac.t[t], q, 0 - q);
    lm_store_run(dst + (ks_key_at(d, 1, t, beta) << logN), blk * 8, r, 8);
}

namespace {

// the factor a key word of limb t is multiplied with: 2^64 (1 for words already in Montgomery form), and P^-1 on the Q limbs
lm_ninv_t key_factors(const lumen_ctx *ctx, bool montgomery_words) {
    const uint32_t L = ctx->L, LK = L + ctx->K;
    lm_ninv_t fac;
    for (uint32_t t = 0; t < LM_MAX_LIMBS; t++) fac.t[t] = h_tw(1, ctx->mod[0] ? ctx->mod[0] : 3);
    for (uint32_t t = 0; t < LK; t++) {
        const uint64_t q = ctx->mod[t];
        uint64_t r = montgomery_words ? 1 : h_r64_mod(q);
        if (t < L) r = h_mulmod(r, h_invmod(h_p_mod(ctx, q), q), q);
        fac.t[t] = h_tw(r, q);
    }
    return fac;
}

// host words [beta][b|a][L+K][N] -> the key in the gadget product's form, on the device; returns with the stream idle.
// a_seed given: the host words are the b halves alone, [beta][L+K][N], and the `a` halves are drawn from stream 16 + t
// of sample indices a_base + d under it (k_key_expand).
int key_to_device(lumen_ctx *ctx, const uint64_t *evk, uint32_t flags, const char *what, lm_dev<u64> &d_new,
                  const uint8_t *a_seed = nullptr, uint64_t a_base = 0) {
    const uint32_t N = ctx->N, L = ctx->L, K = ctx->K, LK = L + K;
    const uint32_t beta = (L + K - 1) / K, halves = a_seed ? 1 : 2;
    const size_t words = (size_t)beta * halves * LK * N, key_words = (size_t)beta * 2 * LK * N;
    // To Montgomery form (one-off per key), on the device since round 4: the host loop of 128-bit divisions cost
    // ~70 ms per key at the headline size, 14 keys per client.  The Q limbs also absorb P^-1 mod q_t: the
    // gadget product then yields u * P^-1 directly and ModDown is u' - lift * P^-1, one multiplication
    // on the unreduced lift (exact: (sum x*k) * P^-1 == sum x * (k * P^-1) mod q_t).  A key that already is in
    // Lattigo's Montgomery form (x * 2^64 mod q: what GadgetCiphertext holds) only takes the P^-1 factor.
    const lm_ninv_t fac = key_factors(ctx, flags & LUMEN_KEY_MONTGOMERY);
    lm_dev<u64> raw; // the staging copy of the host words
    uint32_t *bad = (uint32_t *)lm_scratch(ctx, "key_bad", 4);
    if (!bad || raw.alloc(ctx, words, ("the staging copy of " + std::string(what)).c_str())) return 1;
    LM_HIP(ctx, hipMemsetAsync(bad, 0xFF, 4, ctx->stream));
    if (int rc = lm_h2d(ctx, raw.get(), evk, words * 8)) return rc; // returns when evk may be reused
    if (int rc = d_new.alloc(ctx, key_words, what)) return rc;
    if (a_seed) {
        hipLaunchKernelGGL(k_key_prepare<1>, dim3(2048), dim3(256), 0, ctx->stream, raw.get(), d_new.get(), ctx->logN, LK, words,
                           ctx->mods, fac, bad);
        // the drawn halves are canonical whatever form b came in: always the full factor
        const uint32_t nb = N >> 3, bs = nb < 256 ? nb : 256;
        hipLaunchKernelGGL(k_key_expand, dim3(nb / bs, beta * LK), dim3(bs), 0, ctx->stream, d_new.get(), a_base, beta, LK, ctx->logN,
                           ctx->mods, lm_sample_lim(ctx, LK), key_factors(ctx, false), lm_sample_seed(a_seed));
    } else {
        hipLaunchKernelGGL(k_key_prepare<2>, dim3(2048), dim3(256), 0, ctx->stream, raw.get(), d_new.get(), ctx->logN, LK, words,
                           ctx->mods, fac, bad);
    }
    uint32_t first_bad = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&first_bad, bad, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return lm_fail(ctx, "key conversion failed: %s", hipGetErrorString(e));
    if (first_bad != 0xFFFFFFFFu)
        return lm_fail(ctx, "key residue out of range (digit %u limb %u)", first_bad / (halves * LK), first_bad % LK);
    return 0; // (the staging copy goes with `raw`: the stream is idle)
}

// gk takes the new words and, once, the gather tables of its automorphism.  Call under LM_SHARED_LOCK.
int key_install(lumen_ctx *ctx, lm_galois_key &gk, lm_dev<u64> &d_new, const std::vector<uint32_t> &index, const char *what) {
    if (gk.d_key) {
        // a key loaded again.  The table is shared with every clone (group ranks on one GPU, CopyNew): its device
        // pointer must stay what a clone may have read a moment ago, so the new words are copied INTO the old
        // block (same size: it only depends on the parameters).  A clone computing at this very moment sees old or
        // new words -- the documented "do not reconfigure under a running clone" -- but never freed memory.
        lm_sync_all(ctx);
        hipError_t ce = hipMemcpyAsync(gk.d_key.get(), d_new.get(), d_new.count() * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (ce == hipSuccess) ce = hipStreamSynchronize(ctx->stream);
        d_new.reset();
        LM_CHECK(ctx, ce == hipSuccess, "replacing %s failed: %s", what, hipGetErrorString(ce));
    } else {
        gk.d_key = std::move(d_new);
    }
    // the gather tables depend on the element alone: a key loaded again keeps them
    std::vector<uint32_t> inv_index(index.size());
    for (uint32_t i = 0; i < index.size(); i++) inv_index[index[i]] = i;
    if (!gk.d_inv_index && gk.d_inv_index.upload(ctx, inv_index, "an automorphism's index table")) return 1;
    if (!gk.d_index && gk.d_index.upload(ctx, index, "an automorphism's index table")) return 1;
    return 0;
}

} // namespace

// a_seed NULL: evk is the full key; given: its b halves (key_to_device).  The callers have refused NULL arguments.
static int load_galois(lumen_ctx *ctx, const char *fn, uint64_t gal_el, const uint64_t *evk, const uint8_t *a_seed, uint32_t flags) {
    LM_ENTER(ctx);
    const uint32_t N = ctx->N;
    LM_CHECK(ctx, ctx->K >= 1, "parameters have no special primes: key switching unavailable");
    LM_CHECK(ctx, (gal_el & 1) && gal_el < 2ull * N, "Galois element %llu is not an odd residue mod 2N",
             (unsigned long long)gal_el);
    LM_CHECK(ctx, !(flags & ~(uint32_t)LUMEN_KEY_MONTGOMERY), "%s: unknown flags 0x%x", fn, flags);
    lm_dev<u64> d_new;
    if (int rc = key_to_device(ctx, evk, flags, "a Galois key", d_new, a_seed, (LM_KG_ID_GALOIS + gal_el) * LM_KG_INDEX_STRIDE)) return rc;
    std::vector<uint32_t> index(N);
    const uint64_t mask = 2ull * N - 1;
    for (uint32_t i = 0; i < N; i++) { // [LATTIGO-RECALL] ring.AutomorphismNTTIndex
        const uint64_t t1 = 2ull * h_bitrev(i, (int)ctx->logN) + 1;
        const uint64_t t2 = ((gal_el * t1 & mask) - 1) >> 1;
        index[i] = h_bitrev((uint32_t)t2, (int)ctx->logN);
    }
    LM_SHARED_LOCK(ctx);
    const std::string what = "Galois key " + std::to_string(gal_el);
    return key_install(ctx, ctx->gkeys[gal_el], d_new, index, what.c_str());
}

extern "C" int lumen_load_galois_key_ex(lumen_ctx *ctx, uint64_t gal_el, const uint64_t *evk, uint32_t flags) {
    LM_CHECK(nullptr, ctx && evk, "lumen_load_galois_key: NULL argument");
    return load_galois(ctx, "lumen_load_galois_key_ex", gal_el, evk, nullptr, flags);
}
extern "C" int lumen_load_galois_key_seeded(lumen_ctx *ctx, uint64_t gal_el, const uint64_t *b, const uint8_t a_seed[32],
                                            uint32_t flags) {
    LM_CHECK(nullptr, ctx && b && a_seed, "lumen_load_galois_key_seeded: NULL argument");
    return load_galois(ctx, "lumen_load_galois_key_seeded", gal_el, b, a_seed, flags);
}

// The relinearisation key (s^2 -> s; lumen_keygen_relin, kgen.GenRelinearizationKeyNew): a switching key like a Galois
// key's, in the same form, whose "automorphism" is the identity -- lm_mulrelin.hip runs it through rotate_accumulate.
// It lives beside the Galois keys, not among them: element 1 of ctx->gkeys stays whatever lumen_load_galois_key(1, .)
// made of it.
static const char *const RELIN_KEY = "relin_key";

static int load_relin(lumen_ctx *ctx, const char *fn, const uint64_t *evk, const uint8_t *a_seed, uint32_t flags) {
    LM_ENTER(ctx);
    LM_CHECK(ctx, ctx->K >= 1, "parameters have no special primes: key switching unavailable");
    LM_CHECK(ctx, !(flags & ~(uint32_t)LUMEN_KEY_MONTGOMERY), "%s: unknown flags 0x%x", fn, flags);
    lm_dev<u64> d_new;
    if (int rc = key_to_device(ctx, evk, flags, "the relinearisation key", d_new, a_seed, LM_KG_ID_RELIN * LM_KG_INDEX_STRIDE)) return rc;
    std::vector<uint32_t> index(ctx->N);
    for (uint32_t i = 0; i < ctx->N; i++) index[i] = i;
    LM_SHARED_LOCK(ctx);
    auto gk = lm_ext_get<lm_galois_key>(ctx, RELIN_KEY);
    if (!gk) {
        gk = std::make_shared<lm_galois_key>();
        if (int rc = key_install(ctx, *gk, d_new, index, "the relinearisation key")) return rc;
        lm_ext_put(ctx, RELIN_KEY, gk); // only a complete key becomes visible
        return 0;
    }
    return key_install(ctx, *gk, d_new, index, "the relinearisation key");
}

extern "C" int lumen_load_relin_key(lumen_ctx *ctx, const uint64_t *evk, uint32_t flags) {
    LM_CHECK(nullptr, ctx && evk, "lumen_load_relin_key: NULL argument");
    return load_relin(ctx, "lumen_load_relin_key", evk, nullptr, flags);
}
extern "C" int lumen_load_relin_key_seeded(lumen_ctx *ctx, const uint64_t *b, const uint8_t a_seed[32], uint32_t flags) {
    LM_CHECK(nullptr, ctx && b && a_seed, "lumen_load_relin_key_seeded: NULL argument");
    return load_relin(ctx, "lumen_load_relin_key_seeded", b, a_seed, flags);
}

std::shared_ptr<lm_galois_key> lm_relin_key(lumen_ctx *ctx) { return lm_ext_get<lm_galois_key>(ctx, RELIN_KEY); }

int ks_find_key(lumen_ctx *ctx, uint64_t gal_el, const lm_galois_key **gk) {
    LM_SHARED_LOCK(ctx);
    auto it = ctx->gkeys.find(gal_el);
    LM_CHECK(ctx, it != ctx->gkeys.end() && it->second.d_key && it->second.d_index && it->second.d_inv_index,
             "Galois key for element %llu not loaded", (unsigned long long)gal_el);
    *gk = &it->second;
    return 0;
}

extern "C" int lumen_load_galois_key(lumen_ctx *ctx, uint64_t gal_el, const uint64_t *evk) {
    return lumen_load_galois_key_ex(ctx, gal_el, evk, 0);
}
