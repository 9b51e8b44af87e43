// The switching keys of the hybrid key switch (lm_keyswitch.hip), Galois keys and the relinearisation key: which
// elements an InnerSum needs, and a key's way to the device -- range check, Montgomery form with P^-1 folded in, the
// gadget product's limb-major layout (ks_key_at) -- with the gather tables of its automorphism (the identity for the
// relinearisation key).  key_to_device and key_install are shared by the two loaders.
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
__global__ __launch_bounds__(256) void k_key_prepare(const u64 *__restrict__ src, u64 *__restrict__ dst, uint32_t logN, uint32_t LK,
                                                     size_t words, lm_mods mods, lm_ninv_t fac, uint32_t *__restrict__ bad) {
    const uint32_t beta = (uint32_t)((words >> logN) / (2 * LK));
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(i >> logN), t = row % LK; // row = (d * 2 + w) * LK + t: the caller's order
        const u64 q = mods.m[t].q, x = src[i];
        if (x >= q) atomicMin(bad, row);
        const size_t o = (ks_key_at(row / (2 * LK), (row / LK) & 1, t, beta) << logN) + (i & (((size_t)1 << logN) - 1));
        dst[o] = lm_shoup_cs(x, fac.t[t], q, 0 - q);
    }
}

namespace {

// host words [beta][b|a][L+K][N] -> the key in the gadget product's form, on the device; returns with the stream idle
int key_to_device(lumen_ctx *ctx, const uint64_t *evk, uint32_t flags, const char *what, lm_dev<u64> &d_new) {
    const uint32_t N = ctx->N, L = ctx->L, K = ctx->K, LK = L + K;
    const uint32_t beta = (L + K - 1) / K;
    const size_t words = (size_t)beta * 2 * LK * N;
    // To Montgomery form (one-off per key), on the device since round 4: the host loop of 128-bit divisions cost
    // ~70 ms per key at the headline size, 14 keys per client.  The Q limbs also absorb P^-1 mod q_t: the
    // gadget product then yields u * P^-1 directly and ModDown is u' - lift * P^-1, one multiplication
    // on the unreduced lift (exact: (sum x*k) * P^-1 == sum x * (k * P^-1) mod q_t).  A key that already is in
    // Lattigo's Montgomery form (x * 2^64 mod q: what GadgetCiphertext holds) only takes the P^-1 factor.
    lm_ninv_t fac;
    for (uint32_t t = 0; t < LM_MAX_LIMBS; t++) fac.t[t] = h_tw(1, ctx->mod[0] ? ctx->mod[0] : 3);
    for (uint32_t t = 0; t < LK; t++) {
        const uint64_t q = ctx->mod[t];
        uint64_t r = (flags & LUMEN_KEY_MONTGOMERY) ? 1 : h_r64_mod(q);
        if (t < L) r = h_mulmod(r, h_invmod(h_p_mod(ctx, q), q), q);
        fac.t[t] = h_tw(r, q);
    }
    lm_dev<u64> raw; // the staging copy of the host words
    uint32_t *bad = (uint32_t *)lm_scratch(ctx, "key_bad", 4);
    if (!bad || raw.alloc(ctx, words, ("the staging copy of " + std::string(what)).c_str())) return 1;
    LM_HIP(ctx, hipMemsetAsync(bad, 0xFF, 4, ctx->stream));
    if (int rc = lm_h2d(ctx, raw.get(), evk, words * 8)) return rc; // returns when evk may be reused
    if (int rc = d_new.alloc(ctx, words, what)) return rc;
    hipLaunchKernelGGL(k_key_prepare, dim3(2048), dim3(256), 0, ctx->stream, raw.get(), d_new.get(), ctx->logN, LK, words, ctx->mods, fac,
                       bad);
    uint32_t first_bad = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&first_bad, bad, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return lm_fail(ctx, "key conversion failed: %s", hipGetErrorString(e));
    if (first_bad != 0xFFFFFFFFu)
        return lm_fail(ctx, "key residue out of range (digit %u limb %u)", first_bad / (2 * LK), first_bad % LK);
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

extern "C" int lumen_load_galois_key_ex(lumen_ctx *ctx, uint64_t gal_el, const uint64_t *evk, uint32_t flags) {
    LM_CHECK(nullptr, ctx && evk, "lumen_load_galois_key: NULL argument");
    LM_ENTER(ctx);
    const uint32_t N = ctx->N;
    LM_CHECK(ctx, ctx->K >= 1, "parameters have no special primes: key switching unavailable");
    LM_CHECK(ctx, (gal_el & 1) && gal_el < 2ull * N, "Galois element %llu is not an odd residue mod 2N",
             (unsigned long long)gal_el);
    LM_CHECK(ctx, !(flags & ~(uint32_t)LUMEN_KEY_MONTGOMERY), "lumen_load_galois_key_ex: unknown flags 0x%x", flags);
    lm_dev<u64> d_new;
    if (int rc = key_to_device(ctx, evk, flags, "a Galois key", d_new)) return rc;
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

// The relinearisation key (s^2 -> s; lumen_keygen_relin, kgen.GenRelinearizationKeyNew): a switching key like a Galois
// key's, in the same form, whose "automorphism" is the identity -- lm_mulrelin.hip runs it through rotate_accumulate.
// It lives beside the Galois keys, not among them: element 1 of ctx->gkeys stays whatever lumen_load_galois_key(1, .)
// made of it.
static const char *const RELIN_KEY = "relin_key";

extern "C" int lumen_load_relin_key(lumen_ctx *ctx, const uint64_t *evk, uint32_t flags) {
    LM_CHECK(nullptr, ctx && evk, "lumen_load_relin_key: NULL argument");
    LM_ENTER(ctx);
    LM_CHECK(ctx, ctx->K >= 1, "parameters have no special primes: key switching unavailable");
    LM_CHECK(ctx, !(flags & ~(uint32_t)LUMEN_KEY_MONTGOMERY), "lumen_load_relin_key: unknown flags 0x%x", flags);
    lm_dev<u64> d_new;
    if (int rc = key_to_device(ctx, evk, flags, "the relinearisation key", d_new)) return rc;
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
