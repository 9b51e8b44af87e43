// Host-side mirror of the reference's `fhe` package, server half (see fhe.hpp).
#include "fhe.hpp"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <stdexcept>
#include <thread>

#include <sys/random.h>

namespace lumenos {
namespace fhe {

using core::InvMod;
using core::MulMod;
using core::PowMod;

// the one throwing helper behind every `check`: ctx NULL reads the library's thread-wide message
static void throw_on(int rc, const char *what, const lumen_ctx *ctx) {
    if (rc) throw std::runtime_error(std::string(what) + ": " + lumen_last_error(ctx));
}

// ------------------------------------------------------------------ OwnedContext
// the contexts this mirror owns and their ring degrees; written by OwnedContext alone, read through ring_degree
static std::mutex g_contexts_mu;
static std::map<lumen_ctx *, uint32_t> g_contexts;

static lumen_ctx *adopt(lumen_ctx *ctx, uint32_t N) {
    std::lock_guard<std::mutex> lock(g_contexts_mu);
    g_contexts[ctx] = N;
    return ctx;
}
static uint32_t ring_degree(lumen_ctx *ctx) {
    std::lock_guard<std::mutex> lock(g_contexts_mu);
    return g_contexts.at(ctx);
}
size_t LiveContextsForTest() {
    std::lock_guard<std::mutex> lock(g_contexts_mu);
    return g_contexts.size();
}

OwnedContext::OwnedContext(const Parameters &params, int device) {
    lumen_params_desc d;
    memset(&d, 0, sizeof(d));
    d.abi_version = LUMEN_ABI_VERSION;
    d.log_n = (uint32_t)params.LogN;
    d.num_q = (uint32_t)params.Q.size();
    d.num_p = (uint32_t)params.P.size();
    d.plaintext_modulus = params.T;
    d.device = device;
    size_t i = 0;
    for (uint64_t m : params.Q) d.moduli[i++] = m;
    for (uint64_t m : params.P) d.moduli[i++] = m;
    for (size_t k = 0; k < params.Psi.size(); k++) d.psi[k] = params.Psi[k];
    lumen_ctx *ctx = nullptr;
    throw_on(lumen_ctx_create(&d, &ctx), "lumen_ctx_create", nullptr);
    ctx_ = adopt(ctx, (uint32_t)params.N());
}

OwnedContext OwnedContext::Clone() const {
    lumen_ctx *twin = nullptr;
    check(lumen_ctx_clone(ctx_, &twin), "lumen_ctx_clone");
    OwnedContext c;
    c.ctx_ = adopt(twin, ring_degree(ctx_));
    return c;
}

OwnedContext &OwnedContext::operator=(OwnedContext &&o) noexcept {
    std::swap(ctx_, o.ctx_); // what this one held goes with `o`
    return *this;
}

OwnedContext::~OwnedContext() {
    if (!ctx_) return;
    {
        std::lock_guard<std::mutex> lock(g_contexts_mu);
        g_contexts.erase(ctx_);
    }
    lumen_ctx_destroy(ctx_);
}

void OwnedContext::check(int rc, const char *what) const { throw_on(rc, what, ctx_); }

// ------------------------------------------------------------------ parameters
ParametersLiteral GenerateBGVParamsForNTT(int nttSize, int logN, uint64_t plaintextModulus) {
    if (nttSize < 2) throw std::invalid_argument("nttSize must be >= 2");
    if (logN <= 0) throw std::invalid_argument("logN must be positive");
    const uint64_t modulus2N = 2ull << logN;
    if (plaintextModulus % modulus2N != 1)
        throw std::invalid_argument("plaintextModulus T (" + std::to_string(plaintextModulus) +
                                    ") does not satisfy T = 1 (mod 2N) (2N=" + std::to_string(modulus2N) + ")");
    int bits = 0;
    while (bits < 64 && (plaintextModulus >> bits)) bits++;
    const int bufferLevels = bits > 45 ? 0 : -2; // bfv.go:147-151
    const int k = __builtin_ctz((unsigned)nttSize) + bufferLevels;
    ParametersLiteral lit;
    lit.LogN = logN;
    for (int i = 0; i < k; i++) lit.LogQ.push_back(i == 0 ? 58 : 56); // bfv.go:163-169
    lit.LogP = {55, 55};                                              // bfv.go:172-178
    lit.PlaintextModulus = plaintextModulus;
    return lit;
}

static std::vector<uint64_t> ntt_primes(int bits, uint64_t nth_root, int count, uint64_t exclude) {
    std::vector<uint64_t> out;
    const uint64_t base = (1ull << bits) + 1;
    uint64_t up = base, down = base - nth_root;
    while ((int)out.size() < count) {
        uint64_t cand;
        if (up - base <= base - down) cand = up, up += nth_root;
        else cand = down, down -= nth_root;
        if (cand != exclude && core::IsPrime(cand)) out.push_back(cand);
    }
    return out;
}

Parameters Parameters::FromModuli(int logN, std::vector<uint64_t> q, std::vector<uint64_t> p, uint64_t T) {
    Parameters P;
    P.LogN = logN;
    P.Q = std::move(q);
    P.P = std::move(p);
    P.T = T;
    const uint64_t two_n = 2ull << logN;
    for (const auto *v : {&P.Q, &P.P})
        for (uint64_t m : *v) {
            if (m % two_n != 1) throw std::invalid_argument("modulus is not 1 mod 2N");
            P.Psi.push_back(PowMod(core::PrimitiveRoot(m), (m - 1) / two_n, m));
        }
    return P;
}

Parameters Parameters::FromLiteral(const ParametersLiteral &lit) {
    const uint64_t two_n = 2ull << lit.LogN;
    std::vector<uint64_t> q, p;
    int n58 = 0, n56 = 0;
    for (int b : lit.LogQ) (b == 58 ? n58 : n56)++;
    std::vector<uint64_t> q58 = ntt_primes(58, two_n, n58, lit.PlaintextModulus);
    std::vector<uint64_t> q56 = ntt_primes(56, two_n, n56, lit.PlaintextModulus);
    size_t i58 = 0, i56 = 0;
    for (int b : lit.LogQ) q.push_back(b == 58 ? q58[i58++] : q56[i56++]);
    p = ntt_primes(55, two_n, (int)lit.LogP.size(), lit.PlaintextModulus);
    return FromModuli(lit.LogN, q, p, lit.PlaintextModulus);
}

uint64_t Parameters::GaloisElement(int k) const {
    // [LATTIGO-RECALL] rlwe.Parameters.GaloisElement: GaloisGen^(k mod 2N) mod 2N, GaloisGen = 5
    const uint64_t two_n = 2ull << LogN;
    return PowMod(5, (uint64_t)k & (two_n - 1), two_n);
}

std::vector<uint64_t> Parameters::GaloisElementsForInnerSum(int batch, int n) const {
    // [LATTIGO-RECALL] rlwe.GaloisElementsForInnerSum: rotations {i*batch, (n - (n & (2i-1)))*batch} for
    // i = 1, 2, 4, ... < n, collected in a map (Go's iteration order is undefined; ascending here) -- for a
    // power of two {1, 2, ..., n/2, n}*batch; bgv.Parameters appends GaloisElementForRowRotation() when
    // n > N/2.  Rotations by N/2 and by N both give the element 1 (5 has order N/2 modulo 2N): the client
    // really generates and posts keys for them.  Count pinned by the reference's key-size logs
    // (tests/test_oracle_kat.py): 12 / 14 / 15 / 16 for the four configurations.
    std::vector<int> rots;
    for (int i = 1; i < n; i <<= 1) {
        rots.push_back(i * batch);
        rots.push_back((n - (n & ((i << 1) - 1))) * batch);
    }
    std::sort(rots.begin(), rots.end());
    rots.erase(std::unique(rots.begin(), rots.end()), rots.end());
    std::vector<uint64_t> out;
    for (int r : rots) out.push_back(GaloisElement(r));
    if (n > N() / 2) out.push_back((2ull << LogN) - 1);
    return out;
}

std::vector<uint64_t> Parameters::GaloisElementsUsedByInnerSum(int n) const {
    const uint64_t two_n = 2ull << LogN;
    std::vector<uint64_t> out;
    const int span = (n == N()) ? n / 2 : n;
    for (int r = 1; r < span; r <<= 1) out.push_back(GaloisElement(r));
    if (n == N()) out.push_back(two_n - 1);
    return out;
}

// ------------------------------------------------------------------ Ciphertexts
Ciphertexts &Ciphertexts::operator=(Ciphertexts &&o) noexcept {
    if (this != &o) {
        if (set_) lumen_set_destroy(ctx_, set_);
        ctx_ = o.ctx_, set_ = o.set_, Meta = o.Meta;
        o.ctx_ = nullptr, o.set_ = nullptr;
    }
    return *this;
}
Ciphertexts::~Ciphertexts() {
    if (set_) lumen_set_destroy(ctx_, set_);
}
int Ciphertexts::Len() const { return set_ ? (int)lumen_set_count(set_) : 0; }
int Ciphertexts::Level() const { return set_ ? (int)lumen_set_limbs(set_) - 1 : -1; }

Ciphertexts Ciphertexts::Upload(ServerBFV &backend, const std::vector<uint64_t> &host, int count, int level) {
    lumen_set *s = nullptr;
    backend.check(lumen_set_create(backend.Context(), (uint32_t)count, (uint32_t)level + 1, &s), "lumen_set_create");
    Ciphertexts c(backend.Context(), s);
    const size_t want = (size_t)count * 2 * (level + 1) * backend.GetParameters().N();
    if (host.size() != want) throw std::invalid_argument("Upload: host buffer has the wrong size");
    if (count) backend.check(lumen_set_upload(backend.Context(), s, 0, (uint32_t)count, host.data()), "lumen_set_upload");
    return c;
}

std::vector<uint64_t> Ciphertexts::Download() const {
    if (!set_) return {};
    const uint32_t count = lumen_set_count(set_), nl = lumen_set_limbs(set_);
    std::vector<uint64_t> out((size_t)count * 2 * nl * ring_degree(ctx_));
    if (count) throw_on(lumen_set_download(ctx_, set_, 0, count, out.data()), "lumen_set_download", ctx_);
    return out;
}

int ShardedCiphertexts::Len() const {
    int n = 0;
    for (const Ciphertexts &b : Blocks) n += b.Len();
    return n;
}
const MetaData &ShardedCiphertexts::Meta() const {
    static const MetaData none;
    return Blocks.empty() ? none : Blocks[0].Meta;
}
std::vector<uint64_t> ShardedCiphertexts::Download() const {
    std::vector<uint64_t> out;
    for (const Ciphertexts &b : Blocks) {
        const std::vector<uint64_t> part = b.Download();
        out.insert(out.end(), part.begin(), part.end());
    }
    return out;
}

uint64_t RescaledScale(const Parameters &params, uint64_t scale, int fromLevel, int toLevel) {
    // Evaluator.Rescale: Scale <- Scale * q_l^-1 mod T for the dropped limb l
    const uint64_t T = params.T;
    for (int l = fromLevel; l > toLevel; l--) scale = MulMod(scale % T, InvMod(params.Q[(size_t)l] % T, T), T);
    return scale;
}

static std::string hex_float(uint64_t v) {
    // big.Float.Text('x', 39) of an integer below 2^64 held at 128 bits of precision
    // ([LATTIGO-RECALL] rlwe.Scale: ScalePrecision = 128, ScalePrecisionLog10 = ceil(128 / log2(10)) = 39
    // digits after the point): 0x1.<39 hex digits>p+EE
    if (!v) return "0x0p+00";
    int e = 63;
    while (!((v >> e) & 1)) e--;
    const uint64_t frac = e ? (v ^ (1ull << e)) << (64 - e) : 0; // the 64 fraction bits that can be non-zero
    char buf[96];
    snprintf(buf, sizeof(buf), "0x1.%016llx%023dp+%02d", (unsigned long long)frac, 0, e);
    return buf;
}

std::string MetaDataJSON(const MetaData &md, uint64_t plaintextModulus) {
    // [LATTIGO-RECALL rlwe/metadata.go, v6]: MarshalBinary = MarshalJSON of
    //   {"PlaintextMetaData":{"Scale":{"Value":..,"Mod":..},"IsBatched":..,"IsBitReversed":..,"LogDimensions":[..,..]},
    //    "CiphertextMetaData":{"IsNTT":..,"IsMontgomery":..}}
    // booleans and log-dimensions as "0x%02x" strings, both numbers of Scale as hex-float text.  281 bytes here.
    // Its LENGTH is pinned by the reference's size logs (tests/test_oracle_kat.py: 269..311 bytes under the
    // length words of SetCiphertextFormat); rounds 1-2 recalled a 222-byte block (32 digits, decimal Mod, no
    // IsBitReversed), which prints "134 MB" where the reference logs "Marshaled MatR: 135 MB".  The field
    // order inside PlaintextMetaData is not pinned by anything on disk.
    char buf[640];
    snprintf(buf, sizeof(buf),
             "{\"PlaintextMetaData\":{\"Scale\":{\"Value\":\"%s\",\"Mod\":\"%s\"},\"IsBatched\":\"0x%02x\","
             "\"IsBitReversed\":\"0x00\",\"LogDimensions\":[\"0x%02x\",\"0x%02x\"]},\"CiphertextMetaData\":{\"IsNTT\":\"0x%02x\","
             "\"IsMontgomery\":\"0x%02x\"}}",
             hex_float(md.Scale).c_str(), hex_float(plaintextModulus).c_str(), md.IsBatched ? 1 : 0,
             (unsigned)md.LogRows, (unsigned)md.LogCols, md.IsNTT ? 1 : 0, md.IsMontgomery ? 1 : 0);
    return buf;
}

// the framing ct.WriteTo gives a ciphertext of this MetaData and level, installed on one context
static void set_format(lumen_ctx *ctx, const MetaData &md, int level, uint64_t T, uint32_t N) {
    auto le64 = [](std::vector<uint8_t> &v, uint64_t x) {
        for (int i = 0; i < 8; i++) v.push_back((uint8_t)(x >> (8 * i)));
    };
    const std::string json = MetaDataJSON(md, T);
    std::vector<uint8_t> head(json.begin(), json.end()), poly, limb;
    le64(head, 2); // structs.Vector[ring.Poly]: two polynomials
    le64(poly, (uint64_t)level + 1);
    le64(limb, (uint64_t)N);
    throw_on(lumen_leaf_format_set(ctx, head.data(), (uint32_t)head.size(), poly.data(), (uint32_t)poly.size(), limb.data(),
                                   (uint32_t)limb.size()),
             "lumen_leaf_format_set", ctx);
}

void SetCiphertextFormat(ServerBFV &backend, const MetaData &md, int level) {
    set_format(backend.Context(), md, level, backend.GetParameters().T, (uint32_t)backend.GetParameters().N());
}

// ------------------------------------------------------------------ host ring helpers
static void host_ntt(std::vector<uint64_t> &a, uint64_t q, uint64_t psi, int logN, bool inverse) {
    // [LATTIGO-RECALL] SubRing.NTT / INTT (negacyclic, bit-reversed output); host-side use only for
    // the single plaintexts / the one zero column the host creates per call
    const uint32_t N = 1u << logN;
    std::vector<uint64_t> tw(N);
    const uint64_t root = inverse ? InvMod(psi, q) : psi;
    uint64_t cur = 1;
    for (uint32_t j = 0; j < N; j++) {
        tw[core::BitReverse64(j, logN)] = cur;
        cur = MulMod(cur, root, q);
    }
    if (!inverse) {
        uint32_t t = N >> 1;
        for (uint32_t m = 1; m < N; m <<= 1, t >>= 1)
            for (uint32_t i = 0; i < m; i++)
                for (uint32_t j = 2 * i * t; j < 2 * i * t + t; j++) {
                    const uint64_t u = a[j], v = MulMod(a[j + t], tw[m + i], q);
                    a[j] = u + v >= q ? u + v - q : u + v;
                    a[j + t] = u >= v ? u - v : u + q - v;
                }
    } else {
        uint32_t t = 1;
        for (uint32_t m = N >> 1; m >= 1; m >>= 1, t <<= 1)
            for (uint32_t i = 0; i < m; i++)
                for (uint32_t j = 2 * i * t; j < 2 * i * t + t; j++) {
                    const uint64_t u = a[j], v = a[j + t];
                    a[j] = u + v >= q ? u + v - q : u + v;
                    a[j + t] = MulMod(u >= v ? u - v : u + q - v, tw[m + i], q);
                }
        const uint64_t ninv = InvMod(N % q, q);
        for (uint64_t &x : a) x = MulMod(x, ninv, q);
    }
}

// ------------------------------------------------------------------ ServerBFV
void OsRandom(uint8_t *out, size_t n) {
    size_t got = 0;
    while (got < n) {
        const ssize_t r = getrandom(out + got, n - got, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            throw std::runtime_error("getrandom failed: no OS entropy for the encryption seed");
        }
        got += (size_t)r;
    }
}

void ServerBFV::check(int rc, const char *what) const { ctx_.check(rc, what); }

// the encoder's root: a primitive 2N-th root of unity modulo T
static uint64_t encoder_root(const Parameters &params) {
    return PowMod(core::PrimitiveRoot(params.T), (params.T - 1) / (2ull << params.LogN), params.T);
}

// rlwe.MetaData of a fresh encryption: Scale 1, NTT domain, batched 2 x N/2 slots
static MetaData fresh_meta(const Parameters &params) {
    MetaData md;
    md.LogCols = params.LogN - 1;
    return md;
}

ServerBFV::ServerBFV(core::PrimeField *plaintextField, const Parameters &params, std::vector<uint64_t> pk,
                     const std::map<uint64_t, std::vector<uint64_t>> &evk, int device)
    : ptField_(plaintextField), params_(params), pk_(std::move(pk)), ctx_(params, device), psiT_(encoder_root(params)) {
    // a throw below unwinds ctx_: the context and every key already loaded leave the device
    check(lumen_field_set(Context(), plaintextField->RootsForward().data(), (uint32_t)plaintextField->N()), "lumen_field_set");
    for (const auto &kv : evk) check(lumen_load_galois_key(Context(), kv.first, kv.second.data()), "lumen_load_galois_key");
    check(lumen_load_public_key(Context(), pk_.data()), "lumen_load_public_key");
    check(lumen_encoder_set(Context(), psiT_), "lumen_encoder_set");
    // the reference keys Lattigo's sampler from crypto/rand: all encryption randomness (u, e0, e1 of every
    // ciphertext this server makes) is the ChaCha20 stream under this key, so the key comes from the
    // kernel's CSPRNG and from nowhere else -- no user-space generator in between
    enc_ = std::make_shared<EncryptorState>();
    OsRandom(enc_->seed, sizeof(enc_->seed));
    // encoder tables ([LATTIGO-RECALL] bgv.Encoder: slot i of row 0 sits at 5^i, row 1 at -5^i)
    const uint64_t two_n = 2ull << params.LogN;
    const int N = params.N(), row = N >> 1;
    slot_index_.resize(N);
    uint64_t pos = 1;
    for (int s = 0; s < row; s++) {
        slot_index_[s] = (uint32_t)core::BitReverse64((pos - 1) >> 1, params.LogN);
        slot_index_[s | row] = (uint32_t)core::BitReverse64((two_n - pos - 1) >> 1, params.LogN);
        pos = (pos * 5) & (two_n - 1);
    }
}

ServerBFV::ServerBFV(ServerBFV &src, OwnedContext clone)
    : ptField_(src.ptField_), params_(src.params_), pk_(src.pk_), ctx_(std::move(clone)), psiT_(src.psiT_),
      slot_index_(src.slot_index_), rs_(src.rs_), enc_(src.enc_) {}

std::unique_ptr<ServerBFV> ServerBFV::CopyNew() { return std::unique_ptr<ServerBFV>(new ServerBFV(*this, ctx_.Clone())); }

ServerBFV::~ServerBFV() = default;

int ServerBFV::MulCounter() const { return (int)lumen_mul_counter(Context()); }

// ------------------------------------------------------------------ ClientBFV
void ClientBFV::check(int rc, const char *what) const { ctx_.check(rc, what); }
int ClientBFV::MulCounter() const { return (int)lumen_mul_counter(Context()); }

ClientBFV::ClientBFV(core::PrimeField *plaintextField, const Parameters &params, const std::vector<uint64_t> &sk, int device)
    : ptField_(plaintextField), params_(params), device_(device) {
    const size_t N = (size_t)params.N(), L = params.Q.size();
    if (sk.size() < L * N) throw std::invalid_argument("NewClientBFV: the secret key has fewer than L * N residues");
    ctx_ = OwnedContext(params, device);
    check(lumen_encoder_set(Context(), encoder_root(params)), "lumen_encoder_set");
    check(lumen_load_secret_key(Context(), sk.data()), "lumen_load_secret_key");
    encSeed_ = std::make_shared<KeySeedBytes>();
    OsRandom(encSeed_->b, sizeof(encSeed_->b));
}

ClientBFV::ClientBFV(core::PrimeField *plaintextField, const Parameters &params, int device)
    : ptField_(plaintextField), params_(params), ctx_(params, device), device_(device) {
    check(lumen_encoder_set(Context(), encoder_root(params)), "lumen_encoder_set");
    keySeed_ = std::make_shared<KeySeedBytes>();
    OsRandom(keySeed_->b, sizeof(keySeed_->b));
    keyForms_ = std::make_shared<KeyForms>(); // the keygen seed's one public seed, for as long as the seed lives
    do OsRandom(keyForms_->aSeed.data(), keyForms_->aSeed.size());
    while (!memcmp(keyForms_->aSeed.data(), keySeed_->b, 32)); // the library refuses equal seeds; 2^-256
    check(lumen_keygen_secret(Context(), keySeed_->b, nullptr), "lumen_keygen_secret");
    encSeed_ = std::make_shared<KeySeedBytes>(); // its own draw: a keygen seed keys nothing else
    OsRandom(encSeed_->b, sizeof(encSeed_->b));
}

std::unique_ptr<ClientBFV> ClientBFV::NewWithGeneratedSecret(core::PrimeField *plaintextField, const Parameters &params,
                                                             int device) {
    return std::unique_ptr<ClientBFV>(new ClientBFV(plaintextField, params, device));
}

const uint8_t *ClientBFV::KeySeed() const {
    if (!keySeed_) throw std::invalid_argument("ClientBFV: the secret key was handed in, not generated on the device");
    return keySeed_->b;
}

const std::array<uint8_t, 32> &ClientBFV::PublicKeySeed() const {
    if (!keyForms_) throw std::invalid_argument("ClientBFV: the secret key was handed in, not generated on the device");
    return keyForms_->aSeed;
}

void ClientBFV::ClaimKeyForm(const std::vector<uint64_t> &keyIds, bool seeded) {
    if (!keyForms_) throw std::invalid_argument("ClientBFV: the secret key was handed in, not generated on the device");
    std::lock_guard<std::mutex> lock(keyForms_->mu);
    for (uint64_t id : keyIds) {
        const auto it = keyForms_->seeded.find(id);
        if (it != keyForms_->seeded.end() && it->second != seeded)
            throw std::logic_error("KeyGenerator: key id " + std::to_string(id) + " was already generated in the " +
                                   (it->second ? "seeded" : "full") + " form; both forms together reveal the secret key");
    }
    for (uint64_t id : keyIds) keyForms_->seeded[id] = seeded;
}

std::vector<uint64_t> ClientBFV::SecretKeyForTest() {
    std::vector<uint64_t> sk((params_.Q.size() + params_.P.size()) * (size_t)params_.N());
    check(lumen_keygen_secret(Context(), KeySeed(), sk.data()), "lumen_keygen_secret");
    return sk;
}

ClientBFV::ClientBFV(ClientBFV &src, OwnedContext clone)
    : ptField_(src.ptField_), params_(src.params_), ctx_(std::move(clone)), device_(src.device_), keySeed_(src.keySeed_),
      keyForms_(src.keyForms_), encSeed_(src.encSeed_) {}

std::unique_ptr<ClientBFV> ClientBFV::CopyNew() { return std::unique_ptr<ClientBFV>(new ClientBFV(*this, ctx_.Clone())); }

ClientBFV::~ClientBFV() = default;

// Encryptor(sk).EncryptNew (fhe/bfv.go:77; vdec/batching_test.go:56) of whole columns on the device
Ciphertexts ClientBFV::EncryptColumnsUnderSeedForTest(const std::vector<uint64_t> &values, int rows, int count,
                                                      const std::array<uint8_t, 32> &aSeed, uint64_t firstIndex) {
    if (rows < 0 || count < 0 || (size_t)rows * count != values.size()) throw std::invalid_argument("EncryptColumnsNew: size mismatch");
    lumen_set *set = nullptr;
    check(lumen_encrypt_sk_values(Context(), values.data(), (uint32_t)rows, (uint32_t)count, encSeed_->b, aSeed.data(), firstIndex,
                                  &set),
          "lumen_encrypt_sk_values");
    return Ciphertexts(Context(), set, fresh_meta(params_));
}

Ciphertexts ClientBFV::EncryptColumnsNew(const std::vector<uint64_t> &values, int rows, int count) {
    std::array<uint8_t, 32> aSeed;
    OsRandom(aSeed.data(), aSeed.size()); // fresh per call: (seed, index) never meets two messages
    return EncryptColumnsUnderSeedForTest(values, rows, count, aSeed, 0);
}

SeededCiphertexts ClientBFV::EncryptColumnsSeeded(const std::vector<uint64_t> &values, int rows, int count) {
    if (rows < 0 || count < 0 || (size_t)rows * count != values.size())
        throw std::invalid_argument("EncryptColumnsSeeded: size mismatch");
    SeededCiphertexts out;
    OsRandom(out.ASeed.data(), out.ASeed.size());
    out.Count = count;
    out.C0.resize((size_t)count * params_.Q.size() * (size_t)params_.N());
    check(lumen_encrypt_sk_seeded(Context(), values.data(), (uint32_t)rows, (uint32_t)count, encSeed_->b, out.ASeed.data(),
                                  out.FirstIndex, out.C0.data()),
          "lumen_encrypt_sk_seeded");
    return out;
}

// ------------------------------------------------------------------ KeyGenerator (cmd/client/main.go:74-81)
static size_t evk_words(const Parameters &P) {
    const size_t L = P.Q.size(), K = P.P.size();
    return K ? (L + K - 1) / K * 2 * (L + K) * (size_t)P.N() : 0;
}

// the sampling contract's key ids (include/lumenos_hip.h)
static const uint64_t KEY_ID_RELIN = 2, KEY_ID_GALOIS = 0x10000;
static std::vector<uint64_t> galois_key_ids(const std::vector<uint64_t> &els) {
    std::vector<uint64_t> ids;
    for (uint64_t g : els) ids.push_back(KEY_ID_GALOIS + g);
    return ids;
}

KeyGenerator::KeyGenerator(ClientBFV &client) : client_(client) {
    if (!client.HasGeneratedSecret())
        throw std::invalid_argument("NewKeyGenerator: the client's secret key was handed in, not generated on the device");
}

std::vector<uint64_t> KeyGenerator::GenKeyPairNew() {
    const Parameters &P = client_.GetParameters();
    std::vector<uint64_t> pk((size_t)2 * (P.Q.size() + P.P.size()) * (size_t)P.N());
    client_.check(lumen_keygen_public(client_.Context(), client_.KeySeed(), pk.data()), "lumen_keygen_public");
    return pk;
}

std::vector<uint64_t> KeyGenerator::GenRelinearizationKeyNew(uint32_t flags) {
    client_.ClaimKeyForm({KEY_ID_RELIN}, false);
    std::vector<uint64_t> rlk(std::max<size_t>(evk_words(client_.GetParameters()), 1));
    client_.check(lumen_keygen_relin(client_.Context(), client_.KeySeed(), rlk.data(), flags), "lumen_keygen_relin");
    return rlk;
}

std::map<uint64_t, std::vector<uint64_t>> KeyGenerator::GenGaloisKeysNew(const std::vector<uint64_t> &galEls, uint32_t flags) {
    const std::set<uint64_t> distinct(galEls.begin(), galEls.end());
    const std::vector<uint64_t> els(distinct.begin(), distinct.end());
    client_.ClaimKeyForm(galois_key_ids(els), false);
    const size_t words = evk_words(client_.GetParameters());
    // one page-locked block for the whole batch: the transfer is a single DMA
    WireBuffer flat(std::max<size_t>(els.size() * words, 1) * 8);
    uint64_t *w = reinterpret_cast<uint64_t *>(flat.data());
    client_.check(lumen_keygen_galois(client_.Context(), client_.KeySeed(), els.data(), (uint32_t)els.size(), w, flags),
                  "lumen_keygen_galois");
    std::map<uint64_t, std::vector<uint64_t>> out;
    for (size_t i = 0; i < els.size(); i++) out[els[i]].assign(w + i * words, w + (i + 1) * words);
    return out;
}

KeySet KeyGenerator::GenKeySetNew(int rows, uint32_t flags, bool withRelin) {
    KeySet ks;
    if (withRelin) ks.Rlk = GenRelinearizationKeyNew(flags);
    ks.Flags = flags;
    ks.Pk = GenKeyPairNew();
    ks.GaloisElements = client_.GetParameters().GaloisElementsForInnerSum(1, rows);
    const auto keys = GenGaloisKeysNew(ks.GaloisElements, flags);
    for (uint64_t g : ks.GaloisElements) ks.GaloisKeys.push_back(keys.at(g));
    return ks;
}

// ---- seeded switching keys: b halves + one public seed per set
static size_t seeded_evk_words(const Parameters &P) { return evk_words(P) / 2; }

SeededKeySet KeyGenerator::GenGaloisKeysSeeded(const std::vector<uint64_t> &galEls, uint32_t flags) {
    const std::set<uint64_t> distinct(galEls.begin(), galEls.end());
    const std::vector<uint64_t> els(distinct.begin(), distinct.end());
    const size_t words = seeded_evk_words(client_.GetParameters());
    SeededKeySet set;
    set.Flags = flags;
    set.ASeed = client_.PublicKeySeed();
    client_.ClaimKeyForm(galois_key_ids(els), true);
    WireBuffer flat(std::max<size_t>(els.size() * words, 1) * 8);
    uint64_t *w = reinterpret_cast<uint64_t *>(flat.data());
    client_.check(lumen_keygen_galois_seeded(client_.Context(), client_.KeySeed(), set.ASeed.data(), els.data(),
                                             (uint32_t)els.size(), w, flags),
                  "lumen_keygen_galois_seeded");
    for (size_t i = 0; i < els.size(); i++) set.GaloisB[els[i]].assign(w + i * words, w + (i + 1) * words);
    return set;
}

void KeyGenerator::GenRelinearizationKeySeeded(SeededKeySet &set) {
    if (set.GaloisB.empty() && set.RlkB.empty()) set.ASeed = client_.PublicKeySeed();
    if (set.ASeed != client_.PublicKeySeed())
        throw std::invalid_argument("GenRelinearizationKeySeeded: the set is under another public seed than this client's");
    client_.ClaimKeyForm({KEY_ID_RELIN}, true);
    std::vector<uint64_t> b(std::max<size_t>(seeded_evk_words(client_.GetParameters()), 1));
    client_.check(lumen_keygen_relin_seeded(client_.Context(), client_.KeySeed(), set.ASeed.data(), b.data(), set.Flags),
                  "lumen_keygen_relin_seeded");
    set.RlkB = std::move(b);
}

SeededKeySet KeyGenerator::GenKeySetSeeded(int rows, uint32_t flags, bool withRelin) {
    SeededKeySet set = GenGaloisKeysSeeded(client_.GetParameters().GaloisElementsForInnerSum(1, rows), flags);
    if (withRelin) GenRelinearizationKeySeeded(set);
    set.Pk = GenKeyPairNew();
    return set;
}

void ServerBFV::LoadSeededKeys(const SeededKeySet &keys) {
    const size_t words = seeded_evk_words(params_);
    for (const auto &kv : keys.GaloisB)
        if (kv.second.size() != words || kv.second.empty())
            throw std::invalid_argument("LoadSeededKeys: a Galois key is not [beta][L+K][N]");
    if (!keys.RlkB.empty() && keys.RlkB.size() != words)
        throw std::invalid_argument("LoadSeededKeys: the relinearisation key is not [beta][L+K][N]");
    for (const auto &kv : keys.GaloisB)
        check(lumen_load_galois_key_seeded(Context(), kv.first, kv.second.data(), keys.ASeed.data(), keys.Flags),
              "lumen_load_galois_key_seeded");
    if (!keys.RlkB.empty())
        check(lumen_load_relin_key_seeded(Context(), keys.RlkB.data(), keys.ASeed.data(), keys.Flags), "lumen_load_relin_key_seeded");
}

std::unique_ptr<ServerBFV> ServerBFV::NewFromKeySet(core::PrimeField *plaintextField, const Parameters &params, int rows,
                                                    const SeededKeySet &keys, int device) {
    for (uint64_t g : params.GaloisElementsForInnerSum(1, rows))
        if (!keys.GaloisB.count(g))
            throw std::invalid_argument("NewFromKeySet: the seeded set lacks an element of GaloisElementsForInnerSum(1, rows)");
    if (keys.Pk.size() != (size_t)2 * (params.Q.size() + params.P.size()) * (size_t)params.N())
        throw std::invalid_argument("NewFromKeySet: the public key is not [2][L+K][N]");
    std::unique_ptr<ServerBFV> s(new ServerBFV(plaintextField, params, keys.Pk, {}, device));
    s->LoadSeededKeys(keys);
    return s;
}

RingSwitchClient NewRingSwitchClient(ClientBFV &client, int logN, int baseTwoDecomposition) {
    if (logN < 0 || logN > 30) throw std::invalid_argument("NewRingSwitchClient: logN out of range");
    const Parameters &P = client.GetParameters();
    RingSwitchClient rs;
    rs.LogN = logN, rs.BaseTwoDecomposition = baseTwoDecomposition;
    rs.SkNew.resize((size_t)1 << logN);
    rs.Evk.resize((size_t)lumen_ringswitch_rns_digits(client.Context()) *
                  lumen_ringswitch_digits(client.Context(), (uint32_t)baseTwoDecomposition) * 2 * (P.Q.size() + P.P.size()) *
                  (size_t)P.N());
    client.check(lumen_keygen_ringswitch(client.Context(), client.KeySeed(), (uint32_t)logN, (uint32_t)baseTwoDecomposition,
                                         rs.Evk.data(), rs.Evk.size(), rs.SkNew.data()),
                 "lumen_keygen_ringswitch");
    return rs;
}

std::unique_ptr<ServerBFV> ServerBFV::NewFromKeySet(core::PrimeField *plaintextField, const Parameters &params, int rows,
                                                    const KeySet &keys, int device) {
    if (keys.GaloisElements != params.GaloisElementsForInnerSum(1, rows))
        throw std::invalid_argument("NewFromKeySet: the Galois elements are not GaloisElementsForInnerSum(1, rows)");
    if (keys.Pk.size() != (size_t)2 * (params.Q.size() + params.P.size()) * (size_t)params.N())
        throw std::invalid_argument("NewFromKeySet: the public key is not [2][L+K][N]");
    if (keys.GaloisKeys.size() != keys.GaloisElements.size())
        throw std::invalid_argument("NewFromKeySet: one Galois key per element expected");
    for (const auto &k : keys.GaloisKeys)
        if (k.size() != evk_words(params)) throw std::invalid_argument("NewFromKeySet: a Galois key has the wrong size");
    std::unique_ptr<ServerBFV> s(new ServerBFV(plaintextField, params, keys.Pk, {}, device));
    for (size_t i = 0; i < keys.GaloisKeys.size(); i++)
        s->check(lumen_load_galois_key_ex(s->Context(), keys.GaloisElements[i], keys.GaloisKeys[i].data(), keys.Flags),
                 "lumen_load_galois_key_ex");
    if (!keys.Rlk.empty()) s->SetRelinearizationKey(keys.Rlk, keys.Flags);
    return s;
}

void ServerBFV::SetRelinearizationKey(const std::vector<uint64_t> &rlk, uint32_t flags) {
    if (rlk.size() != evk_words(params_) || rlk.empty())
        throw std::invalid_argument("SetRelinearizationKey: the key is not [beta][b|a][L+K][N]");
    check(lumen_load_relin_key(Context(), rlk.data(), flags), "lumen_load_relin_key");
}

Ciphertexts ServerBFV::MulRelinNew(const Ciphertexts &a, const Ciphertexts &b) {
    if (!a.Handle() || !b.Handle()) throw std::invalid_argument("MulRelinNew: an operand holds no ciphertexts");
    lumen_set *set = nullptr;
    check(lumen_mul_relin(Context(), a.Handle(), b.Handle(), &set), "lumen_mul_relin");
    MetaData md = a.Meta;
    const uint64_t T = params_.T;
    md.Scale = MulMod(a.Scale() % T, b.Scale() % T, T); // bgv: Scale_a * Scale_b
    return Ciphertexts(Context(), set, md);
}

Ciphertexts ServerBFV::DotRelinNew(const Ciphertexts &a, const Ciphertexts &b, uint32_t n) {
    if (!a.Handle() || !b.Handle()) throw std::invalid_argument("DotRelinNew: an operand holds no ciphertexts");
    if (n == 0) throw std::invalid_argument("DotRelinNew: a sum of no terms (n == 0)");
    if (a.Len() % (int)n) throw std::invalid_argument("DotRelinNew: the first operand's count is no multiple of n");
    if (b.Len() != a.Len() && b.Len() != (int)n)
        throw std::invalid_argument("DotRelinNew: the second operand has neither the first one's count nor n ciphertexts");
    if (a.Level() != b.Level()) throw std::invalid_argument("DotRelinNew: the operands have different levels");
    lumen_set *set = nullptr;
    check(lumen_mul_relin_dot(Context(), a.Handle(), b.Handle(), n, &set), "lumen_mul_relin_dot");
    MetaData md = a.Meta;
    const uint64_t T = params_.T;
    md.Scale = MulMod(a.Scale() % T, b.Scale() % T, T); // bgv: Scale_a * Scale_b, MulRelinNew's
    return Ciphertexts(Context(), set, md);
}

void ServerBFV::LoadGaloisKeys(const std::map<uint64_t, std::vector<uint64_t>> &keys, uint32_t flags) {
    for (const auto &kv : keys)
        if (kv.second.size() != evk_words(params_) || kv.second.empty())
            throw std::invalid_argument("LoadGaloisKeys: a Galois key is not [beta][b|a][L+K][N]");
    for (const auto &kv : keys)
        check(lumen_load_galois_key_ex(Context(), kv.first, kv.second.data(), flags), "lumen_load_galois_key_ex");
}

Ciphertexts ServerBFV::AutomorphismNew(const Ciphertexts &ct, uint64_t galEl) {
    if (!ct.Handle()) throw std::invalid_argument("AutomorphismNew: the operand holds no ciphertexts");
    lumen_set *set = nullptr;
    check(lumen_automorphism(Context(), ct.Handle(), galEl, &set), "lumen_automorphism");
    return Ciphertexts(Context(), set, ct.Meta);
}

Ciphertexts ServerBFV::RotateColumnsNew(const Ciphertexts &ct, int k) {
    if (!ct.Handle()) throw std::invalid_argument("RotateColumnsNew: the operand holds no ciphertexts");
    lumen_set *set = nullptr;
    check(lumen_rotate_columns(Context(), ct.Handle(), k, &set), "lumen_rotate_columns");
    return Ciphertexts(Context(), set, ct.Meta);
}

Ciphertexts ServerBFV::RotateRowsNew(const Ciphertexts &ct) {
    if (!ct.Handle()) throw std::invalid_argument("RotateRowsNew: the operand holds no ciphertexts");
    lumen_set *set = nullptr;
    check(lumen_rotate_rows(Context(), ct.Handle(), &set), "lumen_rotate_rows");
    return Ciphertexts(Context(), set, ct.Meta);
}

std::map<int, Ciphertexts> ServerBFV::RotateHoistedNew(const Ciphertexts &ct, const std::vector<int> &rotations) {
    if (!ct.Handle()) throw std::invalid_argument("RotateHoistedNew: the operand holds no ciphertexts");
    const std::set<int> distinct(rotations.begin(), rotations.end()); // the reference fills a map: one entry per rotation
    const std::vector<int> rots(distinct.begin(), distinct.end());
    std::vector<uint64_t> els;
    for (int r : rots) els.push_back(lumen_galois_element(Context(), r));
    std::vector<lumen_set *> sets(std::max<size_t>(rots.size(), 1), nullptr);
    const uint64_t none = 1; // (the list pointer is never NULL, even for no rotation at all)
    check(lumen_rotate_hoisted(Context(), ct.Handle(), els.empty() ? &none : els.data(), (uint32_t)els.size(), sets.data()),
          "lumen_rotate_hoisted");
    std::map<int, Ciphertexts> out;
    for (size_t i = 0; i < rots.size(); i++) out.emplace(rots[i], Ciphertexts(Context(), sets[i], ct.Meta));
    return out;
}

// ---- the diagonal linear transform
LinearTransformation &LinearTransformation::operator=(LinearTransformation &&o) noexcept {
    if (this != &o) {
        if (lt_) lumen_lintrans_destroy(ctx_, lt_);
        ctx_ = o.ctx_, lt_ = o.lt_, level_ = o.level_, diagonals_ = o.diagonals_;
        o.ctx_ = nullptr, o.lt_ = nullptr, o.level_ = -1, o.diagonals_ = 0;
    }
    return *this;
}

LinearTransformation::~LinearTransformation() {
    if (lt_) lumen_lintrans_destroy(ctx_, lt_);
}

std::vector<uint64_t> LinearTransformation::GaloisElements() const {
    std::vector<uint64_t> els(std::max<size_t>(2 * diagonals_, 1)); // double-hoisted: a baby's and a giant's per diagonal
    els.resize(lumen_lintrans_galois_elements(lt_, els.data()));
    return els;
}

// both forms: babySteps < 0 single-hoisted, 0 the best count of baby steps, > 0 that count
LinearTransformation ServerBFV::newLinearTransformation(const std::map<int, std::vector<uint64_t>> &diagonals, int level, int babySteps,
                                                        const char *what) {
    if (diagonals.empty()) throw std::invalid_argument(std::string(what) + ": no diagonal");
    if (level < 0 || level >= (int)params_.Q.size()) throw std::invalid_argument(std::string(what) + ": no such level");
    std::vector<int64_t> ks;
    std::vector<uint64_t> pts;
    for (const auto &kv : diagonals) {
        const Plaintext pt = EncodeQP(kv.second, level);
        ks.push_back(kv.first);
        pts.insert(pts.end(), pt.Value.begin(), pt.Value.end());
    }
    LinearTransformation lt;
    if (babySteps < 0) {
        check(lumen_lintrans_load(Context(), ks.data(), pts.data(), (uint32_t)ks.size(), (uint32_t)level + 1, &lt.lt_), "lumen_lintrans_load");
    } else {
        uint32_t n1 = (uint32_t)babySteps;
        if (!n1) {
            n1 = lumen_lintrans_best_baby_steps((uint32_t)params_.LogN, ks.data(), (uint32_t)ks.size());
            if (!n1) throw std::invalid_argument(std::string(what) + ": a diagonal outside (-N/2, N/2)");
        }
        check(lumen_lintrans_load_bsgs(Context(), ks.data(), pts.data(), (uint32_t)ks.size(), (uint32_t)level + 1, n1, &lt.lt_),
              "lumen_lintrans_load_bsgs");
    }
    lt.ctx_ = Context(), lt.level_ = level, lt.diagonals_ = ks.size();
    return lt;
}

LinearTransformation ServerBFV::NewLinearTransformation(const std::map<int, std::vector<uint64_t>> &diagonals, int level) {
    return newLinearTransformation(diagonals, level, -1, "NewLinearTransformation");
}

LinearTransformation ServerBFV::NewLinearTransformationBSGS(const std::map<int, std::vector<uint64_t>> &diagonals, int level, int babySteps) {
    if (babySteps < 0) throw std::invalid_argument("NewLinearTransformationBSGS: a negative number of baby steps");
    return newLinearTransformation(diagonals, level, babySteps, "NewLinearTransformationBSGS");
}

Ciphertexts ServerBFV::LinearTransformationNew(const Ciphertexts &ct, const LinearTransformation &lt) {
    if (!ct.Handle()) throw std::invalid_argument("LinearTransformationNew: the operand holds no ciphertexts");
    if (!lt.Handle()) throw std::invalid_argument("LinearTransformationNew: an empty transformation");
    lumen_set *set = nullptr;
    check(lumen_linear_transform(Context(), ct.Handle(), lt.Handle(), &set), "lumen_linear_transform");
    return Ciphertexts(Context(), set, ct.Meta);
}

std::vector<Ciphertexts> ServerBFV::LinearTransformationsNew(const Ciphertexts &ct, const std::vector<const LinearTransformation *> &lts) {
    if (!ct.Handle()) throw std::invalid_argument("LinearTransformationsNew: the operand holds no ciphertexts");
    std::vector<const lumen_lintrans *> hs;
    for (const LinearTransformation *lt : lts) {
        if (!lt || !lt->Handle()) throw std::invalid_argument("LinearTransformationsNew: an empty transformation");
        hs.push_back(lt->Handle());
    }
    std::vector<lumen_set *> sets(std::max<size_t>(hs.size(), 1), nullptr);
    const lumen_lintrans *none = nullptr; // (the list pointer is never NULL, even for no transformation at all)
    check(lumen_linear_transforms(Context(), ct.Handle(), hs.empty() ? &none : hs.data(), (uint32_t)hs.size(), sets.data()),
          "lumen_linear_transforms");
    std::vector<Ciphertexts> out;
    for (size_t i = 0; i < hs.size(); i++) out.emplace_back(Context(), sets[i], ct.Meta);
    return out;
}

Ciphertexts ServerBFV::InnerSumNew(const Ciphertexts &ct, int batchSize, int n) {
    if (!ct.Handle()) throw std::invalid_argument("InnerSumNew: the operand holds no ciphertexts");
    if (batchSize < 1 || n < 1) throw std::invalid_argument("InnerSumNew: batchSize and n must be at least 1");
    lumen_set *set = nullptr;
    check(lumen_inner_sum_general(Context(), ct.Handle(), (uint32_t)batchSize, (uint32_t)n, &set), "lumen_inner_sum_general");
    return Ciphertexts(Context(), set, ct.Meta);
}

// ---- the embedded evaluator's linear operations, for ServerBFV and ClientBFV alike
namespace {
void need_set(const char *what, const Ciphertexts &ct) {
    if (!ct.Handle()) throw std::invalid_argument(std::string(what) + ": an operand holds no ciphertexts");
}
void need_scales(const char *what, uint64_t a, uint64_t b) {
    if (a != b)
        throw std::invalid_argument(std::string(what) + ": operands of scale " + std::to_string(a) + " and " + std::to_string(b) +
                                    ": scales are not matched here, bring the operands to one scale first");
}
} // namespace

void LinearEvaluator::finish(lumen_set *set, const MetaData &md, Ciphertexts &out) {
    if (out.Handle() == set)
        out.Meta = md; // written in place
    else
        out = Ciphertexts(Context(), set, md);
}

void LinearEvaluator::Add(const Ciphertexts &a, const Ciphertexts &b, Ciphertexts &out) {
    need_set("Add", a), need_set("Add", b), need_scales("Add", a.Scale(), b.Scale());
    const MetaData md = a.Meta;
    lumen_set *set = out.Handle();
    check(lumen_add(Context(), a.Handle(), b.Handle(), &set), "lumen_add");
    finish(set, md, out);
}

void LinearEvaluator::Sub(const Ciphertexts &a, const Ciphertexts &b, Ciphertexts &out) {
    need_set("Sub", a), need_set("Sub", b), need_scales("Sub", a.Scale(), b.Scale());
    const MetaData md = a.Meta;
    lumen_set *set = out.Handle();
    check(lumen_sub(Context(), a.Handle(), b.Handle(), &set), "lumen_sub");
    finish(set, md, out);
}

Ciphertexts LinearEvaluator::AddNew(const Ciphertexts &a, const Ciphertexts &b) {
    Ciphertexts out;
    Add(a, b, out);
    return out;
}

Ciphertexts LinearEvaluator::SubNew(const Ciphertexts &a, const Ciphertexts &b) {
    Ciphertexts out;
    Sub(a, b, out);
    return out;
}

void LinearEvaluator::Mul(const Ciphertexts &ct, uint64_t w, Ciphertexts &out) {
    need_set("Mul", ct);
    const MetaData md = ct.Meta; // a scalar leaves the scale alone
    lumen_set *set = out.Handle();
    check(lumen_mul_scalar(Context(), ct.Handle(), w, &set), "lumen_mul_scalar");
    finish(set, md, out);
}

Ciphertexts LinearEvaluator::MulNew(const Ciphertexts &ct, uint64_t w) {
    Ciphertexts out;
    Mul(ct, w, out);
    return out;
}

void LinearEvaluator::MulThenAdd(const Ciphertexts &ct, uint64_t w, Ciphertexts &acc) {
    need_set("MulThenAdd", ct), need_set("MulThenAdd", acc), need_scales("MulThenAdd", acc.Scale(), ct.Scale());
    check(lumen_mul_scalar_then_add(Context(), ct.Handle(), w, acc.Handle()), "lumen_mul_scalar_then_add");
}

Ciphertexts LinearEvaluator::LinearCombinationNew(const std::vector<const Ciphertexts *> &in, const std::vector<uint64_t> &w) {
    if (in.empty() || in.size() != w.size())
        throw std::invalid_argument("LinearCombinationNew: " + std::to_string(in.size()) + " operands for " + std::to_string(w.size()) +
                                    " scalars");
    std::vector<const lumen_set *> sets;
    for (const Ciphertexts *c : in) {
        if (!c) throw std::invalid_argument("LinearCombinationNew: an operand is null");
        need_set("LinearCombinationNew", *c), need_scales("LinearCombinationNew", in[0]->Scale(), c->Scale());
        sets.push_back(c->Handle());
    }
    lumen_set *set = nullptr;
    check(lumen_linear_combination(Context(), sets.data(), w.data(), (uint32_t)sets.size(), &set), "lumen_linear_combination");
    return Ciphertexts(Context(), set, in[0]->Meta);
}

// the first limbs of a plaintext at ct's level or above
const uint64_t *LinearEvaluator::limbs_for(const char *what, const Ciphertexts &ct, const Plaintext &pt) const {
    need_set(what, ct);
    const size_t N = (size_t)GetParameters().N();
    if (pt.Level < ct.Level() || pt.Value.size() != (size_t)(pt.Level + 1) * N)
        throw std::invalid_argument(std::string(what) + ": a plaintext of level " + std::to_string(pt.Level) + " (" +
                                    std::to_string(pt.Value.size()) + " words) for ciphertexts of level " + std::to_string(ct.Level()));
    return pt.Value.data();
}

void LinearEvaluator::plain_sum(const char *what, const Ciphertexts &ct, const Plaintext &pt, Ciphertexts &out, bool sub) {
    const uint64_t *words = limbs_for(what, ct, pt);
    need_scales(what, ct.Scale(), pt.Scale);
    const MetaData md = ct.Meta;
    lumen_set *set = out.Handle();
    check((sub ? lumen_sub_plain : lumen_add_plain)(Context(), ct.Handle(), words, &set), sub ? "lumen_sub_plain" : "lumen_add_plain");
    finish(set, md, out);
}

void LinearEvaluator::Add(const Ciphertexts &ct, const Plaintext &pt, Ciphertexts &out) { plain_sum("Add", ct, pt, out, false); }
void LinearEvaluator::Sub(const Ciphertexts &ct, const Plaintext &pt, Ciphertexts &out) { plain_sum("Sub", ct, pt, out, true); }

Ciphertexts LinearEvaluator::AddNew(const Ciphertexts &ct, const Plaintext &pt) {
    Ciphertexts out;
    plain_sum("Add", ct, pt, out, false);
    return out;
}

Ciphertexts LinearEvaluator::SubNew(const Ciphertexts &ct, const Plaintext &pt) {
    Ciphertexts out;
    plain_sum("Sub", ct, pt, out, true);
    return out;
}

Ciphertexts LinearEvaluator::MulNew(const Ciphertexts &ct, const Plaintext &pt) {
    const uint64_t *words = limbs_for("MulNew", ct, pt);
    lumen_set *set = nullptr;
    check(lumen_mul_plain(Context(), ct.Handle(), words, &set), "lumen_mul_plain");
    MetaData md = ct.Meta;
    const uint64_t T = GetParameters().T;
    md.Scale = MulMod(ct.Scale() % T, pt.Scale % T, T); // bgv: Scale_ct * Scale_pt
    return Ciphertexts(Context(), set, md);
}

void LinearEvaluator::MulThenAdd(const Ciphertexts &ct, const Plaintext &pt, Ciphertexts &acc) {
    const uint64_t *words = limbs_for("MulThenAdd", ct, pt);
    need_set("MulThenAdd", acc);
    const uint64_t T = GetParameters().T;
    need_scales("MulThenAdd", acc.Scale(), MulMod(ct.Scale() % T, pt.Scale % T, T));
    check(lumen_mul_plain_then_add(Context(), ct.Handle(), words, acc.Handle()), "lumen_mul_plain_then_add");
}

Plaintext ServerBFV::Encode(const std::vector<uint64_t> &values) const { return encode_limbs(values, params_.MaxLevel(), false); }

Plaintext ServerBFV::EncodeQP(const std::vector<uint64_t> &values, int level) const {
    if (level < 0 || level > params_.MaxLevel()) throw std::invalid_argument("cannot EncodeQP: no such level");
    return encode_limbs(values, level, true);
}

// the limbs of Q up to `level`, then (withP) those of P: one lift of every coefficient, in [0, T)
Plaintext ServerBFV::encode_limbs(const std::vector<uint64_t> &values, int level, bool withP) const {
    const int N = params_.N(), nq = level + 1, nl = nq + (withP ? (int)params_.P.size() : 0);
    if ((int)values.size() > N) throw std::invalid_argument("cannot Encode: too many values for the ring degree");
    std::vector<uint64_t> m(N, 0);
    for (size_t i = 0; i < values.size(); i++) m[slot_index_[i]] = values[i] % params_.T; // raw u64 reduce implicitly
    host_ntt(m, params_.T, psiT_, params_.LogN, true);
    Plaintext pt;
    pt.Level = level;
    pt.Value.resize((size_t)nl * N);
    for (int l = 0; l < nl; l++) {
        const size_t mi = l < nq ? (size_t)l : params_.Q.size() + (size_t)(l - nq); // Psi: Q then P
        const uint64_t q = l < nq ? params_.Q[l] : params_.P[l - nq], tinv = InvMod(params_.T % q, q);
        std::vector<uint64_t> limb(N);
        for (int k = 0; k < N; k++) limb[k] = MulMod(m[k] % q, tinv, q);
        host_ntt(limb, q, params_.Psi[mi], params_.LogN, false);
        memcpy(&pt.Value[(size_t)l * N], limb.data(), (size_t)N * 8);
    }
    return pt;
}

std::vector<uint64_t> ServerBFV::EncryptNew(const Plaintext &pt) {
    // rlwe.Encryptor with a public key: (u*pk0 + e0 + pt, u*pk1 + e1), ternary u, Gaussian e (sigma 3.2).
    // One ciphertext of the device encryptor: its samples are ChaCha20(seed, index) of the shared encryptor state, the same
    // stream EncryptNewBatch / EncryptColumnsNew draw from, never a host-side generator.  The path only
    // encrypts at MaxLevel (fhe/code.go:15-19: NewPlaintext(params, MaxLevel)).
    if ((size_t)pt.Level + 1 != params_.Q.size()) throw std::invalid_argument("EncryptNew: plaintext must be at MaxLevel");
    lumen_set *set = nullptr;
    check(lumen_encrypt_pk(Context(), pt.Value.data(), 1, enc_->seed, enc_->next.fetch_add(1), &set), "lumen_encrypt_pk");
    return Ciphertexts(Context(), set).Download();
}

Ciphertexts ServerBFV::EncryptNewBatch(const std::vector<Plaintext> &pts) {
    // the EncryptNew loop of cmd/server/main.go:199-208 as one device call; column i of this server's
    // lifetime draws its randomness from ChaCha20(seed, i)
    const size_t N = (size_t)params_.N(), L = params_.Q.size();
    std::vector<uint64_t> flat(pts.size() * L * N);
    for (size_t i = 0; i < pts.size(); i++) {
        if ((size_t)pts[i].Level + 1 != L) throw std::invalid_argument("EncryptNewBatch: plaintexts must be at MaxLevel");
        memcpy(&flat[i * L * N], pts[i].Value.data(), L * N * 8);
    }
    lumen_set *set = nullptr;
    check(lumen_encrypt_pk(Context(), flat.data(), (uint32_t)pts.size(), enc_->seed, enc_->next.fetch_add(pts.size()), &set),
          "lumen_encrypt_pk");
    return Ciphertexts(Context(), set, fresh_meta(params_));
}

Ciphertexts ServerBFV::EncryptColumnsNew(const std::vector<uint64_t> &values, int rows, int count) {
    // Encoder.Encode + EncryptNew of `count` columns of `rows` slot values (cmd/server/main.go:188-208)
    // in one device call: only the raw values cross PCIe
    if ((size_t)rows * count != values.size()) throw std::invalid_argument("EncryptColumnsNew: size mismatch");
    lumen_set *set = nullptr;
    check(lumen_encrypt_values(Context(), values.data(), (uint32_t)rows, (uint32_t)count, enc_->seed,
                               enc_->next.fetch_add((uint64_t)count), &set),
          "lumen_encrypt_values");
    return Ciphertexts(Context(), set, fresh_meta(params_));
}

Ciphertexts ServerBFV::ExpandSeeded(const SeededCiphertexts &seeded) {
    if (seeded.Count < 0 || seeded.C0.size() != (size_t)seeded.Count * params_.Q.size() * (size_t)params_.N())
        throw std::invalid_argument("ExpandSeeded: C0 is not [Count][L][N]");
    lumen_set *set = nullptr;
    check(lumen_ct_expand_seeded(Context(), seeded.C0.data(), (uint32_t)seeded.Count, seeded.ASeed.data(), seeded.FirstIndex, &set),
          "lumen_ct_expand_seeded");
    return Ciphertexts(Context(), set, fresh_meta(params_));
}

core::Element ServerBFV::EvaluateColumns(const std::vector<uint64_t> &values, int rows, int count, int cols, core::Element z,
                                         uint64_t firstColumn) {
    if (rows < 0 || count < 0 || cols < 0 || (size_t)rows * count != values.size())
        throw std::invalid_argument("EvaluateColumns: size mismatch");
    core::ScopedSpan span("Evaluate polynomial", nullptr);
    uint64_t value = 0;
    check(lumen_poly_eval_columns(Context(), values.data(), (uint32_t)rows, (uint32_t)count, firstColumn, (uint32_t)cols, z, &value),
          "lumen_poly_eval_columns");
    return value;
}

// ------------------------------------------------------------------ ring switch
RingSwitchServer::RingSwitchServer(ServerBFV &backend, const std::vector<uint64_t> &ringSwitchEvk, int logN,
                                   int baseTwoDecomposition)
    : logN_(logN) {
    // the whole key the client posts, [rns][pw2][b|a][L+K][N], or its RNS digit 0 alone: nothing else is read
    const Parameters &P = backend.GetParameters();
    const size_t digit0 = (size_t)lumen_ringswitch_digits(backend.Context(), (uint32_t)baseTwoDecomposition) * 2 *
                          (P.Q.size() + P.P.size()) * (size_t)P.N();
    const size_t whole = digit0 * lumen_ringswitch_rns_digits(backend.Context());
    if (ringSwitchEvk.size() != whole && ringSwitchEvk.size() != digit0)
        throw std::invalid_argument("NewRingSwitchServer: ringSwitchEvk has " + std::to_string(ringSwitchEvk.size()) +
                                    " words, expected " + std::to_string(whole) + " (or RNS digit 0 alone: " +
                                    std::to_string(digit0) + ")");
    backend.check(lumen_load_ringswitch_key(backend.Context(), (uint32_t)logN, (uint32_t)baseTwoDecomposition,
                                            ringSwitchEvk.data(), ringSwitchEvk.size()),
                  "lumen_load_ringswitch_key");
}

std::vector<uint64_t> RingSwitchServer::RingSwitchNew(const Ciphertexts &cts, ServerBFV &backend) const {
    std::vector<uint64_t> out((size_t)cts.Len() * 2 * ((size_t)1 << logN_));
    if (cts.Len()) backend.check(lumen_ring_switch(backend.Context(), cts.Handle(), out.data()), "lumen_ring_switch");
    return out;
}

// ------------------------------------------------------------------ ServerGroup
ServerGroup::ServerGroup(std::vector<ServerBFV *> ranks, uint32_t transport) : ranks_(std::move(ranks)) {
    const size_t W = ranks_.size();
    if (!W || (W & (W - 1))) throw std::invalid_argument("ServerGroup: the number of ranks must be a power of two");
    uint32_t logw = 0;
    while (((size_t)1 << logw) < W) logw++;
    std::vector<lumen_ctx *> ctxs;
    for (ServerBFV *s : ranks_) {
        if (!s) throw std::invalid_argument("ServerGroup: NULL rank");
        ctxs.push_back(s->Context());
        s->enc_ = ranks_[0]->enc_; // one encryptor: every rank draws from rank 0's stream
    }
    check(lumen_group_create(ctxs.data(), logw, transport, &group_), "lumen_group_create");
}
ServerGroup::~ServerGroup() { lumen_group_destroy(group_); }
void ServerGroup::check(int rc, const char *what) const { throw_on(rc, what, nullptr); }
void ServerGroup::Sync() const { check(lumen_group_sync(group_), "lumen_group_sync"); }

ShardedCiphertexts ServerGroup::EncryptColumnsNew(const std::vector<uint64_t> &values, int rows, int count) {
    const int W = World();
    if ((size_t)rows * count != values.size()) throw std::invalid_argument("EncryptColumnsNew: size mismatch");
    if (count % W) throw std::invalid_argument("EncryptColumnsNew: the columns do not split evenly over the ranks");
    const int own = count / W;
    const uint64_t first = ranks_[0]->enc_->next.fetch_add((uint64_t)count);
    ShardedCiphertexts out;
    for (int r = 0; r < W; r++) {
        ServerBFV &s = Rank(r);
        lumen_set *set = nullptr;
        s.check(lumen_encrypt_values(s.Context(), values.data() + (size_t)r * own * rows, (uint32_t)rows, (uint32_t)own,
                                     s.enc_->seed, first + (uint64_t)r * own, &set),
                "lumen_encrypt_values");
        out.Blocks.emplace_back(s.Context(), set, fresh_meta(s.GetParameters()));
    }
    return out;
}

core::Element ServerGroup::EvaluateColumns(const std::vector<uint64_t> &values, int rows, int count, int cols, core::Element z) {
    const int W = World();
    if (rows < 0 || count < 0 || (size_t)rows * count != values.size()) throw std::invalid_argument("EvaluateColumns: size mismatch");
    if (count % W) throw std::invalid_argument("EvaluateColumns: the columns do not split evenly over the ranks");
    const int own = count / W; // the split of EncryptColumnsNew
    std::vector<const uint64_t *> blocks((size_t)W);
    std::vector<uint32_t> counts((size_t)W, (uint32_t)own);
    for (int r = 0; r < W; r++) blocks[(size_t)r] = values.data() + (size_t)r * own * rows;
    core::ScopedSpan span("Evaluate polynomial", nullptr);
    uint64_t value = 0;
    check(lumen_group_poly_eval(group_, blocks.data(), (uint32_t)rows, counts.data(), (uint32_t)cols, z, &value),
          "lumen_group_poly_eval");
    return value;
}

// ------------------------------------------------------------------ Encode / NTT
Ciphertexts Encode(const Ciphertexts &matrix, int rows, int rhoInv, ServerBFV &backend) {
    // code.go:15-22: one fresh encryption of the zero vector, copied into every padding column
    Plaintext zeroColPt = backend.Encode(std::vector<uint64_t>((size_t)rows, 0));
    const std::vector<uint64_t> zeroCol = backend.EncryptNew(zeroColPt);
    lumen_set *enc = nullptr;
    backend.check(lumen_encode(backend.Context(), matrix.Handle(), zeroCol.data(), (uint32_t)rhoInv, &enc), "lumen_encode");
    return Ciphertexts(backend.Context(), enc, matrix.Meta); // Add / Sub / Mul by a scalar keep the scale
}

ShardedCiphertexts Encode(const ShardedCiphertexts &matrix, int rows, int rhoInv, ServerGroup &group) {
    const int W = group.World();
    if ((int)matrix.Blocks.size() != W) throw std::invalid_argument("Encode: one block of columns per rank is required");
    // code.go:15-22: ONE fresh encryption of the zero vector (rank 0's encoder and the group's encryptor stream);
    // every rank takes its lanes of it
    ServerBFV &lead = group.Rank(0);
    Plaintext zeroColPt = lead.Encode(std::vector<uint64_t>((size_t)rows, 0));
    const std::vector<uint64_t> zeroCol = lead.EncryptNew(zeroColPt);
    std::vector<const lumen_set *> in;
    for (const Ciphertexts &b : matrix.Blocks) in.push_back(b.Handle());
    std::vector<lumen_set *> enc((size_t)W, nullptr);
    group.check(lumen_group_encode(group.Handle(), in.data(), zeroCol.data(), (uint32_t)rhoInv, enc.data()), "lumen_group_encode");
    ShardedCiphertexts out;
    for (int r = 0; r < W; r++) out.Blocks.emplace_back(group.Rank(r).Context(), enc[(size_t)r], matrix.Meta());
    return out;
}

void NTT(Ciphertexts &values, int size, ServerBFV &backend) {
    backend.check(lumen_ct_ntt(backend.Context(), values.Handle(), (uint32_t)size), "lumen_ct_ntt");
}

// ------------------------------------------------------------------ Ligero
int calculateQueries(double securityBits, int rhoInv) {
    const double t = std::log2(1.0 + 1.0 / (double)rhoInv);
    if (1.0 - t <= 0) return 0;
    return (int)std::ceil(securityBits / (1.0 - t));
}

LigeroCommitter LigeroCommitter::NewLigeroCommitter(double securityBits, int rows, int cols, int rhoInv) {
    if ((long long)rows * cols <= 0) throw std::invalid_argument("size must be positive");
    if (securityBits <= 0) throw std::invalid_argument("securityBits must be positive");
    LigeroCommitter c;
    c.Metadata = {rows, cols, rhoInv, calculateQueries(securityBits, rhoInv)};
    return c;
}

void LigeroMetadata::WriteTo(std::vector<uint8_t> &buf) const {
    auto le = [&](uint64_t v, int n) {
        for (int i = 0; i < n; i++) buf.push_back((uint8_t)(v >> (8 * i)));
    };
    le((uint32_t)Rows, 4), le((uint32_t)Cols, 4), le((uint8_t)RhoInv, 1), le((uint16_t)Queries, 2);
}

// the end of both Commits: the prover's state around the level-1 columns and their tree, and the root
static std::pair<LigeroProver, std::vector<uint8_t>> make_prover(const LigeroCommitter *committer, const Ciphertexts *matrix,
                                                                 const ShardedCiphertexts *shards, ShardedCiphertexts level1,
                                                                 core::MerkleTree tree) {
    LigeroProver prover;
    prover.Committer = committer;
    prover.Matrix = matrix;
    prover.MatrixShards = shards;
    prover.EncodedLevel1 = std::move(level1);
    prover.Tree = std::move(tree);
    std::vector<uint8_t> root = prover.Tree.MerkleRoot();
    return {std::move(prover), std::move(root)};
}

std::pair<LigeroProver, std::vector<uint8_t>> LigeroCommitter::Commit(const Ciphertexts &matrix, ServerBFV &backend,
                                                                       core::Span *ctx) const {
    lumen_ctx *h = backend.Context();
    core::ScopedSpan encodeSpan("Encode", ctx);
    Ciphertexts encoded = Encode(matrix, Metadata.Rows, Metadata.RhoInv, backend);
    backend.check(lumen_sync(h), "lumen_sync");
    encodeSpan.End();

    core::ScopedSpan treeSpan("Merkle tree built", ctx);
    // processLeafParallel (ligero.go:126-183): mod-switch every column to level 1, serialise, hash
    lumen_set *lvl1 = nullptr;
    backend.check(lumen_rescale(h, encoded.Handle(), 2, &lvl1), "lumen_rescale");
    MetaData md = encoded.Meta; // Encode keeps the scale (Mul by a scalar, Add, Sub: ntt.go)
    md.Scale = RescaledScale(backend.GetParameters(), md.Scale, encoded.Level(), 1);
    Ciphertexts level1(h, lvl1, md);
    SetCiphertextFormat(backend, md, 1); // what ct.WriteTo(buf) would emit for these leaves (ligero.go:156-157)
    std::vector<core::Digest> leaves((size_t)level1.Len());
    if (!leaves.empty()) backend.check(lumen_leaf_digests(h, lvl1, leaves[0].data()), "lumen_leaf_digests");
    core::MerkleTree tree = core::MerkleTree::FromLeafDigests(std::move(leaves)); // core.NewTree
    treeSpan.End();

    return make_prover(this, &matrix, nullptr, ShardedCiphertexts(std::move(level1)), std::move(tree));
}

std::pair<LigeroProver, std::vector<uint8_t>> LigeroCommitter::Commit(const ShardedCiphertexts &matrix, ServerGroup &group,
                                                                       core::Span *ctx) const {
    const int W = group.World();
    core::ScopedSpan encodeSpan("Encode", ctx);
    ShardedCiphertexts encoded = Encode(matrix, Metadata.Rows, Metadata.RhoInv, group);
    group.Sync();
    encodeSpan.End();

    core::ScopedSpan treeSpan("Merkle tree built", ctx);
    // processLeafParallel (ligero.go:126-183) on every rank's block of encoded columns; the leaves are hashed on
    // the ranks' side streams, then ONE all-gather puts the S digests on every rank
    MetaData md = encoded.Meta();
    md.Scale = RescaledScale(group.Rank(0).GetParameters(), md.Scale, encoded.Level(), 1);
    ShardedCiphertexts level1;
    for (int r = 0; r < W; r++) {
        ServerBFV &s = group.Rank(r);
        lumen_set *lvl1 = nullptr;
        s.check(lumen_rescale(s.Context(), encoded.Blocks[(size_t)r].Handle(), 2, &lvl1), "lumen_rescale");
        level1.Blocks.emplace_back(s.Context(), lvl1, md);
        SetCiphertextFormat(s, md, 1);
        s.check(lumen_leaf_digests_begin(s.Context(), lvl1), "lumen_leaf_digests_begin");
    }
    group.check(lumen_group_all_gather_digests(group.Handle()), "lumen_group_all_gather_digests");
    std::vector<core::Digest> leaves((size_t)level1.Len());
    uint32_t n = 0;
    group.check(lumen_group_digests(group.Handle(), leaves[0].data(), leaves.size() * 32, &n), "lumen_group_digests");
    if (n != leaves.size()) throw std::runtime_error("Commit: the all-gather returned another number of leaves");
    core::MerkleTree tree = core::MerkleTree::FromLeafDigests(std::move(leaves)); // core.NewTree
    // the same root built on the device from the gathered digests (what a rank that keeps no tree would use)
    uint8_t droot[32];
    group.check(lumen_group_merkle_root(group.Handle(), droot), "lumen_group_merkle_root");
    if (memcmp(droot, tree.MerkleRoot().data(), 32)) throw std::runtime_error("Commit: device and host Merkle roots differ");
    treeSpan.End();

    return make_prover(this, nullptr, &matrix, std::move(level1), std::move(tree));
}

Ciphertexts matrixInnerSumEval(const Ciphertexts &matrix, const Plaintext &plaintext, int rows, ServerBFV &backend) {
    lumen_set *out = nullptr;
    // Evaluator.InnerSum works at ct.Level() and InnerSum(col, 1, rows) takes any rows (ligero.go:325): one entry point
    // serves every level and length, and makes lumen_matrix_inner_sum's calls for a power of two at the top level.  The
    // device reads matrix.Level() + 1 limbs of the plaintext, which holds Level + 1 of them.
    if (plaintext.Level != matrix.Level()) throw std::invalid_argument("matrixInnerSumEval: plaintext and matrix at different levels");
    backend.check(lumen_matrix_inner_sum_general(backend.Context(), matrix.Handle(), plaintext.Value.data(), (uint32_t)rows, &out),
                  "lumen_matrix_inner_sum_general");
    // MulNew: Scale_ct * Scale_pt (Encoder.Encode leaves 1); InnerSum keeps it; the Rescale loop to level 1
    MetaData md = matrix.Meta;
    md.Scale = RescaledScale(backend.GetParameters(), md.Scale, matrix.Level(), 1);
    return Ciphertexts(backend.Context(), out, md);
}

std::vector<int> sampleQueryIndices(core::Transcript &transcript, int queries, int extCols) {
    std::vector<int> idx((size_t)queries);
    for (int &q : idx) q = (int)(transcript.SampleUint64("query") % (uint64_t)extCols);
    return idx;
}

// The prover's challenge (ligero.go:198-222, 880-890): r comes out of the transcript before anything else, as raw u64
// words that are reduced where they are multiplied (ligero.go:202-203); b_i = (z^cols)^i reads no transcript.  The root
// is not written to the transcript, for compatibility with LigeroProveReference (ligero.go:198-199).
struct Challenge {
    std::vector<uint64_t> r, b;
};
static Challenge sample_challenge(core::Transcript &transcript, const core::PrimeField &field, int rows, int cols,
                                  core::Element point) {
    Challenge c{std::vector<uint64_t>((size_t)rows), std::vector<uint64_t>((size_t)rows)};
    transcript.SampleUints("r", c.r);
    const core::Element zPow = field.Pow((uint64_t)cols, point);
    core::Element powB = 1;
    for (uint64_t &bi : c.b) bi = powB, powB = field.Mul(powB, zPow);
    return c;
}

// The opening step of both Proves (ligero.go:262-290), entered once `point` is in the transcript: the query indices are the
// last thing drawn from it.  gather(idx) collects those columns of EncodedLevel1 into one set on `ctx`; which call does
// that is the caller's (lumen_gather on one GPU, lumen_group_gather onto rank 0 of a group).
template <class Gather>
static EncryptedProof open_columns(const LigeroProver &prover, core::Transcript &transcript, lumen_ctx *ctx, uint64_t T,
                                   core::Span *parent, Gather gather) {
    const LigeroMetadata &md = prover.Committer->Metadata;
    EncryptedProof proof;
    core::ScopedSpan span("Query columns", parent);
    proof.QueryIndices = sampleQueryIndices(transcript, md.Queries, md.Cols * md.RhoInv);
    const std::vector<uint32_t> idx(proof.QueryIndices.begin(), proof.QueryIndices.end());
    proof.QueriedCols = Ciphertexts(ctx, gather(idx), prover.EncodedLevel1.Meta());
    for (int i : proof.QueryIndices) proof.MerklePaths.push_back(prover.Tree.GetMerklePath((unsigned)i));
    span.End();
    proof.Metadata = md;
    proof.Root = prover.Tree.MerkleRoot();
    proof.PlaintextModulus = T;
    return proof;
}

EncryptedProof LigeroProver::Prove(core::Element point, ServerBFV &backend, core::Transcript &transcript, core::Span *ctx) {
    const int cols = Committer->Metadata.Cols, rows = Committer->Metadata.Rows;
    const Challenge ch = sample_challenge(transcript, *backend.Field(), rows, cols, point);
    const Plaintext rPt = backend.Encode(ch.r), bPt = backend.Encode(ch.b);

    if (!Matrix) throw std::invalid_argument("Prove: this prover was committed on a ServerGroup; prove on that group");
    auto inner = [&](const Plaintext &pt, ServerBFV &s) {
        Ciphertexts out = matrixInnerSumEval(*Matrix, pt, rows, s);
        s.check(lumen_sync(s.Context()), "lumen_sync");
        return out;
    };
    Ciphertexts matR, matZ;
    if (ConcurrentRZ) {
        // ligero.go:231-242 as written: two goroutines, each on its own CopyNew (here: the server itself and one
        // copy -- a lumen_ctx_clone with its own streams); both spans cover the overlapped evaluation
        std::unique_ptr<ServerBFV> copy = backend.CopyNew();
        core::ScopedSpan spanR("InnerProduct(Matrix, r)", ctx), spanZ("InnerProduct(Matrix, b)", ctx);
        std::exception_ptr errZ;
        lumen_set *zset = nullptr;
        MetaData zmeta;
        std::thread tz([&] {
            try {
                Ciphertexts z = inner(bPt, *copy);
                zmeta = z.Meta;
                zset = z.Release(); // the set outlives the copy: from here on it is the server's to destroy
            } catch (...) {
                errZ = std::current_exception();
            }
        });
        try {
            matR = inner(rPt, backend);
        } catch (...) {
            tz.join();
            throw;
        }
        spanR.End();
        tz.join();
        if (errZ) std::rethrow_exception(errZ);
        matZ = Ciphertexts(backend.Context(), zset, zmeta);
        spanZ.End();
    } else {
        // one device context runs them back to back on its stream
        core::ScopedSpan spanR("InnerProduct(Matrix, r)", ctx);
        matR = inner(rPt, backend);
        spanR.End();
        core::ScopedSpan spanZ("InnerProduct(Matrix, b)", ctx);
        matZ = inner(bPt, backend);
        spanZ.End();
    }

    transcript.AppendField("point", point);

    // the reference rescales the queried entries of its top-level EncodedMatrix in place (ligero.go:268-273); the
    // level-1 columns Commit hashed are those very ciphertexts
    EncryptedProof proof = open_columns(*this, transcript, backend.Context(), backend.GetParameters().T, ctx,
                                        [&](const std::vector<uint32_t> &idx) {
                                            lumen_set *q = nullptr;
                                            backend.check(lumen_gather(backend.Context(), EncodedLevel1.Blocks.at(0).Handle(),
                                                                       idx.data(), (uint32_t)idx.size(), &q),
                                                          "lumen_gather");
                                            return q;
                                        });
    if (RingSwitchServer *rs = backend.RingSwitch()) { // ligero.go:336-342: RingSwitchNew on every inner-product output
        proof.RingSwitchLogN = rs->LogN();
        proof.MatRSwitched = rs->RingSwitchNew(matR, backend);
        proof.MatZSwitched = rs->RingSwitchNew(matZ, backend);
    }
    proof.MatR = ShardedCiphertexts(std::move(matR));
    proof.MatZ = ShardedCiphertexts(std::move(matZ));
    return proof;
}

EncryptedProof LigeroProver::Prove(core::Element point, ServerGroup &group, core::Transcript &transcript, core::Span *ctx) {
    const int cols = Committer->Metadata.Cols, rows = Committer->Metadata.Rows, W = group.World();
    if (!MatrixShards || (int)MatrixShards->Blocks.size() != W || (int)EncodedLevel1.Blocks.size() != W)
        throw std::invalid_argument("Prove: this prover was not committed on a group of this size");
    ServerBFV &lead = group.Rank(0);
    const Challenge ch = sample_challenge(transcript, *lead.Field(), rows, cols, point);
    const Plaintext rPt = lead.Encode(ch.r), bPt = lead.Encode(ch.b);

    // every rank evaluates its own block of columns; the calls only enqueue, so the W GPUs run side by side
    auto inner = [&](const Plaintext &pt) {
        ShardedCiphertexts out;
        for (int k = 0; k < W; k++) out.Blocks.push_back(matrixInnerSumEval(MatrixShards->Blocks[(size_t)k], pt, rows, group.Rank(k)));
        group.Sync();
        return out;
    };
    core::ScopedSpan spanR("InnerProduct(Matrix, r)", ctx);
    ShardedCiphertexts matR = inner(rPt);
    spanR.End();
    core::ScopedSpan spanZ("InnerProduct(Matrix, b)", ctx);
    ShardedCiphertexts matZ = inner(bPt);
    spanZ.End();

    transcript.AppendField("point", point);

    EncryptedProof proof = open_columns(*this, transcript, lead.Context(), lead.GetParameters().T, ctx,
                                        [&](const std::vector<uint32_t> &idx) {
                                            std::vector<const lumen_set *> blocks;
                                            for (const Ciphertexts &c : EncodedLevel1.Blocks) blocks.push_back(c.Handle());
                                            lumen_set *q = nullptr;
                                            group.check(lumen_group_gather(group.Handle(), blocks.data(), idx.data(),
                                                                           (uint32_t)idx.size(), &q),
                                                        "lumen_group_gather");
                                            return q;
                                        });
    if (lead.RingSwitch()) { // ligero.go:336-342 on every rank's block (the key is loaded on every rank's context)
        proof.RingSwitchLogN = lead.RingSwitch()->LogN();
        for (int k = 0; k < W; k++) {
            ServerBFV &s = group.Rank(k);
            const RingSwitchServer *rs = s.RingSwitch() ? s.RingSwitch() : lead.RingSwitch();
            const std::vector<uint64_t> pr = rs->RingSwitchNew(matR.Blocks[(size_t)k], s), pz = rs->RingSwitchNew(matZ.Blocks[(size_t)k], s);
            proof.MatRSwitched.insert(proof.MatRSwitched.end(), pr.begin(), pr.end());
            proof.MatZSwitched.insert(proof.MatZSwitched.end(), pz.begin(), pz.end());
        }
    }
    proof.MatR = std::move(matR);
    proof.MatZ = std::move(matZ);
    return proof;
}

// The plain backend of LigeroProveReference and EncodeRows: a context of ring degree 2^logN whose one modulus is T with
// the field's table on it, `count` columns of 2^(logN+1) lanes uploaded as a one-limb set, and their core.Encode
struct PlainEncoded {
    OwnedContext ctx; // declared first: the sets go before their context
    Ciphertexts columns, encoded;
};
static PlainEncoded plain_encode(core::PrimeField &field, int logN, int device, const std::vector<uint64_t> &columns,
                                 size_t count, int rhoInv) {
    PlainEncoded p;
    p.ctx = OwnedContext(field.Modulus(), logN, device);
    lumen_ctx *h = p.ctx.get();
    p.ctx.check(lumen_field_set(h, field.RootsForward().data(), (uint32_t)field.N()), "lumen_field_set");
    lumen_set *m = nullptr, *enc = nullptr;
    p.ctx.check(lumen_set_create(h, (uint32_t)count, 1, &m), "lumen_set_create");
    p.columns = Ciphertexts(h, m);
    p.ctx.check(lumen_set_upload(h, m, 0, (uint32_t)count, columns.data()), "lumen_set_upload");
    const std::vector<uint64_t> zero((size_t)2 << logN, 0);
    p.ctx.check(lumen_encode(h, m, zero.data(), (uint32_t)rhoInv, &enc), "lumen_encode");
    p.encoded = Ciphertexts(h, enc);
    return p;
}

Proof LigeroProveReference(const LigeroCommitter &c, const std::vector<uint64_t> &matrix, core::Element point,
                           core::PrimeField &field, core::Transcript &transcript, int device) {
    const int rows = c.Metadata.Rows, cols = c.Metadata.Cols, rhoInv = c.Metadata.RhoInv, S = cols * rhoInv;
    if ((size_t)rows * cols != matrix.size()) throw std::invalid_argument("LigeroProveReference: matrix size mismatch");
    if (rows < 512 || (rows & (rows - 1))) throw std::invalid_argument("LigeroProveReference: rows must be a power of two >= 512");
    // the plain backend: ring degree rows/2, the one modulus T
    int logN = 0;
    while ((2 << logN) < rows) logN++;
    // Commit: columns as lanes, core.Encode of every row (ligero.go:806-857), leaves = column bytes (866-872)
    std::vector<uint64_t> columns((size_t)cols * rows);
    for (int i = 0; i < rows; i++)
        for (int j = 0; j < cols; j++) columns[(size_t)j * rows + i] = matrix[(size_t)i * cols + j];
    const PlainEncoded plain = plain_encode(field, logN, device, columns, (size_t)cols, rhoInv);
    lumen_ctx *ctx = plain.ctx.get();
    const uint8_t none = 0;
    plain.ctx.check(lumen_leaf_format_set(ctx, &none, 0, &none, 0, &none, 0), "lumen_leaf_format_set");
    std::vector<core::Digest> leaves((size_t)S);
    plain.ctx.check(lumen_leaf_digests(ctx, plain.encoded.Handle(), leaves[0].data()), "lumen_leaf_digests");
    core::MerkleTree tree = core::MerkleTree::FromLeafDigests(std::move(leaves));
    // Prove (ligero.go:880-918)
    Proof proof;
    proof.Metadata = c.Metadata;
    const Challenge ch = sample_challenge(transcript, field, rows, cols, point);
    proof.MatR.resize((size_t)cols), proof.MatZ.resize((size_t)cols);
    plain.ctx.check(lumen_plain_inner_products(ctx, plain.columns.Handle(), ch.r.data(), proof.MatR.data()), "lumen_plain_inner_products");
    plain.ctx.check(lumen_plain_inner_products(ctx, plain.columns.Handle(), ch.b.data(), proof.MatZ.data()), "lumen_plain_inner_products");
    transcript.AppendField("point", point);
    proof.QueryIndices = sampleQueryIndices(transcript, c.Metadata.Queries, S);
    const std::vector<uint32_t> idx(proof.QueryIndices.begin(), proof.QueryIndices.end());
    lumen_set *q = nullptr;
    plain.ctx.check(lumen_gather(ctx, plain.encoded.Handle(), idx.data(), (uint32_t)idx.size(), &q), "lumen_gather");
    const std::vector<uint64_t> opened = Ciphertexts(ctx, q).Download(); // [queries][rows]
    for (size_t k = 0; k < idx.size(); k++) {
        proof.QueriedCols.emplace_back(opened.begin() + (long)(k * rows), opened.begin() + (long)((k + 1) * rows));
        proof.MerklePaths.push_back(tree.GetMerklePath((unsigned)proof.QueryIndices[k]));
    }
    proof.Root = tree.MerkleRoot();
    return proof;
}

// ------------------------------------------------------------------ proof wire format
WireBuffer::WireBuffer(size_t n) : n_(n) {
    p_ = (uint8_t *)lumen_host_alloc(n ? n : 1);
    if (!p_) throw std::runtime_error(std::string("lumen_host_alloc: ") + lumen_last_error(nullptr));
}
WireBuffer &WireBuffer::operator=(WireBuffer &&o) noexcept {
    if (this != &o) {
        if (p_) lumen_host_free(p_);
        p_ = o.p_, n_ = o.n_;
        o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
}
WireBuffer::~WireBuffer() {
    if (p_) lumen_host_free(p_);
}

std::string HumanizeBytes(uint64_t s) {
    // dustin/go-humanize humanateBytes(s, 1000, ...): one decimal below 10, none above
    char buf[64];
    if (s < 10) {
        snprintf(buf, sizeof(buf), "%llu B", (unsigned long long)s);
        return buf;
    }
    static const char *sizes[] = {"B", "kB", "MB", "GB", "TB", "PB", "EB"};
    const double e = std::floor(std::log((double)s) / std::log(1000.0));
    const double val = std::floor((double)s / std::pow(1000.0, e) * 10 + 0.5) / 10;
    snprintf(buf, sizeof(buf), val < 10 ? "%.1f %s" : "%.0f %s", val, sizes[(int)e]);
    return buf;
}

// ct.WriteTo of a ring-switched ciphertext (level 0 of the small ring): framed on the host, 16 KB each
static size_t small_ct_size(const MetaData &md, uint64_t T, int logn) {
    return MetaDataJSON(md, T).size() + 8 + 2 * (8 + 8 + ((size_t)8 << logn));
}
static uint8_t *write_small_cts(uint8_t *o, const std::vector<uint64_t> &res, const MetaData &md, uint64_t T, int logn) {
    const size_t n = (size_t)1 << logn, count = res.size() / (2 * n);
    const std::string json = MetaDataJSON(md, T);
    auto le64 = [&](uint64_t x) {
        for (int i = 0; i < 8; i++) *o++ = (uint8_t)(x >> (8 * i));
    };
    for (size_t c = 0; c < count; c++) {
        memcpy(o, json.data(), json.size()), o += json.size();
        le64(2);
        for (int k = 0; k < 2; k++) {
            le64(1), le64(n);
            memcpy(o, res.data() + (c * 2 + (size_t)k) * n, n * 8), o += n * 8; // little-endian host
        }
    }
    return o;
}

// bytes of a slice in the framing of ITS OWN MetaData and level (the context's current format is whatever the
// last Commit / Unmarshal left there): each ciphertext is MetaData | LE64(2) | 2 x (LE64(limbs) | limbs x (LE64(N) | N words))
static size_t slice_size(const Ciphertexts &c, uint64_t T) {
    if (!c.Len()) return 0;
    const size_t N = ring_degree(c.Context()), nl = (size_t)c.Level() + 1;
    return (MetaDataJSON(c.Meta, T).size() + 8 + 2 * (8 + nl * (8 + N * 8))) * (size_t)c.Len();
}
static size_t slice_size(const ShardedCiphertexts &s, uint64_t T) {
    size_t n = 0;
    for (const Ciphertexts &b : s.Blocks) n += slice_size(b, T);
    return n;
}

size_t EncryptedProof::MarshaledSize() const {
    size_t n = 11;
    if (RingSwitchLogN)
        n += small_ct_size(MatR.Meta(), PlaintextModulus, RingSwitchLogN) * (MatRSwitched.size() + MatZSwitched.size()) /
             ((size_t)2 << RingSwitchLogN);
    else
        n += slice_size(MatR, PlaintextModulus) + slice_size(MatZ, PlaintextModulus);
    n += slice_size(QueriedCols, PlaintextModulus);
    for (const auto &path : MerklePaths) n += path.size() * 32;
    return n + Root.size();
}

void EncryptedProof::MarshalInto(uint8_t *out, size_t cap, bool pageLocked) const {
    if (cap < MarshaledSize()) throw std::invalid_argument("MarshalInto: buffer too small");
    std::vector<uint8_t> md;
    Metadata.WriteTo(md); // ligero.go:660
    memcpy(out, md.data(), md.size());
    uint8_t *o = out + md.size();
    std::set<lumen_ctx *> used; // every context a DMA into `out` was enqueued on
    auto put1 = [&](const Ciphertexts &c) -> size_t { // ct.WriteTo(buf) for every ciphertext of the slice
        const size_t bytes = slice_size(c, PlaintextModulus);
        if (bytes) {
            // the framing of THIS slice's MetaData and level, not whatever format the context was left with
            set_format(c.Context(), c.Meta, c.Level(), PlaintextModulus, ring_degree(c.Context()));
            if (lumen_ct_serialized_size(c.Context(), (uint32_t)c.Level() + 1) * (size_t)c.Len() != bytes)
                throw std::runtime_error("MarshalInto: the device's serialised size differs from the framing's");
            throw_on(pageLocked ? lumen_ct_serialize_async(c.Context(), c.Handle(), 0, (uint32_t)c.Len(), o, bytes)
                                : lumen_ct_serialize(c.Context(), c.Handle(), 0, (uint32_t)c.Len(), o, bytes),
                     "lumen_ct_serialize", c.Context());
            used.insert(c.Context());
        }
        o += bytes;
        return bytes;
    };
    auto put = [&](const ShardedCiphertexts &sc) -> size_t { // the blocks in rank order = column order
        size_t bytes = 0;
        for (const Ciphertexts &b : sc.Blocks) bytes += put1(b);
        return bytes;
    };
    size_t szR, szZ;
    if (RingSwitchLogN) {
        uint8_t *o0 = o;
        o = write_small_cts(o, MatRSwitched, MatR.Meta(), PlaintextModulus, RingSwitchLogN);
        szR = (size_t)(o - o0), o0 = o;
        o = write_small_cts(o, MatZSwitched, MatZ.Meta(), PlaintextModulus, RingSwitchLogN);
        szZ = (size_t)(o - o0);
    } else {
        szR = put(MatR); // ligero.go:664-671
        szZ = put(MatZ); // ligero.go:674-681
    }
    const size_t szQ = put1(QueriedCols); // ligero.go:684-691
    for (const auto &path : MerklePaths)
        for (const core::Digest &d : path) memcpy(o, d.data(), 32), o += 32; // ligero.go:694-698
    memcpy(o, Root.data(), Root.size()), o += Root.size();                    // ligero.go:700
    // the bytes are in place once EVERY context that moved a slice has drained (MatR / MatZ may live on clones
    // or on other GPUs than the queried columns)
    if (pageLocked)
        for (lumen_ctx *c : used) throw_on(lumen_sync(c), "lumen_sync", c);
    if (!core::Span::quiet) {
        printf("Marshaled MatR: %s\n", HumanizeBytes(szR).c_str());
        printf("Marshaled MatZ: %s\n", HumanizeBytes(szZ).c_str());
        printf("Marshaled QueriedCols: %s\n", HumanizeBytes(szQ).c_str());
    }
}

// UnmarshalBinary on one context of ring degree N and plaintext modulus T (a server's or a client's)
static EncryptedProof unmarshal(const uint8_t *data, size_t len, lumen_ctx *ctx, uint64_t T, uint32_t N, const MetaData &meta) {
    if (len < 11 + 32) throw std::invalid_argument("UnmarshalBinary: too short");
    EncryptedProof p;
    auto le = [&](size_t at, int n) {
        uint64_t v = 0;
        for (int i = 0; i < n; i++) v |= (uint64_t)data[at + i] << (8 * i);
        return v;
    };
    p.Metadata = {(int)le(0, 4), (int)le(4, 4), (int)le(8, 1), (int)le(9, 2)}; // LigeroMetadata.ReadFrom (ligero.go:763-778)
    p.PlaintextModulus = T;
    set_format(ctx, meta, 1, T, N);
    const size_t each = lumen_ct_serialized_size(ctx, 2);
    size_t off = 11;
    auto take = [&](int count) {
        const size_t bytes = each * (size_t)count;
        if (off + bytes > len) throw std::invalid_argument("UnmarshalBinary: truncated ciphertext slice");
        lumen_set *s = nullptr;
        throw_on(lumen_ct_deserialize(ctx, data + off, bytes, (uint32_t)count, 2, &s), "lumen_ct_deserialize", ctx);
        off += bytes;
        return Ciphertexts(ctx, s, meta);
    };
    p.MatR = ShardedCiphertexts(take(p.Metadata.Cols)); // ligero.go:712-718
    p.MatZ = ShardedCiphertexts(take(p.Metadata.Cols)); // ligero.go:720-726
    p.QueriedCols = take(p.Metadata.Queries); // ligero.go:728-734
    const int merkleLen = p.Metadata.Cols * p.Metadata.RhoInv; // ligero.go:736-739
    int depth = 0;
    while ((1 << depth) < merkleLen) depth++;
    if (off + (size_t)p.Metadata.Queries * depth * 32 + 32 != len) throw std::invalid_argument("UnmarshalBinary: length mismatch");
    for (int q = 0; q < p.Metadata.Queries; q++) {
        std::vector<core::Digest> path((size_t)depth);
        for (auto &d : path) memcpy(d.data(), data + off, 32), off += 32;
        p.MerklePaths.push_back(std::move(path));
    }
    p.Root.assign(data + off, data + off + 32);
    return p;
}

EncryptedProof EncryptedProof::UnmarshalBinary(const uint8_t *data, size_t len, ServerBFV &backend, const MetaData &meta) {
    return unmarshal(data, len, backend.Context(), backend.GetParameters().T, (uint32_t)backend.GetParameters().N(), meta);
}

EncryptedProof EncryptedProof::UnmarshalBinary(const uint8_t *data, size_t len, ClientBFV &client, const MetaData &meta) {
    return unmarshal(data, len, client.Context(), client.GetParameters().T, (uint32_t)client.GetParameters().N(), meta);
}

// ------------------------------------------------------------------ the client: Decrypt and Verify
Proof EncryptedProof::Decrypt(ClientBFV &client, core::Span *ctx) {
    if (RingSwitchLogN || !MatRSwitched.empty() || !MatZSwitched.empty())
        throw std::runtime_error("Decrypt: a ring-switched proof is read with the client's small-ring key; it is not verified "
                                 "(cmd/client/main.go:210-212) and not supported here");
    if (MatR.Blocks.size() != 1 || MatZ.Blocks.size() != 1)
        throw std::runtime_error("Decrypt: MatR / MatZ must be one block on the client's device");
    const int rows = Metadata.Rows;
    lumen_ctx *h = client.Context();
    Proof proof;
    core::ScopedSpan colSpan("Decrypt queried columns", ctx);
    const int nq = QueriedCols.Len();
    std::vector<uint64_t> values((size_t)nq * (size_t)rows);
    if (nq) client.check(lumen_decrypt(h, QueriedCols.Handle(), QueriedCols.Scale(), (uint32_t)rows, values.data()), "lumen_decrypt");
    for (int i = 0; i < nq; i++)
        proof.QueriedCols.emplace_back(values.begin() + (long)((size_t)i * rows), values.begin() + (long)((size_t)(i + 1) * rows));
    colSpan.End();

    core::ScopedSpan rowSpan("Decrypt row inner products", ctx);
    auto single = [&](const Ciphertexts &c) { // decodeSingleElement of every ciphertext
        std::vector<uint64_t> out((size_t)c.Len());
        if (c.Len()) client.check(lumen_decrypt(h, c.Handle(), c.Scale(), 1, out.data()), "lumen_decrypt");
        return out;
    };
    proof.MatR = single(MatR.Blocks[0]);
    proof.MatZ = single(MatZ.Blocks[0]);
    rowSpan.End();

    proof.Metadata = Metadata;
    proof.Root = Root;
    proof.MerklePaths = MerklePaths;
    proof.QueriedCts = std::make_shared<Ciphertexts>(std::move(QueriedCols));
    return proof;
}

std::vector<std::vector<core::Element>> EncodeRows(const std::vector<std::vector<core::Element>> &rows, int rhoInv,
                                                   core::PrimeField &field, int device) {
    const int logN = 8, N = 1 << logN, lanes = 2 * N; // the smallest degree with kernels: 512 lanes per "ciphertext"
    if (rows.empty()) return {};
    const size_t len = rows[0].size();
    for (const auto &r : rows)
        if (r.size() != len) throw std::invalid_argument("EncodeRows: rows of unequal length");
    if ((int)rows.size() > lanes) throw std::invalid_argument("EncodeRows: more than 512 rows");
    if ((size_t)field.N() != len * (size_t)rhoInv) throw std::invalid_argument("EncodeRows: the field's table is not of len * rhoInv entries");
    const uint64_t T = field.Modulus();
    std::vector<uint64_t> columns(len * (size_t)lanes, 0); // column j = lane i holds rows[i][j]
    for (size_t i = 0; i < rows.size(); i++)
        for (size_t j = 0; j < len; j++) columns[j * lanes + i] = rows[i][j] % T;
    const PlainEncoded plain = plain_encode(field, logN, device, columns, len, rhoInv);
    const size_t S = len * (size_t)rhoInv;
    const std::vector<uint64_t> out = plain.encoded.Download(); // [S][lanes]
    std::vector<std::vector<core::Element>> res(rows.size(), std::vector<core::Element>(S));
    for (size_t i = 0; i < rows.size(); i++)
        for (size_t k = 0; k < S; k++) res[i][k] = out[k * lanes + i];
    return res;
}

std::string VerifyColumnError(uint32_t status, int queryColIdx) {
    if (status & LUMEN_VERIFY_BAD_PATH) return "failed to verify merkle path for column " + std::to_string(queryColIdx);
    if (status & LUMEN_VERIFY_BAD_R) return "well-formedness R check failed for column " + std::to_string(queryColIdx);
    if (status & LUMEN_VERIFY_BAD_B) return "well-formedness B check failed for column " + std::to_string(queryColIdx);
    return "";
}

void Proof::Verify(core::Element point, core::Element value, core::PrimeField &field, core::Transcript &transcript,
                   ClientBFV &client) const {
    const int rows = Metadata.Rows, cols = Metadata.Cols;
    std::vector<uint64_t> r((size_t)rows);
    transcript.SampleUints("r", r); // raw words (SampleFields), reduced where they are multiplied

    // Encode row inner products
    const std::vector<std::vector<core::Element>> encoded = EncodeRows({MatR, MatZ}, Metadata.RhoInv, field, client.Device());
    const std::vector<core::Element> &encodedMatR = encoded[0], &encodedMatZ = encoded[1];

    transcript.AppendField("point", point);

    // a = [1, z, z^2, ..., z^(cols-1)]
    std::vector<core::Element> a((size_t)cols);
    core::Element powA = 1;
    for (core::Element &ai : a) ai = powA, powA = field.Mul(powA, point);
    // b = [1, z^cols, z^(2 cols), ...] is built on the device from zPow
    const core::Element zPow = field.Pow((uint64_t)cols, point);
    if (zPow != powA) throw std::runtime_error("zPow is not equal to powA");

    const int extCols = cols * Metadata.RhoInv;
    const std::vector<int> queryIndices = sampleQueryIndices(transcript, Metadata.Queries, extCols);
    const size_t nq = queryIndices.size();
    if (nq) {
        if (!QueriedCts || (size_t)QueriedCts->Len() != nq)
            throw std::runtime_error("Verify: the proof holds " + std::to_string(QueriedCts ? QueriedCts->Len() : 0) +
                                     " opened ciphertexts for " + std::to_string(nq) + " queries");
        uint32_t depth = 0;
        while ((1u << depth) < (uint32_t)extCols) depth++;
        std::vector<uint8_t> paths(nq * depth * 32, 0);
        std::vector<uint32_t> idx(nq), status(nq, 0);
        std::vector<uint64_t> wantR(nq), wantZ(nq), got(2 * nq);
        if (Root.size() != 32) throw std::runtime_error(VerifyColumnError(LUMEN_VERIFY_BAD_PATH, queryIndices[0])); // no root to reach
        std::vector<bool> noPath(nq, false); // a missing path, or one of another length: it cannot lead to the root
        for (size_t i = 0; i < nq; i++) {
            idx[i] = (uint32_t)queryIndices[i];
            wantR[i] = encodedMatR[(size_t)queryIndices[i]], wantZ[i] = encodedMatZ[(size_t)queryIndices[i]];
            if (i >= MerklePaths.size() || MerklePaths[i].size() != depth) {
                noPath[i] = true;
                continue;
            }
            for (uint32_t k = 0; k < depth; k++) memcpy(&paths[(i * depth + k) * 32], MerklePaths[i][k].data(), 32);
        }
        lumen_ctx *h = client.Context();
        set_format(h, QueriedCts->Meta, QueriedCts->Level(), client.GetParameters().T, (uint32_t)client.GetParameters().N());
        client.check(lumen_verify_columns(h, QueriedCts->Handle(), QueriedCts->Scale(), (uint32_t)rows, r.data(), zPow, wantR.data(),
                                          wantZ.data(), idx.data(), paths.data(), depth, Root.data(), status.data(), got.data(),
                                          nullptr),
                     "lumen_verify_columns");
        for (size_t i = 0; i < nq; i++) {
            const uint32_t st = noPath[i] ? status[i] | LUMEN_VERIFY_BAD_PATH : status[i];
            if (!st) continue;
            if (!(st & LUMEN_VERIFY_BAD_PATH) && (st & LUMEN_VERIFY_BAD_R))
                printf("well-formedness R check failed for column expected %llu got %llu\n", (unsigned long long)wantR[i],
                       (unsigned long long)got[2 * i]);
            throw std::runtime_error(VerifyColumnError(st, queryIndices[i]));
        }
    }

    core::Element claim = 0;
    for (int j = 0; j < cols; j++) claim = field.Add(claim, field.Mul(MatZ.at((size_t)j), a[(size_t)j]));
    if (claim != value) throw std::runtime_error(" claimed value does not match the evaluation of the committed polynomial");
}

vdec::Witness Proof::ProveDecrypt(ClientBFV &client, core::Span *ctx) const {
    (void)ctx; // ligero.go:505 starts the span at the top level whatever the caller's span is
    core::ScopedSpan span("Verifiable decrypt", nullptr, "Verifiable decrypt...");
    core::Transcript transcript("vdec");
    if (!QueriedCts || QueriedCts->Len() == 0)
        throw std::runtime_error("ProveDecrypt: the proof holds no opened ciphertexts (QueriedCts is empty: Decrypt fills it)");
    if ((size_t)QueriedCts->Len() != QueriedCols.size())
        throw std::runtime_error("ProveDecrypt: " + std::to_string(QueriedCols.size()) + " decrypted columns for " +
                                 std::to_string(QueriedCts->Len()) + " opened ciphertexts");
    const Parameters &params = client.GetParameters();
    lumen_ctx *h = client.Context();

    core::ScopedSpan colSpan("Batching decrypted columns", span.get());
    auto batched = vdec::BatchColumns(QueriedCols, *client.Field(), transcript);
    const std::vector<core::Element> &m = batched.first;
    colSpan.End();

    core::ScopedSpan ctSpan("Batching ciphertexts", span.get());
    Ciphertexts batchCt = vdec::BatchCiphertexts(*QueriedCts, batched.second, client);
    ctSpan.End();

    // for batchCt.LevelQ() > 0 { Rescale } (prover.go:84-87)
    if (batchCt.Level() > 0) {
        lumen_set *low = nullptr;
        client.check(lumen_rescale(h, batchCt.Handle(), 1, &low), "lumen_rescale");
        MetaData md = batchCt.Meta;
        md.Scale = RescaledScale(params, md.Scale, batchCt.Level(), 0);
        batchCt = Ciphertexts(h, low, md);
    }

    core::ScopedSpan witSpan("Witness generation", span.get());
    const size_t N = (size_t)params.N();
    vdec::Witness w;
    w.sk.resize(N), w.ct0.resize(N), w.ct1.resize(N), w.mDelta.resize(N), w.err.resize(N);
    w.Degree = (int)std::min<size_t>(2048, N); // `degree` of prover.go:92
    client.check(lumen_vdec_witness(h, batchCt.Handle(), m.data(), (uint32_t)m.size(), batchCt.Scale(), w.sk.data(), w.ct0.data(),
                                    w.ct1.data(), w.mDelta.data(), w.err.data()),
                 "lumen_vdec_witness");
    witSpan.End();

    // the decryption relation: m is what the batch ciphertext decrypts to iff |err| * 2T < q_0
    uint64_t emax = 0;
    for (int64_t e : w.err) emax = std::max<uint64_t>(emax, (uint64_t)(e < 0 ? -e : e));
    const unsigned __int128 lhs = (unsigned __int128)emax * 2 * params.T;
    if (lhs >= params.Q[0])
        throw std::runtime_error("ProveDecrypt: the batch of " + std::to_string(QueriedCts->Len()) +
                                 " ciphertexts does not decrypt to the batched columns (max |err| = " + std::to_string(emax) +
                                 ", |err| * 2T >= q_0): outside the noise budget T * count * N * T * (B + 1) < Q_level / 2 "
                                 "of a full-size plaintext product -- see tools/noise_budget.py --vdec");
    // Here vdec.CallVdecProver (prover.go:121-) fills lazer's polyvecs from the five arrays and calls ProveVdecLnpTbox.
    // lazer is not part of this project ("Proof of decryption"): the witness is the result.
    return w;
}

std::vector<uint8_t> EncryptedProof::MarshalBinary() const {
    std::vector<uint8_t> buf(MarshaledSize());
    MarshalInto(buf.data(), buf.size(), false);
    return buf;
}

WireBuffer EncryptedProof::MarshalBinaryPinned() const {
    WireBuffer w(MarshaledSize());
    MarshalInto(w.data(), w.size(), true);
    return w;
}

} // namespace fhe

namespace vdec {
std::pair<std::vector<core::Element>, std::vector<std::vector<uint64_t>>>
BatchColumns(const std::vector<std::vector<core::Element>> &matrixColMajor, core::PrimeField &field, core::Transcript &transcript) {
    if (matrixColMajor.empty()) throw std::invalid_argument("BatchColumns: no columns");
    const size_t rows = matrixColMajor[0].size(), cols = matrixColMajor.size();
    const uint64_t T = field.Modulus();
    std::vector<std::vector<uint64_t>> alphas(cols);
    for (auto &a : alphas) {
        a.assign(rows, 0);
        transcript.SampleUints("pod_alpha", a);
    }
    std::vector<core::Element> batchCol(rows, 0);
    for (size_t j = 0; j < cols; j++) {
        if (matrixColMajor[j].size() != rows) throw std::invalid_argument("BatchColumns: columns of unequal length");
        for (size_t i = 0; i < rows; i++)
            batchCol[i] = field.Add(batchCol[i], field.Mul(matrixColMajor[j][i] % T, alphas[j][i] % T));
    }
    return {std::move(batchCol), std::move(alphas)};
}

fhe::Ciphertexts BatchCiphertexts(const fhe::Ciphertexts &cts, const std::vector<std::vector<uint64_t>> &alphasColMajor,
                                  fhe::ClientBFV &client) {
    if (alphasColMajor.empty() || (int)alphasColMajor.size() != cts.Len())
        throw std::invalid_argument("BatchCiphertexts: " + std::to_string(alphasColMajor.size()) + " challenge columns for " +
                                    std::to_string(cts.Len()) + " ciphertexts");
    const size_t rows = alphasColMajor[0].size();
    std::vector<uint64_t> flat;
    flat.reserve(alphasColMajor.size() * rows);
    for (const auto &a : alphasColMajor) {
        if (a.size() != rows) throw std::invalid_argument("BatchCiphertexts: challenge columns of unequal length");
        flat.insert(flat.end(), a.begin(), a.end());
    }
    lumen_set *out = nullptr;
    client.check(lumen_batch_ciphertexts(client.Context(), cts.Handle(), flat.data(), (uint32_t)rows, cts.Scale(), &out),
                 "lumen_batch_ciphertexts");
    fhe::MetaData md = cts.Meta;
    const uint64_t T = client.GetParameters().T;
    md.Scale = core::MulMod(cts.Scale() % T, cts.Scale() % T, T); // MulNew: Scale_ct * Scale_pt
    return fhe::Ciphertexts(client.Context(), out, md);
}
} // namespace vdec
} // namespace lumenos
