// The client of cmd/client/main.go:64-81 through the host mirror, with every key generated on the device.
//   test_keygen_host elements <logN> <rows>
//       CPU: "gen g" for every element of GaloisElementsForInnerSum(1, rows) in order (what GenKeySetNew generates and
//       NewFromKeySet expects), "used g" for the ones InnerSum applies.
//   test_keygen_host e2e <logN> <rows> <cols> <numQ> [ringSwitchLogN]
//       GPU: ClientBFV::NewWithGeneratedSecret -> KeyGenerator: GenKeyPairNew, GenRelinearizationKeyNew,
//       GenGaloisKeysNew(GaloisElementsForInnerSum(1, rows)); the server loads the posted pk and Galois keys, encrypts
//       the witness, commits and proves; the client, holding only its generated secret, unmarshals, decrypts and
//       verifies.  With ringSwitchLogN: NewRingSwitchClient's key is loaded as well and MatR / MatZ come back switched
//       into the small ring, where they are decrypted under skNew (the reference skips Verify there,
//       cmd/client/main.go:210-212).
//   test_keygen_host refuse
//       GPU: a ServerBFV that the library refuses half-way through its constructor (an even Galois element, after the
//       context and the field table exist) leaves no context behind; servers and CopyNews made and destroyed on two
//       threads at once leave none either (fhe::LiveContextsForTest).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../oracle/lo_common.h"
#include "twin.hpp"

using namespace lumenos;

static const uint64_t Modulus = 144115188075593729ull; // fhe/ligero_test.go:16, cmd/server/main.go:22
static const int rhoInv = 2;

static int elements_mode(int argc, char **argv) {
    REQUIRE(argc == 4, "usage: elements <logN> <rows>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]);
    fhe::Parameters params;
    params.LogN = LogN;
    for (uint64_t g : params.GaloisElementsForInnerSum(1, rows)) printf("gen %llu\n", (unsigned long long)g);
    for (uint64_t g : params.GaloisElementsUsedByInnerSum(rows)) printf("used %llu\n", (unsigned long long)g);
    return 0;
}

// Phases of ring-switched ciphertexts in the small ring, c0 + c1 * skNew to the coefficient domain, through a context of
// the small ring's own parameters (degree n, the single modulus q_0, psi^(N/n)): what the reference's small-ring
// client computes first (ring_switch.go:30-41).  cts: [count][2][n]; out: [count][n].
static int small_phases(int logn, uint64_t q0, uint64_t psi_small, const std::vector<int8_t> &skNew,
                        const std::vector<uint64_t> &cts, int count, std::vector<uint64_t> &out) {
    const size_t n = (size_t)1 << logn;
    lumen_params_desc d;
    memset(&d, 0, sizeof(d));
    d.abi_version = LUMEN_ABI_VERSION, d.log_n = (uint32_t)logn, d.num_q = 1, d.num_p = 0, d.plaintext_modulus = Modulus;
    d.moduli[0] = q0, d.psi[0] = psi_small;
    lumen_ctx *ctx = nullptr;
    REQUIRE(!lumen_ctx_create(&d, &ctx), "small-ring context: %s", lumen_last_error(nullptr));
    auto transform = [&](std::vector<uint64_t> &polys, int npoly, int inverse) -> int { // polys: [npoly][n] in poly 0 of a ciphertext
        std::vector<uint64_t> host((size_t)npoly * 2 * n, 0);
        for (int i = 0; i < npoly; i++) memcpy(&host[(size_t)i * 2 * n], &polys[(size_t)i * n], n * 8);
        lumen_set *s = nullptr;
        REQUIRE(!lumen_set_create(ctx, (uint32_t)npoly, 1, &s), "set: %s", lumen_last_error(ctx));
        int rc = lumen_set_upload(ctx, s, 0, (uint32_t)npoly, host.data());
        if (!rc) rc = lumen_set_ntt(ctx, s, inverse);
        if (!rc) rc = lumen_set_download(ctx, s, 0, (uint32_t)npoly, host.data());
        lumen_set_destroy(ctx, s);
        REQUIRE(!rc, "small-ring transform: %s", lumen_last_error(ctx));
        for (int i = 0; i < npoly; i++) memcpy(&polys[(size_t)i * n], &host[(size_t)i * 2 * n], n * 8);
        return 0;
    };
    std::vector<uint64_t> s(n);
    for (size_t k = 0; k < n; k++) s[k] = skNew[k] >= 0 ? (uint64_t)skNew[k] : q0 - (uint64_t)(-(int)skNew[k]);
    if (transform(s, 1, 0)) return 1;
    out.assign((size_t)count * n, 0);
    for (int c = 0; c < count; c++)
        for (size_t k = 0; k < n; k++) {
            const uint64_t c0 = cts[((size_t)c * 2) * n + k], c1 = cts[((size_t)c * 2 + 1) * n + k];
            out[(size_t)c * n + k] = (c0 + core::MulMod(c1, s[k], q0)) % q0;
        }
    const int rc = transform(out, count, 1);
    lumen_ctx_destroy(ctx);
    return rc;
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 6, "usage: e2e <logN> <rows> <cols> <numQ> [ringSwitchLogN]");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), numQ = atoi(argv[5]);
    const int rsLogN = argc > 6 ? atoi(argv[6]) : 0;
    core::Span::quiet = false;
    const fhe::Parameters params = make_params(LogN, cols, numQ);
    const int N = params.N(), L = (int)params.Q.size(), K = (int)params.P.size();
    core::PrimeField ptField(params.PlaintextModulus(), cols * rhoInv);

    // ---- the client's keys (cmd/client/main.go:64-81): nothing below comes from a CPU key generator
    core::ScopedSpan keySpan("Generate keys", nullptr);
    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    // the Montgomery (Lattigo storage) form on the ring-switch run, the standard form otherwise: both reach the server
    const uint32_t flags = rsLogN ? LUMEN_KEY_MONTGOMERY : 0;
    fhe::KeySet keys = kgen.GenKeySetNew(rows, flags);
    const std::vector<uint64_t> rlk = kgen.GenRelinearizationKeyNew(flags);
    keySpan.End();
    const size_t evkWords = (size_t)((L + K - 1) / K) * 2 * (L + K) * N;
    REQUIRE(keys.Pk.size() == (size_t)2 * (L + K) * N && rlk.size() == evkWords, "key sizes");
    REQUIRE(keys.GaloisElements == params.GaloisElementsForInnerSum(1, rows) && keys.GaloisKeys.size() == keys.GaloisElements.size(),
            "GenKeySetNew's elements");
    for (const auto &k : keys.GaloisKeys) REQUIRE(k.size() == evkWords, "Galois key size");
    printf("PASS keys generated on the device: pk, rlk, %zu Galois keys (%.1f MB)\n", keys.GaloisKeys.size(),
           (double)(keys.Pk.size() + rlk.size() + keys.GaloisKeys.size() * evkWords) * 8 / 1e6);
    {
        // deterministic in the client's seed; another client draws another seed and another key
        REQUIRE(kgen.GenKeyPairNew() == keys.Pk, "GenKeyPairNew twice gives other words");
        const uint64_t g = keys.GaloisElements[0];
        REQUIRE(kgen.GenGaloisKeysNew({g}, flags).at(g) == keys.GaloisKeys[0], "a key generated alone differs from the batch's");
        std::unique_ptr<fhe::ClientBFV> other = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
        const uint8_t zero32[32] = {0};
        REQUIRE(memcmp(client->KeySeed(), other->KeySeed(), 32) != 0 && memcmp(client->KeySeed(), zero32, 32) != 0, "key seeds");
        REQUIRE(fhe::KeyGenerator(*other).GenKeyPairNew() != keys.Pk, "two clients share a public key");
        std::vector<uint64_t> sk((size_t)(L + K) * N, 0);
        fhe::ClientBFV handed(&ptField, params, sk);
        bool threw = false;
        try {
            fhe::KeyGenerator bad(handed);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        REQUIRE(threw, "NewKeyGenerator accepted a client whose key was handed in");
        printf("PASS key generation is deterministic in the client's seed, seeds differ between clients\n");
    }

    // ---- the server (cmd/server/main.go:100-140, 187-266) loads what the client posted
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);
    fhe::RingSwitchClient rs;
    std::unique_ptr<fhe::RingSwitchServer> rsServer;
    if (rsLogN) {
        rs = fhe::NewRingSwitchClient(*client, rsLogN);
        REQUIRE(rs.Evk.size() == evkWords, "with two special primes the ring-switch key is one Galois key's size");
        rsServer.reset(new fhe::RingSwitchServer(*server, rs.Evk, rsLogN));
        server->SetRingSwitchServer(rsServer.get());
    }
    const std::vector<uint64_t> matrix = core::RandomMatrixRowMajor(rows, cols, Modulus);
    std::vector<uint64_t> columns((size_t)cols * rows);
    for (int j = 0; j < cols; j++)
        for (int i = 0; i < rows; i++) columns[(size_t)j * rows + i] = matrix[(size_t)i * cols + j];
    const uint64_t z = random_point(Modulus);
    fhe::LigeroCommitter ligero = fhe::LigeroCommitter::NewLigeroCommitter(128, rows, cols, rhoInv);
    fhe::Ciphertexts cts = server->EncryptColumnsNew(columns, rows, cols);
    auto commit = ligero.Commit(cts, *server, nullptr);
    core::Transcript transcript("demo");
    fhe::EncryptedProof proof = commit.first.Prove(z, *server, transcript, nullptr);
    const uint64_t value = server->EvaluateColumns(columns, rows, cols, cols, z);
    core::Transcript refTranscript("demo");
    const fhe::Proof ref = fhe::LigeroProveReference(ligero, matrix, z, ptField, refTranscript);

    if (!rsLogN) {
        // ---- the client (cmd/client/main.go:181-221)
        const fhe::MetaData meta = proof.QueriedCols.Meta;
        const std::vector<uint8_t> marshaled = proof.MarshalBinary();
        fhe::EncryptedProof ep = fhe::EncryptedProof::UnmarshalBinary(marshaled.data(), marshaled.size(), *client, meta);
        core::ScopedSpan decryptSpan("Decrypt proof", nullptr, "Decrypting proof...");
        fhe::Proof plain = ep.Decrypt(*client, decryptSpan.get());
        decryptSpan.End();
        REQUIRE(plain.MatR == ref.MatR && plain.MatZ == ref.MatZ, "MatR / MatZ differ from LigeroProveReference's");
        for (size_t k = 0; k < ref.QueriedCols.size(); k++)
            REQUIRE(plain.QueriedCols[k] == ref.QueriedCols[k], "opened column %zu decrypts to other values than the plain prover's", k);
        printf("PASS decrypt under the generated secret: MatR / MatZ / opened columns = LigeroProveReference's\n");
        core::Transcript vt("demo");
        core::ScopedSpan verifySpan("Verify proof", nullptr);
        plain.Verify(z, value, *client->Field(), vt, *client);
        verifySpan.End();
        printf("PASS client verify: rows=%d cols=%d LogN=%d, every key generated on the device\n", rows, cols, LogN);
        // the claim is bound to the keys: value + 1 fails
        bool threw = false;
        try {
            core::Transcript t2("demo");
            plain.Verify(z, (value + 1) % Modulus, *client->Field(), t2, *client);
        } catch (const std::runtime_error &) {
            threw = true;
        }
        REQUIRE(threw, "Verify accepted value + 1");
        printf("PASS value + 1 is refused\n");
        return 0;
    }

    // ---- ring switch: MatR / MatZ arrive as level-0 ciphertexts of the ring of degree n.  Under skNew their phase
    // c0 + c1 * skNew equals, coefficient by coefficient, the phase of the level-1 ciphertext under sk at X^(i N/n), up to
    // the key switch's own noise.  Bound (hybrid switch, alpha = K = 2): sum over beta digits of digit * e / P with
    // digit < 2^114, |e| <= 19, N terms, P > 2^109 -- below beta * N * 19 * 2^5 < 2^25 at N = 2^12, beta = 5 -- plus
    // ModDown's rounding (1 + N) * K / 2 < 2^13: 2^26 against a modulus of 58 bits.
    REQUIRE(K == 2, "the ring-switch run uses the reference's two special primes");
    const size_t n = (size_t)1 << rsLogN, gap = (size_t)N / n;
    REQUIRE(proof.MatRSwitched.size() == (size_t)cols * 2 * n && proof.MatZSwitched.size() == proof.MatRSwitched.size(),
            "ring-switched slices have the wrong size");
    const uint64_t q0 = params.Q[0];
    const std::vector<uint64_t> sk = client->SecretKeyForTest(), hR = proof.MatR.Download(), hZ = proof.MatZ.Download();
    std::vector<uint64_t> moduli(params.Q);
    moduli.insert(moduli.end(), params.P.begin(), params.P.end());
    lo_params *op = lo_params_new(LogN, L, K, moduli.data(), Modulus);
    REQUIRE(op, "oracle params");
    std::vector<uint64_t> phR, phZ;
    const uint64_t psiSmall = core::PowMod(params.Psi[0], (uint64_t)gap, q0);
    REQUIRE(!small_phases(rsLogN, q0, psiSmall, rs.SkNew, proof.MatRSwitched, cols, phR), "small phases of MatR");
    REQUIRE(!small_phases(rsLogN, q0, psiSmall, rs.SkNew, proof.MatZSwitched, cols, phZ), "small phases of MatZ");
    std::vector<uint64_t> big((size_t)N);
    uint64_t worst = 0;
    const int stride = 16;
    for (int w = 0; w < 2; w++)
        for (int j = 0; j < cols; j += stride) {
            const uint64_t *ct = (w ? hZ : hR).data() + (size_t)j * 4 * N; // [2][2][N], limb 0 of both polynomials
            for (int k = 0; k < N; k++) big[(size_t)k] = (ct[k] + core::MulMod(ct[(size_t)2 * N + k], sk[(size_t)k], q0)) % q0;
            lo_limb_intt(op, 0, big.data());
            const uint64_t *small = (w ? phZ : phR).data() + (size_t)j * n;
            for (size_t i = 0; i < n; i++) {
                const uint64_t d = (small[i] + q0 - big[i * gap]) % q0, a = d > q0 / 2 ? q0 - d : d;
                worst = std::max(worst, a);
                REQUIRE(a < (1ull << 26), "Mat%c[%d] coefficient %zu: the small-ring phase is %llu away from the big ring's", w ? 'Z' : 'R',
                        j, i, (unsigned long long)a);
            }
        }
    lo_params_free(op);
    printf("PASS ring switch to LogN %d under the generated key: small-ring phases under skNew = the big ring's at X^(i N/n) (largest gap %llu)\n",
           rsLogN, (unsigned long long)worst);
    return 0;
}

static int refuse_mode() {
    // LogN 10, L = 2, K = 2: the smallest parameters that have a key switch
    const int cols = 16;
    fhe::ParametersLiteral lit = fhe::GenerateBGVParamsForNTT(4, 10, Modulus);
    const fhe::Parameters params = fhe::Parameters::FromLiteral(lit);
    const size_t N = (size_t)params.N(), L = params.Q.size(), K = params.P.size();
    REQUIRE(L == 2 && K == 2, "L = %zu K = %zu", L, K);
    const size_t evkWords = (L + K - 1) / K * 2 * (L + K) * N;
    core::PrimeField ptField(Modulus, cols * rhoInv);
    const size_t n0 = fhe::LiveContextsForTest();

    std::string what;
    try {
        const std::map<uint64_t, std::vector<uint64_t>> even = {{2, std::vector<uint64_t>(evkWords, 0)}};
        fhe::ServerBFV refused(&ptField, params, std::vector<uint64_t>(2 * (L + K) * N, 0), even);
        REQUIRE(false, "a server with the Galois element 2 was constructed");
    } catch (const std::runtime_error &e) {
        what = e.what();
    }
    REQUIRE(what.find("not an odd residue mod 2N") != std::string::npos, "refused with another message: %s", what.c_str());
    REQUIRE(fhe::LiveContextsForTest() == n0, "the refused server left %zu context(s) behind", fhe::LiveContextsForTest() - n0);

    {
        std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
        fhe::KeyGenerator kgen(*client);
        const std::vector<uint64_t> pk = kgen.GenKeyPairNew();
        const std::map<uint64_t, std::vector<uint64_t>> evk = kgen.GenGaloisKeysNew({params.GaloisElement(1)});
        size_t seen[2] = {0, 0};
        std::string err[2];
        auto run = [&](int t) {
            try {
                fhe::ServerBFV server(&ptField, params, pk, evk);
                std::unique_ptr<fhe::ServerBFV> copy = server.CopyNew();
                seen[t] = fhe::LiveContextsForTest();
            } catch (const std::exception &e) {
                err[t] = e.what();
            }
        };
        std::thread a(run, 0), b(run, 1);
        a.join(), b.join();
        for (int t = 0; t < 2; t++) {
            REQUIRE(err[t].empty(), "thread %d: %s", t, err[t].c_str());
            // the client's, this thread's server and its copy at the least; the other thread's two at the most
            REQUIRE(seen[t] >= n0 + 3 && seen[t] <= n0 + 5, "thread %d saw %zu live contexts over %zu", t, seen[t], n0);
        }
        REQUIRE(fhe::LiveContextsForTest() == n0 + 1, "servers and copies of two threads left contexts behind");
    }
    REQUIRE(fhe::LiveContextsForTest() == n0, "%zu context(s) left at the end", fhe::LiveContextsForTest() - n0);
    printf("PASS refused server leaves no context\n");
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_keygen_host elements|e2e|refuse ...",
                     {{"elements", elements_mode}, {"e2e", e2e_mode}, {"refuse", [](int, char **) { return refuse_mode(); }}});
}
