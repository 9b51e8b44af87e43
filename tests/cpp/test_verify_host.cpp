// The client's sequence of cmd/client/main.go:181-221 through the host mirror: UnmarshalBinary -> Decrypt -> Verify.
//   test_verify_host host <name> <rows> <cols> <rhoInv> <queries> <z>
//       CPU: what Proof::Verify derives from the transcript `name` before it touches the device -- "r i v" for every
//       sampled word, "w v" (z^cols), "a j v" / "b i v" for the first and last powers, "query k idx" -- and "message s
//       text" for every status word 0..7 at column 41; tests/test_verify_host.py recomputes them in Python.
//   test_verify_host e2e <logN> <rows> <cols> <numQ>
//       GPU: the server encrypts TestLigeroE2E's witness, commits, proves at a random z != 1, evaluates P(z) and
//       marshals; the client (fhe::ClientBFV) unmarshals, decrypts and verifies.  MatR / MatZ equal LigeroProveReference's,
//       the two core.Encode rows of Verify equal the oracle's lo_plain_encode, and every tampering of the marshaled
//       bytes makes Verify throw the reference's string with the reference's column number.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../oracle/lo_common.h"
#include "twin.hpp"

using namespace lumenos;

static const uint64_t Modulus = 144115188075593729ull; // fhe/ligero_test.go:16, cmd/server/main.go:22
static const int rhoInv = 2;

// the verifier's transcript up to its query indices (fhe/ligero.go:522-552)
static std::vector<int> verifier_indices(const std::string &name, int rows, int cols, int rho, int queries, uint64_t z,
                                         std::vector<uint64_t> *r_out = nullptr) {
    core::Transcript t(name);
    std::vector<uint64_t> r((size_t)rows);
    t.SampleUints("r", r);
    t.AppendField("point", z);
    if (r_out) *r_out = r;
    return fhe::sampleQueryIndices(t, queries, cols * rho);
}

static int host_mode(int argc, char **argv) {
    REQUIRE(argc == 8, "usage: host <name> <rows> <cols> <rhoInv> <queries> <z>");
    const std::string name = argv[2];
    const int rows = atoi(argv[3]), cols = atoi(argv[4]), rho = atoi(argv[5]), queries = atoi(argv[6]);
    const uint64_t z = strtoull(argv[7], nullptr, 10);
    core::PrimeField field(Modulus, 2);
    std::vector<uint64_t> r;
    const std::vector<int> idx = verifier_indices(name, rows, cols, rho, queries, z, &r);
    for (int i = 0; i < rows; i++) printf("r %d %llu\n", i, (unsigned long long)r[(size_t)i]);
    const uint64_t w = field.Pow((uint64_t)cols, z);
    printf("w %llu\n", (unsigned long long)w);
    uint64_t p = 1;
    for (int j = 0; j < cols; j++, p = field.Mul(p, z))
        if (j < 4 || j == cols - 1) printf("a %d %llu\n", j, (unsigned long long)p);
    p = 1;
    for (int i = 0; i < rows; i++, p = field.Mul(p, w))
        if (i < 4 || i == rows - 1) printf("b %d %llu\n", i, (unsigned long long)p);
    for (int k = 0; k < queries; k++) printf("query %d %d\n", k, idx[(size_t)k]);
    for (uint32_t s = 0; s < 8; s++) printf("message %u %s\n", s, fhe::VerifyColumnError(s, 41).c_str());
    return 0;
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 6, "usage: e2e <logN> <rows> <cols> <numQ>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), numQ = atoi(argv[5]);
    core::Span::quiet = false;
    fhe::ParametersLiteral lit = fhe::GenerateBGVParamsForNTT(cols, LogN, Modulus);
    while ((int)lit.LogQ.size() < numQ) lit.LogQ.push_back(56);
    fhe::Parameters params = fhe::Parameters::FromLiteral(lit);
    const int N = params.N(), L = (int)params.Q.size(), K = (int)params.P.size();
    std::vector<uint64_t> moduli(params.Q);
    moduli.insert(moduli.end(), params.P.begin(), params.P.end());
    lo_params *op = lo_params_new(LogN, L, K, moduli.data(), Modulus);
    REQUIRE(op, "oracle params");
    lo_rng rng;
    lo_rng_seed(&rng, 11);
    std::vector<uint64_t> sk((size_t)(L + K) * N), pk((size_t)2 * (L + K) * N);
    lo_keygen_secret(op, &rng, sk.data());
    lo_keygen_public(op, &rng, sk.data(), pk.data());
    std::map<uint64_t, std::vector<uint64_t>> evk;
    for (uint64_t g : params.GaloisElementsUsedByInnerSum(rows)) {
        evk[g].resize(lo_evk_words(op));
        lo_keygen_galois(op, &rng, sk.data(), g, evk[g].data());
    }
    core::PrimeField ptField(params.PlaintextModulus(), cols * rhoInv);
    fhe::ServerBFV server(&ptField, params, pk, evk);
    fhe::ClientBFV client(&ptField, params, sk);
    REQUIRE(client.Field() == &ptField, "ClientBFV::Field");

    const std::vector<uint64_t> matrix = core::RandomMatrixRowMajor(rows, cols, Modulus);
    std::vector<uint64_t> columns((size_t)cols * rows);
    for (int j = 0; j < cols; j++)
        for (int i = 0; i < rows; i++) columns[(size_t)j * rows + i] = matrix[(size_t)i * cols + j];
    const uint64_t z = random_point(Modulus);
    printf("point z = %llu\n", (unsigned long long)z);

    // ---- the server (cmd/server/main.go:187-266)
    fhe::LigeroCommitter ligero = fhe::LigeroCommitter::NewLigeroCommitter(128, rows, cols, rhoInv);
    const int queries = ligero.Metadata.Queries;
    std::vector<uint8_t> marshaled;
    fhe::MetaData meta;
    uint64_t value = 0;
    {
        fhe::Ciphertexts cts = server.EncryptColumnsNew(columns, rows, cols);
        auto commit = ligero.Commit(cts, server, nullptr);
        core::Transcript transcript("demo");
        fhe::EncryptedProof proof = commit.first.Prove(z, server, transcript, nullptr);
        value = server.EvaluateColumns(columns, rows, cols, cols, z);
        meta = proof.QueriedCols.Meta;
        marshaled = proof.MarshalBinary();
    }
    // the plain prover's MatR / MatZ (LigeroProveReference, the same transcript)
    core::Transcript refTranscript("demo");
    const fhe::Proof ref = fhe::LigeroProveReference(ligero, matrix, z, ptField, refTranscript);
    const std::vector<int> idx = verifier_indices("demo", rows, cols, rhoInv, queries, z);
    REQUIRE(idx == ref.QueryIndices, "the verifier's query indices are not the plain prover's");

    // ---- the client (cmd/client/main.go:181-221)
    auto run = [&](const std::vector<uint8_t> &bytes, const std::string &name, uint64_t claimed, fhe::Proof *out) {
        fhe::EncryptedProof ep = fhe::EncryptedProof::UnmarshalBinary(bytes.data(), bytes.size(), client, meta);
        core::Span *span = core::Span::StartSpan("Decrypt proof", nullptr, "Decrypting proof...");
        fhe::Proof proof = ep.Decrypt(client, span);
        span->End();
        delete span;
        core::Transcript transcript(name);
        span = core::Span::StartSpan("Verify proof", nullptr);
        try {
            proof.Verify(z, claimed, *client.Field(), transcript, client);
        } catch (...) {
            delete span;
            if (out) *out = std::move(proof);
            throw;
        }
        span->End();
        delete span;
        if (out) *out = std::move(proof);
    };
    fhe::Proof honest;
    run(marshaled, "demo", value, &honest);
    REQUIRE(honest.MatR == ref.MatR, "Proof.MatR differs from LigeroProveReference's");
    REQUIRE(honest.MatZ == ref.MatZ, "Proof.MatZ differs from LigeroProveReference's");
    REQUIRE((int)honest.QueriedCols.size() == queries && honest.QueriedCts && honest.QueriedCts->Len() == queries, "QueriedCols");
    for (int k = 0; k < queries; k++)
        REQUIRE(honest.QueriedCols[(size_t)k] == ref.QueriedCols[(size_t)k], "opened column %d decrypts to other values than the plain prover's", k);
    printf("PASS honest proof: rows=%d cols=%d LogN=%d queries=%d verified, MatR / MatZ / opened columns = LigeroProveReference's\n", rows,
           cols, LogN, queries);

    // core.Encode of the two rows as Verify computes it, against the oracle
    {
        const auto enc = fhe::EncodeRows({honest.MatR, honest.MatZ}, rhoInv, ptField);
        std::vector<uint64_t> want((size_t)cols * rhoInv);
        lo_plain_encode(honest.MatR.data(), (uint32_t)cols, rhoInv, Modulus, ptField.RootsForward().data(), (uint32_t)ptField.N(), want.data());
        REQUIRE(enc[0] == want, "EncodeRows(MatR) differs from lo_plain_encode");
        lo_plain_encode(honest.MatZ.data(), (uint32_t)cols, rhoInv, Modulus, ptField.RootsForward().data(), (uint32_t)ptField.N(), want.data());
        REQUIRE(enc[1] == want, "EncodeRows(MatZ) differs from lo_plain_encode");
        printf("PASS EncodeRows = lo_plain_encode for MatR and MatZ\n");
    }
    // a CopyNew of the client verifies too (its own streams and scratch, the shared key)
    {
        std::unique_ptr<fhe::ClientBFV> twin = client.CopyNew();
        fhe::EncryptedProof ep = fhe::EncryptedProof::UnmarshalBinary(marshaled.data(), marshaled.size(), *twin, meta);
        fhe::Proof p = ep.Decrypt(*twin, nullptr);
        core::Transcript t("demo");
        p.Verify(z, value, *twin->Field(), t, *twin);
        printf("PASS ClientBFV::CopyNew verifies\n");
    }

    // ---- tampering: each on a fresh copy of the marshaled bytes.  Layout: 11 bytes of metadata | MatR | MatZ | opened
    // columns (ciphertexts of `ct` bytes, the last 8 N of each being the last limb of c1) | paths | root
    core::Span::quiet = true;
    const size_t ct = lumen_ct_serialized_size(client.Context(), 2);
    int depth = 0;
    while ((1 << depth) < cols * rhoInv) depth++;
    const size_t oR = 11, oZ = oR + (size_t)cols * ct, oQ = oZ + (size_t)cols * ct, oP = oQ + (size_t)queries * ct,
                 oRoot = oP + (size_t)queries * depth * 32;
    REQUIRE(oRoot + 32 == marshaled.size(), "layout: %zu + 32 != %zu", oRoot, marshaled.size());
    auto limb_byte = [&](size_t slice, int i, int word) { return slice + (size_t)i * ct + ct - (size_t)8 * N + (size_t)8 * word; };
    int failures = 0;
    auto expect = [&](const char *what, const std::function<void(std::vector<uint8_t> &)> &mutate, const std::string &name,
                      uint64_t claimed, const std::string &message) {
        std::vector<uint8_t> bytes = marshaled;
        mutate(bytes);
        try {
            run(bytes, name, claimed, nullptr);
            fprintf(stderr, "FAIL %s: Verify accepted\n", what);
            failures++;
        } catch (const std::runtime_error &e) {
            if (message != e.what()) {
                fprintf(stderr, "FAIL %s: Verify threw \"%s\", expected \"%s\"\n", what, e.what(), message.c_str());
                failures++;
            } else {
                printf("PASS %s: \"%s\"\n", what, e.what());
            }
        }
    };
    // a query whose column no earlier query opened (so the queries before it pass), not the first
    int k = 1;
    for (;; k++) {
        REQUIRE(k < queries, "no query with a fresh column");
        bool fresh = true;
        for (int j = 0; j < k; j++) fresh = fresh && idx[(size_t)j] != idx[(size_t)k];
        if (fresh) break;
    }
    const std::string path_k = "failed to verify merkle path for column " + std::to_string(idx[(size_t)k]);
    const std::string path_0 = "failed to verify merkle path for column " + std::to_string(idx[0]);
    expect("a limb byte of opened column k", [&](std::vector<uint8_t> &b) { b[limb_byte(oQ, k, 5)] ^= 1; }, "demo", value, path_k);
    expect("a byte of query k's Merkle path", [&](std::vector<uint8_t> &b) { b[oP + ((size_t)k * depth + 1) * 32 + 9] ^= 0x10; }, "demo",
           value, path_k);
    expect("a byte of the root", [&](std::vector<uint8_t> &b) { b[oRoot + 31] ^= 0x80; }, "demo", value, path_0);
    expect("a limb byte of one MatR ciphertext", [&](std::vector<uint8_t> &b) { b[limb_byte(oR, cols / 2, 3)] ^= 1; }, "demo", value,
           "well-formedness R check failed for column " + std::to_string(idx[0]));
    expect("a limb byte of one MatZ ciphertext", [&](std::vector<uint8_t> &b) { b[limb_byte(oZ, cols / 3, 7)] ^= 1; }, "demo", value,
           "well-formedness B check failed for column " + std::to_string(idx[0]));
    expect("value + 1", [](std::vector<uint8_t> &) {}, "demo", (value + 1) % Modulus,
           " claimed value does not match the evaluation of the committed polynomial");
    // a verifier transcript under another name: its indices are not the prover's; pick a name whose FIRST one differs
    std::string other;
    std::vector<int> oidx;
    for (int s = 0;; s++) {
        other = "other" + std::to_string(s);
        oidx = verifier_indices(other, rows, cols, rhoInv, queries, z);
        if (oidx[0] != idx[0]) break;
    }
    expect("a verifier transcript under another name", [](std::vector<uint8_t> &) {}, other, value,
           "failed to verify merkle path for column " + std::to_string(oidx[0]));
    // the framing is lumen_ct_deserialize's to reject
    {
        std::vector<uint8_t> bytes = marshaled;
        bytes[oQ + (size_t)k * ct + 5] ^= 0x20; // a byte of the MetaData block of opened column k
        try {
            run(bytes, "demo", value, nullptr);
            fprintf(stderr, "FAIL a framing byte: accepted\n");
            failures++;
        } catch (const std::runtime_error &e) {
            if (!strstr(e.what(), "differ from the serialisation format")) {
                fprintf(stderr, "FAIL a framing byte: \"%s\"\n", e.what());
                failures++;
            } else {
                printf("PASS a framing byte is refused by UnmarshalBinary\n");
            }
        }
    }
    // ... and the untouched bytes still verify on the same client afterwards
    run(marshaled, "demo", value, nullptr);
    REQUIRE(!failures, "%d tampering cases failed", failures);
    printf("PASS client verify: rows=%d cols=%d LogN=%d\n", rows, cols, LogN);
    lo_params_free(op);
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_verify_host host|e2e ...",
                     {{"host", host_mode}, {"e2e", e2e_mode}});
}
