// The claimed value of GET /prove?point=z (cmd/server/main.go:255-258) through the host mirror.
//   test_poly_eval_host host <rows> <cols> <random|max> <matrix.bin> <z>...
//       CPU: writes the witness (row-major u64) to matrix.bin and prints core::DensePoly::Evaluate at every z, one
//       "value <z> <P(z)>" line each -- tests/test_poly_eval_host.py recomputes them with Python integers.
//   test_poly_eval_host e2e <logN> <rows> <cols> <numQ> [world]
//       GPU: TestLigeroE2E's witness encrypted on the device, Commit, Prove at a random z != 1, MatZ decrypted with
//       lumen_decrypt; the verifier's claim sum_j z^j * MatZ[j] (fhe/ligero.go:569) must equal the device P(z)
//       (ServerBFV::EvaluateColumns, whole and in uneven column blocks) and the host Horner (DensePoly::Evaluate).
//       With world = W > 1 a ServerGroup of the server and W-1 CopyNew()s evaluates the same witness.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../oracle/lo_common.h"
#include "twin.hpp"

using namespace lumenos;

static const uint64_t Modulus = 144115188075593729ull; // fhe/ligero_test.go:16, cmd/server/main.go:22
static const int rhoInv = 2;

static std::vector<uint64_t> witness(int rows, int cols, const std::string &kind) {
    if (kind == "max") return std::vector<uint64_t>((size_t)rows * cols, Modulus - 1);
    return core::RandomMatrixRowMajor(rows, cols, Modulus);
}

static int host_mode(int argc, char **argv) {
    REQUIRE(argc >= 7, "usage: host <rows> <cols> <random|max> <matrix.bin> <z>...");
    const int rows = atoi(argv[2]), cols = atoi(argv[3]);
    const std::vector<uint64_t> m = witness(rows, cols, argv[4]);
    FILE *f = fopen(argv[5], "wb");
    REQUIRE(f && fwrite(m.data(), 8, m.size(), f) == m.size(), "cannot write %s", argv[5]);
    fclose(f);
    core::PrimeField field(Modulus, 2);
    const core::DensePoly poly = core::NewDensePolyFromMatrix(m, rows, cols);
    for (int a = 6; a < argc; a++) {
        const uint64_t z = strtoull(argv[a], nullptr, 10);
        printf("value %llu %llu\n", (unsigned long long)z, (unsigned long long)poly.Evaluate(field, z));
    }
    return 0;
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 6, "usage: e2e <logN> <rows> <cols> <numQ> [world]");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), numQ = atoi(argv[5]);
    const int world = argc > 6 ? atoi(argv[6]) : 1;
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
    lo_rng_seed(&rng, 7);
    std::vector<uint64_t> sk((size_t)(L + K) * N), pk((size_t)2 * (L + K) * N);
    lo_keygen_secret(op, &rng, sk.data());
    lo_keygen_public(op, &rng, sk.data(), pk.data());
    std::map<uint64_t, std::vector<uint64_t>> evk;
    for (uint64_t g : params.GaloisElementsUsedByInnerSum(rows)) {
        evk[g].resize(lo_evk_words(op));
        lo_keygen_galois(op, &rng, sk.data(), g, evk[g].data());
    }
    core::PrimeField ptField(params.PlaintextModulus(), cols * 2);
    fhe::ServerBFV server(&ptField, params, pk, evk);

    const std::vector<uint64_t> matrix = core::RandomMatrixRowMajor(rows, cols, Modulus);
    std::vector<uint64_t> columns((size_t)cols * rows); // [cols][rows]: what EncryptColumnsNew takes
    for (int j = 0; j < cols; j++)
        for (int i = 0; i < rows; i++) columns[(size_t)j * rows + i] = matrix[(size_t)i * cols + j];
    // the client's point: random, != 0 and != 1 (the twin of TestLigeroE2E proves at 1 only)
    const uint64_t z = random_point(Modulus);
    printf("point z = %llu\n", (unsigned long long)z);

    fhe::Ciphertexts cts = server.EncryptColumnsNew(columns, rows, cols);
    fhe::LigeroCommitter ligero = fhe::LigeroCommitter::NewLigeroCommitter(128, rows, cols, rhoInv);
    core::Span *span = core::Span::StartSpan("Commit FHE evaluation", nullptr);
    auto commit = ligero.Commit(cts, server, span);
    span->End();
    delete span;
    core::Transcript transcript("test");
    span = core::Span::StartSpan("Prove FHE evaluation", nullptr);
    fhe::EncryptedProof proof = commit.first.Prove(z, server, transcript, span);
    span->End();
    delete span;

    // cmd/server/main.go:255-258 on the device, then the reference's Horner on the host
    const uint64_t value = server.EvaluateColumns(columns, rows, cols, cols, z);
    core::Span *hspan = core::Span::StartSpan("Evaluate polynomial (host Horner)", nullptr);
    const uint64_t horner = core::NewDensePolyFromMatrix(matrix, rows, cols).Evaluate(ptField, z);
    hspan->End();
    delete hspan;
    REQUIRE(value == horner, "device P(z) = %llu, host Horner %llu", (unsigned long long)value, (unsigned long long)horner);

    // the client: decrypt MatZ (slot 0 of every column) on the device, InnerProduct(MatZ, a) with a = [1, z, z^2, ...]
    REQUIRE(proof.MatZ.Blocks.size() == 1, "MatZ blocks");
    REQUIRE(!lumen_load_secret_key(server.Context(), sk.data()), "lumen_load_secret_key: %s", lumen_last_error(server.Context()));
    std::vector<uint64_t> matZ((size_t)cols);
    REQUIRE(!lumen_decrypt(server.Context(), proof.MatZ.Blocks[0].Handle(), proof.MatZ.Scale(), 1, matZ.data()),
            "lumen_decrypt: %s", lumen_last_error(server.Context()));
    uint64_t claim = 0, a = 1;
    for (int j = 0; j < cols; j++) claim = ptField.Add(claim, ptField.Mul(a, matZ[(size_t)j])), a = ptField.Mul(a, z);
    REQUIRE(claim == value, "InnerProduct(MatZ, a) = %llu, P(z) = %llu", (unsigned long long)claim, (unsigned long long)value);

    // uneven column blocks, each evaluated at its first column: the partials sum to P(z)
    core::Span::quiet = true;
    const int cuts[] = {0, 1, cols / 3, cols / 3 + 7 < cols ? cols / 3 + 7 : cols, cols};
    uint64_t sum = 0;
    for (int k = 0; k + 1 < (int)(sizeof(cuts) / sizeof(cuts[0])); k++) {
        const int c0 = cuts[k], n = cuts[k + 1] - cuts[k];
        if (n <= 0) continue;
        std::vector<uint64_t> block(columns.begin() + (size_t)c0 * rows, columns.begin() + (size_t)(c0 + n) * rows);
        sum = ptField.Add(sum, server.EvaluateColumns(block, rows, n, cols, z, (uint64_t)c0));
    }
    core::Span::quiet = false;
    REQUIRE(sum == value, "column blocks sum to %llu, P(z) = %llu", (unsigned long long)sum, (unsigned long long)value);
    printf("PASS claimed value: rows=%d cols=%d LogN=%d P(z) = InnerProduct(MatZ, a) = host Horner = %llu\n", rows, cols,
           LogN, (unsigned long long)value);

    if (world > 1) {
        std::vector<std::unique_ptr<fhe::ServerBFV>> copies;
        std::vector<fhe::ServerBFV *> ranks{&server};
        for (int k = 1; k < world; k++) {
            copies.push_back(server.CopyNew());
            ranks.push_back(copies.back().get());
        }
        fhe::ServerGroup group(ranks, LUMEN_TRANSPORT_AUTO);
        const uint64_t gv = group.EvaluateColumns(columns, rows, cols, cols, z);
        REQUIRE(gv == value, "ServerGroup W=%d: P(z) = %llu, one GPU %llu", world, (unsigned long long)gv, (unsigned long long)value);
        printf("PASS ServerGroup W=%d (%s): same P(z)\n", world, group.Transport().c_str());
    }
    lo_params_free(op);
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_poly_eval_host host|e2e ...",
                     {{"host", host_mode}, {"e2e", e2e_mode}});
}
