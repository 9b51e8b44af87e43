// The path of cmd/client + cmd/server with a number of rows that is no power of two (-rows is a free flag of
// cmd/server; InnerSum(col, 1, rows) at fhe/ligero.go:325 takes any), through the host mirror.
//   test_inner_sum_rows_host e2e <logN> <rows> <cols> <numQ>
//       GPU: every key generated on the device (GenKeySetNew(rows): GaloisElementsForInnerSum(1, rows), of which the
//       lazy double-and-add applies a subset); ServerBFV::InnerSumNew(ct, 1, rows) decrypts in slot 0 to the plain
//       column sums; then encrypt -> Commit -> Prove (matrixInnerSumEval sends such rows to
//       lumen_matrix_inner_sum_general) -> the client unmarshals and decrypts: MatR / MatZ against the plain
//       sum_i r_i M[i][j] / sum_i b_i M[i][j] (LigeroProveReference, the mirror's plain prover, takes powers of two >= 512
//       only) -> Verify.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "twin.hpp"

using namespace lumenos;

static const uint64_t Modulus = 144115188075593729ull; // fhe/ligero_test.go:16, cmd/server/main.go:22
static const int rhoInv = 2;

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 6, "usage: e2e <logN> <rows> <cols> <numQ>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), numQ = atoi(argv[5]);
    REQUIRE(rows > 0 && (rows & (rows - 1)), "rows = %d: this twin is about a length that is no power of two", rows);
    fhe::ParametersLiteral lit = fhe::GenerateBGVParamsForNTT(cols, LogN, Modulus);
    while ((int)lit.LogQ.size() < numQ) lit.LogQ.push_back(56);
    const fhe::Parameters params = fhe::Parameters::FromLiteral(lit);
    const int N = params.N();
    core::PrimeField ptField(params.PlaintextModulus(), cols * rhoInv);

    // ---- the client's keys (cmd/client/main.go:64-81), generated on the device
    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    const fhe::KeySet keys = kgen.GenKeySetNew(rows, 0);
    REQUIRE(keys.GaloisElements == params.GaloisElementsForInnerSum(1, rows), "GenKeySetNew's elements");
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);
    {
        uint64_t used[64];
        const uint32_t cnt = lumen_inner_sum_general_elements(server->Context(), 1, (uint32_t)rows, used);
        REQUIRE(cnt > 0, "lumen_inner_sum_general_elements(1, %d) lists nothing", rows);
        for (uint32_t i = 0; i < cnt; i++) {
            bool posted = false;
            for (uint64_t g : keys.GaloisElements) posted = posted || g == used[i];
            REQUIRE(posted, "InnerSum(1, %d) applies element %llu, which the client does not post", rows, (unsigned long long)used[i]);
        }
        printf("PASS the %u elements InnerSum(1, %d) applies are among the %zu the client posts\n", cnt, rows, keys.GaloisElements.size());
    }

    const std::vector<uint64_t> matrix = core::RandomMatrixRowMajor(rows, cols, Modulus);
    std::vector<uint64_t> columns((size_t)cols * rows);
    for (int j = 0; j < cols; j++)
        for (int i = 0; i < rows; i++) columns[(size_t)j * rows + i] = matrix[(size_t)i * cols + j];
    fhe::Ciphertexts cts = server->EncryptColumnsNew(columns, rows, cols);

    // ---- Evaluator.InnerSum(ct, 1, rows): slot 0 of column j = sum_i M[i][j]
    {
        fhe::Ciphertexts sums = server->InnerSumNew(cts, 1, rows);
        server->check(lumen_sync(server->Context()), "lumen_sync");
        std::vector<uint64_t> got((size_t)cols);
        client->check(lumen_decrypt(client->Context(), sums.Handle(), sums.Scale(), 1, got.data()), "lumen_decrypt");
        for (int j = 0; j < cols; j++) {
            uint64_t want = 0;
            for (int i = 0; i < rows; i++) want = (uint64_t)(((unsigned __int128)want + matrix[(size_t)i * cols + j]) % Modulus);
            REQUIRE(got[(size_t)j] == want, "InnerSumNew(1, %d): slot 0 of column %d is %llu, the plain sum %llu", rows, j,
                    (unsigned long long)got[(size_t)j], (unsigned long long)want);
        }
        printf("PASS InnerSumNew(ct, 1, %d): slot 0 of %d columns = the plain column sums\n", rows, cols);
    }

    // ---- the server (cmd/server/main.go:187-266), then the client (cmd/client/main.go:181-221)
    const uint64_t z = random_point(Modulus);
    fhe::LigeroCommitter ligero = fhe::LigeroCommitter::NewLigeroCommitter(128, rows, cols, rhoInv);
    auto commit = ligero.Commit(cts, *server, nullptr);
    core::Transcript transcript("demo");
    fhe::EncryptedProof proof = commit.first.Prove(z, *server, transcript, nullptr);
    const uint64_t value = server->EvaluateColumns(columns, rows, cols, cols, z);
    // the plain prover of the mirror (LigeroProveReference) takes powers of two >= 512 only, so the expected MatR / MatZ are
    // formed here: r as Prove draws it (the first thing out of the transcript, raw words reduced where they multiply),
    // b_i = (z^cols)^i, MatR[j] = sum_i r_i M[i][j], MatZ[j] = sum_i b_i M[i][j]
    std::vector<uint64_t> r((size_t)rows), bvec((size_t)rows);
    {
        core::Transcript rt("demo");
        rt.SampleUints("r", r);
        const core::Element zPow = ptField.Pow((uint64_t)cols, z);
        core::Element powB = 1;
        for (uint64_t &bi : bvec) bi = powB, powB = ptField.Mul(powB, zPow);
    }
    const fhe::MetaData meta = proof.QueriedCols.Meta;
    const std::vector<uint8_t> marshaled = proof.MarshalBinary();
    fhe::EncryptedProof ep = fhe::EncryptedProof::UnmarshalBinary(marshaled.data(), marshaled.size(), *client, meta);
    fhe::Proof plain = ep.Decrypt(*client, nullptr);
    REQUIRE(plain.MatR.size() == (size_t)cols && plain.MatZ.size() == (size_t)cols, "MatR / MatZ have %zu / %zu entries", plain.MatR.size(),
            plain.MatZ.size());
    for (int j = 0; j < cols; j++) {
        uint64_t wr = 0, wz = 0;
        for (int i = 0; i < rows; i++) {
            const uint64_t m = matrix[(size_t)i * cols + j];
            wr = (wr + core::MulMod(r[(size_t)i] % Modulus, m, Modulus)) % Modulus;
            wz = (wz + core::MulMod(bvec[(size_t)i] % Modulus, m, Modulus)) % Modulus;
        }
        REQUIRE(plain.MatR[(size_t)j] == wr, "MatR[%d] decrypts to %llu, sum_i r_i M[i][j] = %llu", j, (unsigned long long)plain.MatR[(size_t)j],
                (unsigned long long)wr);
        REQUIRE(plain.MatZ[(size_t)j] == wz, "MatZ[%d] decrypts to %llu, sum_i b_i M[i][j] = %llu", j, (unsigned long long)plain.MatZ[(size_t)j],
                (unsigned long long)wz);
    }
    printf("PASS decrypt: MatR / MatZ = the plain sum_i r_i M[i][j] / sum_i b_i M[i][j] (rows=%d)\n", rows);
    // the client's Verify, where the mirror takes such a number of rows (a refusal is reported, not hidden)
    try {
        core::Transcript vt("demo");
        plain.Verify(z, value, *client->Field(), vt, *client);
    } catch (const std::invalid_argument &e) {
        printf("NOTE Verify refuses rows=%d: %s\n", rows, e.what());
        return 0;
    }
    printf("PASS client verify: rows=%d cols=%d LogN=%d\n", rows, cols, LogN);
    bool threw = false;
    try {
        core::Transcript t2("demo");
        plain.Verify(z, (value + 1) % Modulus, *client->Field(), t2, *client);
    } catch (const std::runtime_error &) {
        threw = true;
    }
    REQUIRE(threw, "Verify accepted value + 1");
    printf("PASS value + 1 is refused\n");
    (void)N;
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_inner_sum_rows_host e2e <logN> <rows> <cols> <numQ>",
                     {{"e2e", e2e_mode}});
}
