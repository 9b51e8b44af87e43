// fhe::matrixInnerSumEval below the top level of the chain, through the host mirror.
//   test_inner_product_levels_host run <logN> <rows> <cols> <numQ> <limbs>
//       GPU: a client with a generated secret posts its key set; the server encrypts `cols` columns of `rows` values,
//       rescales them to `limbs` limbs and calls matrixInnerSumEval with the plaintext at that level.  The result is at
//       level 1 with the scale the rescales leave, and the client decrypts slot 0 of every column to sum_i r_i col_i --
//       the values the top-level call on the unrescaled matrix decrypts to.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "twin.hpp"

using namespace lumenos;

static const uint64_t Modulus = 144115188075593729ull; // fhe/ligero_test.go:16, cmd/server/main.go:22

// slot 0 of every ciphertext of `cts` (resident on the server), decrypted by the client
static int decrypt_slot0(fhe::ClientBFV &client, const fhe::Ciphertexts &cts, std::vector<uint64_t> &out) {
    const std::vector<uint64_t> host = cts.Download();
    const uint32_t count = (uint32_t)cts.Len();
    lumen_set *s = nullptr;
    REQUIRE(!lumen_set_create(client.Context(), count, (uint32_t)cts.Level() + 1, &s), "set: %s", lumen_last_error(client.Context()));
    int rc = lumen_set_upload(client.Context(), s, 0, count, host.data());
    out.assign(count, 0);
    if (!rc) rc = lumen_decrypt(client.Context(), s, cts.Scale(), 1, out.data());
    lumen_set_destroy(client.Context(), s);
    REQUIRE(!rc, "decrypt: %s", lumen_last_error(client.Context()));
    return 0;
}

static int run_mode(int argc, char **argv) {
    REQUIRE(argc >= 7, "usage: run <logN> <rows> <cols> <numQ> <limbs>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), numQ = atoi(argv[5]), limbs = atoi(argv[6]);
    fhe::ParametersLiteral lit = fhe::GenerateBGVParamsForNTT(cols, LogN, Modulus);
    while ((int)lit.LogQ.size() < numQ) lit.LogQ.push_back(56);
    const fhe::Parameters params = fhe::Parameters::FromLiteral(lit);
    const size_t N = (size_t)params.N();
    REQUIRE((int)params.Q.size() == numQ && limbs >= 1 && limbs < numQ, "%d limbs of a chain of %zu", limbs, params.Q.size());
    core::PrimeField ptField(params.PlaintextModulus(), cols * 2);

    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    const fhe::KeySet keys = kgen.GenKeySetNew(rows, 0);
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);

    const std::vector<uint64_t> columns = core::RandomMatrixRowMajor(cols, rows, Modulus); // [cols][rows]
    const std::vector<uint64_t> r = core::RandomMatrixRowMajor(1, rows, Modulus);
    std::vector<uint64_t> want((size_t)cols);
    for (int j = 0; j < cols; j++) {
        unsigned __int128 acc = 0;
        for (int i = 0; i < rows; i++) acc = (acc + (unsigned __int128)columns[(size_t)j * rows + i] * r[(size_t)i]) % Modulus;
        want[(size_t)j] = (uint64_t)acc;
    }

    fhe::Ciphertexts top = server->EncryptColumnsNew(columns, rows, cols);
    REQUIRE(top.Level() == params.MaxLevel(), "the witness is not at the top level");
    const fhe::Plaintext pt = server->Encode(r);

    // Rescale looped down to `limbs` limbs, as a host that lowers the matrix before the inner product would
    lumen_set *low_set = nullptr;
    server->check(lumen_rescale(server->Context(), top.Handle(), (uint32_t)limbs, &low_set), "lumen_rescale");
    fhe::MetaData md = top.Meta;
    md.Scale = fhe::RescaledScale(params, md.Scale, top.Level(), limbs - 1);
    fhe::Ciphertexts low(server->Context(), low_set, md);
    REQUIRE(low.Level() == limbs - 1, "the rescaled matrix is at level %d", low.Level());
    fhe::Plaintext ptLow; // the plaintext at the matrix's level: the first `limbs` limbs of the encoding
    ptLow.Level = limbs - 1;
    ptLow.Value.assign(pt.Value.begin(), pt.Value.begin() + (size_t)limbs * N);

    fhe::Ciphertexts out = fhe::matrixInnerSumEval(low, ptLow, rows, *server);
    REQUIRE(out.Len() == cols && out.Level() == 1, "the result is %d ciphertexts at level %d", out.Len(), out.Level());
    REQUIRE(out.Scale() == fhe::RescaledScale(params, 1, params.MaxLevel(), 1), "the result's scale is not the rescales'");
    std::vector<uint64_t> got;
    if (decrypt_slot0(*client, out, got)) return 1;
    for (int j = 0; j < cols; j++)
        REQUIRE(got[(size_t)j] == want[(size_t)j], "column %d at %d limbs decrypts to %llu, the inner product is %llu", j, limbs,
                (unsigned long long)got[(size_t)j], (unsigned long long)want[(size_t)j]);
    printf("PASS %d limbs: %d inner products of %d rows\n", limbs, cols, rows);

    // a plaintext at another level than the matrix is refused before the device sees it
    bool threw = false;
    try {
        (void)fhe::matrixInnerSumEval(low, pt, rows, *server);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    REQUIRE(threw, "a top-level plaintext was accepted for a lower-level matrix");
    printf("PASS level mismatch is refused\n");

    fhe::Ciphertexts outTop = fhe::matrixInnerSumEval(top, pt, rows, *server);
    if (decrypt_slot0(*client, outTop, got)) return 1;
    for (int j = 0; j < cols; j++) REQUIRE(got[(size_t)j] == want[(size_t)j], "column %d at the top level", j);
    printf("PASS top level: the same values\n");
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_inner_product_levels_host run <logN> <rows> <cols> <numQ> <limbs>",
                     {{"run", run_mode}});
}
