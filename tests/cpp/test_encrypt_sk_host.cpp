// The client's own encryptor (fhe/bfv.go:77) through the host mirror: the witness is encrypted under the SECRET key on
// the client's device and uploaded in seeded form; the server expands it with no key and proves.
//   test_encrypt_sk_host e2e <logN> <rows> <cols> <numQ>
//       GPU: ClientBFV::NewWithGeneratedSecret -> KeyGenerator::GenKeySetNew; ClientBFV::EncryptColumnsSeeded(witness);
//       ServerBFV::NewFromKeySet -> ExpandSeeded -> Commit -> Prove -> MarshalBinary; the client unmarshals, decrypts and
//       verifies.  MatR / MatZ and the opened columns equal LigeroProveReference's, value + 1 is refused, the expanded
//       set equals the client's own full encryption under the same seeds, and a c0 with one word changed no longer
//       verifies.
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

// the server's whole answer to an uploaded witness, then the client's check of it; throws what Verify throws
static fhe::Proof prove_and_open(fhe::ServerBFV &server, fhe::ClientBFV &client, fhe::LigeroCommitter &ligero,
                                 const fhe::SeededCiphertexts &upload, uint64_t z) {
    fhe::Ciphertexts cts = server.ExpandSeeded(upload);
    auto commit = ligero.Commit(cts, server, nullptr);
    core::Transcript transcript("demo");
    fhe::EncryptedProof proof = commit.first.Prove(z, server, transcript, nullptr);
    const fhe::MetaData meta = proof.QueriedCols.Meta;
    const std::vector<uint8_t> marshaled = proof.MarshalBinary();
    fhe::EncryptedProof ep = fhe::EncryptedProof::UnmarshalBinary(marshaled.data(), marshaled.size(), client, meta);
    return ep.Decrypt(client, nullptr);
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 6, "usage: e2e <logN> <rows> <cols> <numQ>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), numQ = atoi(argv[5]);
    const fhe::Parameters params = make_params(LogN, cols, numQ);
    const size_t N = (size_t)params.N(), L = params.Q.size();
    core::PrimeField ptField(params.PlaintextModulus(), cols * rhoInv);

    // ---- the client: keys generated on the device, the witness encrypted under the secret one
    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    const fhe::KeySet keys = kgen.GenKeySetNew(rows, 0);
    const std::vector<uint64_t> matrix = core::RandomMatrixRowMajor(rows, cols, Modulus);
    std::vector<uint64_t> columns((size_t)cols * rows);
    for (int j = 0; j < cols; j++)
        for (int i = 0; i < rows; i++) columns[(size_t)j * rows + i] = matrix[(size_t)i * cols + j];
    fhe::SeededCiphertexts upload = client->EncryptColumnsSeeded(columns, rows, cols);
    REQUIRE(upload.Count == cols && upload.C0.size() == (size_t)cols * L * N, "the seeded upload is not [cols][L][N]");
    const uint8_t zero32[32] = {0};
    REQUIRE(memcmp(upload.ASeed.data(), zero32, 32) != 0, "the public seed is all zero");
    {
        const std::vector<uint64_t> two(columns.begin(), columns.begin() + (size_t)2 * rows);
        const fhe::SeededCiphertexts again = client->EncryptColumnsSeeded(two, rows, 2);
        REQUIRE(again.ASeed != upload.ASeed, "two calls share a public seed");
    }
    printf("PASS seeded upload: %d columns, %.1f MB instead of %.1f MB\n", cols, (double)upload.C0.size() * 8 / 1e6,
           (double)upload.C0.size() * 16 / 1e6);

    // ---- the server: no secret, and no use of its public key
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);
    {
        const std::vector<uint64_t> expanded = server->ExpandSeeded(upload).Download();
        const std::vector<uint64_t> own =
            client->EncryptColumnsUnderSeedForTest(columns, rows, cols, upload.ASeed, upload.FirstIndex).Download();
        REQUIRE(expanded.size() == (size_t)cols * 2 * L * N && expanded == own,
                "the expanded set differs from the client's full encryption under the same seeds");
        for (int j = 0; j < cols; j += 97)
            REQUIRE(!memcmp(&expanded[(size_t)j * 2 * L * N], &upload.C0[(size_t)j * L * N], L * N * 8), "c0 of column %d", j);
        printf("PASS ExpandSeeded = the client's EncryptColumnsNew under the same seeds, bit for bit\n");
    }
    const uint64_t z = random_point(Modulus);
    fhe::LigeroCommitter ligero = fhe::LigeroCommitter::NewLigeroCommitter(128, rows, cols, rhoInv);
    const uint64_t value = server->EvaluateColumns(columns, rows, cols, cols, z);
    core::Transcript refTranscript("demo");
    const fhe::Proof ref = fhe::LigeroProveReference(ligero, matrix, z, ptField, refTranscript);

    fhe::Proof plain = prove_and_open(*server, *client, ligero, upload, z);
    REQUIRE(plain.MatR == ref.MatR && plain.MatZ == ref.MatZ, "MatR / MatZ differ from LigeroProveReference's");
    for (size_t k = 0; k < ref.QueriedCols.size(); k++)
        REQUIRE(plain.QueriedCols[k] == ref.QueriedCols[k], "opened column %zu decrypts to other values than the plain prover's", k);
    printf("PASS decrypt: MatR / MatZ / opened columns = LigeroProveReference's\n");
    {
        core::Transcript vt("demo");
        plain.Verify(z, value, *client->Field(), vt, *client);
        printf("PASS client verify: rows=%d cols=%d LogN=%d, witness encrypted under the secret key\n", rows, cols, LogN);
    }
    bool threw = false;
    try {
        core::Transcript t2("demo");
        plain.Verify(z, (value + 1) % Modulus, *client->Field(), t2, *client);
    } catch (const std::runtime_error &) {
        threw = true;
    }
    REQUIRE(threw, "Verify accepted value + 1");
    printf("PASS value + 1 is refused\n");

    // ---- one word of one c0 changed on the way: the proof over it no longer verifies
    fhe::SeededCiphertexts bad = upload;
    uint64_t &w = bad.C0[((size_t)5 * L + 0) * N + 7];
    w = (w + 1) % params.Q[0];
    threw = false;
    std::string what;
    try {
        fhe::Proof p2 = prove_and_open(*server, *client, ligero, bad, z);
        core::Transcript t3("demo");
        p2.Verify(z, value, *client->Field(), t3, *client);
    } catch (const std::runtime_error &e) {
        threw = true, what = e.what();
    }
    REQUIRE(threw, "Verify accepted a proof over a c0 with one word changed");
    printf("PASS a changed c0 word is refused (%s)\n", what.c_str());
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_encrypt_sk_host e2e <logN> <rows> <cols> <numQ>",
                     {{"e2e", e2e_mode}});
}
