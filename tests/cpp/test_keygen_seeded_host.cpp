// Seeded switching keys through the host mirror: the protocol of test_keygen_host.cpp (cmd/client/main.go:64-81, the
// `/keys` handler of cmd/server/main.go:66, prove, decrypt, verify) run twice on one witness encryption and one commitment --
//   run 1: the server holds the SEEDED set (fhe::KeyGenerator::GenKeySetSeeded -> ServerBFV::NewFromKeySet): b halves
//          and one public seed, the `a` halves drawn on the device;
//   run 2: the same server after FULL keys were loaded over them, assembled here from the same b words and the `a`
//          halves expanded on the CPU (ChaCha20 of the oracle, the sampling contract's rejection rule).
// Both runs must give the same Merkle root and a byte-identical marshalled proof, and the client must verify it.
//   test_keygen_seeded_host e2e <logN> <rows> <cols> <numQ>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../oracle/lo_common.h"
#include "twin.hpp"

using namespace lumenos;

static const uint64_t Modulus = 144115188075593729ull; // fhe/ligero_test.go:16, cmd/server/main.go:22
static const int rhoInv = 2;

// a of limb m (modulus q) of the entry with sample index I under aSeed: stream 16 + m as little-endian 64-bit words,
// attempt t of coefficient k is word t * N + k, the first x < 2^64 - (2^64 mod q) is kept as x mod q
static void expand_a(const uint8_t aSeed[32], uint64_t I, uint32_t m, uint64_t q, size_t N, uint64_t *a) {
    uint8_t nonce[12];
    for (int i = 0; i < 8; i++) nonce[i] = (uint8_t)(I >> (8 * i));
    const uint32_t stream = 16 + m;
    for (int i = 0; i < 4; i++) nonce[8 + i] = (uint8_t)(stream >> (8 * i));
    const uint64_t r64 = (uint64_t)(((unsigned __int128)1 << 64) % q), bound = 0 - r64;
    std::vector<uint8_t> buf(N * 8);
    std::vector<char> done(N, 0);
    size_t left = N;
    for (uint32_t t = 0; left; t++) {
        std::fill(buf.begin(), buf.end(), 0);
        lo_chacha20_xor(aSeed, nonce, (uint32_t)(t * (N / 8)), buf.data(), buf.size());
        for (size_t k = 0; k < N; k++) {
            if (done[k]) continue;
            uint64_t x = 0;
            for (int i = 0; i < 8; i++) x |= (uint64_t)buf[k * 8 + i] << (8 * i);
            if (x < bound) a[k] = x % q, done[k] = 1, left--;
        }
    }
}

// b [beta][L+K][N] + the expanded a -> [beta][b|a][L+K][N]
static std::vector<uint64_t> full_key(const std::vector<uint64_t> &b, const uint8_t aSeed[32], uint64_t keyId,
                                      const std::vector<uint64_t> &moduli, size_t beta, size_t N) {
    const size_t LK = moduli.size();
    std::vector<uint64_t> key(beta * 2 * LK * N);
    for (size_t d = 0; d < beta; d++)
        for (size_t m = 0; m < LK; m++) {
            memcpy(&key[((d * 2 + 0) * LK + m) * N], &b[(d * LK + m) * N], N * 8);
            expand_a(aSeed, keyId * 4096 + d, (uint32_t)m, moduli[m], N, &key[((d * 2 + 1) * LK + m) * N]);
        }
    return key;
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc == 6, "usage: e2e <logN> <rows> <cols> <numQ>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]), numQ = atoi(argv[5]);
    const fhe::Parameters params = make_params(LogN, cols, numQ);
    const size_t N = (size_t)params.N(), L = params.Q.size(), K = params.P.size(), beta = (L + K - 1) / K;
    std::vector<uint64_t> moduli(params.Q);
    moduli.insert(moduli.end(), params.P.begin(), params.P.end());
    core::PrimeField ptField(params.PlaintextModulus(), cols * rhoInv);

    // ---- the client: every key generated on the device, the switching keys in seeded form
    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    const fhe::SeededKeySet seeded = kgen.GenKeySetSeeded(rows, 0, true);
    const size_t bWords = beta * (L + K) * N;
    const std::vector<uint64_t> galEls = params.GaloisElementsForInnerSum(1, rows);
    for (uint64_t g : galEls) REQUIRE(seeded.GaloisB.count(g) && seeded.GaloisB.at(g).size() == bWords, "b half of element %llu", (unsigned long long)g);
    REQUIRE(seeded.RlkB.size() == bWords && seeded.Pk.size() == 2 * (L + K) * N, "relinearisation b / pk sizes");
    const uint8_t zero32[32] = {0};
    REQUIRE(memcmp(seeded.ASeed.data(), client->KeySeed(), 32) != 0 && memcmp(seeded.ASeed.data(), zero32, 32) != 0,
            "the public seed is the secret seed, or was never drawn");
    {
        // ONE public seed per keygen seed: a second set of this client's is the same seed and, key by key, the same words
        // (a key under two different `a` would give the secret away); another client has another seed
        REQUIRE(seeded.ASeed == client->PublicKeySeed(), "the set is not under the client's public seed");
        const fhe::SeededKeySet again = kgen.GenGaloisKeysSeeded({galEls[0]});
        REQUIRE(again.ASeed == seeded.ASeed, "two key sets of one client are under two public seeds");
        REQUIRE(again.GaloisB.at(galEls[0]) == seeded.GaloisB.at(galEls[0]), "a key generated again has other words");
        fhe::SeededKeySet rl; // the relinearisation key alone: still the client's seed, the same b
        kgen.GenRelinearizationKeySeeded(rl);
        REQUIRE(rl.ASeed == seeded.ASeed && rl.RlkB == seeded.RlkB, "a set of rlk alone");
        REQUIRE(client->CopyNew()->PublicKeySeed() == seeded.ASeed, "a CopyNew has another public seed");
        std::unique_ptr<fhe::ClientBFV> other = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
        REQUIRE(other->PublicKeySeed() != seeded.ASeed && memcmp(other->PublicKeySeed().data(), other->KeySeed(), 32) != 0,
                "two clients share a public seed, or one's is its secret seed");
        // one form per key: the full form of a key that left in seeded form is refused before anything is generated, and
        // the other way round; a set under a foreign seed is refused
        int refused = 0;
        try {
            kgen.GenGaloisKeysNew({galEls[0]});
        } catch (const std::logic_error &) {
            refused++;
        }
        try {
            kgen.GenRelinearizationKeyNew();
        } catch (const std::logic_error &) {
            refused++;
        }
        fhe::KeyGenerator okgen(*other);
        okgen.GenRelinearizationKeyNew();
        try {
            fhe::SeededKeySet o;
            okgen.GenRelinearizationKeySeeded(o);
        } catch (const std::logic_error &) {
            refused++;
        }
        try {
            fhe::SeededKeySet foreign = again; // this client's seed, the other client's generator
            okgen.GenRelinearizationKeySeeded(foreign);
        } catch (const std::invalid_argument &) {
            refused++;
        }
        REQUIRE(refused == 4, "%d of 4 second forms / foreign seeds were refused", refused);
        okgen.GenGaloisKeysNew({galEls[0]}); // a key that never left in seeded form: the full form is fine
    }
    size_t galWords = 0;
    for (const auto &kv : seeded.GaloisB) galWords += kv.second.size();
    printf("PASS seeded keys generated on the device: %zu Galois keys + rlk, %.1f MB of b halves for %.1f MB of keys\n",
           seeded.GaloisB.size(), (double)(galWords + bWords) * 8 / 1e6, (double)(galWords + bWords) * 16 / 1e6);

    // ---- run 1: the server loads the seeded set
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, seeded);
    const std::vector<uint64_t> matrix = core::RandomMatrixRowMajor(rows, cols, Modulus);
    std::vector<uint64_t> columns((size_t)cols * rows);
    for (int j = 0; j < cols; j++)
        for (int i = 0; i < rows; i++) columns[(size_t)j * rows + i] = matrix[(size_t)i * cols + j];
    const uint64_t z = random_point(Modulus);
    fhe::LigeroCommitter ligero = fhe::LigeroCommitter::NewLigeroCommitter(128, rows, cols, rhoInv);
    fhe::Ciphertexts cts = server->EncryptColumnsNew(columns, rows, cols);
    fhe::Ciphertexts pair = server->EncryptColumnsNew(std::vector<uint64_t>(columns.begin(), columns.begin() + 2 * (size_t)rows), rows, 2);
    const uint64_t value = server->EvaluateColumns(columns, rows, cols, cols, z);

    struct Run {
        std::vector<uint8_t> root, marshaled;
        std::vector<uint64_t> product;
        fhe::MetaData meta;
    };
    // ONE commitment for all runs: Commit needs no switching key, and it draws a fresh encryption of zero for the padding
    // columns (code.go:15-22), so two Commits never agree.  What the keys decide is Prove: the two inner products.
    auto commit = ligero.Commit(cts, *server, nullptr);
    auto prove = [&](Run &r) {
        core::Transcript transcript("demo");
        fhe::EncryptedProof proof = commit.first.Prove(z, *server, transcript, nullptr);
        r.root = proof.Root;
        r.meta = proof.QueriedCols.Meta;
        r.marshaled = proof.MarshalBinary();
        r.product = server->MulRelinNew(pair, pair).Download(); // the relinearisation key's turn
    };
    Run seededRun, fullRun;
    prove(seededRun);

    // ---- run 2: full keys from the same b and the a halves expanded on the CPU, loaded over the seeded ones
    std::map<uint64_t, std::vector<uint64_t>> full;
    for (const auto &kv : seeded.GaloisB) full[kv.first] = full_key(kv.second, seeded.ASeed.data(), 0x10000 + kv.first, moduli, beta, N);
    server->LoadGaloisKeys(full, 0);
    server->SetRelinearizationKey(full_key(seeded.RlkB, seeded.ASeed.data(), 2, moduli, beta, N), 0);
    prove(fullRun);
    REQUIRE(seededRun.root == commit.second && fullRun.root == commit.second, "a proof carries another Merkle root than the commitment's");
    REQUIRE(seededRun.marshaled.size() == fullRun.marshaled.size() && seededRun.marshaled == fullRun.marshaled,
            "the marshalled proofs of the seeded and the full run differ");
    REQUIRE(seededRun.product == fullRun.product, "MulRelinNew differs between the seeded and the full relinearisation key");
    printf("PASS seeded and full keys: same Merkle root, byte-identical proof (%zu bytes), same MulRelinNew\n", fullRun.marshaled.size());
    // ... and back: the seeded set over the full keys
    server->LoadSeededKeys(seeded);
    Run backRun;
    prove(backRun);
    REQUIRE(backRun.marshaled == seededRun.marshaled && backRun.product == seededRun.product, "the seeded set loaded over full keys");

    // ---- the client (cmd/client/main.go:181-221) on the seeded run's bytes
    fhe::EncryptedProof ep = fhe::EncryptedProof::UnmarshalBinary(seededRun.marshaled.data(), seededRun.marshaled.size(), *client, seededRun.meta);
    fhe::Proof plain = ep.Decrypt(*client, nullptr);
    core::Transcript refTranscript("demo");
    const fhe::Proof ref = fhe::LigeroProveReference(ligero, matrix, z, ptField, refTranscript);
    REQUIRE(plain.MatR == ref.MatR && plain.MatZ == ref.MatZ, "MatR / MatZ differ from LigeroProveReference's");
    core::Transcript vt("demo");
    plain.Verify(z, value, *client->Field(), vt, *client);
    printf("PASS client verify under seeded keys: rows=%d cols=%d LogN=%d\n", rows, cols, LogN);
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_keygen_seeded_host e2e <logN> <rows> <cols> <numQ>",
                     {{"e2e", e2e_mode}});
}
