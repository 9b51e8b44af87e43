// The client of TestLigeroPPD (cmd/client/main.go:203-208, -vdec) up to lazer, through the host mirror.
//   test_vdec_host host <name> <rows> <cols> <T>
//       CPU: vdec::BatchColumns over a deterministic matrix under the transcript <name>; prints the challenges and the
//       batched column for tests/test_vdec_host.py to compare with the oracle's transcript and Python integers.
//   test_vdec_host e2e <logN> <rows> <cols>
//       GPU, T = 0x3ee0001 (the reference's vdec tests, vdec/batching_test.go): generated keys, client encryption,
//       Commit, Prove, Unmarshal, Decrypt, Proof::ProveDecrypt.  The witness satisfies ct0 + ct1 * sk - mDelta = err
//       mod q_0 (recomputed here by a schoolbook negacyclic product), |err| * 2T < q_0, a second ProveDecrypt gives the
//       same witness, and a proof without QueriedCts throws.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "twin.hpp"

using namespace lumenos;

static const uint64_t Modulus = 0x3ee0001ull; // ring_switch_test.go:17, the vdec tests' plaintext modulus
static const int rhoInv = 2;

static std::vector<std::vector<uint64_t>> columns_of(const std::vector<uint64_t> &matrix, int rows, int cols) {
    std::vector<std::vector<uint64_t>> c((size_t)cols, std::vector<uint64_t>((size_t)rows));
    for (int j = 0; j < cols; j++)
        for (int i = 0; i < rows; i++) c[(size_t)j][(size_t)i] = matrix[(size_t)i * cols + j];
    return c;
}

static int host_mode(int argc, char **argv) {
    REQUIRE(argc >= 6, "usage: host <name> <rows> <cols> <T>");
    const int rows = atoi(argv[3]), cols = atoi(argv[4]);
    const uint64_t T = strtoull(argv[5], nullptr, 10);
    core::PrimeField field(T, 16);
    core::Transcript transcript(argv[2]);
    const auto colMajor = columns_of(core::RandomMatrixRowMajor(rows, cols, T), rows, cols);
    const auto batched = vdec::BatchColumns(colMajor, field, transcript);
    REQUIRE((int)batched.first.size() == rows && (int)batched.second.size() == cols, "shapes");
    for (int j = 0; j < cols; j++)
        for (int i = 0; i < rows; i++)
            printf("col %d %d %llu\nalpha %d %d %llu\n", j, i, (unsigned long long)colMajor[(size_t)j][(size_t)i], j, i,
                   (unsigned long long)batched.second[(size_t)j][(size_t)i]);
    for (int i = 0; i < rows; i++) printf("m %d %llu\n", i, (unsigned long long)batched.first[(size_t)i]);
    printf("next %llu\n", (unsigned long long)transcript.SampleUint64("pod_alpha")); // where the transcript stands
    return 0;
}

static int64_t centred(unsigned __int128 x, uint64_t q) {
    const uint64_t v = (uint64_t)(x % q);
    return v > q / 2 ? -(int64_t)(q - v) : (int64_t)v;
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 5, "usage: e2e <logN> <rows> <cols>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]);
    const fhe::Parameters params = fhe::Parameters::FromLiteral(fhe::GenerateBGVParamsForNTT(cols, LogN, Modulus));
    const size_t N = (size_t)params.N();
    const uint64_t q0 = params.Q[0], T = params.T;
    core::PrimeField ptField(T, cols * rhoInv);

    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    const fhe::KeySet keys = kgen.GenKeySetNew(rows, 0);
    const std::vector<uint64_t> matrix = core::RandomMatrixRowMajor(rows, cols, T);
    std::vector<uint64_t> columns((size_t)cols * rows);
    for (int j = 0; j < cols; j++)
        for (int i = 0; i < rows; i++) columns[(size_t)j * rows + i] = matrix[(size_t)i * cols + j];
    const fhe::SeededCiphertexts upload = client->EncryptColumnsSeeded(columns, rows, cols);

    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);
    fhe::LigeroCommitter ligero = fhe::LigeroCommitter::NewLigeroCommitter(128, rows, cols, rhoInv);
    const uint64_t z = 0x1234567ull % T;
    fhe::Ciphertexts cts = server->ExpandSeeded(upload);
    auto commit = ligero.Commit(cts, *server, nullptr);
    core::Transcript transcript("demo");
    fhe::EncryptedProof enc = commit.first.Prove(z, *server, transcript, nullptr);
    const fhe::MetaData meta = enc.QueriedCols.Meta;
    const std::vector<uint8_t> marshaled = enc.MarshalBinary();
    fhe::EncryptedProof ep = fhe::EncryptedProof::UnmarshalBinary(marshaled.data(), marshaled.size(), *client, meta);
    fhe::Proof proof = ep.Decrypt(*client, nullptr);
    {
        const uint64_t value = server->EvaluateColumns(columns, rows, cols, cols, z);
        core::Transcript vt("demo");
        proof.Verify(z, value, ptField, vt, *client);
        printf("PASS client verify: rows=%d cols=%d LogN=%d T=%llu, %d opened columns\n", rows, cols, LogN, (unsigned long long)T,
               proof.QueriedCts->Len());
    }

    const vdec::Witness w = proof.ProveDecrypt(*client, nullptr);
    REQUIRE(w.sk.size() == N && w.ct0.size() == N && w.ct1.size() == N && w.mDelta.size() == N && w.err.size() == N, "witness sizes");
    REQUIRE(w.Degree == (int)std::min<size_t>(2048, N), "Degree %d", w.Degree);
    int64_t emax = 0;
    bool ternary = true, nonzero = false;
    for (size_t i = 0; i < N; i++) {
        emax = std::max<int64_t>(emax, w.err[i] < 0 ? -w.err[i] : w.err[i]);
        ternary = ternary && w.sk[i] >= -1 && w.sk[i] <= 1;
        nonzero = nonzero || w.sk[i] != 0;
    }
    REQUIRE(ternary && nonzero, "sk is not a nonzero ternary polynomial");
    REQUIRE(emax > 0 && (unsigned __int128)emax * 2 * T < q0, "max |err| = %lld: |err| * 2T >= q_0", (long long)emax);
    printf("PASS budget: max |err| = %lld, |err| * 2T < q_0\n", (long long)emax);
    // ct0 + ct1 * sk - mDelta = err mod q_0 in Z_q0[X]/(X^N + 1), the first 64 output coefficients by the schoolbook
    for (size_t k = 0; k < 64 && k < N; k++) {
        unsigned __int128 acc = 0; // every term is lifted into [0, q0)
        auto lift = [&](int64_t v) { return (uint64_t)(v < 0 ? (int64_t)q0 + v : v); };
        for (size_t i = 0; i < N; i++) {
            const size_t j = (k + N - i) % N; // i + j = k or k + N
            const int8_t s = w.sk[j];
            if (!s) continue;
            const bool wrap = i > k; // X^N = -1
            const uint64_t c = lift(w.ct1[i]);
            acc += ((s > 0) != wrap) ? c : q0 - c;
            if (acc >> 100) acc %= q0;
        }
        acc += lift(w.ct0[k]);
        acc += q0 - lift(w.mDelta[k]);
        REQUIRE(centred(acc, q0) == w.err[k], "coefficient %zu: ct0 + ct1 * sk - mDelta = %lld, err = %lld", k,
                (long long)centred(acc, q0), (long long)w.err[k]);
    }
    printf("PASS relation: ct0 + ct1 * sk - mDelta = err mod q_0 (schoolbook, 64 coefficients)\n");

    const vdec::Witness again = proof.ProveDecrypt(*client, nullptr);
    REQUIRE(again.sk == w.sk && again.ct0 == w.ct0 && again.ct1 == w.ct1 && again.mDelta == w.mDelta && again.err == w.err,
            "a second ProveDecrypt gives another witness");
    printf("PASS a second ProveDecrypt gives the same witness\n");

    fhe::Proof bare;
    bare.Metadata = proof.Metadata, bare.QueriedCols = proof.QueriedCols; // the host values without the ciphertexts
    bool threw = false;
    std::string what;
    try {
        (void)bare.ProveDecrypt(*client, nullptr);
    } catch (const std::runtime_error &e) {
        threw = true, what = e.what();
    }
    REQUIRE(threw && what.find("QueriedCts") != std::string::npos, "a proof without QueriedCts: %s", threw ? what.c_str() : "no throw");
    printf("PASS a proof without QueriedCts is refused (%s)\n", what.c_str());
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_vdec_host host <name> <rows> <cols> <T> | e2e <logN> <rows> <cols>",
                     {{"host", host_mode}, {"e2e", e2e_mode}});
}
