// The diagonal linear transform through the host mirror, with no CPU-generated key anywhere.
//   test_lintrans_host e2e <logN> <rows> <count>
//       GPU: ClientBFV::NewWithGeneratedSecret -> KeyGenerator::GenKeySetNew(rows) for the server's constructor; the server
//       encodes a dense 8 x 8 matrix M, replicated along the slot rows, by its 8 diagonals d_k[i] = M[i mod 8][(i + k) mod 8]
//       (ServerBFV::NewLinearTransformation) and asks for the keys of LinearTransformation::GaloisElements(), which the
//       client generates (KeyGenerator::GenGaloisKeysNew, ServerBFV::LoadGaloisKeys); the client encrypts `count` columns
//       of N slot values under its secret key and uploads them in seeded form, column 0 of period 8; the server applies
//       LinearTransformationNew; the client decrypts and finds sum_k d_k[i] * v[(i + k) mod N/2] modulo T on both slot
//       rows -- on column 0 the plain product M x.  LinearTransformationsNew gives the single results.
//   T = 0x3ee0001 (the reference's vdec tests).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "twin.hpp"

using namespace lumenos;

static const uint64_t T = 0x3ee0001ull;

static uint64_t mulmod(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % T); }

// sum_k d_k[i] * x[(i + k) mod N/2] on each slot row of the columns x, [count][N]
static std::vector<uint64_t> transformed(const std::vector<uint64_t> &x, int N, const std::map<int, std::vector<uint64_t>> &diags) {
    const long h = N / 2;
    std::vector<uint64_t> out(x.size(), 0);
    for (size_t c = 0; c < x.size() / N; c++)
        for (const auto &kv : diags)
            for (long row = 0; row < 2; row++)
                for (long i = 0; i < h; i++) {
                    uint64_t &o = out[c * N + row * h + i];
                    o = (o + mulmod(kv.second[row * h + i], x[c * N + row * h + (((i + kv.first) % h) + h) % h])) % T;
                }
    return out;
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 5, "usage: e2e <logN> <rows> <count>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), count = atoi(argv[4]);
    fhe::ParametersLiteral lit;
    lit.LogN = LogN, lit.LogQ = {58, 56, 56}, lit.LogP = {55, 55}, lit.PlaintextModulus = T;
    const fhe::Parameters params = fhe::Parameters::FromLiteral(lit);
    const int N = params.N(), h = N / 2;
    core::PrimeField ptField(T, 64);

    // ---- the client: every key generated on the device
    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    const fhe::KeySet keys = kgen.GenKeySetNew(rows, LUMEN_KEY_MONTGOMERY);
    std::vector<uint64_t> x = random_values((size_t)count * N, T);
    for (int i = 8; i < N; i++) x[i] = x[i % 8]; // column 0: a vector of 8 replicated along both rows
    const fhe::SeededCiphertexts up = client->EncryptColumnsSeeded(x, N, count);

    // ---- the server: the matrix by its diagonals, at the level of the columns
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);
    fhe::Ciphertexts cx = server->ExpandSeeded(up);
    REQUIRE(decrypt(*server, *client, cx, N) == x, "the columns do not decrypt to themselves");
    const std::vector<uint64_t> M = random_values(64, T);
    std::map<int, std::vector<uint64_t>> diags;
    for (int k = 0; k < 8; k++) {
        std::vector<uint64_t> d(N);
        for (int i = 0; i < N; i++) d[i] = M[((i % h) % 8) * 8 + ((i % h) + k) % 8];
        diags[k] = d;
    }
    {
        const fhe::Plaintext q = server->Encode(diags[3]), qp = server->EncodeQP(diags[3], params.MaxLevel());
        REQUIRE(qp.Value.size() == (params.Q.size() + params.P.size()) * (size_t)N && qp.Level == params.MaxLevel(), "shape of EncodeQP");
        REQUIRE(!memcmp(q.Value.data(), qp.Value.data(), q.Value.size() * 8), "EncodeQP's limbs of Q are not Encode's");
    }
    fhe::LinearTransformation lt = server->NewLinearTransformation(diags, cx.Level());
    const std::vector<uint64_t> els = lt.GaloisElements();
    REQUIRE(els.size() == 7 && lt.Level() == cx.Level(), "GaloisElements() of 8 diagonals: %zu elements", els.size());
    for (int k = 1; k < 8; k++) REQUIRE(els[k - 1] == params.GaloisElement(k), "element of diagonal %d", k);
    {
        bool threw = false;
        std::string what;
        try {
            server->LinearTransformationNew(cx, lt);
        } catch (const std::runtime_error &e) {
            threw = true, what = e.what();
        }
        REQUIRE(threw && what.find("not loaded") != std::string::npos, "a server without the keys transformed (%s)", what.c_str());
    }
    const std::map<uint64_t, std::vector<uint64_t>> gks = kgen.GenGaloisKeysNew(els, LUMEN_KEY_MONTGOMERY);
    REQUIRE(gks.size() == els.size(), "GenGaloisKeysNew returned %zu keys for %zu elements", gks.size(), els.size());
    server->LoadGaloisKeys(gks, LUMEN_KEY_MONTGOMERY);
    const int before = server->MulCounter();
    const std::vector<uint64_t> words = cx.Download();

    fhe::Ciphertexts y = server->LinearTransformationNew(cx, lt);
    REQUIRE(y.Len() == count && y.Level() == cx.Level() && y.Scale() == cx.Scale(), "shape / scale of the transform");
    const std::vector<uint64_t> got = decrypt(*server, *client, y, N), want = transformed(x, N, diags);
    REQUIRE(got == want, "LinearTransformationNew: other slots than sum_k d_k[i] v[i + k]");
    for (int i = 0; i < N; i++) {
        uint64_t mx = 0;
        for (int c = 0; c < 8; c++) mx = (mx + mulmod(M[((i % h) % 8) * 8 + c], x[c])) % T;
        REQUIRE(got[i] == mx, "slot %d of column 0 is not (M x)[%d]", i, (i % h) % 8);
    }
    REQUIRE(server->MulCounter() == before && cx.Download() == words, "MulCounter moved / the input changed");
    printf("PASS LinearTransformationNew: a dense 8 x 8 matrix on %d columns of %d slots (LogN=%d)\n", count, N, LogN);

    {
        std::map<int, std::vector<uint64_t>> only0 = {{0, diags[5]}}, back = {{-2, diags[1]}};
        fhe::LinearTransformation lt0 = server->NewLinearTransformation(only0, cx.Level());
        REQUIRE(lt0.GaloisElements().empty(), "diagonal 0 alone needs a key");
        fhe::LinearTransformation ltb = server->NewLinearTransformation(back, cx.Level());
        server->LoadGaloisKeys(kgen.GenGaloisKeysNew(ltb.GaloisElements(), LUMEN_KEY_MONTGOMERY), LUMEN_KEY_MONTGOMERY);
        std::vector<fhe::Ciphertexts> outs = server->LinearTransformationsNew(cx, {&lt, &lt0, &ltb});
        REQUIRE(outs.size() == 3, "LinearTransformationsNew returned %zu sets", outs.size());
        server->check(lumen_sync(server->Context()), "lumen_sync");
        REQUIRE(outs[0].Download() == y.Download(), "LinearTransformationsNew and LinearTransformationNew differ");
        fhe::Ciphertexts prod = server->MulNew(cx, server->Encode(diags[5]));
        server->check(lumen_sync(server->Context()), "lumen_sync");
        REQUIRE(outs[1].Download() == prod.Download(), "diagonal 0 alone is not MulNew");
        REQUIRE(decrypt(*server, *client, outs[2], N) == transformed(x, N, back), "the diagonal -2");
        REQUIRE(server->LinearTransformationsNew(cx, {}).empty(), "no transformation, but a set");
        fhe::LinearTransformation moved = std::move(ltb);
        REQUIRE(!ltb.Handle() && moved.Handle() && moved.GaloisElements().size() == 1, "a moved transformation");
        std::unique_ptr<fhe::ServerBFV> copy = server->CopyNew();
        fhe::Ciphertexts again = copy->LinearTransformationNew(cx, lt);
        copy->check(lumen_sync(copy->Context()), "lumen_sync");
        REQUIRE(again.Download() == y.Download(), "a CopyNew computes other words");
        printf("PASS LinearTransformationsNew = the single results; diagonal 0 alone = MulNew; CopyNew shares keys and transform\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_lintrans_host e2e <logN> <rows> <count>",
                     {{"e2e", e2e_mode}});
}
