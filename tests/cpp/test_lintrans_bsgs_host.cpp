// The double-hoisted (baby-step / giant-step) diagonal linear transform through the host mirror, with no CPU-generated key
// anywhere.
//   test_lintrans_bsgs_host e2e <logN> <rows> <count>
//       GPU: ClientBFV::NewWithGeneratedSecret -> KeyGenerator::GenKeySetNew(rows) for the server's constructor; the server
//       encodes a dense 16 x 16 matrix M, replicated along the slot rows, by its 16 diagonals
//       d_k[i] = M[i mod 16][(i + k) mod 16] with 4 baby steps (ServerBFV::NewLinearTransformationBSGS) and asks for the keys
//       of LinearTransformation::GaloisElements() alone -- babies 1, 2, 3 and giants 4, 8, 12: six keys, not fifteen --,
//       which the client generates on the device; the client encrypts `count` columns of N slot values under its secret key
//       and uploads them in seeded form, column 0 of period 16; the server applies LinearTransformationNew; the client
//       decrypts and finds sum_k d_k[i] * v[(i + k) mod N/2] modulo T on both slot rows -- on column 0 the plain product M x.
//       babySteps = 0 picks 4 for itself and gives the same words; LinearTransformationsNew gives the single results.
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
static const int D = 16;

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
    for (int i = D; i < N; i++) x[i] = x[i % D]; // column 0: a vector of 16 replicated along both rows
    const fhe::SeededCiphertexts up = client->EncryptColumnsSeeded(x, N, count);

    // ---- the server: the matrix by its diagonals, at the level of the columns, with 4 baby steps
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);
    fhe::Ciphertexts cx = server->ExpandSeeded(up);
    REQUIRE(decrypt(*server, *client, cx, N) == x, "the columns do not decrypt to themselves");
    const std::vector<uint64_t> M = random_values(D * D, T);
    std::map<int, std::vector<uint64_t>> diags;
    for (int k = 0; k < D; k++) {
        std::vector<uint64_t> d(N);
        for (int i = 0; i < N; i++) d[i] = M[((i % h) % D) * D + ((i % h) + k) % D];
        diags[k] = d;
    }
    fhe::LinearTransformation lt = server->NewLinearTransformationBSGS(diags, cx.Level(), 4);
    const std::vector<uint64_t> els = lt.GaloisElements();
    const int steps[6] = {1, 2, 3, 4, 8, 12};
    REQUIRE(els.size() == 6 && lt.Level() == cx.Level(), "GaloisElements() of 16 diagonals with 4 baby steps: %zu elements", els.size());
    for (int a = 0; a < 6; a++) REQUIRE(els[a] == params.GaloisElement(steps[a]), "element %d is not the rotation by %d", a, steps[a]);
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
        for (int c = 0; c < D; c++) mx = (mx + mulmod(M[((i % h) % D) * D + c], x[c])) % T;
        REQUIRE(got[i] == mx, "slot %d of column 0 is not (M x)[%d]", i, (i % h) % D);
    }
    REQUIRE(server->MulCounter() == before && cx.Download() == words, "MulCounter moved / the input changed");
    printf("PASS NewLinearTransformationBSGS: a dense 16 x 16 matrix, 4 baby steps, 6 keys, on %d columns of %d slots (LogN=%d)\n", count, N,
           LogN);

    {
        // 0 baby steps: the best count, 4 for 16 dense diagonals -- the same keys, the same words
        fhe::LinearTransformation best = server->NewLinearTransformationBSGS(diags, cx.Level(), 0);
        REQUIRE(best.GaloisElements() == els, "babySteps = 0 did not pick 4 baby steps");
        // a single-hoisted transform on keys that are loaded, and diagonal 0 alone in the double-hoisted form
        std::map<int, std::vector<uint64_t>> few = {{0, diags[0]}, {1, diags[1]}, {2, diags[2]}, {3, diags[3]}}, only0 = {{0, diags[5]}};
        fhe::LinearTransformation plain = server->NewLinearTransformation(few, cx.Level());
        fhe::LinearTransformation babies = server->NewLinearTransformationBSGS(few, cx.Level(), 4);
        fhe::LinearTransformation lt0 = server->NewLinearTransformationBSGS(only0, cx.Level(), 4);
        REQUIRE(lt0.GaloisElements().empty(), "diagonal 0 alone needs a key");
        REQUIRE(babies.GaloisElements() == plain.GaloisElements(), "every diagonal a baby: other keys than the single-hoisted form");
        std::vector<fhe::Ciphertexts> outs = server->LinearTransformationsNew(cx, {&lt, &plain, &best, &lt0, &babies});
        REQUIRE(outs.size() == 5, "LinearTransformationsNew returned %zu sets", outs.size());
        server->check(lumen_sync(server->Context()), "lumen_sync");
        REQUIRE(outs[0].Download() == y.Download(), "LinearTransformationsNew and LinearTransformationNew differ");
        REQUIRE(outs[2].Download() == y.Download(), "babySteps = 0 computes other words than babySteps = 4");
        REQUIRE(decrypt(*server, *client, outs[1], N) == transformed(x, N, few), "the single-hoisted transform behind a double-hoisted one");
        REQUIRE(outs[4].Download() == outs[1].Download(), "every diagonal a baby: other words than the single-hoisted form");
        fhe::Ciphertexts prod = server->MulNew(cx, server->Encode(diags[5]));
        server->check(lumen_sync(server->Context()), "lumen_sync");
        REQUIRE(outs[3].Download() == prod.Download(), "diagonal 0 alone is not MulNew");
        bool threw = false;
        try {
            server->NewLinearTransformationBSGS(diags, cx.Level(), -1);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        REQUIRE(threw, "a negative number of baby steps was accepted");
        std::unique_ptr<fhe::ServerBFV> copy = server->CopyNew();
        fhe::Ciphertexts again = copy->LinearTransformationNew(cx, lt);
        copy->check(lumen_sync(copy->Context()), "lumen_sync");
        REQUIRE(again.Download() == y.Download(), "a CopyNew computes other words");
        printf("PASS LinearTransformationsNew = the single results; babySteps 0 = 4; all babies = single-hoisted; CopyNew shares keys and transform\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_lintrans_bsgs_host e2e <logN> <rows> <count>",
                     {{"e2e", e2e_mode}});
}
