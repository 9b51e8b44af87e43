// Rotations through the host mirror, with no CPU-generated key anywhere.
//   test_rotate_host e2e <logN> <rows> <count>
//       GPU: ClientBFV::NewWithGeneratedSecret -> KeyGenerator::GenKeySetNew(rows) for the server's constructor and
//       KeyGenerator::GenGaloisKeysNew for the elements of the rotations below (ServerBFV::LoadGaloisKeys); the client
//       encrypts `count` columns of N slot values under its secret key and uploads them in seeded form; the server
//       rotates by k = 1 and -3 (RotateColumnsNew), swaps the rows (RotateRowsNew), rotates hoisted by {1, 2, 5}
//       (RotateHoistedNew) and applies AutomorphismNew; the client decrypts and finds the slot permutation:
//       slot i of each half-row = v[(i + k) mod N/2] of that half-row; the row swap exchanges the half-rows.
//   T = 0x3ee0001 (the reference's vdec tests).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "twin.hpp"

using namespace lumenos;

static const uint64_t T = 0x3ee0001ull;

// what a rotation by k (swap: then the row swap) makes of the columns x, [count][N]
static std::vector<uint64_t> permuted(const std::vector<uint64_t> &x, int N, long k, bool swap) {
    const long h = N / 2;
    std::vector<uint64_t> out(x.size());
    for (size_t c = 0; c < x.size() / N; c++)
        for (long row = 0; row < 2; row++)
            for (long i = 0; i < h; i++)
                out[c * N + row * h + i] = x[c * N + (swap ? 1 - row : row) * h + (((i + k) % h) + h) % h];
    return out;
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 5, "usage: e2e <logN> <rows> <count>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), count = atoi(argv[4]);
    fhe::ParametersLiteral lit;
    lit.LogN = LogN, lit.LogQ = {58, 56, 56}, lit.LogP = {55, 55}, lit.PlaintextModulus = T;
    const fhe::Parameters params = fhe::Parameters::FromLiteral(lit);
    const int N = params.N();
    core::PrimeField ptField(T, 64);
    REQUIRE(params.GaloisElement(0) == 1 && params.GaloisElement(N / 2) == 1 && params.GaloisElement(1) == 5 &&
                params.GaloisElementForRowRotation() == 2ull * N - 1,
            "Galois elements");

    // ---- the client: every key generated on the device
    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    const fhe::KeySet keys = kgen.GenKeySetNew(rows, LUMEN_KEY_MONTGOMERY);
    const std::vector<uint64_t> els = {params.GaloisElement(1), params.GaloisElement(-3), params.GaloisElement(2), params.GaloisElement(5),
                                       params.GaloisElementForRowRotation()};
    const std::map<uint64_t, std::vector<uint64_t>> gks = kgen.GenGaloisKeysNew(els, LUMEN_KEY_MONTGOMERY);
    REQUIRE(gks.size() == els.size(), "GenGaloisKeysNew returned %zu keys for %zu elements", gks.size(), els.size());
    const std::vector<uint64_t> x = random_values((size_t)count * N, T);
    const fhe::SeededCiphertexts up = client->EncryptColumnsSeeded(x, N, count);

    // ---- the server: the posted key set, the rotations' keys beside it, no secret
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);
    fhe::Ciphertexts cx = server->ExpandSeeded(up);
    REQUIRE(decrypt(*server, *client, cx, N) == x, "the columns do not decrypt to themselves");
    {
        bool threw = false;
        std::string what;
        try {
            server->RotateColumnsNew(cx, -3);
        } catch (const std::runtime_error &e) {
            threw = true, what = e.what();
        }
        REQUIRE(threw && what.find("not loaded") != std::string::npos, "a server without the key rotated (%s)", what.c_str());
    }
    server->LoadGaloisKeys(gks, LUMEN_KEY_MONTGOMERY);
    const int before = server->MulCounter();
    const std::vector<uint64_t> words = cx.Download();

    for (int k : {1, -3}) {
        fhe::Ciphertexts r = server->RotateColumnsNew(cx, k);
        REQUIRE(r.Len() == count && r.Level() == cx.Level() && r.Scale() == cx.Scale(), "shape / scale of a rotation");
        REQUIRE(decrypt(*server, *client, r, N) == permuted(x, N, k, false), "RotateColumnsNew(%d) moved the slots elsewhere", k);
        fhe::Ciphertexts a = server->AutomorphismNew(cx, params.GaloisElement(k));
        server->check(lumen_sync(server->Context()), "lumen_sync");
        REQUIRE(a.Download() == r.Download(), "AutomorphismNew(GaloisElement(%d)) computes other words", k);
    }
    printf("PASS RotateColumnsNew by 1 and -3: %d columns of %d slots (LogN=%d)\n", count, N, LogN);

    {
        fhe::Ciphertexts r = server->RotateRowsNew(cx);
        REQUIRE(decrypt(*server, *client, r, N) == permuted(x, N, 0, true), "RotateRowsNew did not swap the rows");
        fhe::Ciphertexts rr = server->RotateColumnsNew(r, 5);
        REQUIRE(decrypt(*server, *client, rr, N) == permuted(x, N, 5, true), "a rotation of the swapped rows");
        printf("PASS RotateRowsNew\n");
    }

    {
        std::map<int, fhe::Ciphertexts> h = server->RotateHoistedNew(cx, {1, 2, 5});
        REQUIRE(h.size() == 3 && h.count(1) && h.count(2) && h.count(5), "RotateHoistedNew returned %zu entries", h.size());
        for (auto &kv : h) {
            REQUIRE(decrypt(*server, *client, kv.second, N) == permuted(x, N, kv.first, false), "hoisted rotation by %d", kv.first);
            fhe::Ciphertexts single = server->RotateColumnsNew(cx, kv.first);
            server->check(lumen_sync(server->Context()), "lumen_sync");
            REQUIRE(single.Download() == kv.second.Download(), "hoisted and single rotation by %d differ", kv.first);
        }
        REQUIRE(server->RotateHoistedNew(cx, {}).empty(), "no rotation, but an entry");
        printf("PASS RotateHoistedNew {1, 2, 5} = the single rotations\n");
    }

    {
        fhe::Ciphertexts id = server->RotateColumnsNew(cx, N / 2); // the identity: a copy
        server->check(lumen_sync(server->Context()), "lumen_sync");
        REQUIRE(id.Download() == words && cx.Download() == words, "the identity / the input changed");
        REQUIRE(server->MulCounter() == before, "a rotation moved MulCounter");
        std::unique_ptr<fhe::ServerBFV> copy = server->CopyNew();
        fhe::Ciphertexts again = copy->RotateColumnsNew(cx, -3), first = server->RotateColumnsNew(cx, -3);
        copy->check(lumen_sync(copy->Context()), "lumen_sync");
        server->check(lumen_sync(server->Context()), "lumen_sync");
        REQUIRE(again.Download() == first.Download(), "a CopyNew computes other words");
        printf("PASS identity, input untouched, CopyNew shares the keys\n");
    }
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_rotate_host e2e <logN> <rows> <count>",
                     {{"e2e", e2e_mode}});
}
