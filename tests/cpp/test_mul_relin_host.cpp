// Ciphertext x ciphertext through the host mirror, with no CPU-generated key anywhere.
//   test_mul_relin_host e2e <logN> <rows> <count>
//       GPU: ClientBFV::NewWithGeneratedSecret -> KeyGenerator::GenKeySetNew(rows, flags, withRelin); the client encrypts
//       two blocks of `count` columns under its secret key and uploads them in seeded form; ServerBFV::NewFromKeySet
//       loads the set (the relinearisation key with it) -> ExpandSeeded -> MulRelinNew -> Rescale to level 1; the client
//       decrypts at the product's scale and finds the slot-wise products.  Also: every column times ONE ciphertext,
//       squares of operands that carry a scale, MulCounter, and a server without the key refusing.
//   T = 0x3ee0001 (the reference's vdec tests): the noise of a product, about T^2 N B, fits two limbs with it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "twin.hpp"

using namespace lumenos;

static const uint64_t T = 0x3ee0001ull;

// Evaluator.Rescale looped to `level`, with the scale it leaves
static fhe::Ciphertexts rescale_to(fhe::ServerBFV &server, const fhe::Ciphertexts &in, int level) {
    lumen_set *out = nullptr;
    server.check(lumen_rescale(server.Context(), in.Handle(), (uint32_t)level + 1, &out), "lumen_rescale");
    fhe::MetaData md = in.Meta;
    md.Scale = fhe::RescaledScale(server.GetParameters(), in.Scale(), in.Level(), level);
    return fhe::Ciphertexts(server.Context(), out, md);
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 5, "usage: e2e <logN> <rows> <count>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), count = atoi(argv[4]);
    fhe::ParametersLiteral lit;
    lit.LogN = LogN, lit.LogQ = {58, 56, 56}, lit.LogP = {55, 55}, lit.PlaintextModulus = T;
    const fhe::Parameters params = fhe::Parameters::FromLiteral(lit);
    core::PrimeField ptField(T, 64);

    // ---- the client: every key generated on the device
    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    const fhe::KeySet keys = kgen.GenKeySetNew(rows, LUMEN_KEY_MONTGOMERY, true);
    REQUIRE(!keys.Rlk.empty() && keys.Rlk.size() == keys.GaloisKeys.at(0).size(), "the key set carries no relinearisation key");
    REQUIRE(kgen.GenKeySetNew(rows, 0).Rlk.empty(), "GenKeySetNew(rows, flags) grew a relinearisation key");
    const std::vector<uint64_t> x = random_values((size_t)count * rows, T), y = random_values((size_t)count * rows, T);
    const fhe::SeededCiphertexts upX = client->EncryptColumnsSeeded(x, rows, count), upY = client->EncryptColumnsSeeded(y, rows, count);

    // ---- the server: the posted key set, no secret
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);
    fhe::Ciphertexts cx = server->ExpandSeeded(upX), cy = server->ExpandSeeded(upY);
    const int before = server->MulCounter();
    fhe::Ciphertexts prod = server->MulRelinNew(cx, cy);
    REQUIRE(server->MulCounter() == before + count, "MulCounter grew by %d, not %d", server->MulCounter() - before, count);
    REQUIRE(prod.Len() == count && prod.Level() == cx.Level() && prod.Scale() == 1, "shape / scale of the product");
    fhe::Ciphertexts low = rescale_to(*server, prod, 1);
    REQUIRE(low.Level() == 1 && low.Scale() != 1, "the rescale left no scale");
    std::vector<uint64_t> got = decrypt(*server, *client, low, rows);
    for (size_t i = 0; i < got.size(); i++)
        REQUIRE(got[i] == core::MulMod(x[i], y[i], T), "column %zu slot %zu: %llu, not x * y = %llu", i / rows, i % rows,
                (unsigned long long)got[i], (unsigned long long)core::MulMod(x[i], y[i], T));
    printf("PASS MulRelinNew + Rescale: %d columns of %d slots decrypt to the slot-wise products (LogN=%d)\n", count, rows, LogN);

    // ---- every column times one ciphertext
    {
        const fhe::SeededCiphertexts upOne = client->EncryptColumnsSeeded(std::vector<uint64_t>(y.begin(), y.begin() + rows), rows, 1);
        fhe::Ciphertexts one = server->ExpandSeeded(upOne);
        got = decrypt(*server, *client, rescale_to(*server, server->MulRelinNew(cx, one), 1), rows);
        for (size_t i = 0; i < got.size(); i++) REQUIRE(got[i] == core::MulMod(x[i], y[i % rows], T), "broadcast: column %zu slot %zu", i / rows, i % rows);
        printf("PASS every column times one ciphertext\n");
    }

    // ---- squares of operands that carry a scale, at level 1: Scale() is the product of the scales
    {
        fhe::Ciphertexts lx = rescale_to(*server, cx, 1);
        fhe::Ciphertexts sq = server->MulRelinNew(lx, lx);
        REQUIRE(sq.Level() == 1 && sq.Scale() == core::MulMod(lx.Scale(), lx.Scale(), T) && sq.Scale() != lx.Scale(), "scale of a square");
        got = decrypt(*server, *client, sq, rows);
        for (size_t i = 0; i < got.size(); i++) REQUIRE(got[i] == core::MulMod(x[i], x[i], T), "square: column %zu slot %zu", i / rows, i % rows);
        printf("PASS squares at level 1, scale = the product of the scales\n");
    }

    // ---- a copy shares the key; a server whose key set carried none refuses
    {
        std::unique_ptr<fhe::ServerBFV> copy = server->CopyNew();
        fhe::Ciphertexts again = copy->MulRelinNew(cx, cy);
        copy->check(lumen_sync(copy->Context()), "lumen_sync");
        REQUIRE(again.Download() == prod.Download(), "a CopyNew computes other words");
        fhe::KeySet bare = keys;
        bare.Rlk.clear();
        std::unique_ptr<fhe::ServerBFV> noKey = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, bare);
        fhe::Ciphertexts nx = noKey->ExpandSeeded(upX);
        bool threw = false;
        std::string what;
        try {
            noKey->MulRelinNew(nx, nx);
        } catch (const std::runtime_error &e) {
            threw = true, what = e.what();
        }
        REQUIRE(threw && what.find("no relinearisation key") != std::string::npos, "a server without the key multiplied (%s)", what.c_str());
        noKey->SetRelinearizationKey(keys.Rlk, keys.Flags);
        REQUIRE(noKey->MulRelinNew(nx, nx).Len() == count, "SetRelinearizationKey did not take");
        printf("PASS CopyNew shares the key; without one: %s\n", what.c_str());
    }
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_mul_relin_host e2e <logN> <rows> <count>",
                     {{"e2e", e2e_mode}});
}
