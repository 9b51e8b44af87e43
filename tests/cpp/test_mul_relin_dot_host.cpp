// Encrypted matrix x encrypted vector through the host mirror, one relinearisation per output, no CPU-generated key anywhere.
//   test_mul_relin_dot_host e2e <logN> <rows> <groups> <n>
//       GPU: ClientBFV::NewWithGeneratedSecret -> KeyGenerator::GenKeySetNew(rows, flags, withRelin); the client encrypts a
//       groups x n matrix of columns and a vector of n columns under its secret key and uploads them in seeded form;
//       ServerBFV::NewFromKeySet -> ExpandSeeded -> DotRelinNew -> Rescale to level 1; the client decrypts at the product's
//       scale and finds, slot-wise, sum_i x[g][i] * y[i].  Also: the pairwise form, MulCounter, the argument errors, a
//       CopyNew giving the same words, and a server without the key refusing until SetRelinearizationKey.
//   T = 0x3ee0001 (the reference's vdec tests): the noise of the sum, about n T^2 N B, fits two limbs with it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
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

template <class F>
static bool invalid(F &&f) {
    try {
        f();
    } catch (const std::invalid_argument &) {
        return true;
    }
    return false;
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 6, "usage: e2e <logN> <rows> <groups> <n>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), groups = atoi(argv[4]), n = atoi(argv[5]);
    REQUIRE(groups >= 2 && n >= 2, "at least two groups of two terms");
    fhe::ParametersLiteral lit;
    lit.LogN = LogN, lit.LogQ = {58, 56, 56}, lit.LogP = {55, 55}, lit.PlaintextModulus = T;
    const fhe::Parameters params = fhe::Parameters::FromLiteral(lit);
    core::PrimeField ptField(T, 64);

    // ---- the client: every key generated on the device
    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    const fhe::KeySet keys = kgen.GenKeySetNew(rows, LUMEN_KEY_MONTGOMERY, true);
    REQUIRE(!keys.Rlk.empty(), "the key set carries no relinearisation key");
    const int count = groups * n;
    const std::vector<uint64_t> x = random_values((size_t)count * rows, T), y = random_values((size_t)count * rows, T);
    const fhe::SeededCiphertexts upX = client->EncryptColumnsSeeded(x, rows, count);
    const fhe::SeededCiphertexts upY = client->EncryptColumnsSeeded(y, rows, count);
    const fhe::SeededCiphertexts upV = client->EncryptColumnsSeeded(std::vector<uint64_t>(y.begin(), y.begin() + (size_t)n * rows), rows, n);
    // slot-wise sum_i x[g n + i] * y[(pairwise ? g n : 0) + i] mod T
    auto dot = [&](int g, int slot, bool pairwise) {
        uint64_t s = 0;
        for (int i = 0; i < n; i++)
            s = (s + core::MulMod(x[((size_t)g * n + i) * rows + slot], y[((size_t)(pairwise ? g * n : 0) + i) * rows + slot], T)) % T;
        return s;
    };

    // ---- the server: the posted key set, no secret
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);
    fhe::Ciphertexts cx = server->ExpandSeeded(upX), cy = server->ExpandSeeded(upY), cv = server->ExpandSeeded(upV);
    const int before = server->MulCounter();
    fhe::Ciphertexts prod = server->DotRelinNew(cx, cv, (uint32_t)n); // 1. matrix x vector
    REQUIRE(server->MulCounter() == before + count, "MulCounter grew by %d, not %d", server->MulCounter() - before, count);
    REQUIRE(prod.Len() == groups && prod.Level() == cx.Level() && prod.Scale() == 1, "shape / scale of the sums");
    fhe::Ciphertexts low = rescale_to(*server, prod, 1); // 2.
    REQUIRE(low.Level() == 1 && low.Scale() != 1, "the rescale left no scale");
    std::vector<uint64_t> got = decrypt(*server, *client, low, rows); // 3.
    REQUIRE(got.size() == (size_t)groups * rows, "decrypted %zu words", got.size());
    for (size_t i = 0; i < got.size(); i++)
        REQUIRE(got[i] == dot((int)(i / rows), (int)(i % rows), false), "group %zu slot %zu: %llu, not the dot product %llu", i / rows,
                i % rows, (unsigned long long)got[i], (unsigned long long)dot((int)(i / rows), (int)(i % rows), false));
    printf("PASS DotRelinNew + Rescale: %d x %d columns of %d slots times a vector decrypt to the slot-wise products (LogN=%d)\n",
           groups, n, rows, LogN);

    // ---- the pairwise form: every group against its own vector
    {
        got = decrypt(*server, *client, rescale_to(*server, server->DotRelinNew(cx, cy, (uint32_t)n), 1), rows);
        for (size_t i = 0; i < got.size(); i++)
            REQUIRE(got[i] == dot((int)(i / rows), (int)(i % rows), true), "pairwise: group %zu slot %zu", i / rows, i % rows);
        printf("PASS the pairwise form\n");
    }

    // ---- the argument errors are std::invalid_argument, and the server computes afterwards
    {
        REQUIRE(invalid([&] { server->DotRelinNew(cx, cv, 0); }), "n == 0 accepted");
        REQUIRE(invalid([&] { server->DotRelinNew(cx, cv, (uint32_t)count + 1); }), "a count that is no multiple of n accepted");
        REQUIRE(invalid([&] { server->DotRelinNew(cv, cx, (uint32_t)n); }), "a second operand of another count accepted");
        REQUIRE(invalid([&] { server->DotRelinNew(cx, rescale_to(*server, cv, 1), (uint32_t)n); }), "operands of two levels accepted");
        REQUIRE(invalid([&] { server->DotRelinNew(fhe::Ciphertexts(), cv, (uint32_t)n); }), "an empty operand accepted");
        server->check(lumen_sync(server->Context()), "lumen_sync");
        REQUIRE(server->DotRelinNew(cx, cv, (uint32_t)n).Download() == prod.Download(), "other words after the refusals");
        printf("PASS argument errors throw std::invalid_argument\n");
    }

    // ---- 4. a copy shares the key; 5. a server whose key set carried none refuses; 6. until it is given one
    {
        std::unique_ptr<fhe::ServerBFV> copy = server->CopyNew();
        fhe::Ciphertexts again = copy->DotRelinNew(cx, cv, (uint32_t)n);
        copy->check(lumen_sync(copy->Context()), "lumen_sync");
        REQUIRE(again.Download() == prod.Download(), "a CopyNew computes other words");
        fhe::KeySet bare = keys;
        bare.Rlk.clear();
        std::unique_ptr<fhe::ServerBFV> noKey = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, bare);
        fhe::Ciphertexts nx = noKey->ExpandSeeded(upX), nv = noKey->ExpandSeeded(upV);
        bool threw = false;
        std::string what;
        try {
            noKey->DotRelinNew(nx, nv, (uint32_t)n);
        } catch (const std::runtime_error &e) {
            threw = true, what = e.what();
        }
        REQUIRE(threw && what.find("no relinearisation key") != std::string::npos, "a server without the key multiplied (%s)", what.c_str());
        noKey->SetRelinearizationKey(keys.Rlk, keys.Flags);
        fhe::Ciphertexts late = noKey->DotRelinNew(nx, nv, (uint32_t)n);
        noKey->check(lumen_sync(noKey->Context()), "lumen_sync");
        REQUIRE(late.Len() == groups && late.Download() == prod.Download(), "SetRelinearizationKey did not take");
        printf("PASS CopyNew shares the key; without one: %s\n", what.c_str());
    }
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_mul_relin_dot_host e2e <logN> <rows> <groups> <n>", {{"e2e", e2e_mode}});
}
