// The evaluator's linear operations through the host mirror, on keys generated on the device.
//   test_linear_host e2e <logN> <rows> <cols>
//       GPU: parameters of GenerateBGVParamsForNTT(cols, logN, T) with TestLigeroE2E's T; the client encrypts 8 columns
//       of `rows` values under its secret key.  The server runs nttInner's hard-coded cases (fhe/ntt.go:24-240, pointer
//       swaps included) on ServerBFV::Add / Sub / Mul over one-ciphertext views and its download is fhe::NTT's, word for
//       word, for sizes 2, 4 and 8.  vdec.BatchCiphertexts as the reference spells it (MulNew + Add, batching.go:24-34) on
//       the client's evaluator is vdec::BatchCiphertexts, word for word.  The client decrypts both.  Add of two slices of
//       different Scale() throws and names the scales.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "twin.hpp"

using namespace lumenos;

static const uint64_t T = 144115188075593729ull; // cmd/server/main.go:22, fhe/ligero_test.go:16
static const int COLS = 8;

// matrix[a:a+1]: a view of one ciphertext (destroyed before its parent)
static fhe::Ciphertexts view_of(fhe::LinearEvaluator &ev, const fhe::Ciphertexts &set, int i) {
    lumen_set *v = nullptr;
    ev.check(lumen_set_slice(ev.Context(), set.Handle(), (uint32_t)i, 1, &v), "lumen_set_slice");
    return fhe::Ciphertexts(ev.Context(), v, set.Meta);
}

// nttInner's cases 2, 4 and 8 (fhe/ntt.go:24-240) on the slice of pointers v, line by line
static void ntt_inner(std::vector<fhe::Ciphertexts *> &v, int size, fhe::ServerBFV &backend) {
    auto bfly = [&](int i, int j) { // vi, vj := v[i].CopyNew(), v[j].CopyNew(); Add(vi, vj, v[i]); Sub(vi, vj, v[j])
        fhe::Ciphertexts vi = backend.LinearCombinationNew({v[i]}, {1}), vj = backend.LinearCombinationNew({v[j]}, {1});
        backend.Add(vi, vj, *v[i]);
        backend.Sub(vi, vj, *v[j]);
    };
    auto mul = [&](int i, uint64_t w) { backend.Mul(*v[i], w, *v[i]); };
    core::PrimeField &f = *backend.Field();
    const uint64_t r4 = f.RootForwardUint64(4), r8 = f.RootForwardUint64(8), r83 = f.Pow(3, f.RootForward(8));
    for (int i = 0; i < (int)v.size(); i += size) {
        if (size == 2) {
            bfly(i, i + 1);
        } else if (size == 4) {
            bfly(i, i + 2), bfly(i + 1, i + 3);
            mul(i + 3, r4);
            bfly(i, i + 1), bfly(i + 2, i + 3);
            std::swap(v[i + 1], v[i + 2]);
        } else {
            for (int k = 0; k < 4; k++) bfly(i + k, i + k + 4);
            mul(i + 5, r8), mul(i + 6, r4), mul(i + 7, r83);
            bfly(i, i + 2), bfly(i + 1, i + 3);
            mul(i + 3, r4);
            bfly(i, i + 1), bfly(i + 2, i + 3), bfly(i + 4, i + 6), bfly(i + 5, i + 7);
            mul(i + 7, r4);
            bfly(i + 4, i + 5), bfly(i + 6, i + 7);
            std::swap(v[i + 1], v[i + 4]), std::swap(v[i + 3], v[i + 6]);
        }
    }
}

static int e2e_mode(int argc, char **argv) {
    REQUIRE(argc >= 5, "usage: e2e <logN> <rows> <cols>");
    const int LogN = atoi(argv[2]), rows = atoi(argv[3]), cols = atoi(argv[4]);
    const fhe::Parameters params = fhe::Parameters::FromLiteral(fhe::GenerateBGVParamsForNTT(cols, LogN, T));
    core::PrimeField ptField(T, cols * 2);

    std::unique_ptr<fhe::ClientBFV> client = fhe::ClientBFV::NewWithGeneratedSecret(&ptField, params);
    fhe::KeyGenerator kgen(*client);
    const fhe::KeySet keys = kgen.GenKeySetNew(rows, 0);
    const std::vector<uint64_t> x = random_values((size_t)COLS * rows, T);
    const fhe::SeededCiphertexts up = client->EncryptColumnsSeeded(x, rows, COLS);
    std::unique_ptr<fhe::ServerBFV> server = fhe::ServerBFV::NewFromKeySet(&ptField, params, rows, keys);
    fhe::Ciphertexts cx = server->ExpandSeeded(up);
    server->check(lumen_sync(server->Context()), "lumen_sync");
    REQUIRE(decrypt(*client, cx, rows) == x, "the columns do not decrypt to themselves");

    // ---- fhe.NTT from Add / Sub / Mul
    for (int size : {2, 4, 8}) {
        fhe::Ciphertexts work = server->LinearCombinationNew({&cx}, {1}), ref = server->LinearCombinationNew({&cx}, {1});
        const int before = server->MulCounter();
        std::vector<uint64_t> got;
        std::vector<int> order;
        {
            std::vector<fhe::Ciphertexts> views;
            for (int i = 0; i < COLS; i++) views.push_back(view_of(*server, work, i));
            std::vector<fhe::Ciphertexts *> v;
            for (auto &w : views) v.push_back(&w);
            ntt_inner(v, size, *server);
            server->check(lumen_sync(server->Context()), "lumen_sync");
            for (fhe::Ciphertexts *p : v) {
                const std::vector<uint64_t> one = p->Download();
                got.insert(got.end(), one.begin(), one.end());
                order.push_back((int)(p - views.data()));
            }
        }
        const int muls = size == 2 ? 0 : size == 4 ? 2 : 5; // scalar products per 8 columns, one ciphertext each
        REQUIRE(server->MulCounter() - before == muls, "size %d: MulCounter moved by %d, the transcription multiplies %d times", size,
                server->MulCounter() - before, muls);
        fhe::NTT(ref, size, *server);
        server->check(lumen_sync(server->Context()), "lumen_sync");
        REQUIRE(got == ref.Download(), "size %d: Add / Sub / Mul compute other words than fhe::NTT", size);
        const std::vector<uint64_t> dw = decrypt(*client, work, rows), dr = decrypt(*client, ref, rows);
        for (int i = 0; i < COLS; i++)
            REQUIRE(!memcmp(&dw[(size_t)order[i] * rows], &dr[(size_t)i * rows], (size_t)rows * 8), "size %d: column %d decrypts differently", size, i);
        if (size == 2)
            for (int r = 0; r < rows; r++) {
                const uint64_t a = x[r], b = x[(size_t)rows + r];
                REQUIRE(dr[r] == ptField.Add(a, b) && dr[(size_t)rows + r] == ptField.Sub(a, b), "size 2, row %d: not (a + b, a - b)", r);
            }
        printf("PASS fhe.NTT size %d from ServerBFV::Add / Sub / Mul = fhe::NTT, decrypted\n", size);
    }

    // ---- vdec.BatchCiphertexts as the reference spells it, on the client's evaluator
    {
        std::vector<std::vector<uint64_t>> alphas((size_t)COLS, std::vector<uint64_t>((size_t)rows));
        std::vector<uint8_t> rnd((size_t)COLS * rows * 8);
        fhe::OsRandom(rnd.data(), rnd.size());
        for (int j = 0; j < COLS; j++) memcpy(alphas[(size_t)j].data(), &rnd[(size_t)j * rows * 8], (size_t)rows * 8);
        std::vector<fhe::Plaintext> pts;
        for (int j = 0; j < COLS; j++) {
            pts.push_back(server->Encode(alphas[(size_t)j])); // backend.Encode(alphasColMajor[i], alphaPts[i])
            pts.back().Scale = cx.Scale();                   // alphaPts[i].MetaData = cts[0].MetaData
        }
        const int before = client->MulCounter();
        std::vector<fhe::Ciphertexts> cts;
        for (int j = 0; j < COLS; j++) cts.push_back(view_of(*client, cx, j));
        fhe::Ciphertexts batchCt = client->MulNew(cts[0], pts[0]);
        for (int j = 1; j < COLS; j++) {
            fhe::Ciphertexts t = client->MulNew(cts[(size_t)j], pts[(size_t)j]);
            client->Add(batchCt, t, batchCt);
        }
        REQUIRE(client->MulCounter() - before == COLS, "MulCounter moved by %d for %d MulNew", client->MulCounter() - before, COLS);
        fhe::Ciphertexts lib = vdec::BatchCiphertexts(cx, alphas, *client);
        client->check(lumen_sync(client->Context()), "lumen_sync");
        REQUIRE(batchCt.Len() == 1 && batchCt.Level() == cx.Level() && batchCt.Scale() == lib.Scale(), "shape / scale of the batch");
        REQUIRE(batchCt.Download() == lib.Download(), "MulNew + Add computes other words than vdec::BatchCiphertexts");
        // the same with MulThenAdd on an accumulator
        fhe::Ciphertexts acc = client->MulNew(cts[0], pts[0]);
        for (int j = 1; j < COLS; j++) client->MulThenAdd(cts[(size_t)j], pts[(size_t)j], acc);
        client->check(lumen_sync(client->Context()), "lumen_sync");
        REQUIRE(acc.Download() == lib.Download(), "MulThenAdd computes other words than vdec::BatchCiphertexts");
        const std::vector<uint64_t> m = decrypt(*client, batchCt, rows), ml = decrypt(*client, lib, rows);
        REQUIRE(m == ml, "the two batches decrypt differently");
        for (int r = 0; r < rows; r++) {
            uint64_t want = 0;
            for (int j = 0; j < COLS; j++) want = ptField.Add(want, ptField.Mul(x[(size_t)j * rows + r], alphas[(size_t)j][(size_t)r] % T));
            REQUIRE(m[(size_t)r] == want, "row %d of the batch decrypts to %llu, BatchColumns gives %llu", r, (unsigned long long)m[(size_t)r],
                    (unsigned long long)want);
        }
        printf("PASS vdec.BatchCiphertexts spelt MulNew + Add = vdec::BatchCiphertexts, decrypted\n");
    }

    // ---- scales are not matched
    {
        fhe::Ciphertexts y = server->MulNew(cx, 5);
        REQUIRE(y.Scale() == cx.Scale(), "Mul by a scalar changed the scale");
        y.Meta.Scale = 7;
        bool threw = false;
        std::string what;
        try {
            (void)server->AddNew(cx, y);
        } catch (const std::invalid_argument &e) {
            threw = true, what = e.what();
        }
        REQUIRE(threw && what.find("scale 1 and 7") != std::string::npos, "Add of scales 1 and 7: %s", threw ? what.c_str() : "no throw");
        printf("PASS Add of two scales is refused (%s)\n", what.c_str());
    }
    return 0;
}

int main(int argc, char **argv) {
    return twin_main(argc, argv, "usage: test_linear_host e2e <logN> <rows> <cols>",
                     {{"e2e", e2e_mode}});
}
