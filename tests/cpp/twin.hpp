// What the C++ twins of tests/cpp/test_*_host.cpp share: the REQUIRE check, the mode dispatch of main, the parameter set
// of the e2e shapes, the client's decryption of a set on the same GPU, and random slot values.  tests/helpers.py lists
// this header among every twin's dependencies.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <vector>

#include "../../lumenos_amd/host/fhe.hpp"

// inside a function that returns int: report the failed condition with its place and return 1
#define REQUIRE(cond, ...)                                       \
    do {                                                         \
        if (!(cond)) {                                           \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, "\n");                               \
            return 1;                                            \
        }                                                        \
    } while (0)

struct TwinMode {
    const char *name;
    int (*run)(int argc, char **argv);
};

// main of a twin: argv[1] selects the mode; an exception out of it is a failure (status 1), no mode prints `usage`
// (status 2)
static inline int twin_main(int argc, char **argv, const char *usage, std::initializer_list<TwinMode> modes) {
    try {
        for (const TwinMode &m : modes)
            if (argc >= 2 && !strcmp(argv[1], m.name)) return m.run(argc, argv);
    } catch (const std::exception &e) {
        fprintf(stderr, "FAIL exception: %s\n", e.what());
        return 1;
    }
    fprintf(stderr, "%s\n", usage);
    return 2;
}

// fhe.GenerateBGVParamsForNTT(cols, LogN, T) with the chain padded to numQ moduli; T: fhe/ligero_test.go:16
static inline lumenos::fhe::Parameters make_params(int LogN, int cols, int numQ) {
    lumenos::fhe::ParametersLiteral lit = lumenos::fhe::GenerateBGVParamsForNTT(cols, LogN, 144115188075593729ull);
    while ((int)lit.LogQ.size() < numQ) lit.LogQ.push_back(56);
    return lumenos::fhe::Parameters::FromLiteral(lit);
}

// the client's Decryptor + Encoder.Decode on a set that lives on the same GPU: [count][n]
static inline std::vector<uint64_t> decrypt(lumenos::fhe::ClientBFV &client, const lumenos::fhe::Ciphertexts &cts, int n) {
    std::vector<uint64_t> out((size_t)cts.Len() * n);
    client.check(lumen_decrypt(client.Context(), cts.Handle(), cts.Scale(), (uint32_t)n, out.data()), "lumen_decrypt");
    return out;
}

// the same on a set the server has just produced: its stream drains first
static inline std::vector<uint64_t> decrypt(lumenos::fhe::ServerBFV &server, lumenos::fhe::ClientBFV &client,
                                            const lumenos::fhe::Ciphertexts &cts, int n) {
    server.check(lumen_sync(server.Context()), "lumen_sync");
    return decrypt(client, cts, n);
}

// `count` words from fhe::OsRandom, each reduced below `bound`
static inline std::vector<uint64_t> random_values(size_t count, uint64_t bound) {
    std::vector<uint8_t> rnd(count * 8);
    lumenos::fhe::OsRandom(rnd.data(), rnd.size());
    std::vector<uint64_t> out(count);
    for (size_t i = 0; i < count; i++) {
        uint64_t a;
        memcpy(&a, &rnd[i * 8], 8);
        out[i] = a % bound;
    }
    return out;
}

// an evaluation point in [2, bound)
static inline uint64_t random_point(uint64_t bound) {
    uint64_t z = 0;
    while (z < 2) z = random_values(1, bound)[0];
    return z;
}
