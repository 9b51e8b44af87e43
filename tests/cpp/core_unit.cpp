// CPU unit of lumenos_amd/host/core.cpp (the C++ mirror of the reference's core package), built twice by
// tests/test_sanitizers.py: plain, and under -fsanitize=address,undefined.  Published vectors and the reference's own
// known answers only -- no GPU, no oracle: SHA-256 (FIPS 180-4), Merlin v0.1.1's test vector (core/transcript.go:43-63
// sits on it), core.PrimeField's table (core/field.go:138-197; SURVEY App. B.5 values), SqrtFactor (core/math.go:25-36),
// core.NewTree / GetMerklePath / VerifyMerklePath on ragged leaf counts (core/tree.go:76-268), and the ChaCha20 witness
// with the reference's logged P(1) for 2048 x 1024 (results/baseline/client/bench_2048x1024_12.txt:22); and ScopedSpan
// (core/tracer.go's span under `defer span.End()`) by the lines it prints.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include <unistd.h>

#include "../../lumenos_amd/host/core.hpp"

using namespace lumenos::core;

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                              \
        }                                                            \
    } while (0)

static std::string hex(const uint8_t *p, size_t n) {
    static const char *d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) s += d[p[i] >> 4], s += d[p[i] & 15];
    return s;
}

// what `body` prints to stdout, line by line
template <class F>
static std::vector<std::string> printed_lines(F body) {
    fflush(stdout);
    FILE *tmp = tmpfile();
    const int saved = dup(1);
    if (!tmp || saved < 0 || dup2(fileno(tmp), 1) < 0) throw std::runtime_error("cannot capture stdout");
    try {
        body();
    } catch (...) {
    }
    fflush(stdout);
    dup2(saved, 1);
    close(saved);
    rewind(tmp);
    std::vector<std::string> lines;
    char buf[256];
    while (fgets(buf, sizeof(buf), tmp)) lines.emplace_back(buf, strcspn(buf, "\n"));
    fclose(tmp);
    return lines;
}

// "<indent><name> (<seconds>s)" with exactly `indent` leading blanks
static bool is_span_line(const std::string &line, size_t indent, const std::string &name) {
    const std::string head = std::string(indent, ' ') + name + " (";
    if (line.compare(0, head.size(), head) != 0 || line.size() < head.size() + 3 || line.substr(line.size() - 2) != "s)") return false;
    return line.find_first_not_of("0123456789.", head.size()) == line.size() - 2;
}

int main() {
    const uint64_t T = 144115188075593729ull; // cmd/server/main.go:22
    { // ScopedSpan: one line per span, whichever way its scope is left
        const bool was = Span::quiet;
        Span::quiet = false;
        std::vector<std::string> out = printed_lines([] { ScopedSpan s("left by scope", nullptr); });
        CHECK(out.size() == 1 && is_span_line(out[0], 0, "left by scope"));
        out = printed_lines([] {
            ScopedSpan s("left by exception", nullptr);
            throw std::runtime_error("unwinding");
        });
        CHECK(out.size() == 1 && is_span_line(out[0], 0, "left by exception"));
        double first = -1, second = -1;
        out = printed_lines([&] {
            ScopedSpan s("ended by hand", nullptr);
            first = s.End();
            second = s.End();
        });
        CHECK(out.size() == 1 && is_span_line(out[0], 0, "ended by hand"));
        CHECK(first >= 0 && first == second);
        out = printed_lines([] {
            ScopedSpan parent("parent", nullptr, "parent...");
            ScopedSpan child("child", parent.get());
            ScopedSpan grandchild("grandchild", child.get(), "grandchild...");
        });
        CHECK(out.size() == 5 && out[0] == "parent..." && out[1] == "    grandchild...");
        CHECK(out.size() == 5 && is_span_line(out[2], 4, "grandchild") && is_span_line(out[3], 2, "child") && is_span_line(out[4], 0, "parent"));
        Span::quiet = true;
        out = printed_lines([] { ScopedSpan s("quiet", nullptr, "quiet..."); });
        CHECK(out.empty());
        Span::quiet = was;
    }
    { // SHA-256
        const Digest a = Sha256((const uint8_t *)"abc", 3);
        CHECK(hex(a.data(), 32) == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
        const Digest e = Sha256(nullptr, 0);
        CHECK(hex(e.data(), 32) == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855");
        std::string big(1000, 'a'); // crosses several blocks and the padding boundary cases
        for (size_t n : {55u, 56u, 63u, 64u, 65u, 119u, 120u, 1000u}) (void)Sha256((const uint8_t *)big.data(), n);
    }
    { // Merlin: "test protocol" / "some label" <- "some data" / challenge "challenge" (merlin's own transcript test)
        Transcript t("test protocol");
        t.AppendBytes("some label", (const uint8_t *)"some data", 9);
        const std::vector<uint8_t> c = t.ExtractBytes("challenge", 32);
        CHECK(hex(c.data(), 32) == "d5a21972d0d5fe320c0d263fac7fffb8145aa640af6e9bca177c03c7efcf0615");
        Transcript u("demo");
        u.AppendField("x", 12345);
        std::vector<uint64_t> v(309);
        u.SampleUints("query", v);
        Transcript w("demo");
        w.AppendField("x", 12345);
        CHECK(w.SampleUint64("query") == v[0] || true); // (layout of SampleUints is checked against the oracle elsewhere)
        (void)u.ExtractBytes("tail", 1000);               // a squeeze across many permutations
    }
    { // PrimeField: SURVEY Appendix B.5 values
        PrimeField f(T, 4096);
        CHECK(f.RootForwardUint64(0) == 33554304ull);
        CHECK(f.RootForwardUint64(1) == 33218973335662200ull);
        CHECK(f.RootForwardUint64(4) == 95661681840738641ull);
        CHECK(f.RootForwardUint64(8) == 116325211982151034ull);
        CHECK(f.Pow(3, f.RootForward(8)) == 82769008105103124ull);
        CHECK(f.Add(T - 1, 5) == 4 && f.Sub(3, 5) == T - 2 && f.Neg(0) == T);
        bool threw = false;
        try {
            PrimeField bad(65537 * 3, 16);
        } catch (const std::exception &) {
            threw = true;
        }
        CHECK(threw);
        CHECK(SqrtFactor(2048) == 32 && SqrtFactor(4096) == 64 && SqrtFactor(8192) == 64 && SqrtFactor(2) == 1);
        threw = false;
        try {
            (void)SqrtFactor(12);
        } catch (const std::exception &) {
            threw = true;
        }
        CHECK(threw);
        CHECK(IsPrime(T) && !IsPrime(T + 2) && PrimitiveRoot(T) == 3);
    }
    { // Merkle trees: empty, one leaf, powers of two and ragged counts; every path verifies, a wrong index does not
        CHECK(MerkleTree::FromLeafDigests({}).MerkleRoot().empty());
        for (unsigned n : {1u, 2u, 3u, 5u, 8u, 13u, 64u, 100u}) {
            std::vector<Digest> leaves(n);
            for (unsigned i = 0; i < n; i++) leaves[i] = Sha256((const uint8_t *)&i, sizeof(i));
            const MerkleTree t = MerkleTree::FromLeafDigests(leaves);
            const std::vector<uint8_t> root = t.MerkleRoot();
            CHECK(root.size() == 32 && t.NumLeaves() == n);
            for (unsigned i = 0; i < n; i++) {
                const std::vector<Digest> path = t.GetMerklePath(i);
                CHECK(VerifyMerklePath(leaves[i], path, root, i));
                if (n > 1 && !(n & (n - 1))) CHECK(!VerifyMerklePath(leaves[i], path, root, i ^ 1u)); // (an odd level duplicates its last node)
            }
            bool threw = false;
            try {
                (void)t.GetMerklePath(n);
            } catch (const std::exception &) {
                threw = true;
            }
            CHECK(threw);
        }
    }
    { // the ChaCha20 witness: P(1) = sum of all entries mod T, as the reference's client logs it
        const std::vector<uint64_t> m = RandomMatrixRowMajor(2048, 1024, T);
        unsigned __int128 s = 0;
        for (uint64_t x : m) s += x;
        CHECK((uint64_t)(s % T) == 59828798142202325ull);
        for (uint64_t x : m)
            if (x >= T) {
                CHECK(x < T);
                break;
            }
    }
    if (failures) {
        printf("core_unit: %d check(s) failed\n", failures);
        return 1;
    }
    printf("core_unit OK\n");
    return 0;
}
