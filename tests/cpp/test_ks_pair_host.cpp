// The launch plan of a pair of key-switch batches (lumenos_amd/csrc/lm_ks_pair.h), without a device: how a group is cut
// into batches, which columns each extension launch takes, and where the gadget product finds a column's digits.
#include <cstdio>
#include <vector>

#include "lm_ks_pair.h"

static int fails = 0;
#define CHECK(c)                                                                                                        \
    do {                                                                                                                \
        if (!(c)) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c), fails++;                                           \
    } while (0)

// the batches of a group of `count` columns, as ks_run cuts it
static std::vector<uint32_t> batches(uint32_t Bmax, bool pair, uint32_t count) {
    std::vector<uint32_t> out;
    for (uint32_t first = 0, B = 0; first < count; first += B) out.push_back(B = lm_ks_take(Bmax, pair, count - first));
    return out;
}

int main() {
    typedef std::vector<uint32_t> V;
    // ---- a group's batches: a pair while more than one batch is left, a last odd batch and a short group as without pairs
    for (uint32_t Bmax : {2u, 64u}) {
        const uint32_t B = Bmax;
        CHECK(batches(B, true, 1) == V{1});
        CHECK(batches(B, true, B) == V{B});                          // one batch: no pair
        CHECK(batches(B, true, 2 * B) == V{2 * B});                  // exactly one pair
        CHECK(batches(B, true, 2 * B + 1) == (V{2 * B, 1}));         // a pair and an odd batch, short
        CHECK(batches(B, true, 3 * B) == (V{2 * B, B}));             // a pair and an odd batch, whole
        CHECK(batches(B, true, 4 * B) == (V{2 * B, 2 * B}));
        CHECK(batches(B, true, 4 * B + 1) == (V{2 * B, 2 * B, 1}));
        CHECK(batches(B, true, 8 * B) == (V{2 * B, 2 * B, 2 * B, 2 * B})); // a group of matrixInnerSumEval: four pairs
        for (uint32_t count = 0; count <= 9 * B; count += (B > 8 ? 7 : 1)) { // without pairs: today's batches; every column once
            uint32_t sum = 0, sum_p = 0;
            for (uint32_t b : batches(B, false, count)) {
                CHECK(b >= 1 && b <= B);
                sum += b;
            }
            for (uint32_t b : batches(B, true, count)) {
                CHECK(b >= 1 && b <= 2 * B);
                sum_p += b;
            }
            CHECK(sum == count && sum_p == count);
        }
    }
    CHECK(batches(2, true, 3) == V{3}); // a pair with a short second half
    CHECK(batches(2, true, 7) == (V{4, 3}));
    CHECK(batches(2, true, 9) == (V{4, 4, 1}));
    printf("PASS batches of a group\n");

    // ---- the extension launches of a batch, and every column's block and local column
    for (int second_first = 0; second_first < 2; second_first++)
        for (uint32_t half : {2u, 64u})
            for (uint32_t B = 1; B <= 2 * half; B++) {
                const lm_ks_ext_plan p = lm_ks_ext_launches(B, half, second_first != 0);
                if (B <= half) { // a single batch on a pair's scratch: as on a scratch of one block
                    const lm_ks_ext_plan q = lm_ks_ext_launches(B, 0);
                    CHECK(p.n == 1 && p.layout == B && p.at[0].first == 0 && p.at[0].count == B && p.at[0].block == 0);
                    CHECK(q.n == 1 && q.layout == B && q.at[0].count == B && q.at[0].block == 0);
                    for (uint32_t b = 0; b < B; b++) CHECK(lm_ks_ext_block(b, p.layout) == 0 && lm_ks_ext_local(b, p.layout) == b);
                    continue;
                }
                // two launches, each at most `half` columns in the layout of `half`, disjoint, covering the pair
                CHECK(p.n == 2 && p.layout == half);
                std::vector<int> seen(B, 0);
                for (uint32_t k = 0; k < p.n; k++) {
                    const lm_ks_ext_launch &h = p.at[k];
                    CHECK(h.count >= 1 && h.count <= half && h.first + h.count <= B && h.block == h.first / half && h.first % half == 0);
                    for (uint32_t c = 0; c < h.count; c++) {
                        const uint32_t b = h.first + c; // the launch writes local column c of its block: where the product reads b
                        seen[b]++;
                        CHECK(lm_ks_ext_block(b, p.layout) == h.block && lm_ks_ext_local(b, p.layout) == c);
                        CHECK(lm_ks_ext_block(b, p.layout) == b / half && lm_ks_ext_local(b, p.layout) == b % half);
                    }
                }
                for (uint32_t b = 0; b < B; b++) CHECK(seen[b] == 1);
                CHECK(p.at[second_first ? 1 : 0].block == 0 && p.at[second_first ? 0 : 1].block == 1); // the order asked for
            }
    printf("PASS extension launches and blocks\n");

    // ---- the headline shape: 128 columns, every other kernel once with B = 2 Bmax, the extension twice with 64
    {
        const V b = batches(64, true, 512);
        CHECK(b.size() == 4);
        const lm_ks_ext_plan p = lm_ks_ext_launches(b[0], 64);
        CHECK(b[0] == 128 && p.n == 2 && p.layout == 64 && p.at[0].count == 64 && p.at[1].count == 64 && p.at[1].first == 64);
    }
    printf("PASS headline shape\n");
    if (!fails) printf("pair plan OK\n");
    return fails ? 1 : 0;
}
