// Pairs of key-switch batches (LUMEN_KS_PAIR): the PLAN alone -- how a group of columns is cut
// into batches, which columns each extension launch of a batch takes, and in which `ext` block and at which local column
// a column's extended digits sit -- so that it runs without a device (tests/cpp/test_ks_pair_host.cpp).  The launches
// themselves are lm_keyswitch.hip's, the loop over a group lm_ks_host.h's.  Plain C++17, no HIP.
//
// A pair is two consecutive batches of `half` columns that go through a rotation as one batch of up to 2 * half: every
// kernel runs once over all of its columns on blocks of that size, except the extension, which runs once per half, on
// the half's own columns of `coef` and `acc` (both column-major: a column base is a pointer offset) and into the half's
// own `ext` block in the layout of a batch of `half` columns, [L+K][half][beta].
#pragma once
#include <algorithm>
#include <cstdint>

// columns of the next batch of a group of which `left` remain: a pair while more than one batch is left (the second half
// may be short), else a single batch -- a last odd batch, and any group of at most Bmax columns, go as without pairs
inline uint32_t lm_ks_take(uint32_t Bmax, bool pair, uint32_t left) {
    return pair && left > Bmax ? std::min(2 * Bmax, left) : std::min(Bmax, left);
}

struct lm_ks_ext_launch {
    uint32_t first, count, block; // columns [first, first + count) of the batch, extended into `ext` block `block`
};
struct lm_ks_ext_plan {
    uint32_t layout = 0; // columns of an `ext` block's layout: ks_ext_at(local column, d, t, layout, beta)
    uint32_t n = 0;      // extension launches, in order
    lm_ks_ext_launch at[2];
};
// The extension launches of a batch of B columns on a scratch whose `ext` blocks hold `half` columns each (0: a scratch
// of one block).  A batch of at most `half` columns is a single one: one launch, the layout of B columns, block 0.
// second_first: the launch of the second half goes first (the half whose coefficients the inverse transform wrote last).
inline lm_ks_ext_plan lm_ks_ext_launches(uint32_t B, uint32_t half, bool second_first = false) {
    lm_ks_ext_plan p;
    if (!half || B <= half) {
        p.layout = B, p.n = 1;
        p.at[0] = {0, B, 0};
        return p;
    }
    p.layout = half, p.n = 2;
    p.at[second_first ? 1 : 0] = {0, half, 0};
    p.at[second_first ? 0 : 1] = {half, B - half, 1};
    return p;
}
// where the gadget product finds column b of a batch: block b / layout at local column b % layout (two blocks at most)
inline uint32_t lm_ks_ext_block(uint32_t b, uint32_t layout) { return b < layout ? 0 : 1; }
inline uint32_t lm_ks_ext_local(uint32_t b, uint32_t layout) { return b < layout ? b : b - layout; }
