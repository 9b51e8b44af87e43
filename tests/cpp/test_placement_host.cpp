// The scratch-placement policy (lumenos_amd/csrc/lm_placement.h) without a device: fake draw / release callables that
// count, a scripted eval.  Conditions (a)-(e) are read off the selection loop as it stood inside get_scratch.
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "lm_placement.h"

static int failures = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            failures++;                                    \
            printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                           \
            printf("\n");                                  \
        }                                                  \
    } while (0)

// hands out fake addresses and counts what happens to them
struct Heap {
    std::vector<lm_place_buf> bufs;
    std::vector<std::vector<void *>> drawn; // per buffer, in draw order
    std::map<void *, int> released;
    std::vector<int> fail_draws; // ordinals (over all draw calls) that return nullptr
    int calls = 0;
    uintptr_t next = 0x1000;
    explicit Heap(std::vector<lm_place_buf> b) : bufs(std::move(b)), drawn(bufs.size()) {}
    void *draw(size_t c) {
        const int ord = calls++;
        for (int f : fail_draws)
            if (f == ord) return nullptr;
        void *p = (void *)(next += 0x1000);
        drawn[c].push_back(p);
        return p;
    }
    std::function<void(void *)> releaser() {
        return [this](void *p) { released[p]++; };
    }
    size_t beyond_first_bytes() const {
        size_t s = 0;
        for (size_t c = 0; c < bufs.size(); c++)
            if (drawn[c].size() > 1) s += (drawn[c].size() - 1) * bufs[c].bytes;
        return s;
    }
    // every drawn block except `kept` released exactly once; `kept` and the fixed blocks never
    void check_released(const std::vector<void *> &kept, const char *what) {
        size_t want = 0;
        for (size_t c = 0; c < bufs.size(); c++)
            for (void *p : drawn[c]) {
                bool k = false;
                for (void *q : kept) k = k || q == p;
                const int n = released.count(p) ? released[p] : 0;
                CHECK(n == (k ? 0 : 1), "%s: block %p of buffer %zu released %d times (kept: %d)", what, p, c, n, (int)k);
                want += k ? 0 : 1;
            }
        CHECK(released.size() == want, "%s: %zu blocks released, %zu expected (a fixed or foreign block among them)", what,
              released.size(), want);
        for (auto &b : bufs)
            if (b.fixed) CHECK(!released.count(b.fixed), "%s: fixed block %p released", what, b.fixed);
    }
};

static char fixed_block[16];
static const size_t MB = (size_t)1 << 20;
static const std::vector<int> ORDER5 = {2, 1, 4, 3, 0};

// five buffers like the key switch's (coef, ext, u, acc2, the group accumulator with four draws), acc2 optionally fixed
static std::vector<lm_place_buf> five(unsigned Kc, bool fix3) {
    return {{48 * MB, nullptr, Kc}, {336 * MB, nullptr, Kc}, {56 * MB, nullptr, Kc}, {48 * MB, fix3 ? (void *)fixed_block : nullptr, Kc},
            {384 * MB, nullptr, 4}};
}

// separable cost: 100 + sum_c w[c][pick[c]]
static float cost(const std::vector<std::vector<float>> &w, const size_t *pick) {
    float s = 100;
    for (size_t c = 0; c < w.size(); c++) s += w[c][pick[c]];
    return s;
}

static void test_argmin_and_eval_count() {
    const unsigned Kc = 6;
    for (int fix = 0; fix < 2; fix++) {
        Heap h(five(Kc, fix));
        std::vector<void *> kept;
        {
            lm_placement place(h.bufs, h.releaser());
            CHECK(place.draw(Kc, (size_t)64 << 30, [&](size_t c) { return h.draw(c); }), "ample memory: no choice");
            const size_t want_n[5] = {6, 6, 6, fix ? 1u : 6u, 4};
            for (int c = 0; c < 5; c++) CHECK(place.count(c) == want_n[c], "buffer %d has %zu candidates", c, place.count(c));
            CHECK(h.drawn[4].size() <= 4, "group accumulator drawn %zu times", h.drawn[4].size());
            // distinct weights, argmin at a different index per buffer (never 0 except for the fixed one)
            std::vector<std::vector<float>> w(5);
            const size_t argmin[5] = {3, 5, 1, fix ? 0u : 2u, 3};
            for (int c = 0; c < 5; c++)
                for (size_t k = 0; k < place.count(c); k++) w[c].push_back(k == argmin[c] ? 1.0f : 2.0f + (float)((k * 7 + c) % 5));
            int evals = 0;
            float first_ms = 0;
            const int rc = place.descend(ORDER5, [&](const size_t *pick, float *ms) {
                *ms = cost(w, pick);
                if (!evals++) first_ms = *ms;
                return 0;
            });
            CHECK(rc == 0, "descend returned %d", rc);
            size_t want_evals = 1;
            for (int c = 0; c < 5; c++) want_evals += place.count(c) - 1;
            CHECK((size_t)evals == want_evals, "(b) eval ran %d times, 1 + sum (n_c - 1) = %zu", evals, want_evals);
            for (int c = 0; c < 5; c++) CHECK(place.chosen(c) == argmin[c], "(a) buffer %d: chose %zu, argmin %zu", c, place.chosen(c), argmin[c]);
            CHECK(place.first == first_ms, "first = %f, the first eval gave %f", place.first, first_ms);
            CHECK(place.best_all == 105.0f, "best_all = %f, the minimum is 105", place.best_all);
            for (int c = 0; c < 5; c++) {
                void *p = place.take(c);
                CHECK(p == (c == 3 && fix ? (void *)fixed_block : h.drawn[c][argmin[c]]), "take(%d) is not the chosen block", c);
                kept.push_back(p);
            }
            CHECK(h.released.empty(), "released before the selection ended");
        }
        h.check_released(kept, fix ? "(e) success, one fixed" : "(e) success");
    }
    printf("PASS argmin, eval count, release on success\n");
}

static void test_ties_keep_the_current_pick() {
    const unsigned Kc = 4;
    // all configurations equally fast: every buffer keeps candidate 0
    {
        Heap h(five(Kc, false));
        lm_placement place(h.bufs, h.releaser());
        CHECK(place.draw(Kc, (size_t)64 << 30, [&](size_t c) { return h.draw(c); }), "no choice");
        place.descend(ORDER5, [&](const size_t *, float *ms) { return *ms = 7.0f, 0; });
        for (int c = 0; c < 5; c++) CHECK(place.chosen(c) == 0, "(c) all equal: buffer %d moved to %zu", c, place.chosen(c));
    }
    // a later candidate that only EQUALS the best so far does not replace it: inside the first buffer of the order
    // (u: candidates 1 and 3 tie for the minimum -> 1), and across buffers (ext: candidate 2 is as fast as the pick -> 0)
    {
        Heap h(five(Kc, false));
        lm_placement place(h.bufs, h.releaser());
        CHECK(place.draw(Kc, (size_t)64 << 30, [&](size_t c) { return h.draw(c); }), "no choice");
        std::vector<std::vector<float>> w = {{0, 1, 1, 1}, {2, 3, 2, 3}, {5, 4, 6, 4}, {0, 1, 2, 3}, {1, 1, 1, 1}};
        place.descend(ORDER5, [&](const size_t *pick, float *ms) { return *ms = cost(w, pick), 0; });
        const size_t want[5] = {0, 0, 1, 0, 0};
        for (int c = 0; c < 5; c++) CHECK(place.chosen(c) == want[c], "(c) tie: buffer %d chose %zu, want %zu", c, place.chosen(c), want[c]);
    }
    printf("PASS ties keep the current pick\n");
}

static void test_budget() {
    const unsigned Kc = 6;
    // first candidates: 872 MB.  Half of what is free, for a range of budgets from "nothing beyond the first" to ample
    for (size_t free_mb : {100u, 1744u, 1800u, 2000u, 2600u, 3500u, 5000u, 9000u, 20000u}) {
        Heap h(five(Kc, false));
        lm_placement place(h.bufs, h.releaser());
        CHECK(place.draw(Kc, free_mb * MB, [&](size_t c) { return h.draw(c); }), "free %zu MB: no choice", free_mb);
        CHECK(h.beyond_first_bytes() <= free_mb * MB / 2, "(d) free %zu MB: %zu MB drawn beyond the first candidates", free_mb,
              h.beyond_first_bytes() / MB);
        CHECK(h.drawn[4].size() <= 4, "(d) group accumulator drawn %zu times", h.drawn[4].size());
        for (int c = 0; c < 5; c++) CHECK(h.drawn[c].size() >= 1 && h.drawn[c].size() <= Kc, "buffer %d drawn %zu times", c, h.drawn[c].size());
        if (free_mb == 100) CHECK(h.calls == 5, "a budget below the first candidates: %d draws, want one per buffer", h.calls);
        if (free_mb == 20000) CHECK(h.calls == 4 * 6 + 4, "ample memory: %d draws, want 28", h.calls);
    }
    // round-robin: the order of the first draws is buffer 0, 1, 2, 3, 4, 0, 1, ...
    {
        Heap h(five(Kc, false));
        std::vector<size_t> seq;
        lm_placement place(h.bufs, h.releaser());
        place.draw(Kc, (size_t)64 << 30, [&](size_t c) { return seq.push_back(c), h.draw(c); });
        for (size_t i = 0; i < 20; i++) CHECK(seq[i] == i % 5, "draw %zu went to buffer %zu", i, seq[i]);
        for (size_t i = 20; i < seq.size(); i++) CHECK(seq[i] == (i - 20) % 4, "draw %zu went to buffer %zu", i, seq[i]);
    }
    printf("PASS budget and draw order\n");
}

static void test_release_on_every_path() {
    const unsigned Kc = 3;
    // a buffer with no candidate: every draw of buffer 2 fails (draw ordinals 2, 6, 10 of 4 drawn buffers per round)
    {
        Heap h(five(Kc, true));
        h.fail_draws = {2, 6, 10};
        {
            lm_placement place(h.bufs, h.releaser());
            CHECK(!place.draw(Kc, (size_t)64 << 30, [&](size_t c) { return h.draw(c); }), "a buffer without candidate must mean no choice");
            h.check_released({}, "(e) no candidate, before the destructor"); // released at once: the caller allocates plainly next
        }
        h.check_released({}, "(e) no candidate");
    }
    // eval fails on its first call, and on a later one
    for (int fail_at : {0, 4}) {
        Heap h(five(Kc, true));
        int evals = 0;
        {
            lm_placement place(h.bufs, h.releaser());
            CHECK(place.draw(Kc, (size_t)64 << 30, [&](size_t c) { return h.draw(c); }), "no choice");
            const int rc = place.descend(ORDER5, [&](const size_t *pick, float *ms) {
                *ms = 10.0f - (float)pick[2];
                return evals++ == fail_at ? 42 : 0;
            });
            CHECK(rc == 42, "descend returned %d, eval failed with 42", rc);
            CHECK(evals == fail_at + 1, "eval ran %d times after failing on call %d", evals, fail_at);
        }
        h.check_released({}, fail_at ? "(e) eval fails on a later call" : "(e) eval fails on its first call");
    }
    printf("PASS release on every path\n");
}

int main() {
    test_argmin_and_eval_count();
    test_ties_keep_the_current_pick();
    test_budget();
    test_release_on_every_path();
    if (failures) return printf("%d check(s) failed\n", failures), 1;
    printf("placement policy OK\n");
    return 0;
}
