// Which of several candidate allocations to keep for each of a few buffers, chosen by timing: the POLICY alone -- the
// budget, the order of the draws, the coordinate descent -- over three callables, so that it runs without a device
// (tests/cpp/test_placement_host.cpp).  The mechanism (hipMalloc, rotations between events) is lm_ks_scratch.hip.
// Plain C++17, no HIP.  The object owns what it drew: whatever take() has not handed out is released by the destructor,
// on every path, exactly once; fixed blocks are the caller's and never released.
#pragma once
#include <cstddef>
#include <functional>
#include <vector>

struct lm_place_buf {
    size_t bytes;       // size of each candidate
    void *fixed;        // an existing block to keep: the buffer's only candidate (nullptr: draw)
    unsigned max_draws; // candidates drawn at most
};

class lm_placement {
    std::vector<lm_place_buf> buf;
    std::vector<std::vector<void *>> cand;
    std::vector<size_t> pick;
    std::function<void(void *)> release;

  public:
    float first = 0, best_all = 0; // time of the first configuration measured, and of the chosen one
    lm_placement(std::vector<lm_place_buf> bufs, std::function<void(void *)> rel)
        : buf(std::move(bufs)), cand(buf.size()), pick(buf.size(), 0), release(std::move(rel)) {
        for (size_t c = 0; c < buf.size(); c++)
            if (buf[c].fixed) cand[c].push_back(buf[c].fixed);
    }
    lm_placement(const lm_placement &) = delete;
    lm_placement &operator=(const lm_placement &) = delete;
    ~lm_placement() { release_all(); }
    void release_all() {
        for (size_t c = 0; c < buf.size(); c++) {
            if (!buf[c].fixed)
                for (void *p : cand[c])
                    if (p) release(p);
            cand[c].clear();
        }
    }
    size_t count(size_t c) const { return cand[c].size(); }
    void *block(size_t c, size_t k) const { return cand[c][k]; }
    size_t chosen(size_t c) const { return pick[c]; }
    // the chosen block of buffer c: the caller's from here on
    void *take(size_t c) {
        void *p = cand[c][pick[c]];
        if (!buf[c].fixed) cand[c][pick[c]] = nullptr;
        return p;
    }
    // Up to Kc candidates per buffer, round-robin over the buffers so that the candidates of one buffer are spread out;
    // a buffer that has a candidate is not drawn again once that would take the draws past half of what was free.
    // draw(c) -> block or nullptr.  false: some buffer has no candidate -- no choice to make, everything is released.
    template <class Draw>
    bool draw(unsigned Kc, size_t free_bytes, Draw &&draw_one) {
        size_t drawn = 0;
        for (unsigned k = 0; k < Kc; k++)
            for (size_t c = 0; c < buf.size(); c++) {
                if (buf[c].fixed || k >= buf[c].max_draws) continue;
                if (!cand[c].empty() && drawn + buf[c].bytes > free_bytes / 2) continue;
                if (void *p = draw_one(c)) cand[c].push_back(p), drawn += buf[c].bytes;
            }
        for (size_t c = 0; c < buf.size(); c++)
            if (cand[c].empty()) return release_all(), false;
        return true;
    }
    // Coordinate descent over the buffers in `order`: eval(pick, &ms) times the configuration pick[] (one candidate index
    // per buffer) and returns non-zero on failure, which ends the descent with that code.  A buffer keeps its current
    // candidate unless another one is strictly faster than everything measured so far.
    template <class Eval>
    int descend(const std::vector<int> &order, Eval &&eval) {
        bool measured = false;
        for (int c : order) {
            float best = 0;
            size_t arg = pick[c];
            for (size_t k = 0; k < cand[c].size(); k++) {
                if (measured && k == pick[c]) continue; // timed already: it is the configuration `best_all` belongs to
                const size_t keep = pick[c];
                pick[c] = k;
                float ms = 0;
                const int rc = eval(pick.data(), &ms);
                pick[c] = keep;
                if (rc) return rc;
                if (first == 0) first = ms;
                if (best == 0 || ms < best) best = ms, arg = k;
            }
            if (best == 0 || (measured && best_all <= best)) arg = pick[c]; // nothing beat the configuration already measured
            else best_all = best;
            if (best != 0) measured = true;
            pick[c] = arg;
        }
        return 0;
    }
};
