// Where in HBM the key switch's scratch buffers sit (host only): candidate allocations, timed rotations, the chosen
// blocks adopted as the context's scratch.  The selection policy itself is lm_placement.h.
#include "lm_ks_host.h"
#include "lm_placement.h"

namespace {

// every return path gives back what the selection borrowed from the context
struct ProfOff { // the timed rotations are not part of anybody's measurement
    lumen_ctx *ctx;
    bool saved;
    explicit ProfOff(lumen_ctx *c) : ctx(c), saved(c->prof) { ctx->prof = false; }
    ~ProfOff() { ctx->prof = saved; }
};
struct EventPair { // two pooled events
    lumen_ctx *ctx;
    hipEvent_t e0, e1;
    explicit EventPair(lumen_ctx *c) : ctx(c), e0(lm_ev_get(c)), e1(lm_ev_get(c)) {}
    ~EventPair() { ctx->ev_pool.push_back(e0), ctx->ev_pool.push_back(e1); }
};

} // namespace

// ---- the key switch's scratch buffers, and WHERE in HBM they sit.
// Measured in round 6 (profiles/r06_exp_ks_mac_placement.txt): the time of the gadget product is a deterministic
// function of the physical placement of its streams -- two processes that draw the same addresses reproduce each
// other's times to 0.2 %; exchanging only the block `u` is written to, or only the block `ext` is read from, for
// another allocation of the same size moves the kernel by up to 16 % / 7 %; the relative offset of the two inside
// one allocation (4 KB .. 64 MB) moves it by nothing, and one stream alone reads / writes every block at the same rate.
// It is the pairing of a read stream's and a write stream's 2 MB pages (high physical address bits: DRAM rank /
// bank-group assignment, invisible and uncontrollable from user space) -- which is why `ks_mac` was constant inside
// a process and 341 .. 381 ms per step between processes.  So the first key switch of a context allocates
// LUMEN_KS_PLACEMENT (6) candidates per buffer and keeps, buffer by buffer, the one under which two rotations of a
// whole batch run fastest (coordinate descent in the order the sensitivities were measured: u, ext, then the
// accumulator's twin and the coefficient buffer); the others are freed.  One-off cost at the headline size: about
// 0.3 s and 14 GB of transient device memory (never more than half of what is free).  Results do not depend on the choice
// (same kernels, same residues).
// group_acc / group_acc_bytes: the caller's accumulator block for a GROUP of batches (lumen_matrix_inner_sum: every batch works in
// its own slice of it) is placed by the same measurement -- in situ the rotations alternate between reading a slice of it
// and reading the twin, and with only the four buffers above chosen the gadget product still came out in two modes from
// process to process (331 / 349 ms per step).
// pair (lm_ks_pair.h; lane 0): coef, u and the twin hold 2 B columns, and a SECOND `ext` block of B columns -- the one lane 1
// would have, under lane 1's name -- is drawn and chosen like the first, right after it; the timed rotations are a pair's.
// The selection's transient memory and time roughly double.
int get_scratch(lumen_ctx *ctx, uint32_t B, KsTables *tb, KsScratch *s, int lane, u64 **group_acc, size_t group_acc_bytes, bool pair) {
    const size_t N = ctx->N, L = ctx->L, LK = ctx->L + ctx->K, beta = tb->beta;
    LM_CHECK(ctx, !pair || lane == 0, "a pair of key-switch batches runs on the first lane");
    enum { COEF, EXT, U, ACC2, ACC, EXT1, NBUF };
    const char *names[2][NBUF] = {{"ks_coef", "ks_ext", "ks_u", "ks_acc2", "ks_acc", "ks_ext_b"}, {"ks_coef_b", "ks_ext_b", "ks_u_b", "ks_acc2_b", "ks_acc", ""}};
    const uint32_t Bt = pair ? 2 * B : B; // columns of the blocks every kernel but the extension works on
    const size_t bytes[NBUF] = {(size_t)Bt * L * N * 8, (size_t)B * beta * LK * N * 8, (size_t)Bt * 2 * LK * N * 8, (size_t)Bt * 2 * L * N * 8,
                                std::max(group_acc_bytes, (size_t)Bt * 2 * L * N * 8), (size_t)B * beta * LK * N * 8};
    u64 *dummy = nullptr;
    u64 **slot[NBUF] = {&s->coef, &s->ext, &s->u, &s->acc2, group_acc ? group_acc : &dummy, &s->ext1};
    std::vector<int> ids = {COEF, EXT, U, ACC2}; // the buffers of this call; at[c]: buffer c's place among them
    if (group_acc) ids.push_back(ACC);
    if (pair) ids.push_back(EXT1);
    int at[NBUF] = {-1, -1, -1, -1, -1, -1};
    for (size_t k = 0; k < ids.size(); k++) at[ids[k]] = (int)k;
    s->ext1 = nullptr, s->half = pair ? B : 0, s->second_first = false;
    const uint32_t Kc = ctx->tune.ks_placement;
    // what is already there and large enough stays (a buffer shared with the other lane, a context whose batch size grew):
    // only the missing buffers are drawn
    std::vector<lm_place_buf> bufs;
    bool have = true;
    for (int c : ids) {
        auto it = ctx->scratch.find(names[lane][c]);
        const bool there = it != ctx->scratch.end() && it->second && it->second.count() >= bytes[c];
        bufs.push_back({bytes[c], there ? it->second.get() : nullptr, c == ACC ? 4u : Kc}); // (the group accumulator is the big one: four draws)
        have = have && there;
    }
    // the key the timed rotations run under: any Galois key, or the relinearisation key where a context's first key
    // switch is a ciphertext x ciphertext product (its placement then serves the InnerSums that follow as well)
    const lm_galois_key *gk = nullptr;
    {
        LM_SHARED_LOCK(ctx);
        if (!ctx->gkeys.empty()) gk = &ctx->gkeys.begin()->second;
    }
    const std::shared_ptr<lm_galois_key> rlk = gk ? nullptr : lm_relin_key(ctx); // kept alive for the selection
    if (!gk) gk = rlk.get();
    auto plain = [&]() -> int {
        bool ok = true;
        for (int c : ids) ok = (*slot[c] = (u64 *)lm_scratch(ctx, names[lane][c], bytes[c])) != nullptr && ok;
        return ok ? 0 : 1;
    };
    // small buffers live in the caches, and without a key no rotation can be timed: plain allocation
    if (have || Kc < 2 || bytes[EXT] < ((size_t)64 << 20) || !gk || !gk->d_key) return plain();
    { // the selection: whatever it drew and did not hand out is freed when this scope ends, on every path
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        lm_dev<u64> probe_acc;
        if (!group_acc) (void)probe_acc.alloc(ctx, bytes[ACC2] / 8, "the placement's probe accumulator");
        lm_placement place(bufs, [](void *p) { hipFree(p); });
        const bool drew = place.draw(Kc, free_b, [&](size_t k) {
            void *p = nullptr;
            return hipMalloc(&p, bytes[ids[k]]) == hipSuccess ? p : nullptr;
        });
        (void)hipGetLastError();
        if (drew && (group_acc || probe_acc)) { // otherwise memory is short: no choice to make
            int rc;
            {
                ProfOff quiet(ctx);
                EventPair ev(ctx);
                // two rotations of a batch (the accumulator ping-pongs with its twin): one pair untimed, two timed -- in the first
                // and in the last batch slice of the group accumulator
                auto eval = [&](const size_t *pick, float *ms) -> int {
                    auto blk = [&](int c) { return (u64 *)place.block((size_t)at[c], pick[at[c]]); };
                    KsScratch t;
                    t.coef = blk(COEF), t.ext = blk(EXT), t.u = blk(U), t.acc2 = blk(ACC2);
                    if (pair) t.ext1 = blk(EXT1), t.half = B;
                    u64 *a0 = group_acc ? blk(ACC) : probe_acc.get();
                    u64 *a1 = group_acc ? a0 + (bytes[ACC] - bytes[ACC2]) / 8 : a0;
                    for (int r = 0; r < 3; r++) {
                        if (r == 1) LM_HIP(ctx, hipEventRecord(ev.e0, ctx->stream));
                        u64 *a = r == 2 ? a1 : a0;
                        if (int e = rotate_accumulate(ctx, a, t.acc2, Bt, *gk, tb, t)) return e;
                        if (int e = rotate_accumulate(ctx, t.acc2, a, Bt, *gk, tb, t)) return e;
                    }
                    LM_HIP(ctx, hipEventRecord(ev.e1, ctx->stream));
                    LM_HIP(ctx, hipEventSynchronize(ev.e1));
                    LM_HIP(ctx, hipEventElapsedTime(ms, ev.e0, ev.e1));
                    return 0;
                };
                // u, ext (both blocks of a pair), the group accumulator, its twin, coef: the order the sensitivities were measured in
                std::vector<int> order;
                for (int c : {U, EXT, EXT1, ACC, ACC2, COEF})
                    if (at[c] >= 0) order.push_back(at[c]);
                rc = place.descend(order, eval);
            }
            if (rc) {
                lm_sync_all(ctx);
                return rc;
            }
            if (ctx->tune.debug)
                fprintf(stderr, "[lumenos_hip] key-switch scratch placement (lane %d, %u columns%s): %zu / %zu / %zu candidates for u / ext / the group "
                                "accumulator, 4 rotations of the first draw %.3f ms, of the chosen blocks %.3f ms\n", lane, Bt, pair ? ", a pair" : "",
                        place.count((size_t)at[U]), place.count((size_t)at[EXT]), group_acc ? place.count((size_t)at[ACC]) : (size_t)0, place.first,
                        place.best_all);
            LM_HIP(ctx, hipStreamSynchronize(ctx->stream)); // nothing may still run on a block that is about to be freed
            for (int c : ids) {
                void *chosen = place.take((size_t)at[c]);
                if (!bufs[(size_t)at[c]].fixed) lm_scratch_adopt(ctx, names[lane][c], chosen, bytes[c]);
                *slot[c] = (u64 *)chosen;
            }
            return 0;
        }
    }
    return plain();
}
