// The batching of the key switch's callers (host only): how many columns go through a rotation together, on how many
// lanes, in what groups, with which scratch.  InnerSum and matrixInnerSumEval (lm_innersum.hip), the rotation on its own
// (lm_rotate.hip) and the ciphertext x ciphertext product (lm_mulrelin.hip) open a run here and hand their per-batch
// work to its loop (ks_run, lm_ks_host.h).
#include "lm_ks_host.h"

// columns processed together (scratch ~ 172 limbs per column): 64 by default, LUMEN_KS_BATCH at context
// creation (lm_tuning)
uint32_t ks_batch(const lumen_ctx *ctx) { return ctx->tune.ks_batch; }

// Lanes: independent column batches alternate between the context's two streams (LaneGuard, lm_ks_host.h) so that the
// HBM-bound steps of one batch (gadget product, correction-bit pass) overlap the VALU-bound transforms of the other.
// Two lanes up to N = 2^13, one at N = 2^14 (round 4, measured on one MI355X, seconds per prover step with 1 / 2
// lanes: 2048x1024 0.0850 / 0.0743, 4096x2048 0.193 / 0.163, 8192x4096 0.864 / 0.799, 16384x4096 1.86 / 1.92).
// Up to 2^13 a limb needs at most half of a CU's LDS, so workgroups of two kernels are resident side by side and
// one batch's memory-bound steps run under the other's transforms; at 2^14 a transform workgroup owns the whole
// LDS and two transform kernels only evict each other's L2 sets (still so with the forward kernels of a rotation two
// workgroups per CU and the inverse ones owning it: 1.677 / 1.718 s, round 10).  LUMEN_KS_LANES = 1 / 2 overrides.  (With two
// lanes a kernel's HIP-event time includes its neighbour's: the roofline is read at N = 2^14, one lane.)
uint32_t ks_lanes(const lumen_ctx *ctx) {
    return ctx->tune.ks_lanes ? ctx->tune.ks_lanes : (ctx->logN <= 13 ? 2 : 1);
}

// Pairs (LUMEN_KS_PAIR; lm_ks_pair.h): on ONE lane, two consecutive batches of a group go through a rotation as one pair
// of 2 x ks_batch columns.  The kernels whose grids have twelve (or two) units per column -- the c1 inverse and its
// packing, the gadget product, the P-limb leg, the lift fold, ModDown, the close -- run once over the pair, on blocks of
// the pair's size: at 64 columns their grids are fractions of a round of the device (ModDown for polynomial 1: 768
// workgroups on 512 slots), two of six digits miss the packing inside the inverse, and the gadget product reads every
// key slice once per 64 columns.  The extension kernel runs once per half, at its 64-column shape, into the half's own
// `ext` block: over 128 columns of one block it loses more than the others gain (EXPERIMENTS 6.6, 6.6b, R21).  Two
// lanes take no pairs: a pair is what the second lane's scratch would hold.  The default is by ring degree, as the
// lanes': pairs at N = 2^14, where a run has one lane (EXPERIMENTS R21).  LUMEN_KS_PAIR = 0 / 1 overrides; a pair's
// callers are InnerSum and matrixInnerSumEval, every other caller of the key switch keeps single batches.
uint32_t ks_pair(const lumen_ctx *ctx) {
    return ctx->tune.ks_pair >= 0 ? (uint32_t)ctx->tune.ks_pair : (ctx->logN == 14 ? 1 : 0);
}

// A set at a level of the chain: full width, 1 <= nl <= L (a set of another context may have more).
int check_level_of_chain(lumen_ctx *ctx, const lumen_set *in, const char *what) {
    LM_FULL_WIDTH(ctx, in, what);
    LM_CHECK(ctx, in->nl >= 1 && in->nl <= ctx->L, "%s: set has %u limbs, the chain has %u", what, in->nl, ctx->L);
    return 0;
}

int ks_run_open(lumen_ctx *ctx, uint32_t count, uint32_t nl, uint32_t max_lanes, bool group_acc, KsRun *run, bool may_pair) {
    if (int rc = get_tables(ctx, &run->top)) return rc; // (refuses K > 2)
    if (int rc = get_tables_at(ctx, nl, &run->tb)) return rc;
    run->Bmax = std::min<uint32_t>(ks_batch(ctx), std::max(count, 1u));
    // what ends a group (the rescale to level 1 of matrixInnerSumEval) runs on groups of batches: one batch alone (2*B
    // polynomials) does not fill the 256 CUs in the kernels that take one workgroup per polynomial
    run->group = group_acc ? std::min<uint32_t>(8 * run->Bmax, std::max(count, 1u)) : std::max(count, 1u);
    run->lanes = std::min(ks_lanes(ctx), max_lanes);
    run->pair = may_pair && ks_pair(ctx) && run->lanes == 1 && count > run->Bmax; // (at most one batch: nothing to pair)
    run->grouped = group_acc;
    run->group_bytes = (size_t)run->group * 2 * ctx->L * ctx->N * 8; // sized for the top level, as the key switch's scratch
    return 0;
}

// The scratch is the top level's whatever the level: a first call low in the chain must not run the placement selection
// on small blocks that the first call at the top would regrow.  The group's accumulators are placed together with the
// first lane's scratch (get_scratch: five buffers drawn instead of four).
int ks_run_scratch(lumen_ctx *ctx, KsRun *run) {
    if (get_scratch(ctx, run->Bmax, run->top, &run->s[0], 0, run->grouped ? &run->acc : nullptr, run->grouped ? run->group_bytes : 0,
                    run->pair) ||
        (run->lanes > 1 && get_scratch(ctx, run->Bmax, run->top, &run->s[1], 1)))
        return 1;
    run->s[0].second_first = run->pair && ks_pair(ctx) == 2;
    return run->grouped && !run->acc ? 1 : 0;
}
