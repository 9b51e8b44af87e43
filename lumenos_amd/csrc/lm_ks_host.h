// Host-side declarations shared by the units of the hybrid key switch: the rotation's kernels and steps
// (lm_keyswitch.hip), the batch driver of its callers (lm_ks_batch.hip), the callers themselves -- InnerSum and
// matrixInnerSumEval (lm_innersum.hip), the rotation on its own (lm_rotate.hip), the ciphertext x ciphertext product
// that ends in a key switch (lm_mulrelin.hip) --, the placement of the scratch buffers (lm_ks_scratch.hip), the closing
// rotation before a rescale (lm_ks_close.hip), the diagonal linear transform (lm_lintrans.hip), the switching keys (lm_ks_key.hip) and the ciphertext x plaintext
// product that precedes an InnerSum (lm_mulplain.hip).
#pragma once
#include "lm_ks_dev.h"
#include "lm_ks_pair.h"

// per-context constants of the key switch at one level of the modulus chain (nl of the context's L limbs; below, L
// stands for nl) and its cached work lists (lm_keyswitch.hip)
struct KsTables {
    lm_dev<bx_t> d_bx;   // [beta][L+K], targets by position (ks_mod_at)
    lm_dev<bx_t> d_bxp;  // [L]  (P -> q_t)
    lm_dev<tw_t> d_pinv; // [L]  P^-1 mod q_t
    lm_dev<sfold_t> d_sfold; // [L]  the c0 fold's reduction of S modulo q_t (lm_ks_dev.h)
    u64 m2_lo = 0, m2_hi = 0; // 2M = 2 p_0 p_1, the offset of a two-limb lift W - 2M (K == 1: 0, the lift is the residue)
    uint32_t lift_bits = 0;   // |W - 2M| < 2^lift_bits
    uint32_t nl = 0;     // the level: Q limbs of the ciphertexts it switches
    uint32_t beta = 0;   // ceil(nl / K) digits
    lm_ninv_t yscale; // per modulus: N^-1 * (M/m)^-1 mod m of the source group the modulus sits in
    std::vector<uint16_t> pairs; // (digit | target << 8) of every extension the key switch needs, target-major
    std::map<uint32_t, lm_dev<uint32_t>> d_work; // per batch size: the workgroup order of the extension kernel
    std::map<uint32_t, lm_dev<uint32_t>> d_work_down; // ... and of the ModDown kernel (bit 31 of the key: polynomial 1 alone)
};
int get_tables(lumen_ctx *ctx, KsTables **out); // the top level's
// the tables of the level with nl limbs, 1 <= nl <= L, built at its first use and cached (nl == L: get_tables)
int get_tables_at(lumen_ctx *ctx, uint32_t nl, KsTables **out);

// the scratch buffers of one lane.  A pair's scratch (lm_ks_pair.h): coef, u and acc2 sized for 2 * half columns, and two
// `ext` blocks of `half` columns each -- a batch of more than `half` columns is extended half by half (rotate_decompose)
// and the gadget product reads both blocks.  half == 0: a scratch of single batches, one `ext` block.
struct KsScratch {
    u64 *coef, *ext, *u, *acc2;
    u64 *ext1 = nullptr;       // the second half's block
    uint32_t half = 0;         // columns per `ext` block
    bool second_first = false; // the second half is extended first (LUMEN_KS_PAIR=2)
};

// ---- the steps of a rotation of B columns (lm_keyswitch.hip).  acc, in, out: [B][2][nl][N] at the level of `tb`.
// s: scratch of a batch of B columns at the TOP level, of which a lower level uses a prefix of every block.
// steps 1-2: the digits of c1 extended to every limb, in s.coef and s.ext; depends on the ciphertext alone
int rotate_decompose(lumen_ctx *ctx, const u64 *acc, uint32_t B, KsTables *tb, const KsScratch &s);
// steps 3-4a under one key: the gadget product in s.u, its limbs modulo P in the coefficient domain and packed
int rotate_product(lumen_ctx *ctx, const u64 *acc, uint32_t B, const lm_galois_key &gk, KsTables *tb, const KsScratch &s);
// ... its two halves.  Step 3: the gadget product in s.u, all nl + K limbs in the NTT domain
int rotate_mac(lumen_ctx *ctx, const u64 *acc, uint32_t B, const lm_galois_key &gk, KsTables *tb, const KsScratch &s);
// step 4a on any block of s.u's layout (ks_u_at): its limbs modulo P to the coefficient domain, packed.  c1_only: those of
// polynomial 1 alone; polynomial 0's stay in the NTT domain (a giant step of the double-hoisted transform, lm_lintrans.hip)
int rotate_p_to_coef(lumen_ctx *ctx, u64 *u, uint32_t B, KsTables *tb, bool c1_only = false);
// after rotate_decompose: acc_out = acc + Rot_galEl(acc) for every column, lazy ([0, 2q)); another block than `acc`
int rotate_add(lumen_ctx *ctx, const u64 *acc, u64 *acc_out, uint32_t B, const lm_galois_key &gk, KsTables *tb, const KsScratch &s);
// all steps: acc_out = acc + Rot_galEl(acc) for every column, lazy ([0, 2q))
int rotate_accumulate(lumen_ctx *ctx, const u64 *acc, u64 *acc_out, uint32_t B, const lm_galois_key &gk,
                      KsTables *tb, const KsScratch &s);
// after rotate_product: out = Rot_galEl(in) for every column, canonical; `out` is another block than `in`.  (s.u may be
// any block of its layout that went through rotate_p_to_coef: InnerSum's lazy accumulator ends so, under the identity)
int rotate_store(lumen_ctx *ctx, const u64 *in, u64 *out, uint32_t B, const lm_galois_key &gk, KsTables *tb, const KsScratch &s);
// ... for polynomial 1 alone (ModDown's c1_only work list): polynomial 1 of `out` = ModDown of polynomial 1 of s.u under gk's
// tables, canonical, after rotate_p_to_coef on that polynomial at least.  `in` is not read, polynomial 0 of `out` not written.
int rotate_store_c1(lumen_ctx *ctx, const u64 *in, u64 *out, uint32_t B, const lm_galois_key &gk, KsTables *tb, const KsScratch &s);
// after rotate_decompose, the last rotation before a rescale: coef_out = the coefficient form of acc + Rot_galEl(acc)
int rotate_close(lumen_ctx *ctx, const u64 *acc, u64 *coef_out, uint32_t B, const lm_galois_key &gk, uint64_t gal_el,
                 KsTables *tb, const KsScratch &s);
// the last rotation of an InnerSum that a rescale follows, after its steps 1-4a (lm_ks_close.hip): out, [B][2][nl][N], gets
// the COEFFICIENT form of acc + Rot_galEl(acc), canonical -- what the rescale's inverse transform would have made of it.
// work_down: ModDown's work list for B columns at the level of `tb`.  fold_s: the folded lifts of polynomial 0, this
// rotation's included (the c0 fold, below), or NULL.
int ks_close_launch(lumen_ctx *ctx, const u64 *acc, u64 *out, uint32_t B, const lm_galois_key &gk, uint64_t gal_el,
                    KsTables *tb, const KsScratch &s, const uint32_t *work_down, const u64 *fold_s = nullptr);

// ---- the c0 fold (LUMEN_KS_C0_FOLD): the doublings of a plain InnerSum that ends in rotate_close keep
// polynomial 0 as c0 = A - P^-1 NTT(S).  A: polynomial 0 of the accumulator, rotated by the gadget product itself
// (k_ks_mac_fold); S: one signed three-word integer per coefficient, [B][3][N], rotated in the coefficient domain
// (k_lift_fold, lm_ks_close.hip); ModDown runs for polynomial 1 alone.  A rotation reads s_in (NULL: the first, S = 0)
// and writes s_out, another block.
// can S of `rotations` doublings be held, and is the ring one the fold's kernels serve?
bool ks_fold_serves(const lumen_ctx *ctx, const KsTables *tb, uint32_t rotations);
inline size_t ks_fold_words(const lumen_ctx *ctx, uint32_t B) { return (size_t)B * 3 * ctx->N; }
// after rotate_decompose: acc_out = acc + Rot_galEl(acc) in the folded form, lazy
int rotate_add_fold(lumen_ctx *ctx, const u64 *acc, u64 *acc_out, uint32_t B, const lm_galois_key &gk, uint64_t gal_el, KsTables *tb,
                    const KsScratch &s, const u64 *s_in, u64 *s_out);
// after rotate_decompose, the last rotation: as rotate_close, from the folded form
int rotate_close_fold(lumen_ctx *ctx, const u64 *acc, u64 *coef_out, uint32_t B, const lm_galois_key &gk, uint64_t gal_el,
                      KsTables *tb, const KsScratch &s, const u64 *s_in, u64 *s_out);
// s_out = s_in + sigma_coef(s_in + W - 2M), W the packed limbs modulo P of polynomial 0 in u (after rotate_p_to_coef)
int lift_fold_launch(lumen_ctx *ctx, const u64 *u, const u64 *s_in, u64 *s_out, uint32_t B, uint64_t gal_el, KsTables *tb);
// the scratch of a batch of B columns on `lane`, placed by measurement at a context's first key switch (lm_ks_scratch.hip).
// tb: always the TOP level's tables, whatever level asks -- the blocks are sized, and the candidates timed, once.
// pair: the scratch of a pair of batches of B columns each (lane 0 alone; the second `ext` block is the one lane 1 would have)
int get_scratch(lumen_ctx *ctx, uint32_t B, KsTables *tb, KsScratch *s, int lane = 0, u64 **group_acc = nullptr,
                size_t group_acc_bytes = 0, bool pair = false);

// step 0, MulNew(ct, pt) (lm_mulplain.hip): the plaintext as the device multiplier pt * T, and out = ct (.) it
int upload_ptT(lumen_ctx *ctx, const uint64_t *pt, uint32_t nl, u64 **out);
// the conversion alone, device to device: raw residues [np][N] by position at the level of nl limbs, np == nl (over Q)
// or nl + K (over Q and P: a diagonal of lumen_lintrans_load), to pt * T in Montgomery form
int launch_pt_prepare(lumen_ctx *ctx, const u64 *raw, u64 *ptM, uint32_t nl, uint32_t np);
int launch_mul_plain(lumen_ctx *ctx, const u64 *ct, u64 *out, const u64 *ptT, size_t words, uint32_t nl,
                     uint32_t ncts);

// ---- InnerSum's lazy accumulator over Q and P (lm_innersum.hip), shared with the diagonal linear transform
// (lm_lintrans.hip).  lazy_blocks: per lane one block of s.u's size and layout at the top level.  identity_tables: the
// identity's gather tables, owned by the context.  lazy_close: out = ModDown(lazy) + cur for every column, canonical; cur
// in [0, 2q), `out` another block than `cur`, lazy is consumed.
struct KsRun;
int lazy_blocks(lumen_ctx *ctx, const KsRun &run, u64 **lazy);
int identity_tables(lumen_ctx *ctx, std::shared_ptr<lm_galois_key> *out);
int lazy_close(lumen_ctx *ctx, const u64 *cur, u64 *out, u64 *lazy, uint32_t B, KsTables *tb, const KsScratch &s);

// the relinearisation key as a switching key with identity gather tables (lm_ks_key.hip); empty before lumen_load_relin_key
std::shared_ptr<lm_galois_key> lm_relin_key(lumen_ctx *ctx);
// the loaded Galois key of an element, complete (key, gather table and its inverse), or a refusal (lm_ks_key.hip).  An
// entry of the map never moves or goes, and a key loaded again keeps its blocks: the pointer outlives the lock.
int ks_find_key(lumen_ctx *ctx, uint64_t gal_el, const lm_galois_key **gk);
// a set at a level of the chain: full width, 1 <= nl <= L (lm_ks_batch.hip)
int check_level_of_chain(lumen_ctx *ctx, const lumen_set *in, const char *what);
// the batching of a key switch: columns per batch, lanes of the context, pairs of batches (lm_ks_batch.hip)
uint32_t ks_batch(const lumen_ctx *ctx);
uint32_t ks_lanes(const lumen_ctx *ctx);
uint32_t ks_pair(const lumen_ctx *ctx); // 0: none; 1: pairs; 2: pairs, the second half extended first
// enqueue on the context's second stream for the lifetime of the guard
struct LaneGuard {
    lumen_ctx *ctx;
    hipStream_t saved;
    LaneGuard(lumen_ctx *c, int lane) : ctx(c), saved(c->stream) {
        if (lane) ctx->stream = ctx->stream2;
    }
    ~LaneGuard() { ctx->stream = saved; }
};

// ---- the batch driver of the key switch's callers (lm_ks_batch.hip): `count` ciphertexts at the level of nl limbs go
// through the key switch in BATCHES of at most Bmax columns, which alternate between the LANES; a caller with an
// accumulator for a GROUP of batches (matrixInnerSumEval, lumen_mul_relin: every batch works in its own slice of it)
// takes groups of 8 batches, the others one group of everything.  With `pair` (one lane, a caller that asked for it:
// InnerSum and matrixInnerSumEval) two consecutive batches of a group go as one pair of up to Bcap = 2 Bmax columns
// (lm_ks_take).
struct KsRun {
    KsTables *top = nullptr, *tb = nullptr; // the top level's tables (they size the scratch) and the level's
    uint32_t Bmax = 0, group = 0, lanes = 1;
    bool grouped = false, pair = false;
    uint32_t Bcap() const { return pair ? 2 * Bmax : Bmax; } // the most columns a batch has: a caller's per-lane blocks are sized for it
    size_t group_bytes = 0; // a group's accumulators at the TOP level
    KsScratch s[2] = {};    // per lane
    u64 *acc = nullptr;     // the group's accumulators (grouped runs)
};
// Opens a run in two steps, because a caller's own refusals and allocations stand between them.  ks_run_open: both table
// sets (it refuses what the key switch cannot serve) and the batching; allocates no scratch.  max_lanes: 1 keeps the run
// on the main stream, 2 gives it the context's lanes.  ks_run_scratch: the lanes' scratch and the group's accumulators.
// may_pair: the caller's per-batch work takes a pair's scratch (every rotate_* step does).
int ks_run_open(lumen_ctx *ctx, uint32_t count, uint32_t nl, uint32_t max_lanes, bool group_acc, KsRun *run, bool may_pair = false);
int ks_run_scratch(lumen_ctx *ctx, KsRun *run);
// The loop: per group fork, batch(g0, first, B, s, acc) for every batch -- ciphertexts [g0 + first, g0 + first + B) of the
// caller's, on the batch's lane, s that lane's scratch, acc the batch's slice of the group's accumulators (words of ctw per
// ciphertext; NULL without) --, join, then end_of_group(g0, gn) on the main stream.  The first non-zero status ends the run.
template <class Batch, class Group>
int ks_run(lumen_ctx *ctx, const KsRun &run, uint32_t count, size_t ctw, Batch &&batch, Group &&end_of_group) {
    for (uint32_t g0 = 0; g0 < count; g0 += run.group) {
        const uint32_t gn = std::min(run.group, count - g0);
        if (run.lanes > 1) { // fork: the second lane starts after everything already enqueued on the main stream
            LM_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
            LM_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
        }
        uint32_t lane = 0;
        for (uint32_t first = 0, B = 0; first < gn; first += B, lane = (lane + 1) % run.lanes) {
            B = lm_ks_take(run.Bmax, run.pair, gn - first);
            LaneGuard guard(ctx, (int)lane);
            if (int rc = batch(g0, first, B, run.s[lane], run.acc ? run.acc + (size_t)first * ctw : nullptr)) return rc;
        }
        if (run.lanes > 1) { // join: the next group reuses the accumulators, and what follows reads on the main stream
            LM_HIP(ctx, hipEventRecord(ctx->ev_join, ctx->stream2));
            LM_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        }
        if (int rc = end_of_group(g0, gn)) return rc;
    }
    return 0;
}
template <class Batch>
int ks_run(lumen_ctx *ctx, const KsRun &run, uint32_t count, size_t ctw, Batch &&batch) {
    return ks_run(ctx, run, count, ctw, batch, [](uint32_t, uint32_t) { return 0; });
}
