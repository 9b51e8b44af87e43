"""Times the prover's inner product (matrixInnerSumEval) on a matrix first rescaled to NL limbs, beside the top-level
call on the matrix as it is.

usage: inner_product_only.py ROWS COLS LOGN [--limbs NL[,NL...]] [--rounds R] [--rows R]...

COLS top-level ciphertexts of uniform residues stand for the matrix Prove multiplies (the kernels are data-independent),
random words for the Galois keys of an InnerSum of ROWS and for the plaintext, as in bench.py.  Per level:
lumen_rescale of the matrix to NL limbs, then lumen_matrix_inner_sum_at_level on the rescaled set with the first NL
limbs of the plaintext; beside them lumen_matrix_inner_sum at the top level.  Wall clock around each call with the
device drained before and after, R rounds after one untimed visit (pools, scratch placement, clocks), then one visit
under lumen_prof_read for the per-kernel table.

--rows R (repeatable; any R the library accepts: R <= N / 2, or a power of two <= N) adds, in the same process and at the
top level, lumen_matrix_inner_sum_general with R rows: for an R that is no power of two the lazy double-and-add --
floor(log2 R) doublings, popcount(R) - 1 lazy terms (a gadget product and ks_lazy_gather each), one step 4a and one
ModDown for the close, one decomposition per iteration -- to be read against a power of two beside it in the same run.

Prove does not use the lower-level path: the reference evaluates at the top level and proof bytes stay as they are.
With the prover's 57-bit plaintext modulus the result decrypts from three limbs up and not from two
(tests/test_inner_product_levels_model.py).  The transform-bound part of a rotation goes with beta_nl (nl + K) against
beta (L + K); the rescale of the matrix and the gadget product's traffic do not scale the same way.  One box, one run:
repeat before quoting a figure (DESIGN.md section 6 has one run's output).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lumenos_amd import params as lp
from lumenos_amd.hip import Context


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rows", type=int)
    ap.add_argument("cols", type=int)
    ap.add_argument("logn", type=int)
    ap.add_argument("--limbs", default="3,4", help="levels to time, in limbs (default 3,4)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", dest="more_rows", type=int, action="append", default=[],
                    help="also time lumen_matrix_inner_sum_general with this many rows at the top level (repeatable)")
    a = ap.parse_args()
    P = lp.generate_bgv_params_for_ntt(a.cols, a.logn)
    L, K, N = len(P.q), len(P.p), P.N
    levels = [int(x) for x in a.limbs.split(",") if x]
    assert all(1 <= nl <= L for nl in levels), (levels, L)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    rng = np.random.default_rng(1)

    def rand_limbs(mods, tail):
        out = np.empty((len(mods),) + tail, dtype=np.uint64)
        for i, m in enumerate(mods):
            out[i] = rng.integers(0, m, size=tail, dtype=np.uint64)
        return out

    beta = (L + K - 1) // K
    els = list(ctx.inner_sum_galois_elements(a.rows))
    for r in a.more_rows:
        used = ctx.inner_sum_general_elements(1, r)
        assert used or r == 1, f"--rows {r}: not a length lumen_matrix_inner_sum_general accepts at N = {N}"
        els += [g for g in used if g not in els]
    for g in els:
        ctx.load_galois_key(g, np.ascontiguousarray(rand_limbs(P.q + P.p, (beta, 2, N)).transpose(1, 2, 0, 3)))
    pt = rand_limbs(P.q, (N,))
    matrix = ctx.new_set(a.cols, L).fill_random(1)
    ctx.sync()
    print(f"# {a.rows}x{a.cols}, LogN = {a.logn}: L = {L}, K = {K}, {a.cols} ciphertexts, InnerSum of {a.rows} "
          f"({len(ctx.inner_sum_galois_elements(a.rows))} rotations)", flush=True)
    for nl in [L] + levels:
        b = -(-nl // K)
        print(f"#   {nl:2d} limbs: {b} digits over {nl + K} limbs = {b * (nl + K)} digit-limbs per rotation", flush=True)

    def timed(ms, name, fn):
        ctx.sync()
        t0 = time.perf_counter()
        out = fn()
        ctx.sync()
        if ms is not None:
            ms.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return out

    def visit(nl, ms=None):
        if nl == L:
            timed(ms, "inner_sum", lambda: ctx.matrix_inner_sum(matrix, pt, a.rows)).free()
            return
        low = timed(ms, "rescale", lambda: ctx.rescale(matrix, nl))
        timed(ms, "inner_sum", lambda: ctx.matrix_inner_sum_at_level(low, pt[:nl], a.rows)).free()
        low.free()

    def visit_rows(r, ms=None):
        timed(ms, "inner_sum", lambda: ctx.matrix_inner_sum_general(matrix, pt, r)).free()

    # the top level first: the scratch placement times top-level rotations
    for nl, r in [(L, None)] + [(nl, None) for nl in levels] + [(L, r) for r in a.more_rows]:
        go = (lambda ms=None: visit(nl, ms)) if r is None else (lambda ms=None: visit_rows(r, ms))
        go()
        ms = {}
        for _ in range(a.rounds):
            go(ms)
        best = {k: min(v) for k, v in ms.items()}
        what = f"rows {r}" if r is not None else "top level" if nl == L else f"{nl} limbs"
        if r is not None:
            print(f"# rows {r}: {len(ctx.inner_sum_general_elements(1, r))} keys, {r.bit_length() - 1} doublings, "
                  f"{bin(r).count('1') - 1} lazy terms", flush=True)
        print(f"{what:>10}: " + "  ".join(f"{k} {best[k]:.1f} ms" for k in ms) + f"  total {sum(best.values()):.1f} ms"
              f"  (best of {a.rounds}; all: " + " ".join(f"{k}=" + "/".join(f"{x:.1f}" for x in v) for k, v in ms.items()) + ")",
              flush=True)
        ctx.prof_reset()
        ctx.prof_enable(True)
        go()
        ctx.prof_enable(False)
        tab = {k: ctx.prof_read(k)[0] for k in ctx.prof_names()}
        print(f"# {what} kernels (ms): " + " ".join(f"{k}={v:.1f}" for k, v in sorted(tab.items()) if v > 0), flush=True)
    matrix.free()
    ctx.close()


if __name__ == "__main__":
    main()
