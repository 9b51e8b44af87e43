"""From how many rotations on does the c0 fold (LUMEN_KS_C0_FOLD) pay?  Times lumen_matrix_inner_sum at the headline
chain (the prover's parameters for 16384 x 4096, LogN 14, L = 12, K = 2) on COUNT columns for several row counts, the
switch alternated call by call inside one process.

usage: c0_fold_rows.py [--rows 4,8,16] [--count 64] [--rounds 5]

rows = 2^k is k rotations: k - 1 doublings and the close.  The library folds a plan of at least
LM_KS_FOLD_MIN_ROTATIONS rotations (3); to time the fold on a plan of two, point LUMEN_HIP_LIB at a build made with
tools/build_variant.sh NAME -DLM_KS_FOLD_MIN_ROTATIONS=2.  Uniform residues and random words for the Galois keys (the
kernels are data-independent).  Event time around each call, one untimed visit of each setting first; per setting the
best and the mean of the rounds.  One box, one run: repeat before quoting a figure."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lumenos_amd import params as lp
from lumenos_amd.hip import Context

SWITCH = "LUMEN_KS_C0_FOLD"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", default="4,8,16")
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    rows = [int(x) for x in a.rows.split(",")]
    P = lp.generate_bgv_params_for_ntt(4096, 14)
    L, K, N = len(P.q), len(P.p), P.N
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    rng = np.random.default_rng(1)
    beta = (L + K - 1) // K
    for g in ctx.inner_sum_galois_elements(max(rows)):
        key = np.empty((L + K, beta, 2, N), dtype=np.uint64)
        for i, m in enumerate(P.q + P.p):
            key[i] = rng.integers(0, m, size=(beta, 2, N), dtype=np.uint64)
        ctx.load_galois_key(g, np.ascontiguousarray(key.transpose(1, 2, 0, 3)))
    cts = ctx.new_set(a.count, L).fill_random(1)
    pt = np.stack([rng.integers(0, m, size=N, dtype=np.uint64) for m in P.q])
    print(f"# headline chain, LogN = 14, L = {L}, K = {K}, {a.count} columns, {a.rounds} rounds, library "
          f"{os.environ.get('LUMEN_HIP_LIB', 'product')}", flush=True)

    def timed(r):
        ctx.sync()
        ctx.timer_start()
        out = ctx.matrix_inner_sum(cts, pt, r)
        t = ctx.timer_stop()
        out.free()
        return t

    for r in rows:
        got = {0: [], 1: []}
        for rnd in range(a.rounds + 1):
            for on in (0, 1):
                ctx.set_tuning(SWITCH, on)
                t = timed(r)
                if rnd:
                    got[on].append(t)
        ctx.prof_enable(True)
        folded = {}
        for on in (0, 1):
            ctx.set_tuning(SWITCH, on)
            ctx.prof_reset()
            ctx.matrix_inner_sum(cts, pt, r).free()
            ctx.sync()
            folded[on] = ctx.prof_read("ks_lift_fold")[1]
        ctx.prof_enable(False)
        m0, m1 = np.mean(got[0]), np.mean(got[1])
        print(f"rows {r:5d} ({r.bit_length() - 1} rotations): off best {min(got[0]):.3f} mean {m0:.3f} ms | on best {min(got[1]):.3f} mean "
              f"{m1:.3f} ms | on / off {(m1 / m0 - 1) * 100:+.2f} % (best {(min(got[1]) / min(got[0]) - 1) * 100:+.2f} %) | lift folds with the "
              f"switch on: {folded[1]} | off rounds " + "/".join(f"{x:.3f}" for x in got[0]) + " | on rounds " + "/".join(f"{x:.3f}" for x in got[1]),
              flush=True)
    ctx.set_tuning(SWITCH, 1)
    cts.free()
    ctx.close()


if __name__ == "__main__":
    main()
