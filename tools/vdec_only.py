"""Times the front end of the proof of decryption (lumen_batch_ciphertexts, lumen_rescale to level 0,
lumen_vdec_witness) at a bench shape.

usage: vdec_only.py [config] [count] [rounds]

`count` level-1 ciphertexts (uniform residues: the kernels are data-independent) stand for the opened columns of a
proof (309 at the headline shape), `count` x N raw 64-bit words for the transcript's challenges.  Wall clock around
each call with the device drained before and after, `rounds` rounds; then one visit under lumen_prof_read for the
per-kernel table, and the batch under LUMEN_BATCH_CHUNKS = 1, 2, 4, ... against the derived default.  The plaintext
modulus is 0x3ee0001, the one the batch fits (tools/noise_budget.py --vdec); the times do not depend on it.
The windows are about a millisecond: repeat the run, and on more than one box, before quoting a figure (DESIGN.md
section 6 has one run's output).
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lumenos_amd import params as lp
from lumenos_amd.hip import Context

CONFIGS = {"2048x1024": (1024, 12), "4096x2048": (2048, 12), "8192x4096": (4096, 13), "16384x4096": (4096, 14)}
T_VDEC = 0x3EE0001


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "16384x4096"
    cols, log_n = CONFIGS[cfg]
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 309
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    P = lp.generate_bgv_params_for_ntt(cols, log_n)
    ctx = Context(P.log_n, P.q, P.p, P.psi, T_VDEC)
    ctx.keygen_secret(bytes(range(32)), want_sk=False)
    ctx.encoder_set(lp.encoder_psi(T_VDEC, P.log_n))
    rng = np.random.default_rng(1)
    cts = np.empty((count, 2, 2, P.N), dtype=np.uint64)
    for l in range(2):
        cts[:, :, l, :] = rng.integers(0, P.q[l], size=(count, 2, P.N), dtype=np.uint64)
    s = ctx.upload(cts)
    alphas = rng.integers(0, 2**64, size=(count, P.N), dtype=np.uint64)
    m = rng.integers(0, T_VDEC, size=P.N, dtype=np.uint64)
    print(f"# {cfg}: {count} level-1 ciphertexts, N = {P.N}: {2 * count} forward limb transforms with the product fused in",
          flush=True)

    def visit(ms=None):
        def timed(name, fn):
            ctx.sync()
            t0 = time.perf_counter()
            out = fn()
            ctx.sync()
            if ms is not None:
                ms.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
            return out
        b = timed("batch", lambda: ctx.batch_ciphertexts(s, alphas, 1))
        b0 = timed("rescale", lambda: ctx.rescale(b, 1))
        timed("witness", lambda: ctx.vdec_witness(b0, m, 1))
        b.free(), b0.free()

    visit()  # warm-up: pools, scratch, clocks
    ms = {}
    for rnd in range(rounds):
        visit(ms)
        print(f"round {rnd}: " + "  ".join(f"{k} {v[-1]:.2f} ms" for k, v in ms.items()), flush=True)
    ctx.prof_reset()
    ctx.prof_enable(True)
    visit()
    ctx.prof_enable(False)
    tab = {k: ctx.prof_read(k)[0] for k in ctx.prof_names()}
    print("# kernels: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(tab.items()) if v > 0), flush=True)
    chunks = 1
    while chunks <= count:
        ctx.set_tuning("LUMEN_BATCH_CHUNKS", chunks)
        x = []
        for _ in range(rounds + 1):
            ctx.sync()
            t0 = time.perf_counter()
            ctx.batch_ciphertexts(s, alphas, 1).free()
            ctx.sync()
            x.append((time.perf_counter() - t0) * 1e3)
        print(f"# LUMEN_BATCH_CHUNKS={chunks}: batch {min(x[1:]):.2f} ms", flush=True)
        chunks *= 2
    ctx.close()


if __name__ == "__main__":
    main()
