"""Times the evaluator's linear operations (lm_linear.hip) beside lumen_mul_plain, the library's own elementwise kernel,
on resident sets in one process, and reports bytes moved per second for each.

usage: linear_only.py COUNT LIMBS LOGN [--rounds R]

COUNT ciphertexts of LIMBS limbs at ring degree 2^LOGN, uniform residues (the kernels are data-independent), on the
prover's moduli for that depth.  Timed, each into an existing destination so that nothing is allocated: add;
mul_scalar (a raw field-table word); linear_combination with n = 4 and, on half the ciphertexts, with n = 8 (eight
distinct operands: distinct halves of the four sets); mul_plain_then_add; lumen_mul_plain.  Bytes moved = inputs read
plus output written, a plaintext operand once per call.  Event time (lumen_timer_*) around each call: R visits (default
5) after one untimed visit; the best, the slowest and the rate at the best are printed.

The yardstick is mul_plain's rate and the spread of its own visits.  One box, one run: repeat before quoting a figure.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lumenos_amd import params as lp
from lumenos_amd.hip import Context


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("count", type=int)
    ap.add_argument("limbs", type=int)
    ap.add_argument("logn", type=int)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert a.count >= 2 and a.count % 2 == 0 and a.limbs >= 2, "an even count (n = 8 runs on halves) and at least two limbs"
    P = lp.generate_bgv_params_for_ntt(1 << a.limbs, a.logn)
    L, N = len(P.q), P.N
    assert L == a.limbs, (L, a.limbs)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    rng = np.random.default_rng(1)
    pt = np.stack([rng.integers(0, m, size=N, dtype=np.uint64) for m in P.q])
    w = int(lp.field_roots_forward(P.T, 16)[5])  # a raw table word, as fhe/ntt.go passes them
    sets = [ctx.new_set(a.count, L).fill_random(1 + i) for i in range(4)]
    out = ctx.new_set(a.count, L)
    half = a.count // 2
    halves = [s.slice(h * half, half) for s in sets for h in range(2)]
    out_half = out.slice(0, half)
    ctx.sync()
    set_bytes = sets[0].nbytes
    print(f"# {a.count} ciphertexts x {L} limbs x 2^{a.logn}: {set_bytes / 1e9:.2f} GB per set", flush=True)
    ws4, ws8 = [w, 1, P.T - 1, w + 1], [w, 1, P.T - 1, w + 1, w + 2, 1, w + 3, P.T - 1]
    cases = [
        ("add", 3 * set_bytes, lambda: ctx.add(sets[0], sets[1], out=out)),
        ("mul_scalar", 2 * set_bytes, lambda: ctx.mul_scalar(sets[0], w, out=out)),
        ("linear_combination n=4", 5 * set_bytes, lambda: ctx.linear_combination(sets, ws4, out=out)),
        ("linear_combination n=8 (halves)", 9 * set_bytes // 2, lambda: ctx.linear_combination(halves, ws8, out=out_half)),
        ("mul_plain_then_add", 3 * set_bytes + pt.nbytes, lambda: ctx.mul_plain_then_add(sets[0], pt, out)),
        ("mul_plain", 2 * set_bytes + pt.nbytes, lambda: ctx.mul_plain(sets[0], pt).free()),
    ]

    def timed(fn):
        ctx.sync()
        ctx.timer_start()
        fn()
        return ctx.timer_stop()

    print(f"{'call':<34}{'best s':>11}{'min..max ms':>22}{'GB moved':>10}{'GB/s at best':>14}")
    for name, nbytes, fn in cases:
        fn()  # the untimed visit: scratch, the pooled output block
        ms = [timed(fn) for _ in range(a.rounds)]
        print(f"{name:<34}{min(ms) / 1e3:>11.6f}{min(ms):>11.3f} ..{max(ms):>8.3f}{nbytes / 1e9:>10.2f}{nbytes / min(ms) / 1e6:>14.0f}",
              flush=True)
    for s in halves + [out_half]:
        s.free()
    for s in sets + [out]:
        s.free()
    ctx.close()


if __name__ == "__main__":
    main()
