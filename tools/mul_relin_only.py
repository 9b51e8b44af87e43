"""Times the ciphertext x ciphertext product with relinearisation (lumen_mul_relin) beside the two things it is made
of, on the same sets in the same process: one rotation (lumen_inner_sum with n = 2) and lumen_mul_plain.

usage: mul_relin_only.py ROWS COLS LOGN [--limbs NL[,NL...]] [--count C] [--rounds R] [--dot N_TERMS]

The parameters are the prover's for a ROWS x COLS witness at LogN (ROWS only names the shape).  C (default COLS)
ciphertexts of uniform residues stand for both operands (the kernels are data-independent), random words for the
relinearisation key, the one Galois key and the plaintext.  Per level NL (default: the top level and 3 limbs): the sets
are the first operand rescaled to NL limbs and a second set filled at that level.  Event time (lumen_timer_*) around each
call, R rounds after one untimed visit, then one visit under lumen_prof_read: the key switch's ks_* scopes, mul_tensor,
relin_close, mul_plain.  The tensor kernel's share of the HBM peak is printed from its profile entry: it reads 4 and
writes 4 words per coefficient of a limb (d0, d1 - d2, the accumulator's 0 and d2).

The product's traffic is one rotation plus three mul_plain passes; what it costs beyond that is the closing pass.  One
box, one run: repeat before quoting a figure.

--dot N_TERMS times the dot product with one relinearisation per sum instead: C ciphertexts per operand (a multiple of
N_TERMS) are C / N_TERMS sums.  On the same two sets, in the same process, per level: (a) lumen_mul_relin_dot; (b) what a
caller does without it, lumen_mul_relin on all C pairs and the sums through lumen_linear_combination (at most eight
operands a pass: the running sum and seven more from the second pass on), which reads the product set term-major -- term
i of every sum a contiguous slice --, the layout a caller of (b) would choose; the kernels are data-independent.  Then one
visit of (a) under lumen_prof_read, per block width of the summed tensor kernel (LUMEN_DOT_PAIRS = 0: by the size of the
launch, 256, 512) and per number of blocks a sum's terms are split over (LUMEN_DOT_PARTS = 0: by the size of the launch,
1, 2, ... 32; the scope then holds the kernel and the pass that adds the parts): it reads 4 words per term and writes 4
per sum and coefficient of a limb, the traffic of the unsplit form, which is what the GB/s of every row is quoted for.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lumenos_amd import params as lp
from lumenos_amd.hip import Context

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rows", type=int)
    ap.add_argument("cols", type=int)
    ap.add_argument("logn", type=int)
    ap.add_argument("--limbs", default="", help="levels to time, in limbs (default: the top level and 3)")
    ap.add_argument("--count", type=int, default=0, help="ciphertexts per operand (default COLS)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dot", type=int, default=0, metavar="N_TERMS", help="time mul_relin_dot on sums of N_TERMS products")
    a = ap.parse_args()
    P = lp.generate_bgv_params_for_ntt(a.cols, a.logn)
    L, K, N = len(P.q), len(P.p), P.N
    count = a.count or a.cols
    levels = [int(x) for x in a.limbs.split(",") if x] or sorted({L, min(3, L)}, reverse=True)
    assert all(1 <= nl <= L for nl in levels), (levels, L)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    rng = np.random.default_rng(1)

    def rand_limbs(mods, tail):
        out = np.empty((len(mods),) + tail, dtype=np.uint64)
        for i, m in enumerate(mods):
            out[i] = rng.integers(0, m, size=tail, dtype=np.uint64)
        return out

    beta = (L + K - 1) // K
    key = lambda: np.ascontiguousarray(rand_limbs(P.q + P.p, (beta, 2, N)).transpose(1, 2, 0, 3))
    (g,) = ctx.inner_sum_galois_elements(2)
    ctx.load_galois_key(g, key())  # first: the scratch placement times rotations under a Galois key
    ctx.load_relin_key(key())
    pt = rand_limbs(P.q, (N,))
    top = ctx.new_set(count, L).fill_random(1)
    ctx.sync()
    print(f"# {a.rows}x{a.cols}, LogN = {a.logn}: L = {L}, K = {K}, {count} ciphertexts per operand", flush=True)

    def timed(ms, name, fn):
        ctx.sync()
        ctx.timer_start()
        out = fn()
        t = ctx.timer_stop()
        if ms is not None:
            ms.setdefault(name, []).append(t)
        return out

    def visit(sa, sb, nl, ms=None):
        timed(ms, "mul_relin", lambda: ctx.mul_relin(sa, sb)).free()
        rot = ctx.inner_sum if nl == L else ctx.inner_sum_at_level
        timed(ms, "rotation", lambda: rot(sa, 2)).free()
        timed(ms, "mul_plain", lambda: ctx.mul_plain(sa, pt[:nl])).free()

    ctx.inner_sum(top, 2).free()  # the top level first: the placement is chosen on top-level rotations
    if a.dot:
        dot_mode(ctx, a, top, levels, L, N, timed)
        top.free()
        ctx.close()
        return
    for nl in levels:
        sa = top if nl == L else ctx.rescale(top, nl)
        sb = ctx.new_set(count, nl).fill_random(2)
        visit(sa, sb, nl)
        ms = {}
        for _ in range(a.rounds):
            visit(sa, sb, nl, ms)
        best = {k: min(v) for k, v in ms.items()}
        what = "top level" if nl == L else f"{nl} limbs"
        budget = best["rotation"] + 3 * best["mul_plain"]
        print(f"{what:>10}: " + "  ".join(f"{k} {best[k]:.2f} ms" for k in ms) +
              f"  rotation + 3 mul_plain {budget:.2f} ms  product / that {best['mul_relin'] / budget:.3f}"
              f"  (best of {a.rounds}; all: " + " ".join(f"{k}=" + "/".join(f"{x:.2f}" for x in v) for k, v in ms.items()) + ")",
              flush=True)
        ctx.prof_reset()
        ctx.prof_enable(True)
        ctx.mul_relin(sa, sb).free()
        ctx.sync()
        ctx.prof_enable(False)
        tab = {k: ctx.prof_read(k)[0] for k in ctx.prof_names()}
        print(f"# {what} mul_relin scopes (ms): " + " ".join(f"{k}={v:.2f}" for k, v in sorted(tab.items()) if v > 0), flush=True)
        t_ms = tab.get("mul_tensor", 0.0)
        if t_ms > 0:
            gb = count * nl * N * 8 * 8 / 1e9
            print(f"# {what} mul_tensor: {gb:.2f} GB in {t_ms:.2f} ms = {gb / t_ms * 1e3:.0f} GB/s, "
                  f"{gb / t_ms * 1e3 / HBM_PEAK_GBS * 100:.0f} % of the {HBM_PEAK_GBS / 1e3:.0f} TB/s HBM peak "
                  f"(event time; with two lanes it includes the neighbour's kernels)", flush=True)
        sb.free()
        if sa is not top:
            sa.free()
    top.free()
    ctx.close()


def dot_mode(ctx, a, top, levels, L, N, timed):
    n, count = a.dot, top.count
    assert n >= 1 and count % n == 0, (count, n)
    groups = count // n

    def today(sa, sb):
        """(b): every product relinearised, then summed: term i of every sum is slice i of the product set"""
        prod = ctx.mul_relin(sa, sb)
        terms = [prod.slice(i * groups, groups) for i in range(n)]
        acc = ctx.linear_combination(terms[:8], [1] * len(terms[:8]))
        for at in range(8, n, 7):
            more = terms[at:at + 7]
            ctx.linear_combination([acc] + more, [1] * (1 + len(more)), out=acc)
        for t in terms:
            t.free()
        prod.free()
        return acc

    def visit(sa, sb, ms=None):
        timed(ms, "mul_relin_dot", lambda: ctx.mul_relin_dot(sa, sb, n)).free()
        timed(ms, "mul_relin+sum", lambda: today(sa, sb)).free()

    print(f"# dot: {groups} sums of {n} products", flush=True)
    for nl in levels:
        sa = top if nl == L else ctx.rescale(top, nl)
        sb = ctx.new_set(count, nl).fill_random(2)
        visit(sa, sb)
        ms = {}
        for _ in range(a.rounds):
            visit(sa, sb, ms)
        best = {k: min(v) for k, v in ms.items()}
        what = "top level" if nl == L else f"{nl} limbs"
        print(f"{what:>10}: " + "  ".join(f"{k} {best[k]:.2f} ms" for k in ms) +
              f"  (a) / (b) {best['mul_relin_dot'] / best['mul_relin+sum']:.3f}"
              f"  (best of {a.rounds}; all: " + " ".join(f"{k}=" + "/".join(f"{x:.2f}" for x in v) for k, v in ms.items()) + ")",
              flush=True)
        gb = (count * 4 + groups * 4) * nl * N * 8 / 1e9
        for pairs, parts in ((0, 0), (256, 1), (512, 1), (0, 2), (0, 4), (0, 8), (0, 16), (0, 32)):
            if parts > max(n // 2, 1):
                continue
            ctx.set_tuning("LUMEN_DOT_PAIRS", pairs)
            ctx.set_tuning("LUMEN_DOT_PARTS", parts)
            ctx.mul_relin_dot(sa, sb, n).free()
            ts = []
            for _ in range(a.rounds):
                ctx.prof_reset()
                ctx.prof_enable(True)
                ctx.mul_relin_dot(sa, sb, n).free()
                ctx.sync()
                ctx.prof_enable(False)
                ts.append(ctx.prof_read("mul_tensor_dot")[0])
            tab = {k: ctx.prof_read(k)[0] for k in ctx.prof_names()}
            t_ms = min(ts)
            print(f"# {what} LUMEN_DOT_PAIRS={pairs} LUMEN_DOT_PARTS={parts} mul_tensor_dot: {gb:.2f} GB in {t_ms:.3f} ms = {gb / t_ms * 1e3:.0f} GB/s, "
                  f"{gb / t_ms * 1e3 / HBM_PEAK_GBS * 100:.0f} % of the {HBM_PEAK_GBS / 1e3:.0f} TB/s HBM peak (event time, best of "
                  f"{a.rounds}: " + "/".join(f"{x:.3f}" for x in ts) + "; with two lanes it includes the neighbour's kernels)  scopes (ms): " +
                  " ".join(f"{k}={v:.2f}" for k, v in sorted(tab.items()) if v > 0), flush=True)
        ctx.set_tuning("LUMEN_DOT_PAIRS", 0)
        ctx.set_tuning("LUMEN_DOT_PARTS", 0)
        sb.free()
        if sa is not top:
            sa.free()


if __name__ == "__main__":
    main()
