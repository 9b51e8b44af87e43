"""Times the diagonal linear transform alone (lumen_linear_transform) against the composition the library offered before
it -- lumen_rotate_hoisted over the same elements, then lumen_mul_plain / lumen_mul_plain_then_add per diagonal -- at a
chosen shape, in one process, the two routes alternating.

usage: lintrans_only.py ROWS COLS LOGN [--limbs NL] [--count C] [--rounds R] [--diagonals D[,D...]] [--bsgs N1]

The parameters are the prover's for a ROWS x COLS witness at LogN (ROWS only names the shape).  C (default 64)
ciphertexts of uniform residues (the kernels are data-independent), random words for the Galois keys and for the
diagonals 0 .. D - 1, which are plaintexts over Q and P.  NL limbs (default: the top level): the set is the top-level one
rescaled to NL limbs.  Event time (lumen_timer_*) around each route, R rounds after one untimed visit of both: median and
spread (max - min over the median) per route.

Per kernel: one more visit of each route under lumen_prof_read, on ONE lane (with two, a kernel's event time includes its
neighbour's).  ks_diag_gather moves data and does one Montgomery product per word: its achieved bytes per second -- the
words it must read and write, from the shapes, over its event time -- are printed against the copy rate of the box,
measured here as a device-to-device copy of the input set (lumen_automorphism by the identity; read + write).
--bsgs N1: the double-hoisted (baby-step / giant-step) form of the same diagonals with N1 baby steps (0: the count
lumen_lintrans_best_baby_steps picks) as a third route, alternating with the other two, its keys counted against the
single-hoisted transform's and its scopes printed as theirs.
One box, one run: repeat before quoting a figure.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from lumenos_amd import params as lp
from lumenos_amd.hip import Context, lintrans_best_baby_steps


def gather_bytes(count, batch, nl, K, N, keyed):
    """what ks_diag_gather must move for `keyed` non-zero diagonals on `count` columns in batches of `batch`"""
    total = 0
    for first in range(0, count, batch):
        B = min(batch, count - first)
        u = 2 * B * (nl + K) * N * 8  # the gadget product, read; the lazy block, written (and read, but for the first term)
        per = u + B * nl * N * 8 + (nl + K) * N * 8 + N * 4 + u  # + c0, the multiplier, the index table
        total += keyed * per + (keyed - 1) * u
    return total


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rows", type=int)
    ap.add_argument("cols", type=int)
    ap.add_argument("logn", type=int)
    ap.add_argument("--limbs", type=int, default=0, help="level to time, in limbs (default: the top level)")
    ap.add_argument("--count", type=int, default=64, help="ciphertexts")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--diagonals", default="4,16", help="numbers of diagonals (0 .. D - 1)")
    ap.add_argument("--bsgs", type=int, default=None, metavar="N1", help="also time the double-hoisted form with N1 baby steps (0: the best)")
    a = ap.parse_args()
    P = lp.generate_bgv_params_for_ntt(a.cols, a.logn)
    L, K, N = len(P.q), len(P.p), P.N
    count, nl = a.count, a.limbs or L
    ds = [int(x) for x in a.diagonals.split(",") if x]
    assert 1 <= nl <= L and all(2 <= d <= 65 for d in ds), (nl, L, ds)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    rng = np.random.default_rng(1)

    def rand_limbs(mods, tail):
        out = np.empty((len(mods),) + tail, dtype=np.uint64)
        for i, m in enumerate(mods):
            out[i] = rng.integers(0, m, size=tail, dtype=np.uint64)
        return out

    beta = (L + K - 1) // K
    els = [ctx.galois_element(r) for r in range(1, max(ds))]
    for g in els:
        ctx.load_galois_key(g, np.ascontiguousarray(rand_limbs(P.q + P.p, (beta, 2, N)).transpose(1, 2, 0, 3)))
    diags = {k: rand_limbs(P.q[:nl] + P.p, (N,)) for k in range(max(ds))}
    top = ctx.new_set(count, L).fill_random(1)
    ctx.inner_sum(top, 2).free()  # the top level first: the scratch placement is chosen on top-level rotations
    s = top if nl == L else ctx.rescale(top, nl)
    ctx.sync()
    print(f"# {a.rows}x{a.cols}, LogN = {a.logn}: L = {L}, K = {K}, {count} ciphertexts at {nl} limbs", flush=True)

    def timed(fn):
        ctx.sync()
        ctx.timer_start()
        out = fn()
        t = ctx.timer_stop()
        for o in out if isinstance(out, list) else [out]:
            o.free()
        return t

    def show(v):
        m = statistics.median(v)
        return m, f"median {m:.2f} ms, spread {(max(v) - min(v)) / m * 100:.1f} % (" + "/".join(f"{x:.2f}" for x in v) + ")"

    def scopes(fn):
        ctx.prof_reset()
        ctx.prof_enable(True)
        for o in fn():
            o.free()
        ctx.sync()
        ctx.prof_enable(False)
        return {k: ctx.prof_read(k) for k in ctx.prof_names()}

    copy_ms, copy_txt = show([timed(lambda: ctx.automorphism(s, 1)) for _ in range(a.rounds + 1)][1:])
    copy_rate = 2 * s.nbytes / (copy_ms * 1e-3)
    print(f"device-to-device copy of the set ({s.nbytes / 2**20:.0f} MiB): {copy_txt}: {copy_rate / 1e12:.2f} TB/s read + write", flush=True)

    for d in ds:
        lt = ctx.lintrans_load({k: diags[k] for k in range(d)}, nl)
        g = ctx.lintrans_galois_elements(lt)
        assert g == els[:d - 1]

        def composed():
            rots = ctx.rotate_hoisted(s, g)
            acc = ctx.mul_plain(s, diags[0][:nl])
            for k, r in enumerate(rots, 1):
                ctx.mul_plain_then_add(r, diags[k][:nl], acc)
                r.free()
            return [acc]

        def fused():
            return [ctx.linear_transform(s, lt)]

        routes = [("lumen_linear_transform", fused), ("composition", composed)]
        lb = None
        if a.bsgs is not None:
            n1 = a.bsgs or lintrans_best_baby_steps(a.logn, range(d))
            lb = ctx.lintrans_load({k: diags[k] for k in range(d)}, nl, baby_steps=n1)
            gb = ctx.lintrans_galois_elements(lb)
            assert set(gb) <= set(els)
            print(f"D = {d}: double-hoisted with n1 = {n1}: {len(gb)} keys against {len(g)}", flush=True)
            routes.append(("double-hoisted", lambda: [ctx.linear_transform(s, lb)]))
        for _, fn in routes:
            timed(fn)
        times = [[] for _ in routes]
        for _ in range(a.rounds):  # alternating: what else runs on the box meets the routes alike
            for t, (_, fn) in zip(times, routes):
                t.append(timed(fn))
        mf, txt_f = show(times[0])
        mc, txt_c = show(times[1])
        print(f"D = {d}: lumen_linear_transform {txt_f}", flush=True)
        print(f"D = {d}: rotate_hoisted + mul_plain_then_add {txt_c}", flush=True)
        print(f"D = {d}: linear_transform / composition = {mf / mc:.3f}", flush=True)
        if lb is not None:
            mb, txt_b = show(times[2])
            print(f"D = {d}: double-hoisted {txt_b}", flush=True)
            print(f"D = {d}: double-hoisted / single-hoisted = {mb / mf:.3f}", flush=True)
        ctx.set_tuning("LUMEN_KS_LANES", 1)
        for name, fn in routes:
            sc = scopes(fn)
            print(f"# D = {d}, {name}, scopes (ms / launches, one lane): " +
                  " ".join(f"{k}={v[0]:.2f}/{v[1]}" for k, v in sorted(sc.items()) if v[0] > 0), flush=True)
            if "ks_diag_gather" in sc and sc["ks_diag_gather"][0] > 0:
                ms = sc["ks_diag_gather"][0]
                rate = gather_bytes(count, min(count, 64), nl, K, N, d - 1) / (ms * 1e-3)
                print(f"D = {d}: ks_diag_gather {ms / sc['ks_diag_gather'][1]:.3f} ms per launch, {rate / 1e12:.2f} TB/s = "
                      f"{rate / copy_rate:.2f} of the copy rate", flush=True)
        ctx.set_tuning("LUMEN_KS_LANES", 0)
        lt.close()
        if lb is not None:
            lb.close()
    if s is not top:
        s.free()
    top.free()
    ctx.close()


if __name__ == "__main__":
    main()
