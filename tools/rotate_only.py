"""Times the rotation alone (lumen_automorphism, lumen_rotate_hoisted) at a chosen shape and level, in one process:
ms per column for one rotation; k hoisted rotations against k single calls; and the new closing kernel against
InnerSum's, per launch, at the same batch and level.

usage: rotate_only.py ROWS COLS LOGN [--limbs NL] [--count C] [--rounds R] [--hoisted K[,K...]]

The parameters are the prover's for a ROWS x COLS witness at LogN (ROWS only names the shape).  C (default COLS)
ciphertexts of uniform residues (the kernels are data-independent), random words for the Galois keys of the rotations by
1 .. max(K).  NL limbs (default: the top level): the set is the top-level one rescaled to NL limbs.  Event time
(lumen_timer_*) around each call, R rounds after one untimed visit, best of R with all of them listed.

Per launch: R visits of one lumen_automorphism and one InnerSum of 2 (one rotation that accumulates) under
lumen_prof_read, on ONE lane (with two, a kernel's event time includes its neighbour's): ks_rotdown_ntt against
ks_moddown_ntt, each with the spread over the visits.  The rotation's kernel reads 2 L N fewer words per column -- no
second read of the accumulator -- so it is expected not to be slower.

Hoisting saves the share of ks_intt_c1 + ks_modup_ntt in one rotation, times (k - 1) / k: printed beside what was
measured.  One box, one run: repeat before quoting a figure.
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
    ap.add_argument("rows", type=int)
    ap.add_argument("cols", type=int)
    ap.add_argument("logn", type=int)
    ap.add_argument("--limbs", type=int, default=0, help="level to time, in limbs (default: the top level)")
    ap.add_argument("--count", type=int, default=0, help="ciphertexts (default COLS)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hoisted", default="2,4,8", help="numbers of rotations to hoist")
    a = ap.parse_args()
    P = lp.generate_bgv_params_for_ntt(a.cols, a.logn)
    L, K, N = len(P.q), len(P.p), P.N
    count = a.count or a.cols
    nl = a.limbs or L
    ks = [int(x) for x in a.hoisted.split(",") if x]
    assert 1 <= nl <= L and all(1 <= k <= 64 for k in ks), (nl, L, ks)
    ctx = Context(P.log_n, P.q, P.p, P.psi, P.T)
    rng = np.random.default_rng(1)

    def rand_limbs(mods, tail):
        out = np.empty((len(mods),) + tail, dtype=np.uint64)
        for i, m in enumerate(mods):
            out[i] = rng.integers(0, m, size=tail, dtype=np.uint64)
        return out

    beta = (L + K - 1) // K
    els = [ctx.galois_element(r) for r in range(1, max(ks + [1]) + 1)]
    for g in els:
        ctx.load_galois_key(g, np.ascontiguousarray(rand_limbs(P.q + P.p, (beta, 2, N)).transpose(1, 2, 0, 3)))
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

    def best(fn):
        timed(fn)
        v = [timed(fn) for _ in range(a.rounds)]
        return min(v), "/".join(f"{x:.2f}" for x in v)

    one, all_one = best(lambda: ctx.automorphism(s, els[0]))
    print(f"one rotation: {one:.2f} ms = {one / count:.4f} ms per column  (best of {a.rounds}: {all_one})", flush=True)

    # ---- the scopes of one rotation and of one accumulating rotation, per launch, one lane
    ctx.set_tuning("LUMEN_KS_LANES", 1)
    per = {"ks_rotdown_ntt": [], "ks_moddown_ntt": []}
    share = []
    for visit in range(a.rounds + 1):
        ctx.prof_reset()
        ctx.prof_enable(True)
        ctx.automorphism(s, els[0]).free()
        ctx.sync()
        ctx.prof_enable(False)
        rot = {k: ctx.prof_read(k) for k in ctx.prof_names()}
        ctx.prof_reset()
        ctx.prof_enable(True)
        ctx.inner_sum_at_level(s, 2).free()
        ctx.sync()
        ctx.prof_enable(False)
        acc = {k: ctx.prof_read(k) for k in ctx.prof_names()}
        if visit == 0:
            continue
        per["ks_rotdown_ntt"].append(rot["ks_rotdown_ntt"][0] / rot["ks_rotdown_ntt"][1])
        per["ks_moddown_ntt"].append(acc["ks_moddown_ntt"][0] / acc["ks_moddown_ntt"][1])
        total = sum(v[0] for k, v in rot.items() if k.startswith("ks_"))
        share.append((rot["ks_intt_c1"][0] + rot["ks_modup_ntt"][0]) / total)
        if visit == a.rounds:
            print("# one rotation's scopes (ms, one lane): " + " ".join(f"{k}={v[0]:.2f}" for k, v in sorted(rot.items()) if v[0] > 0), flush=True)
    ctx.set_tuning("LUMEN_KS_LANES", 0)
    for k, v in per.items():
        print(f"{k}: {min(v):.3f} ms per launch (B = {min(count, 64)}, {nl} limbs; visits: " + "/".join(f"{x:.3f}" for x in v) +
              f"; spread {(max(v) - min(v)) / min(v) * 100:.1f} %)", flush=True)
    r, m = min(per["ks_rotdown_ntt"]), min(per["ks_moddown_ntt"])
    print(f"ks_rotdown_ntt / ks_moddown_ntt per launch: {r / m:.3f}", flush=True)
    sh = sum(share) / len(share)
    print(f"ks_intt_c1 + ks_modup_ntt are {sh * 100:.1f} % of one rotation's kernels", flush=True)

    # ---- k hoisted rotations against k single calls
    for k in ks:
        g = els[:k]
        singles, all_s = best(lambda: [ctx.automorphism(s, x) for x in g])
        hoisted, all_h = best(lambda: ctx.rotate_hoisted(s, g))
        print(f"k = {k}: {k} single calls {singles:.2f} ms, hoisted {hoisted:.2f} ms: saved {(1 - hoisted / singles) * 100:.1f} %, "
              f"expected {sh * (k - 1) / k * 100:.1f} %  (best of {a.rounds}; singles {all_s}; hoisted {all_h})", flush=True)
    if s is not top:
        s.free()
    top.free()
    ctx.close()


if __name__ == "__main__":
    main()
