"""The diagonal linear transform, double-hoisted (baby-step / giant-step) -- [LATTIGO-RECALL] Evaluator.MultiplyByDiagMatrixBSGS,
the BSGS branch of LinearTransformation -- restated on the pieces of tests/inner_sum_model.py and tests/lintrans_model.py.
The judge of lumen_lintrans_load_bsgs and of lumen_linear_transform on such an object; nothing here reads the device's output.

Diagonals normalised as in lintrans_model.normalise: e = k mod N/2.  With n1 >= 1 baby steps e = j + i, i = e mod n1 the baby,
j = e - i the giant, g_x the Galois element of a rotation by x:

    m_e    = pt_e * T per limb
    m'_e   = sigma_{g_j}^-1(m_e)                       pre-rotated by -j: the NTT-domain gather under g_{N/2 - j}
    dig    = decompose(c1)                             once
    baby_0 = (P c0, P c1) on Q, 0 on P
    baby_i = sigma_{g_i}(gadget(dig, key g_i) + (P c0 on Q, 0))            over Q and P, no ModDown
    for every giant j that occurs:
        tmp_j = sum_i m'_{j+i} (.) baby_i                                  over Q and P, both polynomials
        j == 0:  acc += tmp_0
        j != 0:  d1 = mod_down(tmp_j)[1];  (v0, v1) = gadget(decompose(d1), key g_j)
                 acc += sigma_{g_j}(v0 + tmp_j[0], v1)                     tmp_j[0] stays in QP
    out = mod_down(acc)                                ONE, for both polynomials

Every accumulate is exact and canonical, so the order of the loops changes no word.  With every diagonal a baby (all
e < n1) the words are lintrans_model.linear_transform's: ModDown(x + P y) = ModDown(x) + y exactly."""
import numpy as np

import inner_sum_model as model
import lintrans_model as lm
from inner_sum_model import _mod_index, _obj


def split(P, diags, n1):
    """[(giant j, baby i, pt)] in the order given"""
    if n1 < 1:
        raise ValueError("a transform has at least one baby step")
    return [(e - e % n1, e % n1, pt) for e, _, pt in lm.normalise(P, diags)]


def babies(P, diags, n1):
    return sorted({i for _, i, _ in split(P, diags, n1) if i})


def giants(P, diags, n1):
    return sorted({j for j, _, _ in split(P, diags, n1) if j})


def elements(P, diags, n1):
    """the Galois elements of the keys: the babies' (i != 0, ascending), then the giants' (j != 0, ascending)"""
    return [P.galois_element(x) for x in babies(P, diags, n1) + giants(P, diags, n1)]


def best_baby_steps(log_n, ks):
    """the power of two n1 in [1, N/2] with the fewest keys, (babies != 0) + (giants != 0); ties go to the smaller"""
    half = (1 << log_n) // 2
    es = [k % half for k in ks]
    best, n1 = None, 1
    while n1 <= half:
        cost = len({e % n1 for e in es if e % n1}) + len({e - e % n1 for e in es if e - e % n1})
        if best is None or cost < best[0]:
            best = (cost, n1)
        n1 *= 2
    return best[1]


def _mods(P, nl):
    return [P.moduli[_mod_index(P, t, nl)] for t in range(nl + P.K)]


def _acc(P, nl, a, b):
    if a is None:
        return b
    q = _mods(P, nl)
    return [[(a[w][t] + b[w][t]) % q[t] for t in range(nl + P.K)] for w in range(2)]


def linear_transform(P, ct, diags, n1, key):
    """ct: [2][nl][N]; diags {k: pt_k [nl + K][N]}; key(g) -> the Galois key of element g.  -> [2][nl][N], canonical"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    nl, half = ct.shape[1], P.N // 2
    q = _mods(P, nl)
    pmod = 1
    for p in P.moduli[P.L:P.L + P.K]:
        pmod *= p
    parts = split(P, diags, n1)
    zero = np.zeros(P.N, dtype=object)

    def lifted(u):  # + P c0 on the Q limbs of polynomial 0
        for t in range(nl):
            u[0][t] = (u[0][t] + (pmod % q[t]) * _obj(ct[0, t])) % q[t]
        return u

    baby = {0: [[(pmod % q[t]) * _obj(ct[w, t]) % q[t] if t < nl else zero for t in range(nl + P.K)] for w in range(2)]}
    dig = None
    for i in sorted({i for _, i, _ in parts if i}):
        dig = model.decompose(P, ct[1]) if dig is None else dig
        g = P.galois_element(i)
        u, idx = lifted(model.gadget(P, dig, nl, key(g))), P.automorphism_index(g)
        baby[i] = [[u[w][t][idx] for t in range(nl + P.K)] for w in range(2)]
    acc = None
    for j in sorted({j for j, _, _ in parts}):
        back = P.automorphism_index(P.galois_element(half - j)) if j else np.arange(P.N)
        tmp = None
        for jj, i, pt in parts:
            if jj != j:
                continue
            pt = np.asarray(pt, dtype=np.uint64)
            assert pt.shape == (nl + P.K, P.N), pt.shape
            m = [x[back] for x in lm._multiplier(P, pt, nl)]
            tmp = _acc(P, nl, tmp, [[m[t] * baby[i][w][t] % q[t] for t in range(nl + P.K)] for w in range(2)])
        if j == 0:
            acc = _acc(P, nl, acc, tmp)
            continue
        g = P.galois_element(j)
        d1 = model.mod_down(P, tmp, nl)[1]
        v, idx = model.gadget(P, model.decompose(P, d1), nl, key(g)), P.automorphism_index(g)
        acc = _acc(P, nl, acc, [[((v[w][t] + tmp[0][t]) % q[t] if w == 0 else v[w][t])[idx] for t in range(nl + P.K)] for w in range(2)])
    return model.mod_down(P, acc, nl)
