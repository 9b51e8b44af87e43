"""The diagonal linear transform, single-hoisted -- [LATTIGO-RECALL] Evaluator.MultiplyByDiagMatrix, the non-BSGS branch of
LinearTransformation -- restated on the pieces of tests/inner_sum_model.py.  The judge of lumen_linear_transform; nothing
here reads the device's output.

    dig = decompose(c1)                                   once
    acc = 0 over the nl limbs of Q and the K of P, two polynomials
    for k != 0:   (u0, u1) = gadget(dig, evk[g_k])
                  acc += m_k (.) sigma_{g_k}(u0 + (P c0 on Q, 0 on P),  u1)
    out = mod_down(acc)                                   ONE, for the whole sum
    if 0 among the diagonals:  out += m_0 (.) (c0, c1)    on the Q limbs

A diagonal is a plaintext over Q and P, [nl + K][N]: limbs 0..nl-1 modulo q_0..q_{nl-1}, limbs nl..nl+K-1 modulo the special
primes, NTT domain, canonical, in Encoder.Encode's form m * T^-1; its multiplier is m_k = pt_k * T per limb (MulNew's).
`per_rotation` is the form a caller composes from the rotation and mul_plain, one ModDown per diagonal: it decrypts alike
and differs in its words."""
import numpy as np

import inner_sum_model as model
from inner_sum_model import _mod_index, _obj, _u64


def normalise(P, diags):
    """{k: pt} -> [(k mod N/2, g_k, pt)] in the order given; |k| < N/2, no duplicates after normalisation"""
    half, out = P.N // 2, []
    for k, pt in diags.items():
        if not -half < k < half:
            raise ValueError(f"diagonal {k} is outside (-N/2, N/2)")
        e = k % half
        if any(e == o[0] for o in out):
            raise ValueError(f"diagonal {k} is given twice (modulo N/2)")
        out.append((e, P.galois_element(e), pt))
    if not out:
        raise ValueError("a transform has at least one diagonal")
    return out


def elements(P, diags):
    """the Galois elements of the non-zero diagonals, in order of first use"""
    return [g for e, g, _ in normalise(P, diags) if e]


def encode_qp(P, values, nl):
    """Encoder.Encode extended to the limbs modulo P: the same lift of every coefficient in [0, T), the same T^-1"""
    pt = P.encode(values, nl=nl)
    q0, T = P.moduli[0], P.T
    assert T < q0  # the coefficient in [0, T) is read back from limb 0
    m = _obj(P.limb_intt(pt[0], 0)) * T % q0
    out = np.zeros((nl + P.K, P.N), dtype=np.uint64)
    out[:nl] = pt
    for a in range(P.K):
        p = P.moduli[P.L + a]
        out[nl + a] = P.limb_ntt(_u64(m % p * pow(T % p, -1, p) % p), P.L + a)
    return out


def _multiplier(P, pt, nl):
    """m = pt * T per position, object arrays"""
    return [_obj(pt[t]) * (P.T % P.moduli[_mod_index(P, t, nl)]) % P.moduli[_mod_index(P, t, nl)] for t in range(nl + P.K)]


def linear_transform(P, ct, diags, key, per_rotation=False):
    """ct: [2][nl][N]; diags {k: pt_k [nl + K][N]}; key(g) -> the Galois key of element g.  -> [2][nl][N], canonical"""
    ct = np.ascontiguousarray(ct, dtype=np.uint64)
    nl = ct.shape[1]
    pmod = 1
    for p in P.moduli[P.L:P.L + P.K]:
        pmod *= p
    acc, out, dig = None, np.zeros_like(ct), None
    for e, g, pt in normalise(P, diags):
        pt = np.asarray(pt, dtype=np.uint64)
        assert pt.shape == (nl + P.K, P.N), pt.shape
        if e == 0 or per_rotation:
            rot = ct if e == 0 else P.automorphism(ct, g, key(g))
            out = model._add(P, out, P.mul_plain(rot, pt[:nl]))
            continue
        dig = model.decompose(P, ct[1]) if dig is None else dig
        m, idx = _multiplier(P, pt, nl), P.automorphism_index(g)
        u = model.gadget(P, dig, nl, key(g))
        for t in range(nl):  # + P * c0 on the Q limbs of polynomial 0; it vanishes modulo P
            u[0][t] = (u[0][t] + (pmod % P.moduli[t]) * _obj(ct[0, t])) % P.moduli[t]
        term = [[m[t] * u[w][t][idx] % P.moduli[_mod_index(P, t, nl)] for t in range(nl + P.K)] for w in range(2)]
        if acc is None:
            acc = term
        else:
            for w in range(2):
                for t in range(nl + P.K):
                    acc[w][t] = (acc[w][t] + term[w][t]) % P.moduli[_mod_index(P, t, nl)]
    if acc is not None:
        out = model._add(P, model.mod_down(P, acc, nl), out)
    return out
