"""The ciphertext x ciphertext product with relinearisation (lumen_mul_relin, lumen_mul_tensor) restated on the CPU
oracle: the tensor in exact Python integers, the key switch through the oracle's own key_switch.

    d0 = t a0 b0        d1 = t (a0 b1 + a1 b0)        d2 = t a1 b1            (mod q_i, every limb i < nl)
    (k0, k1) = key_switch(d2, nl, rlk)
    out = (d0 + k0, d1 + k1)

t is T mod q_i, the factor lo_mul_plain gives its plaintext (`t_factor=False` leaves it out: the negative case of
tests/test_mul_relin_model.py).  key_switch is static in oracle/lo_eval.c and reachable through lo_automorphism with
Galois element 1, whose index table is the identity: for ct = (x, d2) it returns (x + k0, k1).  So the model is
automorphism((d0, d2), 1, rlk) plus d1 on the second half.  Nothing here reads the device's output."""
import numpy as np


def _mod(x, q):
    return (x % q).astype(np.uint64)


def tensor(P, a, b, t_factor=True):
    """a, b: [2][nl][N] -> (d0, d1, d2) as [3][nl][N]"""
    assert a.shape == b.shape and a.shape[0] == 2
    nl = a.shape[1]
    out = np.zeros((3, nl, P.N), dtype=np.uint64)
    for l in range(nl):
        q = P.moduli[l]
        t = P.T % q if t_factor else 1
        a0, a1, b0, b1 = (x.astype(object) for x in (a[0, l], a[1, l], b[0, l], b[1, l]))
        out[0, l] = _mod(t * a0 * b0, q)
        out[1, l] = _mod(t * (a0 * b1 + a1 * b0), q)
        out[2, l] = _mod(t * a1 * b1, q)
    return out


def relinearise(P, d, rlk):
    """(d0, d1, d2) [3][nl][N] -> (d0 + k0, d1 + k1) [2][nl][N]"""
    nl = d.shape[1]
    ks = P.automorphism(np.stack([d[0], d[2]]), 1, rlk)  # (d0 + k0, k1)
    out = ks.copy()
    for l in range(nl):
        out[1, l] = _mod(ks[1, l].astype(object) + d[1, l].astype(object), P.moduli[l])
    return out


def mul_relin(P, a, b, rlk, t_factor=True):
    return relinearise(P, tensor(P, a, b, t_factor), rlk)


def _pairs(A, B):
    assert len(B) in (len(A), 1), (len(A), len(B))
    return [(a, B[i if len(B) == len(A) else 0]) for i, a in enumerate(A)]


def mul_tensor_sets(P, A, B):
    """A: [count][2][nl][N]; B: as many ciphertexts, or one (every ciphertext of A times it) -> [count][3][nl][N]"""
    return np.stack([tensor(P, a, b) for a, b in _pairs(A, B)])


def mul_relin_sets(P, A, B, rlk):
    """-> [count][2][nl][N]"""
    return np.stack([mul_relin(P, a, b, rlk) for a, b in _pairs(A, B)])
