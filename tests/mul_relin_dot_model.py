"""Sums of ciphertext products with one relinearisation per sum (lumen_mul_relin_dot, lumen_mul_tensor_dot) restated on
the CPU oracle: the group sums in exact Python integers, the key switch through tests/mul_relin_model.relinearise.

    e = g n + i, term i of group g;  b_e = B[g n + i] (B of A's count) or B[i] (B of n ciphertexts)
    D0 = t sum_i a0_e b0_e      D1 = t sum_i (a0_e b1_e + a1_e b0_e)      D2 = t sum_i a1_e b1_e      (mod q_l, every limb)
    out[g] = relinearise(D0, D1, D2)

The sums are formed over the integers and reduced ONCE, with t = T mod q_l applied to the sum: no chunk, no lazy range, no
Montgomery form -- what the device's words must equal whatever its order of reductions.  Nothing here reads the device's
output."""
import numpy as np

import mul_relin_model as mr


def _b_of(A, B, n):
    assert n >= 1 and len(A) % n == 0 and len(B) in (len(A), n), (len(A), len(B), n)
    return (lambda e: B[e]) if len(B) == len(A) else (lambda e: B[e % n])


def tensor_dot(P, A, B, n):
    """A: [groups * n][2][nl][N]; B: as many ciphertexts, or n -> (D0, D1, D2) as [groups][3][nl][N]"""
    b_of = _b_of(A, B, n)
    groups, nl = len(A) // n, A.shape[2]
    out = np.zeros((groups, 3, nl, P.N), dtype=np.uint64)
    for g in range(groups):
        for l in range(nl):
            q = P.moduli[l]
            s0 = s1 = s2 = 0  # object arrays from the first term on
            for e in range(g * n, (g + 1) * n):
                a, b = A[e], b_of(e)
                a0, a1, b0, b1 = (x.astype(object) for x in (a[0, l], a[1, l], b[0, l], b[1, l]))
                s0 = s0 + a0 * b0
                s1 = s1 + a0 * b1 + a1 * b0
                s2 = s2 + a1 * b1
            t = P.T % q
            for w, s in enumerate((s0, s1, s2)):
                out[g, w, l] = (t * s % q).astype(np.uint64)
    return out


def mul_relin_dot(P, A, B, n, rlk):
    """-> [groups][2][nl][N]"""
    d = tensor_dot(P, A, B, n)
    if not len(d):
        return np.zeros((0, 2, A.shape[2], P.N), dtype=np.uint64)
    return np.stack([mr.relinearise(P, x, rlk) for x in d])
