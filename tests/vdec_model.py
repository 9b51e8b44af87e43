"""The front end of the proof of decryption (vdec/batching.go, vdec/prover.go:104-119) restated on the CPU oracle's
existing calls -- encode, mul_plain, rescale, limb_intt, rescale_scale -- with exact Python integers for every sum.
What lumen_batch_ciphertexts and lumen_vdec_witness are compared with, word for word."""
import numpy as np


def scaled(P, values, scale):
    """values * scale mod T, as Encoder.Encode scales a plaintext's values (modulo T, ahead of the transform)"""
    T, s = P.T, scale % P.T
    return np.array([(int(v) % T) * s % T for v in values], dtype=np.uint64)


def batch_columns(T, cols, alphas):
    """vdec.BatchColumns: m[i] = sum_j alphas[j][i] * cols[j][i] mod T"""
    cols, alphas = np.asarray(cols), np.asarray(alphas)
    assert cols.shape == alphas.shape
    return np.array([sum(int(a) * int(c) for a, c in zip(alphas[:, i], cols[:, i])) % T for i in range(cols.shape[1])],
                    dtype=np.uint64)


def batch_ciphertexts(P, cts, alphas, pt_scale=1):
    """vdec.BatchCiphertexts: sum_j mul_plain(ct_j, encode(alphas[j] * pt_scale mod T)); cts [count][2][nl][N]"""
    count, _, nl, N = cts.shape
    assert len(alphas) == count
    acc = np.zeros((2, nl, N), dtype=object)
    for ct, a in zip(cts, alphas):
        acc = acc + P.mul_plain(ct, P.encode(scaled(P, a, pt_scale), nl)).astype(object)
    out = np.zeros((2, nl, N), dtype=np.uint64)
    for l in range(nl):
        out[:, l] = (acc[:, l] % P.moduli[l]).astype(np.uint64)
    return out


def rescale_to(P, ct, target):
    while ct.shape[1] > target:
        ct = P.rescale(ct)
    return ct


def centre(x, q):
    x = np.asarray(x).astype(object)
    return np.where(x > q // 2, x - q, x).astype(np.int64)


def witness(P, sk, ct, m, scale):
    """The witness on ONE one-limb ciphertext ct [2][1][N]: centred coefficient vectors of sk, c0, c1, of the message
    at `scale` (m_delta = Encode(m * scale) = coefficients * T^-1 mod q_0) and err = c0 + c1 * sk - m_delta."""
    assert ct.shape == (2, 1, P.N)
    q = P.moduli[0]
    md = P.limb_intt(P.encode(scaled(P, m, scale), 1)[0], 0)
    ph = np.array([(int(a) + int(b) * int(s)) % q for a, b, s in zip(ct[0, 0], ct[1, 0], sk[0])], dtype=np.uint64)
    e = np.array([(int(x) - int(y)) % q for x, y in zip(P.limb_intt(ph, 0), md)], dtype=object)
    return {"sk": centre(P.limb_intt(sk[0], 0), q).astype(np.int8), "c0": centre(P.limb_intt(ct[0, 0], 0), q),
            "c1": centre(P.limb_intt(ct[1, 0], 0), q), "m_delta": centre(md, q), "err": centre(e, q)}
