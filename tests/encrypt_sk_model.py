"""The contract of secret-key encryption (include/lumenos_hip.h, lumen_encrypt_sk_*), restated in Python on top of the
oracle's exported primitives (lo_chacha20_xor, lo_det_small, lo_limb_ntt, Encoder.Encode) and Python integers for the
products, with keygen_model's keystream and rejection sampler.  Nothing here reads the device's output.

    ciphertext i     has sample index I = first_index + i
    error            e = det_small(secret_seed, I, stream 3), one sample for every limb
    c1[l] = a_l      stream 16 + l of I under a_seed, key generation's rejection rule, Q limbs only
    c0[l]            NTT_l(e) + pt_l - a_l * NTT_l(s)  (mod q_l),  pt = Encoder.Encode(values)
"""
import numpy as np

import keygen_model as km

ERR_STREAM = 3


def error(P, secret_seed, index):
    return P.det_small(km._seed(secret_seed), int(index), ERR_STREAM)


def mask(P, a_seed, index):
    """-> (a [L][N], redraw lists per limb)"""
    a = np.zeros((P.L, P.N), dtype=np.uint64)
    redraws = []
    for l in range(P.L):
        a[l], rd = km.uniform(P, a_seed, 0, int(index), l)  # sample_index(0, I) = I
        redraws.append(rd)
    return a, redraws


def zero_encryption(P, s, secret_seed, a_seed, index):
    """-> (base [L][N] = NTT(e) - a * s, a [L][N], e int8 [N], redraws per limb): the ciphertext of the zero plaintext"""
    e = error(P, secret_seed, index)
    en = km.ntt_small(P, e)
    a, redraws = mask(P, a_seed, index)
    base = np.zeros((P.L, P.N), dtype=np.uint64)
    for l in range(P.L):
        q = P.moduli[l]
        base[l] = np.array([(int(x) - int(y) * int(z)) % q for x, y, z in zip(en[l], a[l], s[l])], dtype=np.uint64)
    return base, a, e, redraws


def add_plaintext(P, base, a, values):
    """-> ct [2][L][N]: c0 = base + Encode(values)"""
    pt = P.encode(np.ascontiguousarray(values, dtype=np.uint64))
    ct = np.zeros((2, P.L, P.N), dtype=np.uint64)
    for l in range(P.L):
        ct[0, l] = (base[l] + pt[l]) % np.uint64(P.moduli[l])  # both below q < 2^58
    ct[1] = a
    return ct


def encrypt(P, s, values, secret_seed, a_seed, first_index):
    """values [count][rows] -> (cts [count][2][L][N], errors int8 [count][N], redraws [count][limb])"""
    values = np.ascontiguousarray(values, dtype=np.uint64)
    cts, errs, redraws = [], [], []
    for i in range(values.shape[0]):
        base, a, e, rd = zero_encryption(P, s, secret_seed, a_seed, first_index + i)
        cts.append(add_plaintext(P, base, a, values[i]))
        errs.append(e)
        redraws.append(rd)
    return np.stack(cts), np.stack(errs), redraws
