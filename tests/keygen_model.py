"""The sampling contract of device key generation (include/lumenos_hip.h, lumen_keygen_*), restated in Python on
top of the oracle's exported primitives (lo_chacha20_xor, lo_det_small, lo_limb_ntt, lo_automorphism_index) and
Python integers for the products.  Nothing here reads the device's output.

    keystream(I, s)  = ChaCha20(key = seed, nonce = LE64(I) || LE32(s), counter = 0, 1, ...)
    I(key_id, e)     = key_id * 4096 + e
    secret           = det_small(seed, I(0, 0), stream 0)
    error of entry e = det_small(seed, I(key_id, e), stream 1), one sample for every limb
    a, limb m        = stream 16 + m as little-endian u64 words; attempt t of coefficient k is word t * N + k; the
                       first x < 2^64 - (2^64 mod q_m) is kept, a[k] = x mod q_m
    b                = NTT(e) - a * s_out + fac * s_in  (mod q_m)
"""
import ctypes as C

import numpy as np

INDEX_STRIDE = 4096
ID_SECRET, ID_PUBLIC, ID_RELIN, ID_RINGSWITCH, ID_GALOIS = 0, 1, 2, 3, 0x10000
UNIFORM_STREAM = 16
_u8p = C.POINTER(C.c_uint8)


def _seed(seed):
    return np.frombuffer(bytes(seed), dtype=np.uint8).copy()


def sample_index(key_id, e):
    return key_id * INDEX_STRIDE + e


def keystream(oracle, seed, index, stream, nbytes, first_block=0):
    seed = _seed(seed)
    nonce = np.frombuffer(int(index).to_bytes(8, "little") + int(stream).to_bytes(4, "little"), dtype=np.uint8).copy()
    buf = np.zeros(nbytes, dtype=np.uint8)
    oracle.lib.lo_chacha20_xor(seed.ctypes.data_as(_u8p), nonce.ctypes.data_as(_u8p), first_block, buf.ctypes.data_as(_u8p),
                               nbytes)
    return buf


def uniform(P, seed, key_id, e, m):
    """-> (a[N] uint64, [coefficients redrawn after attempt 0, after attempt 1, ...])"""
    N, q = P.N, P.moduli[m]
    bound = (1 << 64) - ((1 << 64) % q)
    a = np.zeros(N, dtype=np.uint64)
    pending = np.ones(N, dtype=bool)
    redraws = []
    t = 0
    while pending.any():
        # attempt t: words t * N .. t * N + N - 1 = the N * 8 bytes from block t * N / 8 on
        w = keystream(P.o, seed, sample_index(key_id, e), UNIFORM_STREAM + m, N * 8, first_block=t * N // 8).view("<u8")
        ok = pending & (w < np.uint64(bound))
        a[ok] = w[ok] % np.uint64(q)
        pending &= ~ok
        if pending.any():
            redraws.append(int(pending.sum()))
        t += 1
    return a, redraws


def secret_coeffs(P, seed):
    return P.det_small(_seed(seed), sample_index(ID_SECRET, 0), 0).astype(np.int64)


def small_secret_coeffs(P, seed, log_n_small):
    return P.det_small(_seed(seed), sample_index(ID_RINGSWITCH, 0), 0)[:1 << log_n_small].astype(np.int64)


def ntt_small(P, coeffs):
    """small signed coefficients -> [L+K][N] NTT-domain residues"""
    out = np.zeros((P.L + P.K, P.N), dtype=np.uint64)
    for m, q in enumerate(P.moduli):
        c = np.asarray(coeffs, dtype=np.int64)
        out[m] = P.limb_ntt(np.where(c >= 0, c, c + q).astype(np.uint64), m)
    return out


def secret(P, seed):
    return ntt_small(P, secret_coeffs(P, seed))


def embedded_small_secret(P, seed, log_n_small):
    """NTT over QP of skNew(X^(N/n))"""
    emb = np.zeros(P.N, dtype=np.int64)
    emb[::P.N >> log_n_small] = small_secret_coeffs(P, seed, log_n_small)
    return ntt_small(P, emb)


def gadget_factor(P, i, j, m, w):
    """P * 2^(w j) mod q_m on the Q limbs of RNS digit i (alpha = max(K, 1)), 0 elsewhere"""
    alpha = max(P.K, 1)
    if not (m < P.L and i * alpha <= m < (i + 1) * alpha):
        return 0
    q = P.moduli[m]
    f = pow(2, w * j, q)
    for p in P.moduli[P.L:]:
        f = f * p % q
    return f


def entry(P, seed, key_id, e, s_out, s_in, fac):
    """One gadget entry: -> (b [L+K][N], a [L+K][N], e int8[N], redraws per limb).  fac: [L+K] integers."""
    LK = P.L + P.K
    err = P.det_small(_seed(seed), sample_index(key_id, e), 1)
    en = ntt_small(P, err)
    b = np.zeros((LK, P.N), dtype=np.uint64)
    a = np.zeros((LK, P.N), dtype=np.uint64)
    redraws = []
    for m, q in enumerate(P.moduli):
        a[m], rd = uniform(P, seed, key_id, e, m)
        redraws.append(rd)
        v = en[m].astype(object) - a[m].astype(object) * s_out[m].astype(object)
        if fac[m]:
            v = v + fac[m] * s_in[m].astype(object)
        b[m] = np.array([int(x) % q for x in v], dtype=np.uint64)
    return b, a, err, redraws


def gadget_key(P, seed, key_id, s_out, s_in, rns, pw2=1, w=0):
    """[rns * pw2][b|a][L+K][N] and the redraw lists [entry][limb]"""
    LK = P.L + P.K
    key = np.zeros((rns * pw2, 2, LK, P.N), dtype=np.uint64)
    redraws = []
    for i in range(rns):
        for j in range(pw2):
            e = i * pw2 + j
            fac = [gadget_factor(P, i, j, m, w) for m in range(LK)]
            key[e, 0], key[e, 1], _, rd = entry(P, seed, key_id, e, s_out, s_in, fac)
            redraws.append(rd)
    return key, redraws


def public_key(P, seed, s):
    b, a, _, _ = entry(P, seed, ID_PUBLIC, 0, s, s, [0] * (P.L + P.K))
    return np.stack([b, a])


def galois_sout(P, s, g):
    """pi_{g^-1}(s): lo_keygen_galois's gather with the index table of g^-1 mod 2N"""
    idx = P.automorphism_index(pow(g, -1, 2 * P.N))
    return np.ascontiguousarray(s[:, idx])


def galois_key(P, seed, s, g):
    return gadget_key(P, seed, ID_GALOIS + g, galois_sout(P, s, g), s, P.beta())


def relin_key(P, seed, s):
    s2 = np.stack([np.array([int(x) * int(x) % q for x in s[m]], dtype=np.uint64) for m, q in enumerate(P.moduli)])
    return gadget_key(P, seed, ID_RELIN, s, s2, P.beta())


def ringswitch_key(P, seed, s, log_n_small, w):
    rns, pw2 = P.rs_key_shape(w)
    key, rd = gadget_key(P, seed, ID_RINGSWITCH, embedded_small_secret(P, seed, log_n_small), s, rns, pw2,
                         0 if P.K >= 2 else w)
    return key.reshape(rns, pw2, 2, P.L + P.K, P.N), rd


def montgomery(P, key):
    """the words times 2^64 mod q_m (limb axis: second to last)"""
    out = np.zeros_like(key)
    for m, q in enumerate(P.moduli):
        r = (1 << 64) % q
        flat = key[..., m, :].reshape(-1)
        out[..., m, :] = np.array([int(x) * r % q for x in flat], dtype=np.uint64).reshape(key[..., m, :].shape)
    return out


def count_redraws(redraws, attempt):
    """coefficients still undecided after `attempt` + 1 attempts, per (entry, limb) stream, flattened"""
    return [rd[attempt] if len(rd) > attempt else 0 for ent in redraws for rd in ent]
