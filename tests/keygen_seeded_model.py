"""The seeded switching keys (include/lumenos_hip.h, lumen_keygen_*_seeded / lumen_load_*_key_seeded) restated on top
of keygen_model.py.  A seeded key takes two seeds:

    seed    key material: the error of entry e is det_small(seed, I(key_id, e), stream 1); the secret is the context's
    a_seed  public: a of limb m of entry e is keygen_model.uniform under a_seed -- stream 16 + m of the SAME index
    b       = NTT(e) - a * s_out + fac * s_in  (mod q_m), Python integers for the product

What travels is b alone, [beta][L+K][N]; the receiver draws a.  Nothing here reads the device's output.
"""
import numpy as np

import keygen_model as km


def entry(P, seed, a_seed, key_id, e, s_out, s_in, fac):
    """One gadget entry: -> (b [L+K][N], a [L+K][N], redraws per limb).  fac: [L+K] integers."""
    LK = P.L + P.K
    en = km.ntt_small(P, P.det_small(km._seed(seed), km.sample_index(key_id, e), 1))
    b = np.zeros((LK, P.N), dtype=np.uint64)
    a = np.zeros((LK, P.N), dtype=np.uint64)
    redraws = []
    for m, q in enumerate(P.moduli):
        a[m], rd = km.uniform(P, a_seed, key_id, e, m)
        redraws.append(rd)
        v = en[m].astype(object) - a[m].astype(object) * s_out[m].astype(object)
        if fac[m]:
            v = v + fac[m] * s_in[m].astype(object)
        b[m] = np.array([int(x) % q for x in v], dtype=np.uint64)
    return b, a, redraws


def gadget_key(P, seed, a_seed, key_id, s_out, s_in):
    """-> (b [beta][L+K][N], a [beta][L+K][N], redraw lists [entry][limb])"""
    LK, beta = P.L + P.K, P.beta()
    b = np.zeros((beta, LK, P.N), dtype=np.uint64)
    a = np.zeros_like(b)
    redraws = []
    for i in range(beta):
        fac = [km.gadget_factor(P, i, 0, m, 0) for m in range(LK)]
        b[i], a[i], rd = entry(P, seed, a_seed, key_id, i, s_out, s_in, fac)
        redraws.append(rd)
    return b, a, redraws


def galois_key(P, seed, a_seed, s, g):
    return gadget_key(P, seed, a_seed, km.ID_GALOIS + g, km.galois_sout(P, s, g), s)


def relin_key(P, seed, a_seed, s):
    s2 = np.stack([np.array([int(x) * int(x) % q for x in s[m]], dtype=np.uint64) for m, q in enumerate(P.moduli)])
    return gadget_key(P, seed, a_seed, km.ID_RELIN, s, s2)


def mask(P, a_seed, key_id):
    """the a halves alone, [beta][L+K][N]: what the loaders draw (no secret, no error)"""
    return np.stack([np.stack([km.uniform(P, a_seed, key_id, i, m)[0] for m in range(P.L + P.K)]) for i in range(P.beta())])


def full_key(b, a):
    """(b, a) -> [beta][b|a][L+K][N], the layout of lumen_load_galois_key / lumen_load_relin_key"""
    return np.ascontiguousarray(np.stack([b, a], axis=1))


# ---- the vectors of the two test files, computed once per process and never modified
SEED = bytes(range(100, 132))  # key material of the tests
A_SEED = bytes(range(32))      # public; the seed constant of test_keygen.py, whose a words that file's redraw test pins
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def params(oracle, log_n, L, K, T=None):
    """-> (P, the model secret under SEED)"""
    from helpers import T_REF, make_params

    def make():
        P = make_params(oracle, log_n, L, num_p=K, T=T_REF if T is None else T)
        return P, km.secret(P, SEED)
    return cached(("params", log_n, L, K, T), make)


def model_galois(oracle, shape, g):
    P, s = params(oracle, *shape)
    return cached(("gal", shape, g), lambda: galois_key(P, SEED, A_SEED, s, g))


def model_relin(oracle, shape):
    P, s = params(oracle, *shape)
    return cached(("rlk", shape), lambda: relin_key(P, SEED, A_SEED, s))
