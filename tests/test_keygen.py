"""Key generation on the device (lumen_keygen_*): every word of every key against the Python restatement of the
sampling contract (keygen_model.py), the generated keys driving the product path with no oracle key anywhere,
determinism and the refusals."""
import ctypes as C

import numpy as np
import pytest

import keygen_model as km
from helpers import T_REF, canonical, make_context, make_params
from lumenos_amd.hip import LUMEN_KEY_MONTGOMERY, SYMBOLS

SEED = bytes(range(32))
SEED2 = bytes(range(1, 33))
T_RS = 0x3EE0001  # TestRingSwitch's plaintext modulus (fhe/ring_switch_test.go:17)
_cache = {}


def _params(oracle, log_n, L, K, T=T_REF):
    """one parameter set and its model secret per shape, shared by the tests and never modified"""
    key = (log_n, L, K, T)
    if key not in _cache:
        P = make_params(oracle, log_n, L, num_p=K, T=T)
        _cache[key] = (P, km.secret(P, SEED))
    return _cache[key]


def _model_galois(oracle, shape, g):
    key = ("gal",) + shape + (g,)
    if key not in _cache:
        P, s = _params(oracle, *shape)
        _cache[key] = km.galois_key(P, SEED, s, g)
    return _cache[key]


# ------------------------------------------------------------------ CPU: the model's vectors contain the hard cases
def test_header_states_the_contract_and_binding_has_the_entry_points():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lumenos_hip.h")).read()
    for name in ("lumen_keygen_secret", "lumen_keygen_public", "lumen_keygen_galois", "lumen_keygen_relin",
                 "lumen_keygen_ringswitch"):
        assert name in SYMBOLS and re.search(r"\bint " + name + r"\(", hdr), name
    assert int(re.search(r"#define LUMEN_KEY_MONTGOMERY (\d+)u", hdr).group(1)) == LUMEN_KEY_MONTGOMERY
    assert "#define LUMEN_ABI_VERSION 4" in hdr  # new symbols only
    flat = " ".join(hdr.split())
    for phrase in ("key_id * 4096 + e", "0x10000 + g", "stream 16 + m", "x < 2^64 - (2^64 mod q_m)",
                   "MUST NOT be passed to lumen_encrypt_*"):
        assert phrase in flat, phrase


def test_model_vectors_contain_redraws(oracle):
    """The rejection sampler's redraw path cannot go untested: the Galois key of g = 5 has first-attempt redraws in
    several limbs at (10, 3, 2) and second-attempt redraws at (12, 3, 2) and (8, 2, 1)."""
    _, rd = _model_galois(oracle, (10, 3, 2), 5)
    P = _params(oracle, 10, 3, 2)[0]
    first = km.count_redraws(rd, 0)
    print("(10,3,2) first-attempt redraws per (entry, limb):", first)
    LK = P.L + P.K
    limbs_hit = {i % LK for i, c in enumerate(first) if c}
    assert len(limbs_hit) >= 2
    for shape in ((12, 3, 2), (8, 2, 1)):
        _, rd = _model_galois(oracle, shape, 5)
        print(shape, "first:", sum(km.count_redraws(rd, 0)), "second:", sum(km.count_redraws(rd, 1)))
        assert sum(km.count_redraws(rd, 1)) >= 1, shape


def test_model_k0_ringswitch_shape(oracle):
    """(10, 1, 0): TestRingSwitch's P-less shape -- five base-2^13 entries of one limb, fac = 2^(13 j)"""
    P, s = _params(oracle, 10, 1, 0, T_RS)
    key, _ = km.ringswitch_key(P, SEED, s, 8, 13)
    assert key.shape == (1, 5, 2, 1, P.N) and canonical(P, key)
    assert [km.gadget_factor(P, 0, j, 0, 13) for j in range(5)] == [pow(2, 13 * j, P.moduli[0]) for j in range(5)]


def test_model_public_key_is_an_encryption_of_zero(oracle):
    """b + a*s = NTT(e) with |e| <= 19: the model's pk is a well-formed rlwe.PublicKey over QP"""
    P, s = _params(oracle, 8, 2, 1)
    pk = km.public_key(P, SEED, s)
    for m, q in enumerate(P.moduli):
        ph = np.array([(int(b) + int(a) * int(x)) % q for b, a, x in zip(pk[0, m], pk[1, m], s[m])], dtype=np.uint64)
        e = P.limb_intt(ph, m).astype(object)
        e = np.where(e > q // 2, e - q, e)
        assert max(abs(int(x)) for x in e) <= 19


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_secret_key_matches_model_and_is_installed(oracle):
    from lumenos_amd import params as lp
    P, s = _params(oracle, 10, 3, 2)
    ctx = make_context(P)
    sk = ctx.keygen_secret(SEED)
    assert sk.shape == (P.L + P.K, P.N) and np.array_equal(sk, s)
    # installed: the oracle's ciphertexts under the oracle's pk of this secret decrypt on the device
    ctx.encoder_set(lp.encoder_psi(T_REF, P.logN))
    P.seed(77)
    pk = P.keygen_public(sk)
    vals = np.random.default_rng(1).integers(0, T_REF, size=(2, P.N), dtype=np.uint64)
    cts = np.stack([P.encrypt(pk, P.encode(v)) for v in vals])
    assert np.array_equal(ctx.decrypt(ctx.upload(cts), P.N), vals)
    # without a buffer the secret stays on the device and is the same one
    ctx2 = make_context(P)
    assert ctx2.keygen_secret(SEED, want_sk=False) is None
    ctx2.encoder_set(lp.encoder_psi(T_REF, P.logN))
    assert np.array_equal(ctx2.decrypt(ctx2.upload(cts), P.N), vals)
    ctx.close(), ctx2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(8, 2, 1), (10, 3, 2), (10, 5, 2), (12, 3, 2)])
def test_every_key_word_matches_model(oracle, shape):
    """pk, the Galois keys of InnerSum(1, 8) and InnerSum(1, N) (the second includes the row swap), rlk: a equals the
    rule, b = NTT(e) - a*s_out + fac*s_in, everything canonical; LUMEN_KEY_MONTGOMERY = the same times 2^64 mod q."""
    P, s = _params(oracle, *shape)
    ctx = make_context(P)
    assert np.array_equal(ctx.keygen_secret(SEED), s)
    pk = ctx.keygen_public(SEED)
    assert np.array_equal(pk, km.public_key(P, SEED, s))
    gal = list(dict.fromkeys(P.inner_sum_galois_elements(8) + P.inner_sum_galois_elements(P.N)))
    assert 2 * P.N - 1 in gal
    got = ctx.keygen_galois(SEED, gal)
    assert got.shape == (len(gal),) + P.evk_shape() and canonical(P, got)
    want = np.stack([_model_galois(oracle, shape, g)[0] for g in gal])
    for i, g in enumerate(gal):
        assert np.array_equal(got[i, :, 1], want[i, :, 1]), ("a", g)
        assert np.array_equal(got[i, :, 0], want[i, :, 0]), ("b", g)
    rlk = ctx.keygen_relin(SEED)
    want_rlk = km.relin_key(P, SEED, s)[0]
    assert np.array_equal(rlk, want_rlk)
    # Lattigo's storage form
    assert np.array_equal(ctx.keygen_galois(SEED, gal[:2], montgomery=True), km.montgomery(P, want[:2]))
    assert np.array_equal(ctx.keygen_relin(SEED, montgomery=True), km.montgomery(P, want_rlk))
    ctx.close()


@pytest.mark.gpu
def test_galois_key_at_two_to_the_14(oracle):
    shape = (14, 2, 1)
    P, s = _params(oracle, *shape)
    ctx = make_context(P)
    assert np.array_equal(ctx.keygen_secret(SEED), s)
    got = ctx.keygen_galois(SEED, [5])[0]
    assert np.array_equal(got, _model_galois(oracle, shape, 5)[0])
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("L,K", [(3, 2), (2, 1), (1, 0)])
def test_ringswitch_key_matches_model_and_switches(oracle, L, K):
    """The key equals the model ([rns][pw2] entries: K = 2 one per RNS digit, K <= 1 base-2^13 digits); loaded, it
    switches oracle-encrypted ciphertexts into the small ring, where they decrypt under the returned sk_small to the
    coefficients X^(i N/n) of the input's plaintext (the contract test_ring_switch_matches_oracle checks)."""
    log_n, logn_small, w = 10, 8, 13
    P, s = _params(oracle, log_n, L, K, T_RS)
    ctx = make_context(P)
    sk = ctx.keygen_secret(SEED)
    key, sk_small = ctx.keygen_ringswitch(SEED, logn_small, w)
    want, _ = km.ringswitch_key(P, SEED, s, logn_small, w)
    assert key.shape == want.shape == (*P.rs_key_shape(w), 2, L + K, P.N)
    assert key.shape[1] == (1 if K == 2 else 5)
    assert np.array_equal(sk_small.astype(np.int64), km.small_secret_coeffs(P, SEED, logn_small))
    assert np.array_equal(key[:, :, 1], want[:, :, 1]) and np.array_equal(key[:, :, 0], want[:, :, 0])
    P.seed(5)
    pk = P.keygen_public(sk)
    rng = np.random.default_rng(9)
    fresh = [P.encrypt(pk, P.encode(rng.integers(0, T_RS, size=P.N, dtype=np.uint64))) for _ in range(2)]
    cts = np.stack([ct if L == 1 else P.rescale_to_level1(ct) for ct in fresh])
    ctx.load_ringswitch_key(logn_small, key, w)
    got = ctx.ring_switch(ctx.upload(cts))
    small = sk_small.astype(np.int64)
    for c in range(2):
        assert np.array_equal(got[c], P.ring_switch(cts[c], key, logn_small, w)), c
        assert np.array_equal(P.decrypt_small_coeffs(small, logn_small, got[c]),
                              P.decrypt_big_coeffs_l0(sk, cts[c])[::P.N >> logn_small]), c
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,n", [((10, 3, 2), 8), ((10, 3, 2), 512), ((10, 3, 2), 1024), ((12, 3, 2), 8)])
def test_generated_keys_drive_the_product_path(oracle, shape, n):
    """keygen_secret -> keygen_public -> load_public_key + encrypt_values -> keygen_galois -> load_galois_key ->
    inner_sum(n) -> decrypt, no oracle key anywhere; the same keys handed to the oracle's InnerSum give the
    device's residues bit for bit; the Montgomery-form output loaded with montgomery=True changes no residue."""
    from lumenos_amd import params as lp
    P, _ = _params(oracle, *shape)
    N, half = P.N, P.N // 2
    ctx = make_context(P)
    ctx.keygen_secret(SEED, want_sk=False)
    ctx.encoder_set(lp.encoder_psi(T_REF, P.logN))
    ctx.load_public_key(ctx.keygen_public(SEED))
    vals = np.random.default_rng(n).integers(0, T_REF, size=(2, N), dtype=np.uint64)
    enc = ctx.encrypt_values(vals, np.arange(100, 132, dtype=np.uint8), 0)  # the encryptor's own seed
    gal = ctx.inner_sum_galois_elements(n)
    evk = ctx.keygen_galois(SEED, gal)
    for g, k in zip(gal, evk):
        ctx.load_galois_key(g, k)
    out = ctx.inner_sum(enc, n)
    res = out.download()
    dec = ctx.decrypt(out, N)
    for c in range(2):
        v = vals[c].astype(object)
        assert int(dec[c, 0]) == int(np.sum(v[:n])) % T_REF
        if n == half:
            assert all(int(x) == int(np.sum(v[:half])) % T_REF for x in dec[c, :half])
            assert all(int(x) == int(np.sum(v[half:])) % T_REF for x in dec[c, half:])
        if n == N:
            assert all(int(x) == int(np.sum(v)) % T_REF for x in dec[c])
    # the layout against the oracle's consumer
    cts = enc.download()
    for c in range(2):
        assert np.array_equal(res[c], P.inner_sum(cts[c], n, list(evk))), c
    for g, k in zip(gal, ctx.keygen_galois(SEED, gal, montgomery=True)):
        ctx.load_galois_key(g, k, montgomery=True)
    assert np.array_equal(ctx.inner_sum(enc, n).download(), res)
    ctx.close()


@pytest.mark.gpu
def test_determinism(oracle):
    P, s = _params(oracle, 10, 3, 2)
    ctx = make_context(P)
    gal = P.inner_sum_galois_elements(8)
    sk = ctx.keygen_secret(SEED)
    pk, evk, rlk = ctx.keygen_public(SEED), ctx.keygen_galois(SEED, gal), ctx.keygen_relin(SEED)
    # the same seed gives the same bytes
    assert np.array_equal(ctx.keygen_public(SEED), pk) and np.array_equal(ctx.keygen_galois(SEED, gal), evk)
    # one batched call == per-element calls, in any order
    for i in reversed(range(len(gal))):
        assert np.array_equal(ctx.keygen_galois(SEED, [gal[i]])[0], evk[i]), gal[i]
    # a clone shares the generated secret and generates the same keys
    cl = ctx.clone()
    assert np.array_equal(cl.keygen_public(SEED), pk) and np.array_equal(cl.keygen_galois(SEED, gal), evk)
    assert np.array_equal(cl.keygen_relin(SEED), rlk)
    cl.close()
    # into page-locked memory: the same bytes
    from lumenos_amd.hip import pinned_empty, pinned_free
    pin = pinned_empty(evk.shape)
    assert np.array_equal(ctx.keygen_galois(SEED, gal, out=pin), evk)
    pinned_free(pin)
    # another seed changes sk and every key
    sk2 = ctx.keygen_secret(SEED2)
    assert not np.array_equal(sk2, sk)
    assert not np.array_equal(ctx.keygen_public(SEED2), pk) and not np.array_equal(ctx.keygen_relin(SEED2), rlk)
    evk2 = ctx.keygen_galois(SEED2, gal)
    assert all(not np.array_equal(evk2[i, d, w], evk[i, d, w]) for i in range(len(gal)) for d in range(evk.shape[1])
               for w in range(2))
    ctx.close()


@pytest.mark.gpu
def test_refusals(oracle):
    from lumenos_amd.hip import LumenError
    P, _ = _params(oracle, 10, 3, 2)
    ctx = make_context(P)
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    seed = np.frombuffer(SEED, dtype=np.uint8).copy()
    sp = seed.ctypes.data_as(u8p)

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    # no generated secret on the context (a LOADED secret key is not one)
    ctx.load_secret_key(np.zeros((P.L, P.N), dtype=np.uint64))
    for fn in (lambda: ctx.keygen_public(SEED), lambda: ctx.keygen_relin(SEED), lambda: ctx.keygen_galois(SEED, [5]),
               lambda: ctx.keygen_ringswitch(SEED, 8)):
        fails(fn, "no generated secret")
    ctx.keygen_secret(SEED)
    pk = ctx.keygen_public(SEED)
    # NULL ctx / seed / output
    lib = ctx.lib
    assert lib.lumen_keygen_public(None, sp, pk.ctypes.data_as(u64p)) != 0
    assert b"NULL" in lib.lumen_last_error(None)
    assert lib.lumen_keygen_secret(None, sp, None) != 0 and b"NULL" in lib.lumen_last_error(None)
    fails(lambda: ctx._ck(lib.lumen_keygen_secret(ctx.h, None, None)), "NULL")
    fails(lambda: ctx._ck(lib.lumen_keygen_public(ctx.h, None, pk.ctypes.data_as(u64p))), "NULL")
    fails(lambda: ctx._ck(lib.lumen_keygen_public(ctx.h, sp, None)), "NULL")
    fails(lambda: ctx._ck(lib.lumen_keygen_relin(ctx.h, sp, None, 0)), "NULL")
    g5 = np.array([5], dtype=np.uint64)
    fails(lambda: ctx._ck(lib.lumen_keygen_galois(ctx.h, sp, g5.ctypes.data_as(u64p), 1, None, 0)), "NULL")
    fails(lambda: ctx._ck(lib.lumen_keygen_galois(ctx.h, sp, None, 1, pk.ctypes.data_as(u64p), 0)), "NULL")
    key = np.zeros(ctx.ringswitch_key_shape(), dtype=np.uint64)
    small = np.zeros(256, dtype=np.int8)
    i8p = C.POINTER(C.c_int8)
    fails(lambda: ctx._ck(lib.lumen_keygen_ringswitch(ctx.h, sp, 8, 13, None, key.size, small.ctypes.data_as(i8p))), "NULL")
    fails(lambda: ctx._ck(lib.lumen_keygen_ringswitch(ctx.h, sp, 8, 13, key.ctypes.data_as(u64p), key.size, None)), "NULL")
    # Galois elements
    fails(lambda: ctx.keygen_galois(SEED, [5, 4]), "odd residue")
    fails(lambda: ctx.keygen_galois(SEED, [2 * P.N + 1]), "odd residue")
    # flags
    evk = np.zeros((1,) + P.evk_shape(), dtype=np.uint64)
    fails(lambda: ctx._ck(lib.lumen_keygen_galois(ctx.h, sp, g5.ctypes.data_as(u64p), 1, evk.ctypes.data_as(u64p), 2)),
          "unknown flags")
    fails(lambda: ctx._ck(lib.lumen_keygen_relin(ctx.h, sp, evk.ctypes.data_as(u64p), 6)), "unknown flags")
    # ring switch: key size and target degree
    fails(lambda: ctx._ck(lib.lumen_keygen_ringswitch(ctx.h, sp, 8, 13, key.ctypes.data_as(u64p), key.size - 1,
                                                      small.ctypes.data_as(i8p))), "expected")
    fails(lambda: ctx.keygen_ringswitch(SEED, P.logN), "not below")
    fails(lambda: ctx.keygen_ringswitch(SEED, P.logN + 1), "not below")
    # count == 0 succeeds and touches nothing
    assert lib.lumen_keygen_galois(ctx.h, sp, None, 0, None, 0) == 0
    assert ctx.keygen_galois(SEED, []).shape == (0,) + P.evk_shape()
    # K = 0: no key switching keys
    P0, _ = _params(oracle, 10, 1, 0, T_RS)
    c0 = make_context(P0)
    c0.keygen_secret(SEED)
    fails(lambda: c0.keygen_galois(SEED, [5]), "no special primes")
    fails(lambda: c0.keygen_relin(SEED), "no special primes")
    c0.close()
    # the context stays usable
    assert np.array_equal(ctx.keygen_public(SEED), pk)
    ctx.close()
