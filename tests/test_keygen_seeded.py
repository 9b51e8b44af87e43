"""Seeded switching keys on the device (lumen_keygen_galois_seeded / lumen_keygen_relin_seeded: the b halves, `a` drawn
inside the transform's storer under a public seed; lumen_load_galois_key_seeded / lumen_load_relin_key_seeded: b
converted, `a` drawn into the gadget product's layout).  Every comparison is exact: against keygen_seeded_model.py, the
full-key entry points and the CPU oracle's consumers.  The shapes are the ones whose `a` words reach the redraw loop at
attempts 1 and 2 (test_keygen_seeded_model.py asserts it).

On the parent of the commit that introduced this file every test here fails: the entry points do not exist."""
import ctypes as C

import numpy as np
import pytest

import keygen_model as km
import keygen_seeded_model as ksm
import mul_relin_model as mrm
from helpers import make_context, make_params, random_cts
from keygen_seeded_model import A_SEED, SEED
from lumenos_amd.hip import LumenError

gpu = pytest.mark.gpu
T_RS = 0x3EE0001
SHAPE = (10, 3, 2)
_u8p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)


def _junk_key(P, seed):
    """canonical words that are no key of anything: what a loader has to replace"""
    rng = np.random.default_rng(seed)
    key = np.zeros(P.evk_shape(), dtype=np.uint64)
    for m, q in enumerate(P.moduli):
        key[:, :, m] = rng.integers(0, q, size=key[:, :, m].shape, dtype=np.uint64)
    return key


# ------------------------------------------------------------------ 1. generation
@gpu
@pytest.mark.parametrize("shape", [(10, 3, 2), (8, 2, 1), (12, 3, 2)])
def test_seeded_keys_match_model(oracle, shape):
    P, s = ksm.params(oracle, *shape)
    ctx = make_context(P)
    assert np.array_equal(ctx.keygen_secret(SEED), s)
    gal = [5, 2 * P.N - 1]
    want = np.stack([ksm.model_galois(oracle, shape, g)[0] for g in gal])
    got = ctx.keygen_galois_seeded(SEED, A_SEED, gal)
    assert got.shape == (2,) + ctx.seeded_evk_shape() == want.shape
    for i, g in enumerate(gal):
        assert np.array_equal(got[i], want[i]), g
    # one call == the keys one at a time, in any order
    for i in (1, 0):
        assert np.array_equal(ctx.keygen_galois_seeded(SEED, A_SEED, [gal[i]])[0], want[i]), gal[i]
    assert np.array_equal(ctx.keygen_galois_seeded(SEED, A_SEED, gal, montgomery=True), km.montgomery(P, want))
    want_rlk = ksm.model_relin(oracle, shape)[0]
    assert np.array_equal(ctx.keygen_relin_seeded(SEED, A_SEED), want_rlk)
    assert np.array_equal(ctx.keygen_relin_seeded(SEED, A_SEED, montgomery=True), km.montgomery(P, want_rlk))
    # the full keys are what they were: a under the keygen seed
    assert not np.array_equal(ctx.keygen_galois(SEED, [5])[0, :, 0], want[0])
    ctx.close()


# ------------------------------------------------------------------ 2. expansion
@gpu
def test_seeded_galois_key_expands_to_the_full_key(oracle):
    P, _ = ksm.params(oracle, *SHAPE)
    g = 5
    b, a, _ = ksm.model_galois(oracle, SHAPE, g)
    full = ksm.full_key(b, a)
    cts = random_cts(P, 3, 3, seed=31)
    want = {nl: np.stack([P.automorphism(np.ascontiguousarray(c[:, :nl]), g, full) for c in cts]) for nl in (3, 2, 1)}
    ctx = make_context(P)
    junk = _junk_key(P, 1)
    ctx.load_galois_key(g, junk)
    clone = ctx.clone()

    def run(c):
        return {nl: c.automorphism(c.upload(np.ascontiguousarray(cts[:, :, :nl])), g).download() for nl in (3, 2, 1)}

    def same(x):
        return all(np.array_equal(x[nl], want[nl]) for nl in want)

    assert not same(run(clone))
    ctx.load_galois_key(g, full)
    assert same(run(ctx))
    for montgomery in (False, True):
        ctx.load_galois_key(g, junk)
        assert not same(run(ctx))
        ctx.load_galois_key_seeded(g, km.montgomery(P, b) if montgomery else b, A_SEED, montgomery=montgomery)
        assert same(run(ctx)), montgomery
        assert same(run(clone)), montgomery  # made before the reload: it sees the replaced key
    # a full key replaces a seeded one
    ctx.load_galois_key(g, junk)
    assert not same(run(ctx))
    clone.close(), ctx.close()


@gpu
def test_seeded_relin_key_expands_to_the_full_key(oracle):
    P, _ = ksm.params(oracle, *SHAPE)
    b, a, _ = ksm.model_relin(oracle, SHAPE)
    full = ksm.full_key(b, a)
    A, B = random_cts(P, 3, 3, seed=32), random_cts(P, 3, 3, seed=33)
    cut = lambda x, nl: np.ascontiguousarray(x[:, :, :nl])  # noqa: E731
    want = {nl: mrm.mul_relin_sets(P, cut(A, nl), cut(B, nl), full) for nl in (3, 2, 1)}
    ctx = make_context(P)
    junk = _junk_key(P, 2)
    ctx.load_relin_key(junk)
    clone = ctx.clone()

    def run(c):
        return {nl: c.mul_relin(c.upload(cut(A, nl)), c.upload(cut(B, nl))).download() for nl in (3, 2, 1)}

    def same(x):
        return all(np.array_equal(x[nl], want[nl]) for nl in want)

    assert not same(run(clone))
    ctx.load_relin_key(full)
    assert same(run(ctx))
    for montgomery in (False, True):
        ctx.load_relin_key(junk)
        assert not same(run(ctx))
        ctx.load_relin_key_seeded(km.montgomery(P, b) if montgomery else b, A_SEED, montgomery=montgomery)
        assert same(run(ctx)), montgomery
        assert same(run(clone)), montgomery
    clone.close(), ctx.close()


@gpu
def test_seeded_key_first_on_a_fresh_context(oracle):
    """no full key was ever loaded for the element: the seeded loader installs the gather tables itself"""
    P, _ = ksm.params(oracle, *SHAPE)
    g = 2 * P.N - 1
    b, a, _ = ksm.model_galois(oracle, SHAPE, g)
    cts = random_cts(P, 2, 3, seed=34)
    ctx = make_context(P)
    ctx.load_galois_key_seeded(g, b, A_SEED)
    got = ctx.automorphism(ctx.upload(cts), g).download()
    assert np.array_equal(got, np.stack([P.automorphism(c, g, ksm.full_key(b, a)) for c in cts]))
    ctx.close()


# ------------------------------------------------------------------ 3. the loader at the split degree
@pytest.fixture(scope="module")
def cell15(oracle):
    """the reference-style chain of test_degree15.py: L = 3, K = 2 at N = 2^15"""
    P = make_params(oracle, 15, 3)
    ctx = make_context(P)
    yield P, ctx
    ctx.close()


@gpu
def test_seeded_loader_at_two_to_the_15(cell15):
    P, ctx = cell15
    g = ctx.galois_element(1)
    assert g == 5
    b = _junk_key(P, 3)[:, 0].copy()  # random canonical b: the key need not be valid for this comparison
    a = ksm.mask(P, A_SEED, km.ID_GALOIS + g)
    cts = random_cts(P, 2, 3, seed=35)
    s = ctx.upload(cts)
    ctx.load_galois_key_seeded(g, b, A_SEED)
    seeded = ctx.rotate_columns(s, 1).download()
    ctx.load_galois_key(g, _junk_key(P, 4))
    assert not np.array_equal(ctx.rotate_columns(s, 1).download(), seeded)
    ctx.load_galois_key(g, ksm.full_key(b, a))
    assert np.array_equal(ctx.rotate_columns(s, 1).download(), seeded)
    ctx.load_galois_key_seeded(g, km.montgomery(P, b), A_SEED, montgomery=True)
    assert np.array_equal(ctx.rotate_columns(s, 1).download(), seeded)


@gpu
def test_keygen_pair_refuses_two_to_the_15(cell15):
    P, ctx = cell15
    before = ctx.mul_counter()
    for fn in (lambda: ctx.keygen_galois_seeded(SEED, A_SEED, [5]), lambda: ctx.keygen_relin_seeded(SEED, A_SEED)):
        with pytest.raises(LumenError) as e:
            fn()
        assert "ring degree 2^15 has no kernel instantiation" in str(e.value), str(e.value)
    assert ctx.mul_counter() == before
    cts = random_cts(P, 1, 2, seed=36)
    assert np.array_equal(ctx.upload(cts).download(), cts)


# ------------------------------------------------------------------ 4. end to end
@gpu
def test_seeded_keys_drive_inner_sum(oracle):
    """secret -> seeded Galois keys -> seeded load -> InnerSum of an encrypted column -> the slot sums; no key and no
    `a` word from anywhere but the device"""
    from lumenos_amd import params as lp
    P, _ = ksm.params(oracle, *SHAPE, T=T_RS)
    n = 4
    ctx = make_context(P)
    ctx.keygen_secret(SEED, want_sk=False)
    ctx.encoder_set(lp.encoder_psi(T_RS, P.logN))
    gal = ctx.inner_sum_galois_elements(n)
    keys = ctx.keygen_galois_seeded(SEED, A_SEED, gal)
    for g, b in zip(gal, keys):
        ctx.load_galois_key_seeded(g, b, A_SEED)
    vals = np.random.default_rng(4).integers(0, T_RS, size=(1, P.N), dtype=np.uint64)
    enc = ctx.encrypt_sk_values(vals, bytes(range(40, 72)), bytes(range(50, 82)))
    dec = ctx.decrypt(ctx.inner_sum(enc, n), P.N)
    half = P.N // 2
    # slot i of a row holds the sum of slots i .. i + n - 1 of that row: every slot whose window does not wrap
    want = np.zeros(P.N, dtype=object)
    for k in range(n):
        want = want + np.roll(vals[0].astype(object), -k)
    want %= T_RS
    keep = np.concatenate([np.arange(half - n + 1), half + np.arange(half - n + 1)])
    assert keep.size == P.N - 2 * (n - 1)
    assert np.array_equal(dec[0, keep].astype(object), want[keep])
    ctx.close()


# ------------------------------------------------------------------ 5. refusals
@gpu
def test_refusals(oracle):
    P, s = ksm.params(oracle, *SHAPE)
    ctx = make_context(P)
    lib = ctx.lib
    seed, a_seed = (np.frombuffer(x, dtype=np.uint8).copy() for x in (SEED, A_SEED))
    sp, ap = seed.ctypes.data_as(_u8p), a_seed.ctypes.data_as(_u8p)
    g5 = np.array([5], dtype=np.uint64)
    gp = g5.ctypes.data_as(_u64p)
    b = np.zeros(ctx.seeded_evk_shape(), dtype=np.uint64)
    bp = b.ctypes.data_as(_u64p)
    cts = random_cts(P, 2, 3, seed=37)

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    # no generated secret on the context (a LOADED secret key is not one)
    ctx.load_secret_key(np.zeros((P.L, P.N), dtype=np.uint64))
    fails(lambda: ctx.keygen_galois_seeded(SEED, A_SEED, [5]), "no generated secret")
    fails(lambda: ctx.keygen_relin_seeded(SEED, A_SEED), "no generated secret")
    ctx.keygen_secret(SEED, want_sk=False)
    good = ctx.keygen_galois_seeded(SEED, A_SEED, [5])[0]
    ctx.load_galois_key_seeded(5, good, A_SEED)
    d = ctx.upload(cts)
    want = ctx.automorphism(d, 5).download()
    before = ctx.mul_counter()
    # equal seeds: in the words of lumen_encrypt_sk_*
    fails(lambda: ctx.keygen_galois_seeded(SEED, SEED, [5]), "the two seeds are equal (a_seed is public")
    fails(lambda: ctx.keygen_relin_seeded(A_SEED, A_SEED), "the two seeds are equal (a_seed is public")
    # NULL arguments
    assert lib.lumen_keygen_galois_seeded(None, sp, ap, gp, 1, bp, 0) != 0 and b"NULL" in lib.lumen_last_error(None)
    assert lib.lumen_keygen_relin_seeded(None, sp, ap, bp, 0) != 0 and b"NULL" in lib.lumen_last_error(None)
    assert lib.lumen_load_galois_key_seeded(None, 5, bp, ap, 0) != 0 and b"NULL" in lib.lumen_last_error(None)
    assert lib.lumen_load_relin_key_seeded(None, bp, ap, 0) != 0 and b"NULL" in lib.lumen_last_error(None)
    for call in (lambda: lib.lumen_keygen_galois_seeded(ctx.h, None, ap, gp, 1, bp, 0),
                 lambda: lib.lumen_keygen_galois_seeded(ctx.h, sp, None, gp, 1, bp, 0),
                 lambda: lib.lumen_keygen_galois_seeded(ctx.h, sp, ap, None, 1, bp, 0),
                 lambda: lib.lumen_keygen_galois_seeded(ctx.h, sp, ap, gp, 1, None, 0),
                 lambda: lib.lumen_keygen_relin_seeded(ctx.h, None, ap, bp, 0),
                 lambda: lib.lumen_keygen_relin_seeded(ctx.h, sp, None, bp, 0),
                 lambda: lib.lumen_keygen_relin_seeded(ctx.h, sp, ap, None, 0)):
        fails(lambda: ctx._ck(call()), "NULL")
    for call in (lambda: lib.lumen_load_galois_key_seeded(ctx.h, 5, None, ap, 0),
                 lambda: lib.lumen_load_galois_key_seeded(ctx.h, 5, bp, None, 0),
                 lambda: lib.lumen_load_relin_key_seeded(ctx.h, None, ap, 0),
                 lambda: lib.lumen_load_relin_key_seeded(ctx.h, bp, None, 0)):
        assert call() != 0 and b"NULL" in lib.lumen_last_error(None)
    # unknown flags
    fails(lambda: ctx._ck(lib.lumen_keygen_galois_seeded(ctx.h, sp, ap, gp, 1, bp, 2)), "unknown flags")
    fails(lambda: ctx._ck(lib.lumen_keygen_relin_seeded(ctx.h, sp, ap, bp, 6)), "unknown flags")
    fails(lambda: ctx._ck(lib.lumen_load_galois_key_seeded(ctx.h, 5, bp, ap, 2)), "unknown flags")
    fails(lambda: ctx._ck(lib.lumen_load_relin_key_seeded(ctx.h, bp, ap, 4)), "unknown flags")
    # an even element, one beyond 2N
    fails(lambda: ctx.keygen_galois_seeded(SEED, A_SEED, [5, 4]), "odd residue")
    fails(lambda: ctx.keygen_galois_seeded(SEED, A_SEED, [2 * P.N + 1]), "odd residue")
    fails(lambda: ctx.load_galois_key_seeded(4, good, A_SEED), "odd residue")
    fails(lambda: ctx.load_galois_key_seeded(2 * P.N + 1, good, A_SEED), "odd residue")
    # a b word >= q: digit and limb by name; the loaded key stays what it was
    bad = good.copy()
    bad[1, 3, 17] = P.moduli[3]
    fails(lambda: ctx.load_galois_key_seeded(5, bad, A_SEED), "key residue out of range (digit 1 limb 3)")
    fails(lambda: ctx.load_relin_key_seeded(bad, A_SEED), "key residue out of range (digit 1 limb 3)")
    # count == 0 succeeds and touches nothing
    assert lib.lumen_keygen_galois_seeded(ctx.h, sp, ap, None, 0, None, 0) == 0
    # K = 0: no key switching keys
    P0, _ = ksm.params(oracle, 10, 1, 0, T=T_RS)
    c0 = make_context(P0)
    c0.keygen_secret(SEED, want_sk=False)
    b0 = np.zeros((1, 1, P0.N), dtype=np.uint64)
    fails(lambda: c0.keygen_galois_seeded(SEED, A_SEED, [5]), "no special primes")
    fails(lambda: c0.keygen_relin_seeded(SEED, A_SEED), "no special primes")
    fails(lambda: c0._ck(lib.lumen_load_galois_key_seeded(c0.h, 5, b0.ctypes.data_as(_u64p), ap, 0)), "no special primes")
    fails(lambda: c0._ck(lib.lumen_load_relin_key_seeded(c0.h, b0.ctypes.data_as(_u64p), ap, 0)), "no special primes")
    c0.close()
    # the context goes on computing, under the key it had, and no product was counted
    assert ctx.mul_counter() == before
    assert np.array_equal(ctx.automorphism(d, 5).download(), want)
    assert np.array_equal(ctx.keygen_galois_seeded(SEED, A_SEED, [5])[0], good)
    ctx.close()
