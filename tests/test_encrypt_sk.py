"""Secret-key encryption and seeded ciphertexts (lumen_encrypt_sk_values / _seeded, lumen_ct_expand_seeded): every word
against the Python restatement of the contract (encrypt_sk_model.py), the seeded form and its expansion, chunking,
the round trip through the decryptors and the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import encrypt_sk_model as em
import keygen_model as km
from helpers import T_REF, make_context, make_params
from lumenos_amd.hip import SYMBOLS

KEY_SEED = bytes(range(32))             # the secret key's (keygen) seed
SECRET_SEED = bytes(range(40, 72))      # the encryptor's error seed: key material
A_SEEDS = [bytes([0xA0 + t] * 32) for t in range(8)]  # candidates for the public seed
FIRST = (1 << 32) + 3                   # both nonce words of the sample index are non-zero
SHAPES = [(logn, L, K) for logn in (8, 10, 12) for (L, K) in ((1, 0), (3, 2), (4, 2))]
SINGLES = [(11, 3, 2), (13, 2, 1), (14, 2, 1)]  # the other instantiated ring degrees, once each
_cache = {}


def _count(shape):
    return 5 if shape in SHAPES else 2


def _params(oracle, shape):
    """one parameter set, its model secret and its witness per shape, shared by the tests and never modified"""
    if shape not in _cache:
        P = make_params(oracle, shape[0], shape[1], num_p=shape[2])
        vals = np.random.default_rng(sum(shape)).integers(0, T_REF, size=(_count(shape), P.N), dtype=np.uint64)
        _cache[shape] = (P, km.secret(P, KEY_SEED), vals)
    return _cache[shape]


def _redraw_possible(P):
    """A limb q_l redraws a word with probability (2^64 mod q_l) / 2^64.  The 58-bit prime the reference's generator
    finds at logN 8 and 10 lies so closely below 2^58 that this is 2^-44: no seed a search can try has a redraw in
    the few thousand words of a one-limb case, and the assertion is dropped exactly there (2^-30 and below)."""
    return any(((1 << 64) % q) >> 34 for q in P.moduli[:P.L])


def _model(oracle, shape):
    """the zero-plaintext halves of the shape's ciphertexts under the first candidate seed whose masks contain a
    redrawn coefficient: (a_seed, [(base, a, e, redraws)] per ciphertext)"""
    key = ("model",) + shape
    if key not in _cache:
        P, s, _ = _params(oracle, shape)
        n = _count(shape)
        seed = A_SEEDS[0]
        for cand in A_SEEDS:
            if sum(sum(rd) for i in range(n) for rd in em.mask(P, cand, FIRST + i)[1]):
                seed = cand
                break
        _cache[key] = (seed, [em.zero_encryption(P, s, SECRET_SEED, seed, FIRST + i) for i in range(n)])
    return _cache[key]


def _model_cts(oracle, shape, rows):
    P, _, vals = _params(oracle, shape)
    seed, parts = _model(oracle, shape)
    return seed, np.stack([em.add_plaintext(P, base, a, vals[i, :rows]) for i, (base, a, _, _) in enumerate(parts)])


def _redraws(parts):
    return sum(sum(rd) for _, _, _, rds in parts for rd in rds)


def _client(P, s, generated=False):
    from lumenos_amd import params as lp
    ctx = make_context(P)
    if generated:
        ctx.keygen_secret(KEY_SEED, want_sk=False)
    else:
        ctx.load_secret_key(s)
    ctx.encoder_set(lp.encoder_psi(T_REF, P.logN))
    return ctx


# ------------------------------------------------------------------ CPU: the model alone
def test_header_states_the_contract_and_binding_has_the_entry_points():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lumenos_hip.h")).read()
    for name in ("lumen_encrypt_sk_values", "lumen_encrypt_sk_seeded", "lumen_ct_expand_seeded"):
        assert name in SYMBOLS and re.search(r"\bint " + name + r"\(", hdr), name
    assert "#define LUMEN_ABI_VERSION 4" in hdr  # new symbols only
    flat = " ".join(hdr.split())
    for phrase in ("fhe/bfv.go:77", "stream 3", "stream 16 + l", "x < 2^64 - (2^64 mod q_l)", "equal seeds are refused",
                   "MUST NOT encrypt two messages", "count == 0 succeeds and touches nothing"):
        assert phrase in flat, phrase


@pytest.mark.parametrize("shape", [(8, 1, 0), (10, 3, 2)])
def test_model_decrypts_and_its_noise_is_the_error(oracle, shape):
    """The model's ciphertexts decrypt under the oracle to the values, and INTT(c0 + c1 * s) - pt is exactly e.  (One
    58-bit limb is no room for a 57-bit T times any noise: the one-limb shape is there for the second property.)"""
    P, s, vals = _params(oracle, shape)
    _, parts = _model(oracle, shape)
    for rows in (1, P.N // 2 + 1, P.N) if P.L > 1 else ():
        _, cts = _model_cts(oracle, shape, rows)
        for i, ct in enumerate(cts):
            assert np.array_equal(P.decrypt(s, ct, rows), vals[i, :rows]), (rows, i)
    _, cts = _model_cts(oracle, shape, P.N)
    for i, ct in enumerate(cts):
        pt = P.encode(vals[i])
        e = parts[i][2].astype(np.int64)
        assert np.abs(e).max() <= 19 and np.abs(e).max() >= 1
        for l in range(P.L):
            q = P.moduli[l]
            ph = np.array([(int(c0) + int(c1) * int(x) - int(p)) % q for c0, c1, x, p in zip(ct[0, l], ct[1, l], s[l], pt[l])],
                          dtype=np.uint64)
            got = P.limb_intt(ph, l).astype(object)
            got = np.where(got > q // 2, got - q, got).astype(np.int64)
            assert np.array_equal(got, e), (i, l)


def test_model_two_public_seeds(oracle):
    """two a_seeds: different c1 (and c0), the same decryption"""
    shape = (8, 3, 2)
    P, s, vals = _params(oracle, shape)
    x, _, _ = em.encrypt(P, s, vals[:2], SECRET_SEED, A_SEEDS[0], FIRST)
    y, _, _ = em.encrypt(P, s, vals[:2], SECRET_SEED, A_SEEDS[1], FIRST)
    for i in range(2):
        assert not np.array_equal(x[i, 1], y[i, 1]) and not np.array_equal(x[i, 0], y[i, 0])
        assert np.array_equal(P.decrypt(s, x[i], P.N), vals[i]) and np.array_equal(P.decrypt(s, y[i], P.N), vals[i])


@pytest.mark.parametrize("shape", SHAPES + SINGLES)
def test_model_vectors_contain_redraws(oracle, shape):
    """The rejection sampler's redraw path cannot go untested: the data every GPU case compares contain a redrawn
    coefficient wherever one can exist (_redraw_possible)."""
    P, _, _ = _params(oracle, shape)
    n = _redraws(_model(oracle, shape)[1])
    print(shape, "redrawn coefficients:", n)
    assert n >= 1 or not _redraw_possible(P), shape
    assert _redraw_possible(P) or (shape[1] == 1 and shape[0] in (8, 10))


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("rows_kind", ["one", "second_row", "full"])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_word_matches_model(oracle, shape, rows_kind):
    P, s, vals = _params(oracle, shape)
    rows = {"one": 1, "second_row": P.N // 2 + 1, "full": P.N}[rows_kind]
    a_seed, want = _model_cts(oracle, shape, rows)
    assert _redraws(_model(oracle, shape)[1]) >= 1 or not _redraw_possible(P)
    ctx = _client(P, s)
    got = ctx.encrypt_sk_values(vals[:, :rows], SECRET_SEED, a_seed, FIRST).download()
    assert got.shape == want.shape == (5, 2, P.L, P.N)
    assert np.array_equal(got[:, 1], want[:, 1]), "c1"
    assert np.array_equal(got[:, 0], want[:, 0]), "c0"
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SINGLES)
def test_every_ring_degree_matches_model(oracle, shape):
    P, s, vals = _params(oracle, shape)
    a_seed, want = _model_cts(oracle, shape, P.N)
    assert _redraws(_model(oracle, shape)[1]) >= 1
    ctx = _client(P, s)
    got = ctx.encrypt_sk_values(vals, SECRET_SEED, a_seed, FIRST).download()
    assert np.array_equal(got[:, 1], want[:, 1]), "c1"
    assert np.array_equal(got[:, 0], want[:, 0]), "c0"
    ctx.close()


@pytest.mark.gpu
def test_seeded_form_and_expansion(oracle):
    """lumen_encrypt_sk_seeded = set[:, 0]; lumen_ct_expand_seeded on a fresh context with no key = the full set; from
    pageable and from page-locked memory."""
    from lumenos_amd.hip import pinned_empty, pinned_free
    shape = (10, 3, 2)
    P, s, vals = _params(oracle, shape)
    a_seed, want = _model_cts(oracle, shape, P.N)
    ctx = _client(P, s)
    full = ctx.encrypt_sk_values(vals, SECRET_SEED, a_seed, FIRST).download()
    assert np.array_equal(full, want)
    c0 = ctx.encrypt_sk_seeded(vals, SECRET_SEED, a_seed, FIRST)
    pin = pinned_empty(c0.shape)
    assert ctx.encrypt_sk_seeded(vals, SECRET_SEED, a_seed, FIRST, out=pin) is pin
    assert np.array_equal(c0, full[:, 0]) and np.array_equal(pin, full[:, 0])
    server = make_context(P)  # no key, no encoder tables
    assert np.array_equal(server.expand_seeded(c0, a_seed, FIRST).download(), full)
    assert np.array_equal(server.expand_seeded(pin, a_seed, FIRST).download(), full)
    # one at a time, out of order: the same bits
    for i in (4, 0, 2):
        assert np.array_equal(server.expand_seeded(np.ascontiguousarray(c0[i:i + 1]), a_seed, FIRST + i).download()[0], full[i])
    pinned_free(pin)
    server.close(), ctx.close()


@pytest.mark.gpu
def test_seeded_form_through_the_bounce_buffers(oracle):
    """40 ciphertexts at (12, 3, 2): 3.9 MB of c0, so a pageable buffer takes the chunked path in both directions."""
    from lumenos_amd.hip import pinned_empty, pinned_free
    shape, n = (12, 3, 2), 40
    P, s, _ = _params(oracle, shape)
    vals = np.random.default_rng(40).integers(0, T_REF, size=(n, 7), dtype=np.uint64)
    a_seed = A_SEEDS[3]
    ctx = _client(P, s)
    full = ctx.encrypt_sk_values(vals, SECRET_SEED, a_seed, 0).download()
    c0 = ctx.encrypt_sk_seeded(vals, SECRET_SEED, a_seed, 0)
    assert c0.nbytes > 1 << 20 and np.array_equal(c0, full[:, 0])
    pin = pinned_empty(c0.shape)
    ctx.encrypt_sk_seeded(vals, SECRET_SEED, a_seed, 0, out=pin)
    assert np.array_equal(pin, c0)
    for i in (0, n - 1):
        want, _, _ = em.encrypt(P, s, vals[i:i + 1], SECRET_SEED, a_seed, i)
        assert np.array_equal(full[i], want[0]), i
    server = make_context(P)
    assert np.array_equal(server.expand_seeded(c0, a_seed, 0).download(), full)
    assert np.array_equal(server.expand_seeded(pin, a_seed, 0).download(), full)
    pinned_free(pin)
    server.close(), ctx.close()


@pytest.mark.gpu
def test_chunk_boundary(oracle):
    """257 ciphertexts cross the 256-ciphertext chunk: 0, 255 and 256 equal single calls, and all of them decrypt"""
    shape, n = (8, 3, 2), 257
    P, s, _ = _params(oracle, shape)
    vals = np.random.default_rng(257).integers(0, T_REF, size=(n, P.N), dtype=np.uint64)
    a_seed = A_SEEDS[2]
    ctx = _client(P, s)
    cts = ctx.encrypt_sk_values(vals, SECRET_SEED, a_seed, FIRST)
    got = cts.download()
    for i in (0, 255, 256):
        one = ctx.encrypt_sk_values(vals[i:i + 1], SECRET_SEED, a_seed, FIRST + i).download()
        assert np.array_equal(one[0], got[i]), i
    want, _, _ = em.encrypt(P, s, vals[255:], SECRET_SEED, a_seed, FIRST + 255)
    assert np.array_equal(got[255:], want)
    assert np.array_equal(ctx.decrypt(cts, P.N), vals)
    c0 = ctx.encrypt_sk_seeded(vals, SECRET_SEED, a_seed, FIRST)
    assert np.array_equal(c0, got[:, 0])
    server = make_context(P)
    assert np.array_equal(server.expand_seeded(c0, a_seed, FIRST).download(), got)
    server.close(), ctx.close()


@pytest.mark.gpu
def test_index_carries_into_the_second_nonce_word(oracle):
    """three ciphertexts from sample index 2^32 - 2: the index crosses 2^32 inside one call.  Every word of the full
    form equals the model, the seeded form is its c0 halves, and a key-less context rebuilds the set."""
    shape, first = (8, 3, 2), (1 << 32) - 2
    P, s, vals = _params(oracle, shape)
    v, a_seed = vals[:3], A_SEEDS[1]
    want, _, _ = em.encrypt(P, s, v, SECRET_SEED, a_seed, first)
    ctx = _client(P, s)
    full = ctx.encrypt_sk_values(v, SECRET_SEED, a_seed, first).download()
    assert np.array_equal(full[:, 1], want[:, 1]), "c1"
    assert np.array_equal(full[:, 0], want[:, 0]), "c0"
    c0 = ctx.encrypt_sk_seeded(v, SECRET_SEED, a_seed, first)
    assert np.array_equal(c0, full[:, 0])
    server = make_context(P)  # no key, no encoder tables
    assert np.array_equal(server.expand_seeded(c0, a_seed, first).download(), full)
    server.close(), ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("generated", [False, True])
def test_round_trip(oracle, generated):
    """lumen_decrypt returns the values under a loaded and under a generated key; the oracle's decryptor agrees"""
    shape = (10, 3, 2)
    P, s, vals = _params(oracle, shape)
    ctx = _client(P, s, generated)
    for rows in (1, P.N // 2 + 1, P.N):
        cts = ctx.encrypt_sk_values(vals[:, :rows], SECRET_SEED, A_SEEDS[1], 7)
        assert np.array_equal(ctx.decrypt(cts, rows), vals[:, :rows]), rows
        assert np.array_equal(P.decrypt_batch(s, cts.download(), rows), vals[:, :rows]), rows
    # a clone shares the key and encrypts to the same bits
    cl = ctx.clone()
    assert np.array_equal(cl.encrypt_sk_values(vals, SECRET_SEED, A_SEEDS[1], 7).download(),
                          ctx.encrypt_sk_values(vals, SECRET_SEED, A_SEEDS[1], 7).download())
    cl.close(), ctx.close()


@pytest.mark.gpu
def test_refusals(oracle):
    from lumenos_amd import params as lp
    from lumenos_amd.hip import LumenError
    P, s, vals = _params(oracle, (10, 3, 2))
    u8p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    ss, sa = (np.frombuffer(x, dtype=np.uint8).copy() for x in (SECRET_SEED, A_SEEDS[0]))
    sp, ap = ss.ctypes.data_as(u8p), sa.ctypes.data_as(u8p)
    v = np.ascontiguousarray(vals[:2])
    vp = v.ctypes.data_as(u64p)
    c0 = np.zeros((2, P.L, P.N), dtype=np.uint64)
    cp = c0.ctypes.data_as(u64p)

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    ctx = make_context(P)
    lib = ctx.lib
    h = C.c_void_p()
    # no secret key, then no encoder tables
    fails(lambda: ctx.encrypt_sk_values(v, SECRET_SEED, A_SEEDS[0]), "no secret key")
    fails(lambda: ctx.encrypt_sk_seeded(v, SECRET_SEED, A_SEEDS[0]), "no secret key")
    ctx.load_secret_key(s)
    fails(lambda: ctx.encrypt_sk_values(v, SECRET_SEED, A_SEEDS[0]), "no encoder tables")
    fails(lambda: ctx.encrypt_sk_seeded(v, SECRET_SEED, A_SEEDS[0]), "no encoder tables")
    ctx.encoder_set(lp.encoder_psi(T_REF, P.logN))
    # NULL ctx / values / seeds / output
    assert lib.lumen_encrypt_sk_values(None, vp, P.N, 2, sp, ap, 0, C.byref(h)) != 0 and b"NULL" in lib.lumen_last_error(None)
    assert lib.lumen_encrypt_sk_seeded(None, vp, P.N, 2, sp, ap, 0, cp) != 0 and b"NULL" in lib.lumen_last_error(None)
    assert lib.lumen_ct_expand_seeded(None, cp, 2, ap, 0, C.byref(h)) != 0 and b"NULL" in lib.lumen_last_error(None)
    for args in ((None, P.N, 2, sp, ap, 0, C.byref(h)), (vp, P.N, 2, None, ap, 0, C.byref(h)), (vp, P.N, 2, sp, None, 0, C.byref(h)),
                 (vp, P.N, 2, sp, ap, 0, None)):
        fails(lambda: ctx._ck(lib.lumen_encrypt_sk_values(ctx.h, *args)), "NULL")
    for args in ((None, P.N, 2, sp, ap, 0, cp), (vp, P.N, 2, None, ap, 0, cp), (vp, P.N, 2, sp, None, 0, cp),
                 (vp, P.N, 2, sp, ap, 0, None)):
        fails(lambda: ctx._ck(lib.lumen_encrypt_sk_seeded(ctx.h, *args)), "NULL")
    for args in ((None, 2, ap, 0, C.byref(h)), (cp, 2, None, 0, C.byref(h)), (cp, 2, ap, 0, None)):
        fails(lambda: ctx._ck(lib.lumen_ct_expand_seeded(ctx.h, *args)), "NULL")
    # rows outside [1, N]
    for rows in (0, P.N + 1):
        fails(lambda: ctx._ck(lib.lumen_encrypt_sk_values(ctx.h, vp, rows, 1, sp, ap, 0, C.byref(h))), "out of range [1, N]")
        fails(lambda: ctx._ck(lib.lumen_encrypt_sk_seeded(ctx.h, vp, rows, 1, sp, ap, 0, cp)), "out of range [1, N]")
    # the public seed must not be the secret one
    fails(lambda: ctx.encrypt_sk_values(v, SECRET_SEED, SECRET_SEED), "two seeds are equal")
    fails(lambda: ctx.encrypt_sk_seeded(v, SECRET_SEED, SECRET_SEED), "two seeds are equal")
    # count == 0 succeeds and touches nothing
    empty = ctx.encrypt_sk_values(np.zeros((0, P.N), dtype=np.uint64), SECRET_SEED, A_SEEDS[0])
    assert empty.count == 0 and empty.nl == P.L
    assert lib.lumen_encrypt_sk_seeded(ctx.h, None, P.N, 0, sp, ap, 0, None) == 0
    assert ctx.expand_seeded(np.zeros((0, P.L, P.N), dtype=np.uint64), A_SEEDS[0]).count == 0
    # the context stays usable
    assert np.array_equal(ctx.decrypt(ctx.encrypt_sk_values(v, SECRET_SEED, A_SEEDS[0]), P.N), v)
    ctx.close()
