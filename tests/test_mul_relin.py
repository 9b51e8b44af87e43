"""Ciphertext x ciphertext product with relinearisation on the device (lumen_load_relin_key, lumen_mul_relin,
lumen_mul_tensor) against tests/mul_relin_model.py -- exact Python integers for the tensor, the oracle's key_switch for
the relinearisation: bit-exact (np.array_equal) everywhere.  The relinearisation key is tests/keygen_model.py's.

Shapes: three limbs and three ciphertexts at every instantiated ring degree, on the reference-style chain and on the
chain right under the context's modulus bound (there the inputs carry rows of q - 1), with two and with one special
prime; L = 4 for the walk through every level (odd levels end in a single-limb digit) at one degree on the
LDS-resident forward transforms and at 2^14, whose forward kernels keep the limb in registers."""
import numpy as np
import pytest

import keygen_model as km
import mul_relin_model as model
from cells import KeyedCell, cell_cache
from helpers import (CHAINS, DEGREES, T_SMALL, _adversarial_cts, bound_chain, canonical, make_context, make_params,
                     random_cts)

gpu = pytest.mark.gpu

KEY_SEED = bytes(range(32))
SECRET_SEED = bytes(range(40, 72))
A_SEED = bytes([0xA5] * 32)


class _Keyed(KeyedCell):
    """Parameters, a secret, its relinearisation key and a context that holds it"""

    def __init__(self, P, seed):
        super().__init__(P, seed)
        self.rlk, _ = km.relin_key(P, KEY_SEED, self.sk)
        self.ctx.load_relin_key(self.rlk)


def _inputs(P, chain, nl, seed):
    """(a, b): three ciphertexts each.  Bound chain: rows 0 and 1 of both are the adversarial patterns (all q - 1
    against all q - 1, alternating, a spike)"""
    if chain == "bound":
        return _adversarial_cts(P, nl, seed=seed), _adversarial_cts(P, nl, seed=seed + 1)
    return random_cts(P, 3, nl, seed=seed), random_cts(P, 3, nl, seed=seed + 1)


# ------------------------------------------------------------------ every degree, two chains, K = 2 and K = 1
@gpu
@pytest.mark.parametrize("K", [2, 1])
@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("log_n", DEGREES)
def test_tensor_and_product_every_degree(oracle, log_n, chain, K):
    P = make_params(oracle, log_n, 3, num_p=K) if chain == "reference" else bound_chain(oracle, log_n, 3, K)
    assert (P.L, P.K) == (3, K)
    k = _Keyed(P, 300 + 10 * log_n + K)
    try:
        ctx = k.ctx
        a, b = _inputs(P, chain, 3, seed=7 * log_n + K)
        da, db = ctx.upload(a), ctx.upload(b)
        want_d = model.mul_tensor_sets(P, a, b)
        got_d = ctx.mul_tensor(da, db)
        assert got_d.shape == (3, 3, 3, P.N)
        assert np.array_equal(got_d, want_d)
        got = ctx.mul_relin(da, db).download()
        assert got.shape == (3, 2, 3, P.N)
        for c in range(3):
            assert np.array_equal(got[c], model.relinearise(P, want_d[c], k.rlk)), c
        assert canonical(P, got)
    finally:
        k.close()


@gpu
@pytest.mark.parametrize("log_n", [8, 14])
def test_tensor_at_the_modulus_bound(oracle, log_n):
    """Words q - 1 in both operands on the largest moduli a context takes: every product of the tensor kernel at its
    largest (the lazy T-scaled operand below 3q, two products below 6 q^2 in one reduction)"""
    P = bound_chain(oracle, log_n, 3, 2)
    ctx = make_context(P)
    try:
        a = _adversarial_cts(P, 3, seed=5)
        for l in range(3):
            a[0, :, l, :] = P.moduli[l] - 1  # both halves: a0 = a1 = q - 1
        got = ctx.mul_tensor(ctx.upload(a), ctx.upload(a))
        assert np.array_equal(got, model.mul_tensor_sets(P, a, a))
        for l in range(3):  # (q - 1)^2 = 1: d0 = d2 = T, d1 = 2T mod q
            q = P.moduli[l]
            assert (got[0, 0, l] == P.T % q).all() and (got[0, 2, l] == P.T % q).all() and (got[0, 1, l] == 2 * P.T % q).all()
    finally:
        ctx.close()


# ------------------------------------------------------------------ every level of a chain of four
class _LevelCell(_Keyed):
    def __init__(self, oracle, log_n):
        P = make_params(oracle, log_n, 4)
        assert (P.L, P.K) == (4, 2)
        super().__init__(P, 77 + log_n)
        self.a, self.b = random_cts(P, 3, 4, seed=log_n), random_cts(P, 3, 4, seed=log_n + 50)


@pytest.fixture(scope="module")
def level_cells(oracle):
    yield from cell_cache(lambda *k: _LevelCell(oracle, *k))


@gpu
@pytest.mark.parametrize("nl", [1, 2, 3, 4])
@pytest.mark.parametrize("log_n", [11, 14])
def test_every_level(level_cells, log_n, nl):
    """L = 4, K = 2: nl = 1 one single-limb digit, 2 one packed digit, 3 a packed digit and a single-limb last one,
    4 two packed digits"""
    cell = level_cells(log_n)
    P, ctx = cell.P, cell.ctx
    a, b = np.ascontiguousarray(cell.a[:, :, :nl]), np.ascontiguousarray(cell.b[:, :, :nl])
    da, db = ctx.upload(a), ctx.upload(b)
    assert np.array_equal(ctx.mul_tensor(da, db), model.mul_tensor_sets(P, a, b))
    got = ctx.mul_relin(da, db).download()
    assert got.shape == (3, 2, nl, P.N)
    assert np.array_equal(got, model.mul_relin_sets(P, a, b, cell.rlk))


# ------------------------------------------------------------------ one small shape shared by the launch-form tests
class _Small(_Keyed):
    """LogN = 10, L = 3, K = 2: five ciphertexts against five, with the model's products"""

    def __init__(self, oracle):
        P = make_params(oracle, 10, 3)
        super().__init__(P, 4242)
        self.a, self.b = random_cts(P, 5, 3, seed=1), random_cts(P, 5, 3, seed=2)
        self.want = model.mul_relin_sets(P, self.a, self.b, self.rlk)


@pytest.fixture(scope="module")
def small(oracle):
    s = _Small(oracle)
    yield s
    s.close()


@gpu
def test_forms_pairwise_broadcast_squares(small):
    P, ctx = small.P, small.ctx
    da, db = ctx.upload(small.a), ctx.upload(small.b)
    before = ctx.mul_counter()
    assert np.array_equal(ctx.mul_relin(da, db).download(), small.want)
    assert ctx.mul_counter() == before + 5
    one = ctx.upload(small.b[3:4])
    assert np.array_equal(ctx.mul_relin(da, one).download(), model.mul_relin_sets(P, small.a, small.b[3:4], small.rlk))
    before = ctx.mul_counter()
    assert np.array_equal(ctx.mul_tensor(da, one), model.mul_tensor_sets(P, small.a, small.b[3:4]))
    assert ctx.mul_counter() == before  # the parity hook counts nothing
    assert np.array_equal(ctx.mul_relin(da, da).download(), model.mul_relin_sets(P, small.a, small.a, small.rlk))
    empty = ctx.mul_relin(ctx.new_set(0, 3), one)
    assert empty.count == 0


@gpu
@pytest.mark.parametrize("settings", [{"LUMEN_KS_BATCH": 2}, {"LUMEN_KS_BATCH": 2, "LUMEN_KS_LANES": 2},
                                      {"LUMEN_KS_BATCH": 2, "LUMEN_KS_LANES": 1}, {"LUMEN_KS_LANES": 2}, {"LUMEN_KS_LANES": 1}],
                         ids=lambda s: "-".join(f"{k[9:].lower()}{v}" for k, v in s.items()))
def test_batches_and_lanes(small, settings):
    """count = 5 with LUMEN_KS_BATCH = 2: two full batches and a remainder, on one lane and alternating between two:
    the words of the default launch (one batch of five), which are the model's"""
    ctx = small.ctx
    da, db = ctx.upload(small.a), ctx.upload(small.b)
    default = ctx.mul_relin(da, db).download()
    assert np.array_equal(default, small.want)
    try:
        for name, v in settings.items():
            ctx.set_tuning(name, v)
        got = ctx.mul_relin(da, db).download()
        got_bc = ctx.mul_relin(da, ctx.upload(small.b[:1])).download()
    finally:
        ctx.set_tuning("LUMEN_KS_BATCH", 64)
        ctx.set_tuning("LUMEN_KS_LANES", 0)
    assert np.array_equal(got, default)
    assert np.array_equal(got_bc[0], default[0])


@gpu
@pytest.mark.parametrize("lanes", [1, 2])
def test_more_than_one_group_of_batches(small, lanes):
    """LUMEN_KS_BATCH = 1 on eleven ciphertexts: a group of eight batches, then a group of three, which reuses the
    first one's accumulator slices"""
    P, ctx = small.P, small.ctx
    a = np.concatenate([small.a, small.b, small.a[:1]])
    b = np.concatenate([small.b, small.a, small.b[:1]])
    da, db = ctx.upload(a), ctx.upload(b)
    default = ctx.mul_relin(da, db).download()
    try:
        ctx.set_tuning("LUMEN_KS_BATCH", 1)
        ctx.set_tuning("LUMEN_KS_LANES", lanes)
        got = ctx.mul_relin(da, db).download()
    finally:
        ctx.set_tuning("LUMEN_KS_BATCH", 64)
        ctx.set_tuning("LUMEN_KS_LANES", 0)
    assert np.array_equal(got, default)
    assert np.array_equal(got[:5], small.want) and np.array_equal(got[10], small.want[0])
    assert np.array_equal(got[5:10], model.mul_relin_sets(P, small.b, small.a, small.rlk))


@gpu
def test_batches_and_lanes_at_2_14(level_cells):
    """the same at the degree that runs one lane by default"""
    cell = level_cells(14)
    ctx = cell.ctx
    a, b = np.concatenate([cell.a, cell.b[:2]]), np.concatenate([cell.b, cell.a[:2]])
    da, db = ctx.upload(a), ctx.upload(b)
    default = ctx.mul_relin(da, db).download()
    try:
        ctx.set_tuning("LUMEN_KS_BATCH", 2)
        ctx.set_tuning("LUMEN_KS_LANES", 2)
        got = ctx.mul_relin(da, db).download()
    finally:
        ctx.set_tuning("LUMEN_KS_BATCH", 64)
        ctx.set_tuning("LUMEN_KS_LANES", 0)
    assert np.array_equal(got, default)


@gpu
def test_on_a_clone(small):
    """key loaded on the parent, product on the clone"""
    ctx = small.ctx
    clone = ctx.clone()
    try:
        got = clone.mul_relin(clone.upload(small.a), clone.upload(small.b)).download()
    finally:
        clone.close()
    assert np.array_equal(got, small.want)


@gpu
def test_key_in_montgomery_form_and_loaded_again(small):
    P = small.P
    ctx = make_context(P)
    try:
        da, db = ctx.upload(small.a), ctx.upload(small.b)
        ctx.load_relin_key(km.montgomery(P, small.rlk), montgomery=True)
        assert np.array_equal(ctx.mul_relin(da, db).download(), small.want)
        # loading again replaces the key: another key, other words; the first one back, the first words
        P.seed(99)
        other, _ = km.relin_key(P, bytes(range(1, 33)), P.keygen_secret())
        ctx.load_relin_key(other)
        assert np.array_equal(ctx.mul_relin(da, db).download(), model.mul_relin_sets(P, small.a, small.b, other))
        ctx.load_relin_key(small.rlk)
        assert np.array_equal(ctx.mul_relin(da, db).download(), small.want)
    finally:
        ctx.close()


@gpu
def test_galois_element_one_is_not_the_relinearisation_key(small):
    """lumen_load_galois_key(1, .) is accepted as before and the two keys do not see each other"""
    P = small.P
    ctx = make_context(P)
    try:
        g1 = P.keygen_galois(small.sk, 1)
        ctx.load_galois_key(1, g1)
        da, db = ctx.upload(small.a), ctx.upload(small.b)
        with pytest.raises(Exception) as e:
            ctx.mul_relin(da, db)
        assert "no relinearisation key" in str(e.value)
        ctx.load_relin_key(small.rlk)
        ctx.load_galois_key(1, g1)
        assert np.array_equal(ctx.mul_relin(da, db).download(), small.want)
    finally:
        ctx.close()


# ------------------------------------------------------------------ coexistence with InnerSum on one context
@gpu
@pytest.mark.parametrize("first", ["mul_relin", "inner_sum"])
def test_coexists_with_inner_sum(small, first):
    """One fresh context, both orders, at level 2 and at the top: shared scratch, per-level tables, placement"""
    P = small.P
    n = 16
    gl = P.inner_sum_galois_elements(n)
    evks = [P.keygen_galois(small.sk, g) for g in gl]
    ctx = make_context(P)
    try:
        for g, e in zip(gl, evks):
            ctx.load_galois_key(g, e)
        ctx.load_relin_key(small.rlk)
        for nl in (2, 3):
            a, b = np.ascontiguousarray(small.a[:, :, :nl]), np.ascontiguousarray(small.b[:, :, :nl])
            da, db = ctx.upload(a), ctx.upload(b)
            want_mul = small.want if nl == 3 else model.mul_relin_sets(P, a, b, small.rlk)
            want_sum = np.stack([P.inner_sum(c, n, evks) for c in a])
            steps = [lambda: np.array_equal(ctx.mul_relin(da, db).download(), want_mul),
                     lambda: np.array_equal(ctx.inner_sum_at_level(da, n).download(), want_sum)]
            if first == "inner_sum":
                steps.reverse()
            for step in steps + steps[:1]:
                assert step(), nl
    finally:
        ctx.close()


# ------------------------------------------------------------------ end to end, no CPU-generated key anywhere
@gpu
def test_end_to_end_device_keys(oracle):
    """lumen_keygen_* -> encrypt_sk_values of two columns -> mul_relin -> rescale to level 1 -> lumen_decrypt at the
    product scale = the slot-wise product (T = 0x3ee0001, LogN = 12, L = 3: T^2 N B fits two limbs)"""
    from lumenos_amd import params as lp
    P = make_params(oracle, 12, 3, T=T_SMALL)
    ctx = make_context(P)
    try:
        ctx.encoder_set(lp.encoder_psi(T_SMALL, P.logN))
        ctx.keygen_secret(KEY_SEED, want_sk=False)
        ctx.load_relin_key(ctx.keygen_relin(KEY_SEED))
        rng = np.random.default_rng(12)
        x = rng.integers(0, T_SMALL, size=(2, P.N), dtype=np.uint64)
        y = rng.integers(0, T_SMALL, size=(2, P.N), dtype=np.uint64)
        ca = ctx.encrypt_sk_values(x, SECRET_SEED, A_SEED, 0)
        cb = ctx.encrypt_sk_values(y, SECRET_SEED, A_SEED, 2)
        prod = ctx.rescale(ctx.mul_relin(ca, cb), 2)
        scale = P.rescale_scale(3, 2)  # 1 * 1 from the operands, q_2^-1 from the rescale
        got = ctx.decrypt(prod, P.N, scale=scale)
        want = np.array([[int(u) * int(v) % T_SMALL for u, v in zip(x[i], y[i])] for i in range(2)], dtype=np.uint64)
        assert np.array_equal(got, want)
        sq = ctx.decrypt(ctx.rescale(ctx.mul_relin(ca, ca), 2), P.N, scale=scale)
        assert np.array_equal(sq, np.array([[int(u) * int(u) % T_SMALL for u in x[i]] for i in range(2)], dtype=np.uint64))
    finally:
        ctx.close()


# ------------------------------------------------------------------ refusals
@gpu
def test_refusals(oracle, small):
    import ctypes as C
    from lumenos_amd.hip import LumenError
    P, ctx = small.P, small.ctx
    lib = ctx.lib

    def fails(fn, text):
        with pytest.raises(LumenError) as e:
            fn()
        assert text in str(e.value), str(e.value)

    def last(rc, text, c=None):
        assert rc != 0
        msg = lib.lumen_last_error(c).decode()
        assert text in msg, msg

    da, db = ctx.upload(small.a), ctx.upload(small.b)
    h = C.c_void_p()
    out3 = np.zeros((5, 3, 3, P.N), dtype=np.uint64)
    p64 = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint64))
    # NULL arguments
    last(lib.lumen_mul_relin(ctx.h, da.h, None, C.byref(h)), "NULL argument")
    last(lib.lumen_mul_relin(ctx.h, da.h, db.h, None), "NULL argument")
    last(lib.lumen_mul_relin(None, da.h, db.h, C.byref(h)), "NULL argument")
    last(lib.lumen_mul_tensor(ctx.h, da.h, db.h, None), "NULL argument")
    last(lib.lumen_mul_tensor(ctx.h, None, db.h, p64(out3)), "NULL argument")
    last(lib.lumen_load_relin_key(ctx.h, None, 0), "NULL argument")
    last(lib.lumen_load_relin_key(None, p64(small.rlk), 0), "NULL argument")
    # unknown flags
    last(lib.lumen_load_relin_key(ctx.h, p64(small.rlk), 2), "unknown flags", ctx.h)
    # a key residue out of range, like a Galois key's
    bad = small.rlk.copy()
    bad[1, 0, 2, 5] = P.moduli[2]
    fails(lambda: ctx.load_relin_key(bad), "out of range")
    # different levels, count mismatch
    d2 = ctx.upload(np.ascontiguousarray(small.b[:, :, :2]))
    fails(lambda: ctx.mul_relin(da, d2), "different levels")
    fails(lambda: ctx.mul_tensor(da, d2), "different levels")
    fails(lambda: ctx.mul_relin(da, ctx.upload(small.b[:2])), "count mismatch")
    fails(lambda: ctx.mul_tensor(da, ctx.upload(small.b[:4])), "count mismatch")
    fails(lambda: ctx.mul_relin(ctx.upload(small.a[:1]), db), "count mismatch")
    # a lane-sharded set, on either side
    lanes = ctx.upload_lanes(np.ascontiguousarray(small.a[..., :P.N // 2]), 1)
    fails(lambda: ctx.mul_relin(lanes, db), "lane-sharded")
    fails(lambda: ctx.mul_relin(da, lanes), "lane-sharded")
    fails(lambda: ctx.mul_tensor(lanes, lanes), "lane-sharded")
    # a set with more limbs than the chain
    P2 = make_params(oracle, 10, 2)
    short = make_context(P2)
    try:
        fails(lambda: short.mul_relin(da, db), "the chain has 2")
        # no relinearisation key loaded
        s2 = short.upload(random_cts(P2, 2, 2, seed=3))
        fails(lambda: short.mul_relin(s2, s2), "no relinearisation key")
    finally:
        short.close()
    # no special primes; three of them (as InnerSum refuses them)
    P0 = make_params(oracle, 10, 2, num_p=0)
    c0 = make_context(P0)
    try:
        s0 = c0.upload(random_cts(P0, 1, 2, seed=4))
        fails(lambda: c0.mul_relin(s0, s0), "no special primes")
        last(lib.lumen_load_relin_key(c0.h, p64(small.rlk), 0), "no special primes", c0.h)
        assert c0.mul_tensor(s0, s0).shape == (1, 3, 2, P0.N)  # the tensor needs no key and no special prime
    finally:
        c0.close()
    P3 = make_params(oracle, 10, 3, num_p=3)
    c3 = make_context(P3)
    try:
        s3 = c3.upload(random_cts(P3, 1, 3, seed=5))
        fails(lambda: c3.mul_relin(s3, s3), "1 or 2 special primes")
    finally:
        c3.close()
    # and after the refusals the context still computes
    assert np.array_equal(ctx.mul_relin(da, db).download(), small.want)
