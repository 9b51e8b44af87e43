"""CPU: the model of the ciphertext x ciphertext product (tests/mul_relin_model.py) is the product.  Its output is
decrypted by the oracle and compared with the slot-wise product of the two encoded vectors; that decryption -- not the
device, not lo_mul_plain -- is what pins the factor T of the tensor.

LogN = 10, L = 3, with K = 2 and with K = 1 special primes, every level nl = 1..3, two plaintext moduli.

WHICH (T, nl) CELLS ARE DECRYPTED.  A ciphertext's phase is m T^-1 + e, so the product's is
T^-1 m_a m_b + m_a e_b + m_b e_a + T e_a e_b (+ the key switch's few bits): noise about T N B for plaintext coefficients
below T and input noise B, and decoding multiplies the phase by T.  It decrypts where T^2 N B < Q_nl / 2.  With N = 2^10
and B < 2^6 (a fresh public-key encryption after its division by P):
    T = 0x3ee0001 (26 bits): 2^68  -- under Q_2 (2^114) and Q_3 (2^170), over Q_1 (2^58): nl = 2, 3 are decrypted;
    T = T_REF (57 bits):     2^130 -- under Q_3 only: nl = 3 is decrypted.
The other three cells are left out for that budget alone: there the test asserts that the model's output does NOT
decrypt to the product (the excess is 2^10 and more), and the pairwise and broadcast forms are still compared with each
other (squares are checked by their decryption, so only where that succeeds).  For either K, three of the six cells decrypt."""
import numpy as np
import pytest

import keygen_model as km
import mul_relin_model as model
from helpers import T_REF, T_SMALL, make_params

LOG_N, L = 10, 3
DECRYPTS = {(T_SMALL, 2), (T_SMALL, 3), (T_REF, 3)}
SEED = bytes(range(40, 72))


class _Cell:
    def __init__(self, oracle, K, T):
        self.P = P = make_params(oracle, LOG_N, L, num_p=K, T=T)
        assert (P.L, P.K) == (L, K)
        P.seed(7 * K + T % 1000)
        self.sk = P.keygen_secret()
        self.pk = P.keygen_public(self.sk)
        self.rlk, _ = km.relin_key(P, SEED, self.sk)
        rng = np.random.default_rng(K)
        self.x = rng.integers(0, T, size=(3, P.N), dtype=np.uint64)
        self.y = rng.integers(0, T, size=(3, P.N), dtype=np.uint64)
        self.A = np.stack([P.encrypt(self.pk, P.encode(v)) for v in self.x])
        self.B = np.stack([P.encrypt(self.pk, P.encode(v)) for v in self.y])

    def at(self, cts, nl):
        """the first nl limbs: the same ciphertexts at a lower level, scale unchanged"""
        return np.ascontiguousarray(cts[:, :, :nl])

    def product(self, x, y):
        return np.array([int(a) * int(b) % self.P.T for a, b in zip(x, y)], dtype=np.uint64)


@pytest.fixture(scope="module")
def cells(oracle):
    made = {}

    def get(K, T):
        if (K, T) not in made:
            made[K, T] = _Cell(oracle, K, T)
        return made[K, T]

    return get


CASES = [(K, T, nl) for K in (2, 1) for T in (T_SMALL, T_REF) for nl in (1, 2, 3)]


@pytest.mark.parametrize("K,T,nl", CASES, ids=[f"K{K}-T{T.bit_length()}-nl{nl}" for K, T, nl in CASES])
def test_model_decrypts_to_the_product(cells, K, T, nl):
    c = cells(K, T)
    P = c.P
    A, B = c.at(c.A, nl), c.at(c.B, nl)
    got = model.mul_relin_sets(P, A, B, c.rlk)
    assert got.shape == (3, 2, nl, P.N)
    assert all(int(got[:, :, l].max()) < P.moduli[l] for l in range(nl))
    # the forms agree: one ciphertext of B broadcast against the pairwise form
    bc = model.mul_relin_sets(P, A, B[1:2], c.rlk)
    assert np.array_equal(bc[1], got[1])
    assert np.array_equal(bc, model.mul_relin_sets(P, A, np.repeat(B[1:2], 3, axis=0), c.rlk))
    if (T, nl) not in DECRYPTS:
        # the budget (module docstring): T^2 N B is over Q_nl / 2 by at least 2^10 in this cell, so the phase wraps and
        # the decoded slots are no product -- the cell is left out because of the noise, not because of the model
        assert not np.array_equal(P.decrypt(c.sk, got[0], P.N, scale=1), c.product(c.x[0], c.y[0]))
        return
    sq = model.mul_relin_sets(P, A, A, c.rlk)  # squares: the same array as both operands
    for i in range(3):
        assert np.array_equal(P.decrypt(c.sk, got[i], P.N, scale=1), c.product(c.x[i], c.y[i])), i
        assert np.array_equal(P.decrypt(c.sk, bc[i], P.N, scale=1), c.product(c.x[i], c.y[1])), i
        assert np.array_equal(P.decrypt(c.sk, sq[i], P.N, scale=1), c.product(c.x[i], c.x[i])), i


@pytest.mark.parametrize("K", [2, 1])
def test_without_the_factor_T_the_same_cell_does_not_decrypt(cells, K):
    """The contract's T: the same cell, the same inputs, the tensor without it -- the phase is then T^-2 m_a m_b + ...,
    a full-size residue after decoding"""
    c = cells(K, T_SMALL)
    P = c.P
    a, b = c.at(c.A, 2)[0], c.at(c.B, 2)[0]
    want = c.product(c.x[0], c.y[0])
    assert np.array_equal(P.decrypt(c.sk, model.mul_relin(P, a, b, c.rlk), P.N), want)
    assert not np.array_equal(P.decrypt(c.sk, model.mul_relin(P, a, b, c.rlk, t_factor=False), P.N), want)


@pytest.mark.parametrize("K", [2, 1])
def test_scale_of_the_product_is_the_product_of_the_scales(cells, K):
    """Both operands rescaled 3 -> 2 limbs (scale q_2^-1 mod T each): the product decrypts at scale_a * scale_b mod T and
    at no other"""
    c = cells(K, T_SMALL)
    P = c.P
    a, b = P.rescale(c.A[0]), P.rescale(c.B[0])
    s = P.rescale_scale(3, 2)
    assert s != 1
    got = model.mul_relin(P, a, b, c.rlk)
    want = c.product(c.x[0], c.y[0])
    assert np.array_equal(P.decrypt(c.sk, got, P.N, scale=s * s % P.T), want)
    assert not np.array_equal(P.decrypt(c.sk, got, P.N, scale=s), want)


def test_tensor_is_degree_two_under_the_secret(cells):
    """d0 + d1 s + d2 s^2 = T (a0 + a1 s)(b0 + b1 s), limb by limb: the tensor alone, before any key"""
    c = cells(2, T_SMALL)
    P = c.P
    a, b = c.A[0], c.B[0]
    d = model.tensor(P, a, b)
    for l in range(L):
        q, s = P.moduli[l], c.sk[l].astype(object)
        lhs = (d[0, l].astype(object) + d[1, l].astype(object) * s + d[2, l].astype(object) * s * s) % q
        rhs = (P.T % q) * (a[0, l].astype(object) + a[1, l].astype(object) * s) * (b[0, l].astype(object) + b[1, l].astype(object) * s) % q
        assert np.array_equal(lhs, rhs), l
