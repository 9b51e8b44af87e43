"""CPU: the model of the dot product with one relinearisation per sum (tests/mul_relin_dot_model.py) is the dot product.
The oracle decrypts its output to sum_i x_e o y_e mod T slot-wise; for n = 1 it is tests/mul_relin_model.mul_relin word
for word; for n >= 2 its words differ from the sum of n separate mul_relin results while both decrypt alike: the model
tells one key switch from n.

LogN = 10, L = 3, K = 2 and K = 1, T = 0x3ee0001.  THE BUDGET: a product's noise is about T^2 N B (tests/
test_mul_relin_model.py: 2^68 here), a sum of n of them n times that, 2^70 for n = 3 and under 2^71 for n = 4 -- far under
Q_3 / 2 (2^169) and Q_2 / 2 (2^113), which are the two levels decrypted; at one limb (Q_1 = 2^58) nothing decrypts, as in
that file."""
import numpy as np
import pytest

import keygen_model as km
import mul_relin_dot_model as model
import mul_relin_model as mr
from helpers import T_SMALL, make_params

LOG_N, L, GROUPS, N_TERMS = 10, 3, 2, 3
SEED = bytes(range(40, 72))


class _Cell:
    def __init__(self, oracle, K):
        self.P = P = make_params(oracle, LOG_N, L, num_p=K, T=T_SMALL)
        assert (P.L, P.K) == (L, K)
        P.seed(31 * K)
        self.sk = P.keygen_secret()
        self.pk = P.keygen_public(self.sk)
        self.rlk, _ = km.relin_key(P, SEED, self.sk)
        rng = np.random.default_rng(100 + K)
        self.x = rng.integers(0, T_SMALL, size=(GROUPS * N_TERMS, P.N), dtype=np.uint64)
        self.y = rng.integers(0, T_SMALL, size=(GROUPS * N_TERMS, P.N), dtype=np.uint64)
        self.A = np.stack([P.encrypt(self.pk, P.encode(v)) for v in self.x])
        self.B = np.stack([P.encrypt(self.pk, P.encode(v)) for v in self.y])

    def dot(self, x, y):
        """slot-wise sum_i x[i] o y[i] mod T"""
        return np.array([sum(int(u) * int(v) for u, v in zip(col_x, col_y)) % T_SMALL for col_x, col_y in zip(x.T, y.T)],
                        dtype=np.uint64)


@pytest.fixture(scope="module")
def cells(oracle):
    made = {}

    def get(K):
        if K not in made:
            made[K] = _Cell(oracle, K)
        return made[K]

    return get


def _add(P, cts):
    """the sum of ciphertexts [count][2][nl][N], limb by limb mod q_l"""
    out = np.zeros_like(cts[0])
    for l in range(cts.shape[2]):
        out[:, l] = (cts[:, :, l].astype(object).sum(axis=0) % P.moduli[l]).astype(np.uint64)
    return out


@pytest.mark.parametrize("nl", [3, 2])
@pytest.mark.parametrize("K", [2, 1])
def test_model_decrypts_to_the_dot_products(cells, K, nl):
    c = cells(K)
    P, n = c.P, N_TERMS
    A, B = np.ascontiguousarray(c.A[:, :, :nl]), np.ascontiguousarray(c.B[:, :, :nl])
    got = model.mul_relin_dot(P, A, B, n, c.rlk)  # pairwise
    assert got.shape == (GROUPS, 2, nl, P.N)
    assert all(int(got[:, :, l].max()) < P.moduli[l] for l in range(nl))
    vec = model.mul_relin_dot(P, A, B[n:2 * n], n, c.rlk)  # every group against the second group's vector
    assert np.array_equal(vec[1], got[1]) and not np.array_equal(vec[0], got[0])
    sq = model.mul_relin_dot(P, A, A, n, c.rlk)
    for g in range(GROUPS):
        rows = slice(g * n, (g + 1) * n)
        assert np.array_equal(P.decrypt(c.sk, got[g], P.N, scale=1), c.dot(c.x[rows], c.y[rows])), g
        assert np.array_equal(P.decrypt(c.sk, vec[g], P.N, scale=1), c.dot(c.x[rows], c.y[n:2 * n])), g
        assert np.array_equal(P.decrypt(c.sk, sq[g], P.N, scale=1), c.dot(c.x[rows], c.x[rows])), g


@pytest.mark.parametrize("K", [2, 1])
def test_one_term_is_the_product(cells, K):
    c = cells(K)
    got = model.mul_relin_dot(c.P, c.A[:2], c.B[:2], 1, c.rlk)
    assert np.array_equal(got, mr.mul_relin_sets(c.P, c.A[:2], c.B[:2], c.rlk))
    assert np.array_equal(model.tensor_dot(c.P, c.A[:2], c.B[:1], 1), mr.mul_tensor_sets(c.P, c.A[:2], c.B[:1]))


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("K", [2, 1])
def test_one_key_switch_is_told_from_n(cells, K, n):
    """The same sum as n separate relinearised products added up: other words (n roundings of the key switch against one),
    the same plaintext; the degree-2 triples, before any key, agree exactly"""
    c = cells(K)
    P = c.P
    A, B = c.A[:n], c.B[:n]
    one = model.mul_relin_dot(P, A, B, n, c.rlk)[0]
    many = _add(P, mr.mul_relin_sets(P, A, B, c.rlk))
    assert not np.array_equal(one, many)
    want = c.dot(c.x[:n], c.y[:n])
    assert np.array_equal(P.decrypt(c.sk, one, P.N, scale=1), want)
    assert np.array_equal(P.decrypt(c.sk, many, P.N, scale=1), want)
    assert np.array_equal(model.tensor_dot(P, A, B, n)[0], _add(P, mr.mul_tensor_sets(P, A, B)))
