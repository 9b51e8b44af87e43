"""CPU: tests/lintrans_model.py, the judge of lumen_linear_transform, is the diagonal method.  N = 2^8 and 2^10, L = 3,
K = 2, T_REF: the model's output decrypts (mul_plain's scale: 1) to sum_k d_k[i] * v[(i + k) mod N/2] on both slot rows,
and its words differ from the per-rotation form's -- one ModDown for the sum against one per diagonal -- while both
decrypt alike."""
import numpy as np
import pytest

import lintrans_model as lm
from helpers import T_REF, make_params


class _Cell:
    def __init__(self, oracle, log_n):
        self.P = P = make_params(oracle, log_n, 3)
        assert (P.L, P.K, P.T) == (3, 2, T_REF)
        P.seed(8800 + log_n)
        self.sk = P.keygen_secret()
        pk = P.keygen_public(self.sk)
        rng = np.random.default_rng(88 + log_n)
        self.v = rng.integers(0, P.T, size=P.N, dtype=np.uint64)
        self.ct = P.encrypt(pk, P.encode(self.v))
        self.rng, self.evks = rng, {}

    def key(self, g):
        if g not in self.evks:
            self.evks[g] = self.P.keygen_galois(self.sk, g)
        return self.evks[g]

    def diagonals(self, ks):
        """{k: slot values [N]}, random in [0, T)"""
        return {k: self.rng.integers(0, self.P.T, size=self.P.N, dtype=np.uint64) for k in ks}

    def encoded(self, values):
        return {k: lm.encode_qp(self.P, d, 3) for k, d in values.items()}

    def want(self, values):
        """sum_k d_k[i] * v[(i + k) mod N/2] on each of the two rows, modulo T"""
        h, T = self.P.N // 2, self.P.T
        out = np.zeros(self.P.N, dtype=object)
        for k, d in values.items():
            rot = np.concatenate([np.roll(self.v[:h], -k), np.roll(self.v[h:], -k)]).astype(object)
            out = (out + d.astype(object) * rot) % T
        return out


@pytest.fixture(scope="module", params=[8, 10])
def cell(oracle, request):
    return _Cell(oracle, request.param)


def _decrypts(cell, ct, want):
    assert np.array_equal(cell.P.decrypt(cell.sk, ct, cell.P.N, scale=1).astype(object), want)


def test_encode_qp_extends_the_encoder(cell):
    P = cell.P
    d = cell.diagonals([3])[3]
    pt = lm.encode_qp(P, d, 2)
    assert pt.shape == (4, P.N) and np.array_equal(pt[:2], P.encode(d, nl=2))
    coef = (P.limb_intt(pt[0], 0).astype(object) * P.T) % P.moduli[0]  # the coefficient's lift in [0, T)
    for a in range(2):
        p = P.moduli[P.L + a]
        assert np.array_equal((P.limb_intt(pt[2 + a], P.L + a).astype(object) * P.T) % p, coef % p), a
        assert int(pt[2 + a].max()) < p


def test_full_matrix_replicated_along_the_row(cell):
    """an 8 x 8 matrix by its 8 diagonals, d_k[i] = M[i mod 8][(i + k) mod 8]: on a vector of period 8 the slots hold M x"""
    P = cell.P
    M = cell.rng.integers(0, P.T, size=(8, 8), dtype=np.uint64)
    i = np.arange(P.N) % (P.N // 2)
    values = {k: M[i % 8, (i + k) % 8] for k in range(8)}
    diags = cell.encoded(values)
    assert lm.elements(P, diags) == [P.galois_element(k) for k in range(1, 8)]
    got = lm.linear_transform(P, cell.ct, diags, cell.key)
    want = cell.want(values)
    _decrypts(cell, got, want)
    # ... and on a vector of period 8 that is the matrix-vector product
    x = cell.rng.integers(0, P.T, size=8, dtype=np.uint64)
    pk = P.keygen_public(cell.sk)
    ctx = P.encrypt(pk, P.encode(np.tile(x, P.N // 8)))
    mx = np.array([sum(int(M[r, c]) * int(x[c]) for c in range(8)) % P.T for r in range(8)], dtype=object)
    assert np.array_equal(P.decrypt(cell.sk, lm.linear_transform(P, ctx, diags, cell.key), P.N, scale=1).astype(object), np.tile(mx, P.N // 8))
    # one ModDown is not eight: other words, the same slots
    each = lm.linear_transform(P, cell.ct, diags, cell.key, per_rotation=True)
    assert not np.array_equal(each, got)
    _decrypts(cell, each, want)


def test_diagonal_zero_alone_is_mul_plain(cell):
    P = cell.P
    values = cell.diagonals([0])
    diags = cell.encoded(values)
    assert lm.elements(P, diags) == []
    got = lm.linear_transform(P, cell.ct, diags, None)
    assert np.array_equal(got, P.mul_plain(cell.ct, diags[0][:3]))
    _decrypts(cell, got, cell.want(values))


def test_one_negative_diagonal(cell):
    P = cell.P
    values = cell.diagonals([-1])
    diags = cell.encoded(values)
    assert lm.elements(P, diags) == [P.galois_element(-1)] == [P.galois_element(P.N // 2 - 1)]
    got = lm.linear_transform(P, cell.ct, diags, cell.key)
    _decrypts(cell, got, cell.want(values))
    each = lm.linear_transform(P, cell.ct, diags, cell.key, per_rotation=True)
    assert not np.array_equal(each, got)  # ModDown before the product is not ModDown behind it
    _decrypts(cell, each, cell.want(values))


def test_index_rules(cell):
    P = cell.P
    pt = np.zeros((5, P.N), dtype=np.uint64)
    for bad in ({P.N // 2: pt}, {-(P.N // 2): pt}, {1: pt, 1 - P.N // 2: pt}, {}):
        with pytest.raises(ValueError):
            lm.normalise(P, bad)
    assert [e for e, _, _ in lm.normalise(P, {-1: pt, 0: pt, P.N // 2 - 2: pt})] == [P.N // 2 - 1, 0, P.N // 2 - 2]
