"""The noise statement behind the lower-level inner product, on the CPU oracle alone.

A fresh encryption rescaled to nl limbs, then matrixInnerSumEval at that level (MulNew, InnerSum, rescale to level 1):
with the prover's 57-bit T the result decrypts to the plain inner products from THREE limbs up.  Two limbs do not
carry it -- T * N * T * rows * (B + 1) < Q_nl / 2 is the budget, the arithmetic of tools/noise_budget.py --vdec -- so
the levels asserted are 5, 4 and 3.  L = 5, K = 2; LogN = 10 with 16 rows, and LogN = 8 with rows = N = 256 (every
column rotation and the row swap)."""
import numpy as np
import pytest

from helpers import T_REF, make_params


@pytest.mark.parametrize("log_n,rows", [(10, 16), (8, 256)], ids=["logn10-rows16", "logn8-rows256"])
def test_inner_product_decrypts_from_three_limbs_up(oracle, log_n, rows):
    P = make_params(oracle, log_n, 5)
    assert (P.L, P.K, P.T) == (5, 2, T_REF)
    P.seed(4000 + log_n)
    sk = P.keygen_secret()
    pk = P.keygen_public(sk)
    evks = [P.keygen_galois(sk, g) for g in P.inner_sum_galois_elements(rows)]
    rng = np.random.default_rng(log_n)
    cols = rng.integers(0, T_REF, size=(3, rows), dtype=np.uint64)  # uniform columns
    r = rng.integers(0, T_REF, size=rows, dtype=np.uint64)
    fresh = [P.encrypt(pk, P.encode(c)) for c in cols]
    want = [int(np.sum(c.astype(object) * r.astype(object)) % T_REF) for c in cols]
    for nl in (5, 4, 3):
        cts = []
        for ct in fresh:
            while ct.shape[1] > nl:
                ct = P.rescale(ct)
            cts.append(ct)
        got = P.matrix_inner_sum(np.stack(cts), P.encode(r, nl=nl), rows, evks)
        assert got.shape == (3, 2, 2, P.N)
        scale = P.rescale_scale(5, nl) * P.rescale_scale(nl, 2) % T_REF
        for i in range(3):
            assert int(P.decrypt(sk, got[i], 1, scale)[0]) == want[i], (nl, i)
