"""The dot product with one relinearisation per sum at ring degree 2^15, the split degree (tests/test_degree15.py): L = 3,
K = 2, on the reference-style chain and on the chain directly below the context's modulus bound (rows of q - 1,
alternating words and a spike among both operands), two groups of two terms, pairwise and against one vector, against
tests/mul_relin_dot_model.py -- bit-exact."""
import numpy as np
import pytest

import keygen_model as km
import mul_relin_dot_model as model
import mul_relin_model as mr
from cells import KeyedCell
from helpers import CHAINS, _adversarial_cts, bound_chain, canonical, make_params, random_cts

gpu = pytest.mark.gpu

LOG_N = 15
KEY_SEED = bytes(range(32))


@gpu
@pytest.mark.parametrize("chain", CHAINS)
def test_dot_at_degree_15(oracle, chain):
    P = make_params(oracle, LOG_N, 3) if chain == "reference" else bound_chain(oracle, LOG_N, 3, 2)
    assert (P.L, P.K, P.N) == (3, 2, 1 << LOG_N)
    k = KeyedCell(P, 1600 + len(chain))
    try:
        ctx = k.ctx
        rlk, _ = km.relin_key(P, KEY_SEED, k.sk)
        ctx.load_relin_key(rlk)
        if chain == "reference":
            a, b = random_cts(P, 4, 3, seed=15), random_cts(P, 4, 3, seed=16)
        else:
            a = np.concatenate([_adversarial_cts(P, 3, seed=15), _adversarial_cts(P, 3, seed=16)[:1]])
            b = np.concatenate([_adversarial_cts(P, 3, seed=17)[:1], _adversarial_cts(P, 3, seed=18)])
        da, db, dv = ctx.upload(a), ctx.upload(b), ctx.upload(b[:2])
        want_d = model.tensor_dot(P, a, b, 2)
        assert np.array_equal(ctx.mul_tensor_dot(da, db, 2), want_d)
        got = ctx.mul_relin_dot(da, db, 2).download()
        assert got.shape == (2, 2, 3, P.N)
        for g in range(2):
            assert np.array_equal(got[g], mr.relinearise(P, want_d[g], rlk)), g
        assert canonical(P, got)
        vec = ctx.mul_relin_dot(da, dv, 2).download()
        assert np.array_equal(vec[0], got[0])  # the first group meets the same two ciphertexts in both forms
        assert np.array_equal(ctx.mul_tensor_dot(da, dv, 2), model.tensor_dot(P, a, b[:2], 2))
    finally:
        k.close()
