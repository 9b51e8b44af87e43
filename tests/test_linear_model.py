"""CPU: tests/linear_model.py against the oracle.  (a) fhe.NTT's hard-coded cases rebuilt from the model's add / sub /
mul_scalar are lo_ct_ntt's words; (b) the oracle decrypts the model's results to the slot arithmetic they stand for;
(c) vdec.BatchCiphertexts spelt as MulNew + Add on the model is tests/vdec_model.py's batch."""
import numpy as np
import pytest

import linear_model as lm
import vdec_model as vm
from helpers import T_REF, T_SMALL, make_params, random_cts


@pytest.mark.parametrize("size", [2, 4, 8])
def test_ntt_base_cases_from_add_sub_mul_scalar(oracle, size):
    P = make_params(oracle, 8, 2)
    roots = oracle.field_roots(T_REF, 16)
    cts = random_cts(P, 8, 2, seed=size)
    v = [cts[i:i + 1].copy() for i in range(8)]
    lm.ntt_base_case(v, size, lm.ModelOps(P), int(roots[4]), int(roots[8]), lm.root8_cubed(P.T, roots))
    assert np.array_equal(np.concatenate(v), P.ct_ntt(cts, size, roots))


def test_centred_scalar_is_the_oracles(oracle):
    q = 0x3fffffffffc0001
    for T in (T_REF, T_SMALL, q):
        for w in (0, 1, T - 1, T >> 1, (T >> 1) + 1, 2**64 - 1, 0x123456789abcdef):
            assert lm.centred_scalar(w, T, q) == int(oracle.lib.lo_centered_scalar(w, T, q)), (T, w)
    assert lm.centred_scalar(2**64 - 1, q, q) == (2**64 - 1) % q  # a plain context: w mod T


@pytest.fixture(scope="module")
def fresh(oracle):
    """LogN = 10, three limbs, T = 0x3ee0001: a secret, three fresh encryptions and their messages"""
    P = make_params(oracle, 10, 3, T=T_SMALL)
    P.seed(77)
    sk = P.keygen_secret()
    pk = P.keygen_public(sk)
    rng = np.random.default_rng(7)
    m = rng.integers(0, P.T, size=(3, 16), dtype=np.uint64)
    cts = np.stack([P.encrypt(pk, P.encode(mi)) for mi in m])
    return P, sk, m, cts


def _dec(P, sk, cts):
    return np.stack([P.decrypt(sk, c, 16) for c in cts]).astype(object)


def test_oracle_decrypts_the_models_results(fresh):
    P, sk, m, cts = fresh
    T, mo = P.T, m.astype(object)
    a, b = cts[:2], cts[1:]
    assert np.array_equal(_dec(P, sk, lm.add(P, a, b)), (mo[:2] + mo[1:]) % T)
    assert np.array_equal(_dec(P, sk, lm.sub(P, a, b)), (mo[:2] - mo[1:]) % T)
    assert np.array_equal(_dec(P, sk, lm.add(P, cts, cts[2:])), (mo + mo[2:]) % T)  # one ciphertext against three
    for w in (0, 1, T - 1, T >> 1, (T >> 1) + 1, 2**64 - 1):
        assert np.array_equal(_dec(P, sk, lm.mul_scalar(P, cts, w)), mo * (w % T) % T), w
    v = np.random.default_rng(8).integers(0, T, size=16, dtype=np.uint64)
    pt, vo = P.encode(v), v.astype(object)
    assert np.array_equal(_dec(P, sk, lm.add_plain(P, cts, pt)), (mo + vo) % T)
    assert np.array_equal(_dec(P, sk, lm.sub_plain(P, cts, pt)), (mo - vo) % T)
    assert np.array_equal(_dec(P, sk, lm.mul_plain_then_add(P, a, pt, b)), (mo[1:] + mo[:2] * vo) % T)
    assert np.array_equal(_dec(P, sk, lm.mul_scalar_then_add(P, a, 5, b)), (mo[1:] + mo[:2] * 5) % T)
    assert np.array_equal(_dec(P, sk, lm.linear_combination(P, [cts[:1], cts[1:2], cts[2:]], [3, T - 1, 1])),
                          (3 * mo[:1] - mo[1:2] + mo[2:]) % T)


def test_min_level_and_broadcast(fresh):
    P, _, _, cts = fresh
    deep, shallow = cts, np.ascontiguousarray(cts[:, :, :2])
    for f in (lm.add, lm.sub):
        assert np.array_equal(f(P, deep, shallow), f(P, shallow, shallow)) and f(P, deep, shallow).shape[2] == 2
        assert np.array_equal(f(P, shallow, deep), f(P, shallow, shallow))
        assert np.array_equal(f(P, cts[:1], cts), np.concatenate([f(P, cts[:1], cts[i:i + 1]) for i in range(3)]))
    assert np.array_equal(lm.mul_plain_then_add(P, deep, P.encode([1, 2, 3]), shallow),
                          lm.mul_plain_then_add(P, shallow, P.encode([1, 2, 3], 2), shallow))
    with pytest.raises(AssertionError):
        lm.add(P, cts, cts[:2])


def test_batch_ciphertexts_spelt_as_mul_new_and_add(fresh):
    """vdec/batching.go:24-34 for three columns"""
    P, _, _, cts = fresh
    alphas = np.random.default_rng(9).integers(0, 2**63, size=(3, 16), dtype=np.uint64)
    acc = np.zeros((1,) + cts.shape[1:], dtype=np.uint64)
    for j in range(3):
        acc = lm.mul_plain_then_add(P, cts[j:j + 1], P.encode(vm.scaled(P, alphas[j], 1)), acc)
    assert np.array_equal(acc[0], vm.batch_ciphertexts(P, cts, alphas))
    for j in range(3):  # and MulNew alone is the oracle's
        zero = np.zeros_like(cts[j:j + 1])
        assert np.array_equal(lm.mul_plain_then_add(P, cts[j:j + 1], P.encode(alphas[j] % P.T), zero)[0],
                              P.mul_plain(cts[j], P.encode(alphas[j] % P.T)))
