"""CPU: the model of the seeded switching keys (keygen_seeded_model.py) against the model of the full keys
(keygen_model.py), and the conditions the GPU tests of test_keygen_seeded.py rely on -- the chosen vectors reach the
redraw path of the fused storer at attempts 1 and 2."""
import os
import re

import numpy as np

import keygen_model as km
import keygen_seeded_model as ksm
from keygen_seeded_model import A_SEED, SEED

SHAPES = ((10, 3, 2), (8, 2, 1), (12, 3, 2))


def test_a_seed_is_the_seed_constant_of_test_keygen():
    """A_SEED must be the constant under which test_keygen.py's test_model_vectors_contain_redraws pins the a words"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_keygen.py")).read()
    assert re.search(r"^SEED = bytes\(range\(32\)\)$", src, re.M)
    assert A_SEED == bytes(range(32)) and SEED != A_SEED


def test_equal_seeds_give_the_full_key(oracle):
    """with both seeds equal b is exactly what lumen_keygen_galois / lumen_keygen_relin return (and a their a)"""
    P, _ = ksm.params(oracle, 8, 2, 1)
    s = km.secret(P, A_SEED)
    for g in (5, 2 * P.N - 1):
        b, a, _ = ksm.galois_key(P, A_SEED, A_SEED, s, g)
        full, _ = km.galois_key(P, A_SEED, s, g)
        assert np.array_equal(b, full[:, 0]) and np.array_equal(a, full[:, 1]), g
        assert np.array_equal(ksm.full_key(b, a), full)
    b, a, _ = ksm.relin_key(P, A_SEED, A_SEED, s)
    full, _ = km.relin_key(P, A_SEED, s)
    assert np.array_equal(b, full[:, 0]) and np.array_equal(a, full[:, 1])


def test_different_seeds_change_both_halves(oracle):
    P, s = ksm.params(oracle, 8, 2, 1)
    LK = P.L + P.K
    for b, a, full in ((*ksm.model_galois(oracle, (8, 2, 1), 5)[:2], km.galois_key(P, SEED, s, 5)[0]),
                       (*ksm.model_relin(oracle, (8, 2, 1))[:2], km.relin_key(P, SEED, s)[0])):
        for d in range(P.beta()):
            for m in range(LK):
                assert not np.array_equal(b[d, m], full[d, 0, m]) and not np.array_equal(a[d, m], full[d, 1, m]), (d, m)
        assert all(int(x[:, m].max()) < q for x in (b, a) for m, q in enumerate(P.moduli))  # canonical
    # the key id separates the streams of one a_seed
    assert not np.array_equal(ksm.model_galois(oracle, (8, 2, 1), 5)[1], ksm.model_relin(oracle, (8, 2, 1))[1])
    # the loaders' mask is the a half
    assert np.array_equal(ksm.mask(P, A_SEED, km.ID_GALOIS + 5), ksm.model_galois(oracle, (8, 2, 1), 5)[1])


def test_b_is_a_switching_key_under_the_secret(oracle):
    """b + a * s_out - fac * s_in = NTT(e) with |e| <= 19, for every limb of every entry"""
    shape, g = (8, 2, 1), 5
    P, s = ksm.params(oracle, *shape)
    b, a, _ = ksm.model_galois(oracle, shape, g)
    s_out = km.galois_sout(P, s, g)
    for d in range(P.beta()):
        for m, q in enumerate(P.moduli):
            f = km.gadget_factor(P, d, 0, m, 0)
            ph = np.array([(int(x) + int(y) * int(z) - f * int(w)) % q for x, y, z, w in zip(b[d, m], a[d, m], s_out[m], s[m])],
                          dtype=np.uint64)
            e = P.limb_intt(ph, m).astype(object)
            e = np.where(e > q // 2, e - q, e)
            assert max(abs(int(x)) for x in e) <= 19, (d, m)


def test_chosen_vectors_reach_the_redraw_path(oracle):
    """Asserted, not assumed: under A_SEED the a words are the ones test_keygen.py pins (same index, same stream, same
    key), so g = 5 has first-attempt redraws in at least two limbs at (10, 3, 2) and second-attempt redraws at (8, 2, 1)
    and (12, 3, 2)."""
    for shape in SHAPES:
        P, _ = ksm.params(oracle, *shape)
        _, a, rd = ksm.model_galois(oracle, shape, 5)
        # a does not depend on the secret or on `seed`: the full key's a under A_SEED, whatever its secret
        assert np.array_equal(a, km.galois_key(P, A_SEED, km.secret(P, A_SEED), 5)[0][:, 1]), shape
        first, second = km.count_redraws(rd, 0), km.count_redraws(rd, 1)
        print(shape, "first-attempt redraws per (entry, limb):", first, "second:", sum(second))
        if shape == (10, 3, 2):
            LK = P.L + P.K
            assert len({i % LK for i, c in enumerate(first) if c}) >= 2
        else:
            assert sum(second) >= 1, shape
